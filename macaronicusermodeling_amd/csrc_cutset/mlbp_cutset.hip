// libmlbp_cutset.so: the model's true marginals and log Z by cutset conditioning (include/mlbp_cutset.h), gfx950 only,
// float64.
//
// Three kernels; the first two are chosen from (X, n_vars, P, U, n_forest) by mlbp_cutset_pick_kernel:
//   cutset_x64_kernel      X = 64: the forest's tables are copied into LDS once per workgroup, already rescaled, rows padded to
//                          65 entries so that a row per lane and a column per lane are both free of bank conflicts.  Then every
//                          WAVE walks configurations of its own (lane = state): its vectors are lane-private LDS slots, a
//                          contraction is 64 FMAs per lane against the LDS table with the vector's entries broadcast by
//                          v_readlane, every reduction is DPP -- no workgroup barrier inside the walk.  A wave writes its own
//                          partial: four per workgroup.
//   cutset_generic_kernel  any X in [2, 1024]: the whole workgroup walks one configuration at a time; tables streamed row by
//                          row with masked tails and rescaled as they are read; the vectors in LDS when they fit, else in the
//                          caller's workspace.
//   cutset_combine_kernel  one workgroup per graph: adds the partials of the graph's chunks in a fixed order, divides by Z, takes
//                          the one logarithm, and the score at the labels.
// Workgroup (g, k) of the generic kernel walks configurations k, k + chunks, ... of graph g; wave w of workgroup (g, k) of the
// X = 64 kernel walks 4 k + w, 4 k + w + 4 chunks, ...  Every scalar a workgroup or wave branches on (exponents, Z_c) comes
// out of a reduction and has the same bits in every thread of it.  Every cross-lane sum is
// mlbp_dev::wave_sum, so a result does not depend on the launch beyond the number of chunks.
// No device-side mutable globals: everything comes through CutsetDev.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/mlbp_cutset.h"
#define MLBP_GRAPH_NO_SWEEPS                // this library runs no sweep program: mlbp_cutset.h has no op kinds
#include "../csrc/mlbp_graph_device.h"
#include "../csrc/mlbp_graph_host.h"
#include "../csrc/mlbp_cutset_plan.h"       // the plan's layout and check, the power-of-two helpers: shared with libmlbp_exactmap.so

namespace {

using namespace mlbp_graph;

struct CutsetDev {
  const int32_t* plan;
  const double* pair_tables; const int32_t* pair_tab;
  const double* unary_tables; const int32_t* unary_tab;
  const int32_t* labels;
  double* partials;                          // [B][parts][n_vars * X + 2], parts = chunks (generic) or 4 chunks (X = 64)
  double* vectors;                           // generic kernel, vectors not in LDS: [B][chunks][5 n_vars + 2][round_up(X, 2)]
  double* log_z; double* marginals; double* score; double* joint_logp;
  int32_t B, X, n_vars, P, U, n_cut, n_free, n_items, n_consts, n_forest, n_pair_tables, n_unary_tables, n_configs, chunks, parts;
};

// ---- contractions: out[i] = sum_j T[i][j] m[j] (tm) or out[j] = sum_i m[i] T[i][j]; a barrier behind the result ---------
__device__ __forceinline__ void contract_stream(const double* T, int X, int te, bool tm, const double* m, double* out) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (tm) {
    for (int row = wave; row < X; row += WG / 64) {
      const double* Tr = T + (size_t)row * X;
      double acc = 0.0;
      for (int j = lane; j < X; j += 64) acc += ldexp(Tr[j], -te) * m[j];
      acc = wave_sum(acc);
      if (lane == 0) out[row] = acc;
    }
  } else {
    for (int j = t; j < X; j += WG) {
      double acc = 0.0;
#pragma unroll 4
      for (int i = 0; i < X; ++i) acc += m[i] * ldexp(T[(size_t)i * X + j], -te);
      out[j] = acc;
    }
  }
  __syncthreads();
}

// ---- any X: the workgroup walks a chunk's configurations ---------------------------------------------------
__global__ __launch_bounds__(WG) void cutset_generic_kernel(CutsetDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X, Xp = (X + 1) & ~1;
  const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  PlanSections<const_i32p> pl;
  carve_plan(as_const(d.plan), d.n_vars, d.P, d.U, d.n_cut, d.n_free, d.n_items, d.n_consts, pl);
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const int n_vars = d.n_vars, P = d.P, U = d.U, n_free = d.n_free, n_cut = d.n_cut;
  const size_t XX = (size_t)X * X;

  // LDS: [vectors, unless in the workspace] [scratch] [integers]
  double* lds = reinterpret_cast<double*>(smem);
  const size_t n_vec = (size_t)(5 * n_vars + 2) * Xp;
  double* vec;
  if (!d.vectors) {
    vec = lds;
    lds += n_vec;
  } else {
    vec = d.vectors + ((size_t)g * d.chunks + k) * n_vec;
  }
  double* scratch = lds;
  lds += 8;
  int* texp = reinterpret_cast<int*>(lds);                     // [P + U] exponent of every factor's table
  int* st = texp + P + U;                                      // [16] states of the configuration
  const size_t vs = (size_t)n_vars * Xp;
  double* acc = vec;                                           // [n_vars][Xp] sum over configurations of Z_c m_c, mantissas
  double* base = acc + vs;                                     // the product of a free variable's unary rows
  double* bel = base + vs;                                     // a free variable's vector: upward, then its full belief
  double* up = bel + vs;                                       // its message to its parent
  double* dn = up + vs;                                        // its parent's message to it
  double* raw = dn + vs;
  double* excl = raw + Xp;

  // every table's exponent
  for (int f = 0; f < P + U; ++f) {
    const double* T = f < P ? d.pair_tables + (size_t)ptab[f] * XX : d.unary_tables + (size_t)utab[f - P] * X;
    const size_t n = f < P ? XX : (size_t)X;
    double m = 0.0;
    for (size_t i = t; i < n; i += WG) m = fmax(m, T[i]);
    m = block_max(m, scratch);
    if (t == 0) texp[f] = exp_of(m);
  }
  __syncthreads();
  int e_fixed = 0;                                             // every factor enters every configuration once
  for (int f = 0; f < P + U; ++f) e_fixed += texp[f];
  for (size_t i = t; i < vs; i += WG) acc[i] = 0.0;
  for (int i = 0; i < n_free; ++i) {
    const int v = pl.order[i];
    for (int j = t; j < X; j += WG) {
      double b = 1.0;
      for (int it = pl.item_off[v]; it < pl.item_off[v + 1]; ++it)
        if (pl.items[3 * it] == MLBP_CUTSET_ITEM_UNARY) {
          const int u = pl.items[3 * it + 1];
          b *= ldexp(d.unary_tables[(size_t)utab[u] * X + j], -texp[P + u]);
        }
      base[(size_t)v * Xp + j] = b;
    }
    __syncthreads();
    e_fixed += rescale(base + (size_t)v * Xp, X, scratch);
  }

  // the free variable's configuration-free part times its cutset-incident rows and columns, at state j
  auto local = [&](int v, int j) {
    double b = base[(size_t)v * Xp + j];
    for (int it = pl.item_off[v]; it < pl.item_off[v + 1]; ++it) {
      const int kind = pl.items[3 * it];
      if (kind == MLBP_CUTSET_ITEM_UNARY) continue;
      const int p = pl.items[3 * it + 1], s = st[pl.items[3 * it + 2]];
      const double* T = d.pair_tables + (size_t)ptab[p] * XX;
      b *= ldexp(kind == MLBP_CUTSET_ITEM_COL ? T[(size_t)j * X + s] : T[(size_t)s * X + j], -texp[p]);
    }
    return b;
  };
  auto contract = [&](int p, bool tm, const double* m) {
    contract_stream(d.pair_tables + (size_t)ptab[p] * XX, X, texp[p], tm, m, raw);
  };

  Scaled sum = {0.0, EMPTY};                                   // sum of Z_c over this chunk
  for (int c = k; c < d.n_configs; c += d.chunks) {
    __syncthreads();
    if (t < n_cut) {
      int r = c;
      for (int q = 0; q < t; ++q) r /= X;
      st[t] = r % X;
    }
    __syncthreads();
    Scaled z = {1.0, e_fixed};
    for (int i = 0; i < d.n_consts; ++i) {
      const int f = pl.consts[4 * i + 1], s0 = st[pl.consts[4 * i + 2]];
      if (pl.consts[4 * i] == MLBP_CUTSET_CONST_UNARY) {
        mul(z, ldexp(d.unary_tables[(size_t)utab[f] * X + s0], -texp[P + f]));
      } else {
        const int s1 = st[pl.consts[4 * i + 3]];
        mul(z, ldexp(d.pair_tables[(size_t)ptab[f] * XX + (size_t)s0 * X + s1], -texp[f]));
      }
    }
    for (int i = 0; i < n_free; ++i) {
      const int v = pl.order[i];
      for (int j = t; j < X; j += WG) bel[(size_t)v * Xp + j] = local(v, j);
    }
    __syncthreads();

    // leaves to roots
    for (int i = 0; i < n_free; ++i) {
      const int v = pl.order[i], p = pl.parent[2 * v];
      double* bv = bel + (size_t)v * Xp;
      z.e += rescale(bv, X, scratch);
      if (p < 0) {
        double s = 0.0;
        for (int j = t; j < X; j += WG) s += bv[j];
        mul(z, block_sum(s, scratch));
      } else {
        const int par = pl.parent[2 * v + 1];
        contract(p, pl.pav[2 * p] != v, bv);
        z.e += rescale(raw, X, scratch);
        for (int j = t; j < X; j += WG) {
          up[(size_t)v * Xp + j] = raw[j];
          bel[(size_t)par * Xp + j] *= raw[j];
        }
        __syncthreads();
      }
    }
    if (z.m == 0.0) continue;                                  // Z_c = 0: nothing to add

    // Z_c joins the chunk's sum: the larger exponent is kept
    if (z.e > sum.e) {
      const int shift = max(sum.e - z.e, MIN_SHIFT);
      for (size_t i = t; i < vs; i += WG) acc[i] = ldexp(acc[i], shift);
      sum.m = ldexp(sum.m, shift);
      sum.e = z.e;
      __syncthreads();
    }
    const double w = ldexp(z.m, max(z.e - sum.e, MIN_SHIFT));
    sum.m += w;
    if (t < n_cut) acc[(size_t)pl.cutset[t] * Xp + st[t]] += w;

    // roots to leaves
    for (int i = n_free - 1; i >= 0; --i) {
      const int v = pl.order[i], p = pl.parent[2 * v];
      double* bv = bel + (size_t)v * Xp;
      if (p >= 0) {
        const int par = pl.parent[2 * v + 1];
        const bool par_has_parent = pl.parent[2 * par] >= 0;
        for (int j = t; j < X; j += WG) {
          double b = local(par, j);
          if (par_has_parent) b *= dn[(size_t)par * Xp + j];
          excl[j] = b;
        }
        for (int q = 0; q < n_free; ++q) {                     // the parent's other children
          const int sib = pl.order[q];
          if (sib == v || pl.parent[2 * sib + 1] != par) continue;
          for (int j = t; j < X; j += WG) excl[j] *= up[(size_t)sib * Xp + j];
        }
        __syncthreads();
        rescale(excl, X, scratch);
        contract(p, pl.pav[2 * p] == v, excl);
        rescale(raw, X, scratch);
        for (int j = t; j < X; j += WG) {
          dn[(size_t)v * Xp + j] = raw[j];
          bv[j] *= raw[j];
        }
      }
      double s = 0.0;
      for (int j = t; j < X; j += WG) s += bv[j];
      s = block_sum(s, scratch);
      for (int j = t; j < X; j += WG) acc[(size_t)v * Xp + j] += w * (bv[j] / s);
      __syncthreads();
    }
  }

  __syncthreads();
  double* out = d.partials + ((size_t)g * d.parts + k) * ((size_t)n_vars * X + 2);
  if (t == 0) {
    out[0] = sum.m;
    out[1] = (double)sum.e;
  }
  for (int v = 0; v < n_vars; ++v)
    for (int j = t; j < X; j += WG) out[2 + (size_t)v * X + j] = acc[(size_t)v * Xp + j];
}

// ---- X = 64: a wave per configuration ---------------------------------------------------------------------
constexpr int ROW = 65;                     // padded row of an LDS table

// The contraction of the padded LDS table with the wave's vector (m: the entry of this lane): lane i returns
// sum_j T[i][j] m[j] (tm) or sum_i m[i] T[i][lane].  Four chains of 16 FMAs, added pairwise.
__device__ __forceinline__ double wave_contract_x64(const double* table, bool tm, double m, int lane) {
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  if (tm) {
    const double* row = table + lane * ROW;
#pragma unroll
    for (int j = 0; j < 64; ++j) a[j & 3] = fma(row[j], read_lane(m, j), a[j & 3]);
  } else {
    const double* col = table + lane;
#pragma unroll
    for (int i = 0; i < 64; ++i) a[i & 3] = fma(read_lane(m, i), col[i * ROW], a[i & 3]);
  }
  return (a[0] + a[1]) + (a[2] + a[3]);
}

__global__ __launch_bounds__(WG) void cutset_x64_kernel(CutsetDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int X = 64;
  const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  PlanSections<const_i32p> pl;
  carve_plan(as_const(d.plan), d.n_vars, d.P, d.U, d.n_cut, d.n_free, d.n_items, d.n_consts, pl);
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const int n_vars = d.n_vars, P = d.P, U = d.U, n_free = d.n_free, n_cut = d.n_cut;

  // LDS: [forest tables, rows of 65] [base] [4 waves x (acc, phi, bel, up, dn)] [scratch] [table exponents]
  double* tabs = reinterpret_cast<double*>(smem);
  double* base = tabs + (size_t)d.n_forest * 64 * ROW;         // [n_vars][64] the product of a variable's unary rows
  const size_t vs = (size_t)n_vars * 64;
  double* acc = base + vs + (size_t)wave * 5 * vs;             // this wave's: sum over its configurations of Z_c m_c, mantissas
  double* phi = acc + vs;                                      // a free variable's own factors under the configuration
  double* bel = phi + vs;                                      // its vector on the way up
  double* up = bel + vs;                                       // its message to its parent
  double* dn = up + vs;                                        // its parent's message to it
  double* scratch = base + vs + 20 * vs;
  int* texp = reinterpret_cast<int*>(scratch + 8);

  for (int f = 0; f < P + U; ++f) {
    const double* T = f < P ? d.pair_tables + (size_t)ptab[f] * 4096 : d.unary_tables + (size_t)utab[f - P] * 64;
    const int n = f < P ? 4096 : 64;
    double m = 0.0;
    for (int i = t; i < n; i += WG) m = fmax(m, T[i]);
    m = block_max(m, scratch);
    if (t == 0) texp[f] = exp_of(m);
  }
  __syncthreads();
  int e_fixed = 0;                                             // every factor enters every configuration once
  for (int f = 0; f < P + U; ++f) e_fixed += texp[f];
  for (int p = 0; p < P; ++p) {
    const int s = pl.fslot[p];
    if (s < 0) continue;
    const double* T = d.pair_tables + (size_t)ptab[p] * 4096;
    const int te = texp[p];
    for (int i = t; i < 4096; i += WG) tabs[(size_t)s * 64 * ROW + (i >> 6) * ROW + (i & 63)] = ldexp(T[i], -te);
  }
  for (int v = 0; v < n_vars; ++v) {                           // the unary rows of every variable, free or cut, multiplied once
    if (t < 64) {
      double b = 1.0;
      for (int u = 0; u < U; ++u)
        if (pl.uvar[u] == v) b *= ldexp(d.unary_tables[(size_t)utab[u] * 64 + t], -texp[P + u]);
      base[(size_t)v * 64 + t] = b;
    }
    __syncthreads();
    e_fixed += rescale(base + (size_t)v * 64, X, scratch);
  }
  for (int v = 0; v < n_vars; ++v) acc[(size_t)v * 64 + lane] = 0.0;
  __syncthreads();                                             // the tables and base are read by every wave from here on

  auto state = [&](int q, int c) { return (c >> (6 * q)) & 63; };
  auto local = [&](int v, int c) {
    double b = base[(size_t)v * 64 + lane];
    for (int it = pl.item_off[v]; it < pl.item_off[v + 1]; ++it) {
      const int kind = pl.items[3 * it];
      if (kind == MLBP_CUTSET_ITEM_UNARY) continue;
      const int p = pl.items[3 * it + 1], s = state(pl.items[3 * it + 2], c);
      const double* T = d.pair_tables + (size_t)ptab[p] * 4096;
      b *= ldexp(kind == MLBP_CUTSET_ITEM_COL ? T[lane * 64 + s] : T[s * 64 + lane], -texp[p]);
    }
    return b;
  };

  Scaled sum = {0.0, EMPTY};                                   // sum of Z_c over this wave's configurations
  for (int c = 4 * k + wave; c < d.n_configs; c += 4 * d.chunks) {
    Scaled z = {1.0, e_fixed};
    for (int q = 0; q < n_cut; ++q) mul(z, base[(size_t)pl.cutset[q] * 64 + state(q, c)]);
    for (int i = 0; i < d.n_consts; ++i) {
      if (pl.consts[4 * i] != MLBP_CUTSET_CONST_PAIR) continue;
      const int f = pl.consts[4 * i + 1], s0 = state(pl.consts[4 * i + 2], c), s1 = state(pl.consts[4 * i + 3], c);
      mul(z, ldexp(d.pair_tables[(size_t)ptab[f] * 4096 + s0 * 64 + s1], -texp[f]));
    }
    for (int i = 0; i < n_free; ++i) {
      const int v = pl.order[i];
      bel[(size_t)v * 64 + lane] = phi[(size_t)v * 64 + lane] = local(v, c);
    }
    // leaves to roots
    for (int i = 0; i < n_free; ++i) {
      const int v = pl.order[i], p = pl.parent[2 * v];
      const double x = wave_rescale(bel[(size_t)v * 64 + lane], z.e);
      bel[(size_t)v * 64 + lane] = x;
      if (p < 0) {
        mul(z, wave_sum(x));
      } else {
        const int par = pl.parent[2 * v + 1];
        const double r = wave_rescale(wave_contract_x64(tabs + (size_t)pl.fslot[p] * 64 * ROW, pl.pav[2 * p] != v, x, lane), z.e);
        up[(size_t)v * 64 + lane] = r;
        bel[(size_t)par * 64 + lane] *= r;
      }
    }
    if (z.m == 0.0) continue;                                  // Z_c = 0: nothing to add

    // Z_c joins the wave's sum: the larger exponent is kept
    if (z.e > sum.e) {
      const int shift = max(sum.e - z.e, MIN_SHIFT);
      for (int v = 0; v < n_vars; ++v) acc[(size_t)v * 64 + lane] = ldexp(acc[(size_t)v * 64 + lane], shift);
      sum.m = ldexp(sum.m, shift);
      sum.e = z.e;
    }
    const double w = ldexp(z.m, max(z.e - sum.e, MIN_SHIFT));
    sum.m += w;
    for (int q = 0; q < n_cut; ++q)
      if (lane == state(q, c)) acc[(size_t)pl.cutset[q] * 64 + lane] += w;

    // roots to leaves
    for (int i = n_free - 1; i >= 0; --i) {
      const int v = pl.order[i], p = pl.parent[2 * v];
      double x = bel[(size_t)v * 64 + lane];
      if (p >= 0) {
        const int par = pl.parent[2 * v + 1];
        double b = phi[(size_t)par * 64 + lane];
        if (pl.parent[2 * par] >= 0) b *= dn[(size_t)par * 64 + lane];
        for (int q = 0; q < n_free; ++q) {                     // the parent's other children
          const int sib = pl.order[q];
          if (sib != v && pl.parent[2 * sib + 1] == par) b *= up[(size_t)sib * 64 + lane];
        }
        int unused = 0;
        b = wave_rescale(b, unused);
        const double r = wave_rescale(wave_contract_x64(tabs + (size_t)pl.fslot[p] * 64 * ROW, pl.pav[2 * p] == v, b, lane), unused);
        dn[(size_t)v * 64 + lane] = r;
        x *= r;
      }
      acc[(size_t)v * 64 + lane] += w * (x / wave_sum(x));
    }
  }

  double* out = d.partials + ((size_t)g * d.parts + 4 * k + wave) * ((size_t)n_vars * 64 + 2);
  if (lane == 0) {
    out[0] = sum.m;
    out[1] = (double)sum.e;
  }
  for (int v = 0; v < n_vars; ++v) out[2 + (size_t)v * 64 + lane] = acc[(size_t)v * 64 + lane];
}

// score at the labels of graph g, by one wave (every lane returns it): NaN when a label is outside [0, X).
__device__ __forceinline__ double wave_score(const CutsetDev& d, const_i32p pav, const_i32p uvar, int g, int lane) {
  const int32_t* lab = d.labels + (size_t)g * d.n_vars;
  const size_t X = (size_t)d.X;
  bool bad = false;
  for (int v = lane; v < d.n_vars; v += 64) bad |= (unsigned)lab[v] >= (unsigned)d.X;
  if (__any(bad)) return __builtin_nan("");
  double sc = 0.0;
  for (int p = lane; p < d.P; p += 64) {
    const int i = lab[pav[2 * p]], j = lab[pav[2 * p + 1]];
    sc += log(d.pair_tables[(size_t)d.pair_tab[(size_t)g * d.P + p] * X * X + (size_t)i * X + j]);
  }
  for (int u = lane; u < d.U; u += 64) sc += log(d.unary_tables[(size_t)d.unary_tab[(size_t)g * d.U + u] * X + lab[uvar[u]]]);
  return wave_sum(sc);
}

// ---- the partials of a graph's chunks -> its outputs ----------------------------------------------------
__global__ __launch_bounds__(WG) void cutset_combine_kernel(CutsetDev d) {
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool want = d.labels && (d.score || d.joint_logp);
  const double nan = __builtin_nan("");
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) {
    if (t == 0) {
      d.log_z[g] = nan;
      if (want && d.score) d.score[g] = nan;
      if (want && d.joint_logp) d.joint_logp[g] = nan;
    }
    return;
  }
  const size_t N = (size_t)d.n_vars * d.X, stride = N + 2;
  const double* ws = d.partials + (size_t)g * d.parts * stride;
  int emax = EMPTY;
  for (int k = 0; k < d.parts; ++k) emax = max(emax, (int)ws[k * stride + 1]);
  double Z = 0.0;
  for (int k = 0; k < d.parts; ++k) Z += ldexp(ws[k * stride], max((int)ws[k * stride + 1] - emax, MIN_SHIFT));
  const double uniform = 1.0 / (double)d.X;
  double* marg = d.marginals + (size_t)g * N;
  for (size_t i = t; i < N; i += WG) {
    double s = 0.0;
    for (int k = 0; k < d.parts; ++k) s += ldexp(ws[k * stride + 2 + i], max((int)ws[k * stride + 1] - emax, MIN_SHIFT));
    marg[i] = Z == 0.0 ? uniform : s / Z;
  }
  if (wave != 0) return;
  const double lz = Z == 0.0 ? -__builtin_huge_val() : fma((double)emax, 0.693147180559945309417232121458, log(Z));
  double sc = nan;
  if (want) {
    PlanSections<const_i32p> pl;
    carve_plan(as_const(d.plan), d.n_vars, d.P, d.U, d.n_cut, d.n_free, d.n_items, d.n_consts, pl);
    sc = wave_score(d, pl.pav, pl.uvar, g, lane);
  }
  if (lane == 0) {
    d.log_z[g] = lz;
    if (want && d.score) d.score[g] = sc;
    if (want && d.joint_logp) d.joint_logp[g] = sc - lz;
  }
}

// ---- host ----------------------------------------------------------------------------------------
thread_local int g_last_kernel = MLBP_CUTSET_KERNEL_NONE;

int64_t ints_bytes(int64_t P, int64_t U) { return 4 * ((P + U + 16 + 3) / 4 * 4); }
int64_t vector_doubles(int64_t n_vars, int64_t X) { return (5 * n_vars + 2) * ((X + 1) / 2 * 2); }
int64_t x64_lds_bytes(int64_t n_vars, int64_t P, int64_t U, int64_t n_forest) {
  return n_forest * 33280 + 21 * n_vars * 512 + 64 + ints_bytes(P, U);
}
int64_t generic_lds_bytes(int64_t n_vars, int64_t P, int64_t U, int64_t X) { return vector_doubles(n_vars, X) * 8 + 64 + ints_bytes(P, U); }

}  // namespace

extern "C" {

const char* mlbp_cutset_arch(void) { return "gfx950"; }
const char* mlbp_cutset_last_error(void) { return g_last_error.c_str(); }
int mlbp_cutset_last_kernel(void) { return g_last_kernel; }

int mlbp_cutset_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest) {
  if (X < 2 || n_vars <= 0 || P < 0 || U < 0 || n_forest < 0 || n_forest > P)
    return fail(MLBP_EINVAL, "pick_kernel: X = %d, n_vars = %d, P = %d, U = %d, n_forest = %d", X, n_vars, P, U, n_forest);
  if (X > MLBP_CUTSET_MAX_X) return fail(MLBP_EUNSUPPORTED, "X = %d: at most %d states are supported", X, MLBP_CUTSET_MAX_X);
  if (X == 64 && x64_lds_bytes(n_vars, P, U, n_forest) <= MLBP_CUTSET_X64_LDS_BYTES) return MLBP_CUTSET_KERNEL_X64;
  if (64 + ints_bytes(P, U) > MLBP_CUTSET_GENERIC_LDS_BYTES)
    return fail(MLBP_EUNSUPPORTED, "P + U = %lld factors: their exponents do not fit the LDS budget", (long long)P + U);
  return MLBP_CUTSET_KERNEL_GENERIC;
}

int mlbp_cutset_chunks(int32_t B, int32_t n_configs) {
  if (B <= 0 || n_configs <= 0) return fail(MLBP_EINVAL, "chunks: B = %d, n_configs = %d", B, n_configs);
  const int32_t spread = (MLBP_CUTSET_MIN_WORKGROUPS + B - 1) / B;
  return n_configs < spread ? n_configs : spread;
}

int64_t mlbp_cutset_workspace_bytes(int32_t B, int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t n_cut) {
  const int which = mlbp_cutset_pick_kernel(X, n_vars, P, U, n_forest);
  if (which < 0) return which;
  if (n_cut < 0 || n_cut > n_vars) return fail(MLBP_EINVAL, "workspace: n_cut = %d with %d variables", n_cut, n_vars);
  const int64_t n_configs = count_configs(X, n_cut);
  if (n_configs < 0) return too_many_configs(X, n_cut);
  const int chunks = mlbp_cutset_chunks(B, (int32_t)n_configs);
  if (chunks < 0) return chunks;
  int64_t per = (int64_t)n_vars * X + 2;
  if (which == MLBP_CUTSET_KERNEL_X64) per *= 4;               // a partial per wave
  else if (generic_lds_bytes(n_vars, P, U, X) > MLBP_CUTSET_GENERIC_LDS_BYTES) per += vector_doubles(n_vars, X);
  return (int64_t)B * chunks * per * 8;
}

int mlbp_cutset_check_plan(const int32_t* plan, int32_t n_words, int32_t X) { return check_packed_plan(plan, n_words, X); }

int mlbp_cutset_f64(const mlbp_cutset_args* a, void* stream) {
  g_last_kernel = MLBP_CUTSET_KERNEL_NONE;
  if (!a) return fail(MLBP_EINVAL, "args is NULL");
  if (a->B <= 0 || a->n_vars <= 0 || a->P < 0 || a->U < 0 || a->P + a->U <= 0 || a->n_cut < 0 || a->n_free < 0 || a->n_items < 0 ||
      a->n_consts < 0 || (int64_t)a->n_cut + a->n_free != a->n_vars)
    return fail(MLBP_EINVAL, "bad sizes: B %d, n_vars %d, P %d, U %d, n_cut %d, n_free %d, n_items %d, n_consts %d", a->B, a->n_vars, a->P,
                a->U, a->n_cut, a->n_free, a->n_items, a->n_consts);
  if (int e = check_states(a->X)) return e;
  const int which = mlbp_cutset_pick_kernel(a->X, a->n_vars, a->P, a->U, a->n_forest);
  if (which < 0) return which;
  if (!a->plan || plan_words(a->n_vars, a->P, a->U, a->n_cut, a->n_free, a->n_items, a->n_consts) != a->plan_words)
    return fail(MLBP_EINVAL, "plan is NULL or plan_words = %d disagrees with the sizes", a->plan_words);
  if (int e = check_args_tables(a)) return e;
  if (!a->log_z || !a->marginals) return fail(MLBP_EINVAL, "log_z or marginals is NULL");
  if ((a->score || a->joint_logp) && !a->labels) return fail(MLBP_EINVAL, "score and joint_logp need labels");
  const int64_t n_configs = count_configs(a->X, a->n_cut);
  if (n_configs < 0) return too_many_configs(a->X, a->n_cut);
  const int chunks = mlbp_cutset_chunks(a->B, (int32_t)n_configs);
  if (chunks < 0) return chunks;
  if ((int64_t)a->n_vars * a->X > 0x7fffffff / 16) return fail(MLBP_EUNSUPPORTED, "n_vars * X = %lld too large", (long long)a->n_vars * a->X);
  const int64_t need = mlbp_cutset_workspace_bytes(a->B, a->X, a->n_vars, a->P, a->U, a->n_forest, a->n_cut);
  if (need < 0) return (int)need;
  if (!a->workspace || a->workspace_bytes < need)
    return fail(MLBP_EINVAL, "workspace is NULL or workspace_bytes = %lld below the %lld the call needs", (long long)a->workspace_bytes, (long long)need);
  if (int e = check_device("libmlbp_cutset.so")) return e;
  CutsetDev d;
  d.plan = a->plan;
  d.pair_tables = a->pair_tables; d.pair_tab = a->pair_tab; d.unary_tables = a->unary_tables; d.unary_tab = a->unary_tab;
  d.labels = a->labels;
  d.partials = a->workspace;
  d.vectors = nullptr;
  d.log_z = a->log_z; d.marginals = a->marginals; d.score = a->score; d.joint_logp = a->joint_logp;
  d.B = a->B; d.X = a->X; d.n_vars = a->n_vars; d.P = a->P; d.U = a->U; d.n_cut = a->n_cut; d.n_free = a->n_free; d.n_items = a->n_items;
  d.n_consts = a->n_consts; d.n_forest = a->n_forest; d.n_pair_tables = a->n_pair_tables; d.n_unary_tables = a->n_unary_tables;
  d.n_configs = (int32_t)n_configs; d.chunks = chunks; d.parts = which == MLBP_CUTSET_KERNEL_X64 ? 4 * chunks : chunks;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(a->B, chunks);
  (void)hipGetLastError();
  if (which == MLBP_CUTSET_KERNEL_X64) {
    if (int e = grant_x64_lds((const void*)cutset_x64_kernel, 0, MLBP_CUTSET_X64_LDS_BYTES)) return e;
    hipLaunchKernelGGL(cutset_x64_kernel, grid, dim3(WG), (size_t)x64_lds_bytes(a->n_vars, a->P, a->U, a->n_forest), st, d);
  } else {
    int64_t lds = generic_lds_bytes(a->n_vars, a->P, a->U, a->X);
    if (lds > MLBP_CUTSET_GENERIC_LDS_BYTES) {
      d.vectors = a->workspace + (int64_t)a->B * chunks * ((int64_t)a->n_vars * a->X + 2);
      lds = 64 + ints_bytes(a->P, a->U);
    }
    hipLaunchKernelGGL(cutset_generic_kernel, grid, dim3(WG), (size_t)lds, st, d);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MLBP_EHIP, "cutset launch failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(cutset_combine_kernel, dim3(a->B), dim3(WG), 0, st, d);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(MLBP_EHIP, "combine launch failed: %s", hipGetErrorString(e));
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
