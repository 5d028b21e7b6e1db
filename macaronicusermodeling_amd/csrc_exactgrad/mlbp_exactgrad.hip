// libmlbp_exactgrad.so: the model's true pairwise marginals, expected features and likelihood gradient by cutset conditioning
// (include/mlbp_exactgrad.h), gfx950 only, float64.
//
// Three kernels; the walk kernel is chosen from (X, n_vars, P, U, n_forest) by mlbp_exactgrad_pick_kernel:
//   exactgrad_x64_kernel<NF>   X = 64, n_forest <= 2, NF = max(n_forest, 1): the walk of cutset_x64_kernel restated -- the forest's tables in LDS,
//                              rows of 65, every WAVE its own configurations, lane = state, no workgroup barrier inside the walk
//                              -- and beside it the wave's pair accumulators: the 64 x 64 sum of rank-1 updates of every forest
//                              factor in registers (lane = column, 64 doubles per lane, 64 FMAs on v_readlane broadcasts per
//                              configuration), the rows of the cutset-incident factors and the cells of the cutset-internal
//                              ones in the wave's own partial in the workspace.
//   exactgrad_generic_kernel   any X in [2, 1024]: the walk of cutset_generic_kernel restated, the workgroup one configuration at
//                              a time; every pair accumulator in the workgroup's partial.
//   exactgrad_combine_kernel   one workgroup per graph: adds the partials in index order, applies the rescaled table to the
//                              forest factors, divides by Z, writes the requested tensors, contracts with phi eight features
//                              at a time, forms the observed features at the labels and takes the one logarithm.
// A global accumulator entry is only ever touched by one lane (X = 64: entry [row][lane] by `lane`), or by threads of one
// workgroup with a barrier between two touches (generic); there is no atomic.  Every scalar a wave or workgroup branches on comes
// out of a reduction and has the same bits in every thread of it.
// No device-side mutable globals: everything comes through GradDev.
#include <hip/hip_runtime.h>

#include "../../include/mlbp_exactgrad.h"
#define MLBP_GRAPH_NO_SWEEPS                // this library runs no sweep program
#include "../csrc/mlbp_graph_device.h"
#include "../csrc/mlbp_graph_host.h"
#include "../csrc/mlbp_cutset_plan.h"       // the plan's layout and check, the power-of-two helpers

namespace {

using namespace mlbp_graph;

constexpr int MAXF = MLBP_EXACTGRAD_MAX_FEATURES;
constexpr int FG = 8;                       // features contracted per pass of the combine kernel

struct GradDev {
  const int32_t* plan;
  const double* pair_tables; const int32_t* pair_tab;
  const double* unary_tables; const int32_t* unary_tab;
  const double* phi_en_en; const double* phi_en_en_w1; const double* phi_en_de;
  const int32_t* pair_phi; const int32_t* unary_kind; const int32_t* unary_obs; const int32_t* labels;
  double* partials;                          // [B][parts][stride]: {sum mantissa, exponent, [n_vars][X], [P][X][X]}
  double* vectors;                           // generic kernel, vectors not in LDS: [B][chunks][5 n_vars + 2][round_up(X, 2)]
  double* log_z; double* marginals; double* pair_marginals; double* expect_ee; double* expect_ed; double* grad_ee; double* grad_ed;
  int64_t stride;
  int32_t B, X, n_vars, P, U, n_cut, n_free, n_items, n_consts, n_forest, n_pair_tables, n_unary_tables, n_configs, chunks, parts;
  int32_t F_ee, F_ed, Vde;
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
__global__ __launch_bounds__(WG) void exactgrad_generic_kernel(GradDev d) {
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
  double* out = d.partials + ((size_t)g * d.parts + k) * d.stride;
  double* pacc = out + 2 + (size_t)n_vars * X;                 // [P][X][X] pair accumulators, mantissas under the sum's exponent

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

    // Z_c joins the chunk's sum: the larger exponent is kept; the first Z_c clears the pair accumulators
    if (z.e > sum.e) {
      const bool first = sum.e == EMPTY;
      const int shift = max(sum.e - z.e, MIN_SHIFT);
      for (size_t i = t; i < vs; i += WG) acc[i] = ldexp(acc[i], shift);
      for (size_t i = t; i < (size_t)P * XX; i += WG) pacc[i] = first ? 0.0 : ldexp(pacc[i], shift);
      sum.m = ldexp(sum.m, shift);
      sum.e = z.e;
      __syncthreads();
    }
    const double w = ldexp(z.m, max(z.e - sum.e, MIN_SHIFT));
    sum.m += w;
    if (t < n_cut) acc[(size_t)pl.cutset[t] * Xp + st[t]] += w;
    if (t == 0)
      for (int i = 0; i < d.n_consts; ++i)
        if (pl.consts[4 * i] == MLBP_CUTSET_CONST_PAIR)          // a factor inside the cutset: its cell gains Z_c
          pacc[(size_t)pl.consts[4 * i + 1] * XX + (size_t)st[pl.consts[4 * i + 2]] * X + st[pl.consts[4 * i + 3]]] += w;

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
        const bool v_on_axis0 = pl.pav[2 * p] == v;
        contract(p, v_on_axis0, excl);
        const int er = rescale(raw, X, scratch);
        // the forest factor's rank-1 update: a = bv (v's vector on the way up), b = excl, a^T T~ b = 2^er sum_i a[i] raw[i]
        double s = 0.0;
        for (int j = t; j < X; j += WG) s += bv[j] * raw[j];
        const double coef = ldexp(w / block_sum(s, scratch), -er);
        const double* v0 = v_on_axis0 ? bv : excl;
        const double* v1 = v_on_axis0 ? excl : bv;
        double* A = pacc + (size_t)p * XX;
        for (int r = 0; r < X; ++r) {
          const double ar = coef * v0[r];
          for (int j = t; j < X; j += WG) A[(size_t)r * X + j] = fma(ar, v1[j], A[(size_t)r * X + j]);
        }
        __syncthreads();
        for (int j = t; j < X; j += WG) {
          dn[(size_t)v * Xp + j] = raw[j];
          bv[j] *= raw[j];
        }
      }
      double s = 0.0;
      for (int j = t; j < X; j += WG) s += bv[j];
      s = block_sum(s, scratch);
      for (int j = t; j < X; j += WG) {
        const double wm = w * (bv[j] / s);
        acc[(size_t)v * Xp + j] += wm;
        for (int it = pl.item_off[v]; it < pl.item_off[v + 1]; ++it)       // row s_q of every cutset-incident factor, [s_q][state of v]
          if (pl.items[3 * it] != MLBP_CUTSET_ITEM_UNARY)
            pacc[(size_t)pl.items[3 * it + 1] * XX + (size_t)st[pl.items[3 * it + 2]] * X + j] += wm;
      }
      __syncthreads();
    }
  }

  __syncthreads();
  if (t == 0) {
    out[0] = sum.m;
    out[1] = (double)sum.e;
  }
  if (sum.e == EMPTY) return;
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

// R[i] += v0[i] * v1[lane]: the rank-1 update of a 64 x 64 accumulator held as 64 registers per lane (lane = column).
__device__ __forceinline__ void rank1_x64(double (&R)[64], double v0, double v1) {
#pragma unroll
  for (int i = 0; i < 64; ++i) R[i] = fma(read_lane(v0, i), v1, R[i]);
}

template <int NF>
__global__ __launch_bounds__(WG) void exactgrad_x64_kernel(GradDev d) {
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
  double* out = d.partials + ((size_t)g * d.parts + 4 * k + wave) * d.stride;
  double* pacc = out + 2 + vs;                                 // [P][64][64] this wave's pair accumulators in its partial

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
  double R[NF][64];                                            // the forest factors' accumulators, [row][lane = column] in table axes
#pragma unroll
  for (int s = 0; s < NF; ++s)
#pragma unroll
    for (int i = 0; i < 64; ++i) R[s][i] = 0.0;
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

    // Z_c joins the wave's sum: the larger exponent is kept; the first Z_c clears the accumulators in the partial
    if (z.e > sum.e) {
      const bool first = sum.e == EMPTY;
      const int shift = max(sum.e - z.e, MIN_SHIFT);
      for (int v = 0; v < n_vars; ++v) acc[(size_t)v * 64 + lane] = ldexp(acc[(size_t)v * 64 + lane], shift);
      for (int p = 0; p < P; ++p) {
        if (pl.fslot[p] >= 0) continue;
        double* A = pacc + (size_t)p * 4096;
        for (int i = lane; i < 4096; i += 64) A[i] = first ? 0.0 : ldexp(A[i], shift);
      }
#pragma unroll
      for (int s = 0; s < NF; ++s)
#pragma unroll
        for (int i = 0; i < 64; ++i) R[s][i] = ldexp(R[s][i], shift);
      sum.m = ldexp(sum.m, shift);
      sum.e = z.e;
    }
    const double w = ldexp(z.m, max(z.e - sum.e, MIN_SHIFT));
    sum.m += w;
    for (int q = 0; q < n_cut; ++q)
      if (lane == state(q, c)) acc[(size_t)pl.cutset[q] * 64 + lane] += w;
    for (int i = 0; i < d.n_consts; ++i) {                     // a factor inside the cutset: its cell gains Z_c
      if (pl.consts[4 * i] != MLBP_CUTSET_CONST_PAIR) continue;
      const int s0 = state(pl.consts[4 * i + 2], c), s1 = state(pl.consts[4 * i + 3], c);
      if (lane == s1) pacc[(size_t)pl.consts[4 * i + 1] * 4096 + s0 * 64 + lane] += w;
    }

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
        int unused = 0, er = 0;
        b = wave_rescale(b, unused);
        const bool v_on_axis0 = pl.pav[2 * p] == v;
        const int slot = pl.fslot[p];
        const double r = wave_rescale(wave_contract_x64(tabs + (size_t)slot * 64 * ROW, v_on_axis0, b, lane), er);
        dn[(size_t)v * 64 + lane] = r;
        const double a = x;                                    // v's vector on the way up
        x *= r;
        const double total = wave_sum(x);                      // a^T T~ b = 2^er total
        const double coef = ldexp(w / total, -er);
        const double v0 = v_on_axis0 ? a : b, v1 = coef * (v_on_axis0 ? b : a);
        if (slot == 0) rank1_x64(R[0], v0, v1);
        else if (NF > 1 && slot == 1) rank1_x64(R[NF - 1], v0, v1);
        x /= total;
      } else {
        x /= wave_sum(x);
      }
      const double wm = w * x;
      acc[(size_t)v * 64 + lane] += wm;
      for (int it = pl.item_off[v]; it < pl.item_off[v + 1]; ++it)       // row s_q of every cutset-incident factor, [s_q][state of v]
        if (pl.items[3 * it] != MLBP_CUTSET_ITEM_UNARY)
          pacc[(size_t)pl.items[3 * it + 1] * 4096 + state(pl.items[3 * it + 2], c) * 64 + lane] += wm;
    }
  }

  if (lane == 0) {
    out[0] = sum.m;
    out[1] = (double)sum.e;
  }
  if (sum.e == EMPTY) return;                                  // an empty partial holds nothing else
  for (int v = 0; v < n_vars; ++v) out[2 + (size_t)v * 64 + lane] = acc[(size_t)v * 64 + lane];
  for (int p = 0; p < P; ++p) {
    const int slot = pl.fslot[p];
    if (slot < 0) continue;
    double* A = pacc + (size_t)p * 4096 + lane;
    if (slot == 0) {
#pragma unroll
      for (int i = 0; i < 64; ++i) A[i * 64] = R[0][i];
    } else if (NF > 1 && slot == 1) {
#pragma unroll
      for (int i = 0; i < 64; ++i) A[i * 64] = R[NF - 1][i];
    }
  }
}

// ---- the partials of a graph's chunks -> its outputs ----------------------------------------------------
__global__ __launch_bounds__(WG) void exactgrad_combine_kernel(GradDev d) {
  __shared__ double scratch[8];
  __shared__ double ex_ee[MAXF], ex_ed[MAXF], ob_ee[MAXF], ob_ed[MAXF];
  const int g = blockIdx.x, t = threadIdx.x;
  const int X = d.X, P = d.P, U = d.U, F_ee = d.F_ee, F_ed = d.F_ed;
  const bool want_expect = d.expect_ee || d.expect_ed || d.grad_ee || d.grad_ed;
  const bool want_grad = d.grad_ee || d.grad_ed;
  const double nan = __builtin_nan("");
  if (!tables_in_range(d.pair_tab, P, d.n_pair_tables, d.unary_tab, U, d.n_unary_tables, g)) {
    if (t == 0) {
      d.log_z[g] = nan;
      for (int f = 0; f < F_ee; ++f) {
        if (d.expect_ee) d.expect_ee[(size_t)g * F_ee + f] = nan;
        if (d.grad_ee) d.grad_ee[(size_t)g * F_ee + f] = nan;
      }
      for (int f = 0; f < F_ed; ++f) {
        if (d.expect_ed) d.expect_ed[(size_t)g * F_ed + f] = nan;
        if (d.grad_ed) d.grad_ed[(size_t)g * F_ed + f] = nan;
      }
    }
    return;
  }
  PlanSections<const_i32p> pl;
  carve_plan(as_const(d.plan), d.n_vars, P, U, d.n_cut, d.n_free, d.n_items, d.n_consts, pl);
  const size_t XX = (size_t)X * X, stride = (size_t)d.stride;
  const double* ws = d.partials + (size_t)g * d.parts * stride;
  int emax = EMPTY;
  for (int k = 0; k < d.parts; ++k) emax = max(emax, (int)ws[k * stride + 1]);
  double Z = 0.0;
  for (int k = 0; k < d.parts; ++k) Z += ldexp(ws[k * stride], max((int)ws[k * stride + 1] - emax, MIN_SHIFT));
  // entry `at` of the partials (behind the two header words), summed in index order; an empty partial holds nothing
  auto summed = [&](size_t at) {
    double s = 0.0;
    for (int k = 0; k < d.parts; ++k) {
      const int e = (int)ws[k * stride + 1];
      if (e != EMPTY) s += ldexp(ws[k * stride + 2 + at], max(e - emax, MIN_SHIFT));
    }
    return s;
  };
  const size_t N = (size_t)d.n_vars * X;
  const double uniform = 1.0 / (double)X;
  if (d.marginals)
    for (size_t i = t; i < N; i += WG) d.marginals[(size_t)g * N + i] = Z == 0.0 ? uniform : summed(i) / Z;
  if (t < MAXF) ex_ee[t] = ex_ed[t] = ob_ee[t] = ob_ed[t] = 0.0;
  __syncthreads();

  // ---- pairwise factors: M_p, then its contraction with phi_p ----
  if (d.pair_marginals || want_expect) {
    for (int p = 0; p < P; ++p) {
      // where the factor was accumulated: a forest factor in table axes (T~ still to be applied), a factor inside the cutset in
      // table axes, a cutset-incident one as [s_q][state of the free variable]: transposed when that variable is on axis 0
      const bool forest = pl.fslot[p] >= 0;
      bool transposed = false;
      for (int it = 0; it < d.n_items; ++it)
        if (pl.items[3 * it] == MLBP_CUTSET_ITEM_COL && pl.items[3 * it + 1] == p) transposed = true;
      const double* T = d.pair_tables + (size_t)d.pair_tab[(size_t)g * P + p] * XX;
      int te = 0;
      if (forest) {
        double m = 0.0;
        for (size_t i = t; i < XX; i += WG) m = fmax(m, T[i]);
        te = exp_of(block_max(m, scratch));
      }
      const double* phi = want_expect ? (d.pair_phi[p] == 0 ? d.phi_en_en : d.phi_en_en_w1) : nullptr;
      double* pm = d.pair_marginals ? d.pair_marginals + ((size_t)g * P + p) * XX : nullptr;
      const int n_pass = want_expect ? (F_ee + FG - 1) / FG : 1;
      for (int pass = 0; pass < n_pass; ++pass) {
        const int f0 = pass * FG;
        double fs[FG];
#pragma unroll
        for (int q = 0; q < FG; ++q) fs[q] = 0.0;
        for (size_t src = t; src < XX; src += WG) {            // in the accumulator's order: the partials are read in whole lines
          const size_t hi = src / X, lo = src - hi * X;
          const size_t idx = transposed ? lo * X + hi : src;   // the entry's place in table axes
          double m = uniform * uniform;
          if (Z != 0.0) {
            m = summed(N + (size_t)p * XX + src) / Z;
            if (forest) m *= ldexp(T[idx], -te);
          }
          if (pm && pass == 0) pm[idx] = m;
          if (want_expect) {
#pragma unroll
            for (int q = 0; q < FG; ++q)
              if (f0 + q < F_ee) fs[q] = fma(m, phi[idx * F_ee + f0 + q], fs[q]);
          }
        }
        if (want_expect) {
#pragma unroll
          for (int q = 0; q < FG; ++q) {
            if (f0 + q >= F_ee) continue;                      // (uniform)
            const double total = block_sum(fs[q], scratch);
            if (t == 0) ex_ee[f0 + q] += total;
          }
        }
      }
    }
  }

  // ---- unary factors: the variable's marginal against phi_u at the observed column ----
  bool bad = false;                                            // a column or selector out of range: no gradient
  if (want_expect) {
    for (int u = 0; u < U; ++u) {
      const int kind = d.unary_kind[u], obs = d.unary_obs[(size_t)g * U + u], v = pl.uvar[u];
      const int cols = kind == 2 ? d.Vde : X;
      if ((unsigned)kind > 2u || (unsigned)obs >= (unsigned)cols) {
        bad = true;
        continue;
      }
      const double* phi = kind == 0 ? d.phi_en_en : kind == 1 ? d.phi_en_en_w1 : d.phi_en_de;
      const int F = kind == 2 ? F_ed : F_ee;
      double* ex = kind == 2 ? ex_ed : ex_ee;
      for (int f0 = 0; f0 < F; f0 += FG) {
        double fs[FG];
#pragma unroll
        for (int q = 0; q < FG; ++q) fs[q] = 0.0;
        for (int i = t; i < X; i += WG) {
          const double m = Z == 0.0 ? uniform : summed((size_t)v * X + i) / Z;
#pragma unroll
          for (int q = 0; q < FG; ++q)
            if (f0 + q < F) fs[q] = fma(m, phi[((size_t)i * cols + obs) * F + f0 + q], fs[q]);
        }
#pragma unroll
        for (int q = 0; q < FG; ++q) {
          if (f0 + q >= F) continue;
          const double total = block_sum(fs[q], scratch);
          if (t == 0) ex[f0 + q] += total;
        }
      }
    }
  }
  if (t != 0) return;

  // ---- thread 0: the observed features at the labels, the outputs ----
  if (want_grad) {
    const int32_t* lab = d.labels + (size_t)g * d.n_vars;
    for (int v = 0; v < d.n_vars; ++v) bad |= (unsigned)lab[v] >= (unsigned)X;
    if (!bad) {
      for (int p = 0; p < P; ++p) {
        const double* phi = (d.pair_phi[p] == 0 ? d.phi_en_en : d.phi_en_en_w1) + ((size_t)lab[pl.pav[2 * p]] * X + lab[pl.pav[2 * p + 1]]) * F_ee;
        for (int f = 0; f < F_ee; ++f) ob_ee[f] += phi[f];
      }
      for (int u = 0; u < U; ++u) {
        const int kind = d.unary_kind[u], obs = d.unary_obs[(size_t)g * U + u];
        const int cols = kind == 2 ? d.Vde : X, F = kind == 2 ? F_ed : F_ee;
        const double* phi = (kind == 0 ? d.phi_en_en : kind == 1 ? d.phi_en_en_w1 : d.phi_en_de) + ((size_t)lab[pl.uvar[u]] * cols + obs) * F;
        double* ob = kind == 2 ? ob_ed : ob_ee;
        for (int f = 0; f < F; ++f) ob[f] += phi[f];
      }
    }
  }
  d.log_z[g] = Z == 0.0 ? -__builtin_huge_val() : fma((double)emax, 0.693147180559945309417232121458, log(Z));
  for (int f = 0; f < F_ee; ++f) {
    if (d.expect_ee) d.expect_ee[(size_t)g * F_ee + f] = ex_ee[f];
    if (d.grad_ee) d.grad_ee[(size_t)g * F_ee + f] = bad ? nan : ob_ee[f] - ex_ee[f];
  }
  for (int f = 0; f < F_ed; ++f) {
    if (d.expect_ed) d.expect_ed[(size_t)g * F_ed + f] = ex_ed[f];
    if (d.grad_ed) d.grad_ed[(size_t)g * F_ed + f] = bad ? nan : ob_ed[f] - ex_ed[f];
  }
}

// ---- host ----------------------------------------------------------------------------------------
thread_local int g_last_kernel = MLBP_EXACTGRAD_KERNEL_NONE;

int64_t ints_bytes(int64_t P, int64_t U) { return 4 * ((P + U + 16 + 3) / 4 * 4); }
int64_t vector_doubles(int64_t n_vars, int64_t X) { return (5 * n_vars + 2) * ((X + 1) / 2 * 2); }
int64_t x64_lds_bytes(int64_t n_vars, int64_t P, int64_t U, int64_t n_forest) {
  return n_forest * 33280 + 21 * n_vars * 512 + 64 + ints_bytes(P, U);
}
int64_t generic_lds_bytes(int64_t n_vars, int64_t P, int64_t U, int64_t X) { return vector_doubles(n_vars, X) * 8 + 64 + ints_bytes(P, U); }

}  // namespace

extern "C" {

const char* mlbp_exactgrad_arch(void) { return "gfx950"; }
const char* mlbp_exactgrad_last_error(void) { return g_last_error.c_str(); }
int mlbp_exactgrad_last_kernel(void) { return g_last_kernel; }

int mlbp_exactgrad_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest) {
  if (X < 2 || n_vars <= 0 || P < 0 || U < 0 || n_forest < 0 || n_forest > P)
    return fail(MLBP_EINVAL, "pick_kernel: X = %d, n_vars = %d, P = %d, U = %d, n_forest = %d", X, n_vars, P, U, n_forest);
  if (X > MLBP_CUTSET_MAX_X) return fail(MLBP_EUNSUPPORTED, "X = %d: at most %d states are supported", X, MLBP_CUTSET_MAX_X);
  if (X == 64 && n_forest <= MLBP_EXACTGRAD_X64_MAX_FOREST && x64_lds_bytes(n_vars, P, U, n_forest) <= MLBP_CUTSET_X64_LDS_BYTES)
    return MLBP_EXACTGRAD_KERNEL_X64;
  if (64 + ints_bytes(P, U) > MLBP_CUTSET_GENERIC_LDS_BYTES)
    return fail(MLBP_EUNSUPPORTED, "P + U = %lld factors: their exponents do not fit the LDS budget", (long long)P + U);
  return MLBP_EXACTGRAD_KERNEL_GENERIC;
}

int mlbp_exactgrad_chunks(int32_t B, int32_t n_configs, int32_t kernel) {
  if (B <= 0 || n_configs <= 0 || (kernel != MLBP_EXACTGRAD_KERNEL_X64 && kernel != MLBP_EXACTGRAD_KERNEL_GENERIC))
    return fail(MLBP_EINVAL, "chunks: B = %d, n_configs = %d, kernel = %d", B, n_configs, kernel);
  const int32_t walkers = kernel == MLBP_EXACTGRAD_KERNEL_X64 ? (n_configs + 3) / 4 : n_configs;
  const int32_t spread = (MLBP_EXACTGRAD_MIN_WORKGROUPS + B - 1) / B;
  return walkers < spread ? walkers : spread;
}

int64_t mlbp_exactgrad_workspace_bytes(int32_t B, int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t n_cut) {
  const int which = mlbp_exactgrad_pick_kernel(X, n_vars, P, U, n_forest);
  if (which < 0) return which;
  if (n_cut < 0 || n_cut > n_vars) return fail(MLBP_EINVAL, "workspace: n_cut = %d with %d variables", n_cut, n_vars);
  const int64_t n_configs = count_configs(X, n_cut);
  if (n_configs < 0) return too_many_configs(X, n_cut);
  const int chunks = mlbp_exactgrad_chunks(B, (int32_t)n_configs, which);
  if (chunks < 0) return chunks;
  int64_t per = 2 + (int64_t)n_vars * X + (int64_t)P * X * X;
  if (which == MLBP_EXACTGRAD_KERNEL_X64) per *= 4;            // a partial per wave
  else if (generic_lds_bytes(n_vars, P, U, X) > MLBP_CUTSET_GENERIC_LDS_BYTES) per += vector_doubles(n_vars, X);
  return (int64_t)B * chunks * per * 8;
}

int mlbp_exactgrad_check_plan(const int32_t* plan, int32_t n_words, int32_t X) { return check_packed_plan(plan, n_words, X); }

int mlbp_exactgrad_f64(const mlbp_exactgrad_args* a, void* stream) {
  g_last_kernel = MLBP_EXACTGRAD_KERNEL_NONE;
  if (!a) return fail(MLBP_EINVAL, "args is NULL");
  if (a->B <= 0 || a->n_vars <= 0 || a->P < 0 || a->U < 0 || a->P + a->U <= 0 || a->n_cut < 0 || a->n_free < 0 || a->n_items < 0 ||
      a->n_consts < 0 || (int64_t)a->n_cut + a->n_free != a->n_vars)
    return fail(MLBP_EINVAL, "bad sizes: B %d, n_vars %d, P %d, U %d, n_cut %d, n_free %d, n_items %d, n_consts %d", a->B, a->n_vars, a->P,
                a->U, a->n_cut, a->n_free, a->n_items, a->n_consts);
  if (int e = check_states(a->X)) return e;
  const int which = mlbp_exactgrad_pick_kernel(a->X, a->n_vars, a->P, a->U, a->n_forest);
  if (which < 0) return which;
  if (!a->plan || plan_words(a->n_vars, a->P, a->U, a->n_cut, a->n_free, a->n_items, a->n_consts) != a->plan_words)
    return fail(MLBP_EINVAL, "plan is NULL or plan_words = %d disagrees with the sizes", a->plan_words);
  if (int e = check_args_tables(a)) return e;
  if (!a->log_z) return fail(MLBP_EINVAL, "log_z is NULL");
  const bool want_grad = a->grad_ee || a->grad_ed, want_expect = want_grad || a->expect_ee || a->expect_ed;
  if (want_expect) {
    if (!a->phi_en_en || !a->phi_en_en_w1 || !a->phi_en_de || a->F_ee < 1 || a->F_ed < 1 || a->Vde < 1 || (a->P > 0 && !a->pair_phi) ||
        (a->U > 0 && (!a->unary_kind || !a->unary_obs)))
      return fail(MLBP_EINVAL, "expect_* and grad_* need the feature inputs: phi_en_en, phi_en_en_w1, phi_en_de, pair_phi, unary_kind, unary_obs "
                               "and F_ee, F_ed, Vde >= 1 (F_ee %d, F_ed %d, Vde %d)", a->F_ee, a->F_ed, a->Vde);
    if (a->F_ee > MAXF || a->F_ed > MAXF)
      return fail(MLBP_EUNSUPPORTED, "F_ee = %d, F_ed = %d: at most %d features each are supported", a->F_ee, a->F_ed, MAXF);
    if (want_grad && !a->labels) return fail(MLBP_EINVAL, "grad_* needs labels");
  }
  const int64_t n_configs = count_configs(a->X, a->n_cut);
  if (n_configs < 0) return too_many_configs(a->X, a->n_cut);
  const int chunks = mlbp_exactgrad_chunks(a->B, (int32_t)n_configs, which);
  if (chunks < 0) return chunks;
  if ((int64_t)a->n_vars * a->X > 0x7fffffff / 16) return fail(MLBP_EUNSUPPORTED, "n_vars * X = %lld too large", (long long)a->n_vars * a->X);
  const int64_t need = mlbp_exactgrad_workspace_bytes(a->B, a->X, a->n_vars, a->P, a->U, a->n_forest, a->n_cut);
  if (need < 0) return (int)need;
  if (!a->workspace || a->workspace_bytes < need)
    return fail(MLBP_EINVAL, "workspace is NULL or workspace_bytes = %lld below the %lld the call needs", (long long)a->workspace_bytes, (long long)need);
  if (int e = check_device("libmlbp_exactgrad.so")) return e;
  GradDev d;
  d.plan = a->plan;
  d.pair_tables = a->pair_tables; d.pair_tab = a->pair_tab; d.unary_tables = a->unary_tables; d.unary_tab = a->unary_tab;
  d.phi_en_en = a->phi_en_en; d.phi_en_en_w1 = a->phi_en_en_w1; d.phi_en_de = a->phi_en_de;
  d.pair_phi = a->pair_phi; d.unary_kind = a->unary_kind; d.unary_obs = a->unary_obs; d.labels = a->labels;
  d.partials = a->workspace;
  d.vectors = nullptr;
  d.log_z = a->log_z; d.marginals = a->marginals; d.pair_marginals = a->pair_marginals;
  d.expect_ee = a->expect_ee; d.expect_ed = a->expect_ed; d.grad_ee = a->grad_ee; d.grad_ed = a->grad_ed;
  d.stride = 2 + (int64_t)a->n_vars * a->X + (int64_t)a->P * a->X * a->X;
  d.B = a->B; d.X = a->X; d.n_vars = a->n_vars; d.P = a->P; d.U = a->U; d.n_cut = a->n_cut; d.n_free = a->n_free; d.n_items = a->n_items;
  d.n_consts = a->n_consts; d.n_forest = a->n_forest; d.n_pair_tables = a->n_pair_tables; d.n_unary_tables = a->n_unary_tables;
  d.n_configs = (int32_t)n_configs; d.chunks = chunks; d.parts = which == MLBP_EXACTGRAD_KERNEL_X64 ? 4 * chunks : chunks;
  d.F_ee = want_expect ? a->F_ee : 0; d.F_ed = want_expect ? a->F_ed : 0; d.Vde = a->Vde;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(a->B, chunks);
  (void)hipGetLastError();
  if (which == MLBP_EXACTGRAD_KERNEL_X64) {
    const size_t lds = (size_t)x64_lds_bytes(a->n_vars, a->P, a->U, a->n_forest);
    if (a->n_forest <= 1) {                                     // NF = max(n_forest, 1): the register accumulators of the instance
      if (int e = grant_x64_lds((const void*)exactgrad_x64_kernel<1>, 0, MLBP_CUTSET_X64_LDS_BYTES)) return e;
      hipLaunchKernelGGL(exactgrad_x64_kernel<1>, grid, dim3(WG), lds, st, d);
    } else {
      if (int e = grant_x64_lds((const void*)exactgrad_x64_kernel<2>, 1, MLBP_CUTSET_X64_LDS_BYTES)) return e;
      hipLaunchKernelGGL(exactgrad_x64_kernel<2>, grid, dim3(WG), lds, st, d);
    }
  } else {
    int64_t lds = generic_lds_bytes(a->n_vars, a->P, a->U, a->X);
    if (lds > MLBP_CUTSET_GENERIC_LDS_BYTES) {
      d.vectors = a->workspace + (int64_t)a->B * chunks * d.stride;
      lds = 64 + ints_bytes(a->P, a->U);
    }
    hipLaunchKernelGGL(exactgrad_generic_kernel, grid, dim3(WG), (size_t)lds, st, d);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MLBP_EHIP, "exactgrad launch failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(exactgrad_combine_kernel, dim3(a->B), dim3(WG), 0, st, d);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(MLBP_EHIP, "combine launch failed: %s", hipGetErrorString(e));
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
