// libmlbp_exactmap.so: the exact MAP assignment and the max-marginals by cutset conditioning (include/mlbp_exactmap.h),
// gfx950 only, float64.  The max form of libmlbp_cutset.so's walk: max where that one sums, compared as (mantissa, exponent)
// pairs, decoded by back-pointers.
//
// Three kernels; the walk is chosen from (X, n_vars, P, U, n_forest) by mlbp_exactmap_pick_kernel, MM = max-marginals asked for:
//   exactmap_x64_kernel<MM>      X = 64: the forest's tables in LDS, rescaled once, rows padded to 65 entries; every WAVE walks
//                                configurations of its own (lane = state); a contraction is 64 multiplies and 64 fmax per lane
//                                against the LDS table with the vector's entries broadcast by v_readlane; every reduction is
//                                DPP -- no workgroup barrier inside the walk.  A wave writes its own partial.
//   exactmap_generic_kernel<MM>  any X in [2, 1024]: the whole workgroup walks one configuration at a time; tables streamed with
//                                masked tails and rescaled as they are read; the vectors in LDS when they fit, else in the
//                                caller's workspace.
//   exactmap_final_kernel        one workgroup per graph: the best partial (ties: the lowest c), that configuration solved once
//                                more with the tables streamed, the states by back-pointers, the logarithms.
// Without MM a walk is the pass from the leaves to the roots alone.  Every scalar a workgroup or wave branches on comes out of a
// reduction and has the same bits in every thread of it.  No sum is formed: a result does not depend on the launch at all.
// No device-side mutable globals: everything comes through ExactDev.
#include <hip/hip_runtime.h>

#include "../../include/mlbp_exactmap.h"
#define MLBP_GRAPH_NO_SWEEPS                // this library runs no sweep program
#include "../csrc/mlbp_graph_device.h"
#include "../csrc/mlbp_graph_host.h"
#include "../csrc/mlbp_cutset_plan.h"

namespace {

using namespace mlbp_graph;

constexpr int PART = MLBP_EXACTMAP_PARTIAL_HEADER;
constexpr double LN2 = 0.693147180559945309417232121458;

struct ExactDev {
  const int32_t* plan;
  const double* pair_tables; const int32_t* pair_tab;
  const double* unary_tables; const int32_t* unary_tab;
  double* partials;                          // [B][parts][per], per = PART (+ n_vars * X with max-marginals)
  double* fvec;                              // the final kernel's vectors: [B][2 n_vars + 1][round_up(X, 2)]
  double* vectors;                           // generic kernel, vectors not in LDS: [B][chunks][5 n_vars + 2][round_up(X, 2)]
  int32_t* assignment; double* score; double* max_marginals;
  int32_t B, X, n_vars, P, U, n_cut, n_free, n_items, n_consts, n_forest, n_pair_tables, n_unary_tables, n_configs, chunks, parts, per;
};

// The best configuration so far: V = m * 2^e at configuration c; c < 0: nothing yet; m = 0: V is zero (or no number).
struct Best { double m; int e; int c; };

// Does V = (m, e) at a HIGHER configuration index beat `b`?  Only by being larger: ties stay with the lower index.
__device__ __forceinline__ void offer(Best& b, Scaled z, int c) {
  const bool pos = z.m > 0.0;
  if (b.c < 0 || (pos && (!(b.m > 0.0) || z.e > b.e || (z.e == b.e && z.m > b.m)))) {
    b.m = pos ? z.m : 0.0;
    b.e = z.e;
    b.c = c;
  }
}

// A max-marginal accumulator entry: v * 2^shift (shift <= 0), dropped below 2^-MLBP_EXACTMAP_DROP_BELOW of the reference.
__device__ __forceinline__ double shifted(double v, int shift) {
  const double y = ldexp(v, max(shift, MIN_SHIFT));
  return y < 0x1p-1000 ? 0.0 : y;
}
static_assert(MLBP_EXACTMAP_DROP_BELOW == 1000, "shifted() states the limit as a literal");

// ---- contractions, max form: out[i] = max_j T[i][j] m[j] (tm) or out[j] = max_i m[i] T[i][j]; a barrier behind the result --
__device__ __forceinline__ void maxcontract_stream(const double* T, int X, int te, bool tm, const double* m, double* out) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (tm) {
    for (int row = wave; row < X; row += WG / 64) {
      const double* Tr = T + (size_t)row * X;
      double acc = 0.0;
      for (int j = lane; j < X; j += 64) acc = fmax(acc, ldexp(Tr[j], -te) * m[j]);
      acc = wave_max(acc);
      if (lane == 0) out[row] = acc;
    }
  } else {
    for (int j = t; j < X; j += WG) {
      double acc = 0.0;
#pragma unroll 4
      for (int i = 0; i < X; ++i) acc = fmax(acc, m[i] * ldexp(T[(size_t)i * X + j], -te));
      out[j] = acc;
    }
  }
  __syncthreads();
}

// The lowest of the workgroup's indices (0xffffffff: none), the same in every thread; two barriers.  Uses scratch[4 .. 6).
__device__ __forceinline__ unsigned block_min_index(unsigned idx, double* scratch) {
  unsigned* s = reinterpret_cast<unsigned*>(scratch + 4);
  const unsigned k = wave_max_u32(~idx);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = k;
  __syncthreads();
  return ~max(max(s[0], s[1]), max(s[2], s[3]));
}

// Every factor's table exponent into texp[P + U]: a pairwise table by the whole workgroup (two barriers each), the unary rows a
// wave each without a barrier -- a maximum does not depend on the order it is taken in.  Ends behind a barrier.
__device__ __forceinline__ void table_exponents(const double* pair_tables, const_i32p ptab, int P, const double* unary_tables,
                                                const_i32p utab, int U, int X, double* scratch, int* texp) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t XX = (size_t)X * X;
  for (int p = 0; p < P; ++p) {
    const double* T = pair_tables + (size_t)ptab[p] * XX;
    double m = 0.0;
    for (size_t i = t; i < XX; i += WG) m = fmax(m, T[i]);
    m = block_max(m, scratch);
    if (t == 0) texp[p] = exp_of(m);
  }
  for (int u = wave; u < U; u += WG / 64) {
    const double* row = unary_tables + (size_t)utab[u] * X;
    double m = 0.0;
    for (int j = lane; j < X; j += 64) m = fmax(m, row[j]);
    m = wave_max(m);
    if (lane == 0) texp[P + u] = exp_of(m);
  }
  __syncthreads();
}

// ---- any X: what the generic walk and the final kernel share -----------------------------------------------------
struct Generic {
  const double* pair_tables; const double* unary_tables;
  PlanSections<const_i32p> pl;
  const_i32p ptab, utab;
  int X, Xp, P, U, n_free, n_cut, n_consts;
  size_t XX;
  double* base;                              // [n_vars][Xp] the product of a free variable's unary rows
  double* bel;                               // [n_vars][Xp] a free variable's vector on the way up
  double* raw;                               // [Xp]
  double* scratch;                           // [8]
  int* texp;                                 // [P + U] exponent of every factor's table
  int* st;                                   // [16] states of the configuration
  int e_fixed;
};

__device__ __forceinline__ void generic_open(Generic& G, const ExactDev& d, int g) {
  G.pair_tables = d.pair_tables; G.unary_tables = d.unary_tables;
  carve_plan(as_const(d.plan), d.n_vars, d.P, d.U, d.n_cut, d.n_free, d.n_items, d.n_consts, G.pl);
  G.ptab = as_const(d.pair_tab) + (size_t)g * d.P;
  G.utab = as_const(d.unary_tab) + (size_t)g * d.U;
  G.X = d.X; G.Xp = (d.X + 1) & ~1; G.P = d.P; G.U = d.U; G.n_free = d.n_free; G.n_cut = d.n_cut; G.n_consts = d.n_consts;
  G.XX = (size_t)d.X * d.X;
}

// Every table's exponent and every free variable's base vector; ends behind a barrier.
__device__ __forceinline__ void generic_setup(Generic& G) {
  const int t = threadIdx.x, X = G.X, P = G.P, U = G.U;
  table_exponents(G.pair_tables, G.ptab, P, G.unary_tables, G.utab, U, X, G.scratch, G.texp);
  int e_fixed = 0;                                             // every factor enters every configuration once
  for (int f = 0; f < P + U; ++f) e_fixed += G.texp[f];
  for (int i = 0; i < G.n_free; ++i) {
    const int v = G.pl.order[i];
    for (int j = t; j < X; j += WG) {
      double b = 1.0;
      for (int it = G.pl.item_off[v]; it < G.pl.item_off[v + 1]; ++it)
        if (G.pl.items[3 * it] == MLBP_CUTSET_ITEM_UNARY) {
          const int u = G.pl.items[3 * it + 1];
          b *= ldexp(G.unary_tables[(size_t)G.utab[u] * X + j], -G.texp[P + u]);
        }
      G.base[(size_t)v * G.Xp + j] = b;
    }
    __syncthreads();
    e_fixed += rescale(G.base + (size_t)v * G.Xp, X, G.scratch);
  }
  G.e_fixed = e_fixed;
}

// the free variable's configuration-free part times its cutset-incident rows and columns, at state j
__device__ __forceinline__ double generic_local(const Generic& G, int v, int j) {
  double b = G.base[(size_t)v * G.Xp + j];
  for (int it = G.pl.item_off[v]; it < G.pl.item_off[v + 1]; ++it) {
    const int kind = G.pl.items[3 * it];
    if (kind == MLBP_CUTSET_ITEM_UNARY) continue;
    const int p = G.pl.items[3 * it + 1], s = G.st[G.pl.items[3 * it + 2]];
    const double* T = G.pair_tables + (size_t)G.ptab[p] * G.XX;
    b *= ldexp(kind == MLBP_CUTSET_ITEM_COL ? T[(size_t)j * G.X + s] : T[(size_t)s * G.X + j], -G.texp[p]);
  }
  return b;
}

// Configuration c, leaves to roots: returns V_c; bel[v] is left holding every free variable's rescaled upward vector, up
// (unless NULL) its rescaled message to its parent.  Reached by every thread; ends behind a barrier.
__device__ __forceinline__ Scaled generic_up(const Generic& G, int c, double* up) {
  const int t = threadIdx.x, X = G.X, Xp = G.Xp;
  __syncthreads();
  if (t < G.n_cut) {
    int r = c;
    for (int q = 0; q < t; ++q) r /= X;
    G.st[t] = r % X;
  }
  __syncthreads();
  Scaled z = {1.0, G.e_fixed};
  for (int i = 0; i < G.n_consts; ++i) {
    const int f = G.pl.consts[4 * i + 1], s0 = G.st[G.pl.consts[4 * i + 2]];
    if (G.pl.consts[4 * i] == MLBP_CUTSET_CONST_UNARY) {
      mul(z, ldexp(G.unary_tables[(size_t)G.utab[f] * X + s0], -G.texp[G.P + f]));
    } else {
      const int s1 = G.st[G.pl.consts[4 * i + 3]];
      mul(z, ldexp(G.pair_tables[(size_t)G.ptab[f] * G.XX + (size_t)s0 * X + s1], -G.texp[f]));
    }
  }
  for (int i = 0; i < G.n_free; ++i) {
    const int v = G.pl.order[i];
    for (int j = t; j < X; j += WG) G.bel[(size_t)v * Xp + j] = generic_local(G, v, j);
  }
  __syncthreads();
  for (int i = 0; i < G.n_free; ++i) {
    const int v = G.pl.order[i], p = G.pl.parent[2 * v];
    double* bv = G.bel + (size_t)v * Xp;
    z.e += rescale(bv, X, G.scratch);
    if (p < 0) {
      double m = 0.0;
      for (int j = t; j < X; j += WG) m = fmax(m, bv[j]);
      mul(z, block_max(m, G.scratch));
    } else {
      const int par = G.pl.parent[2 * v + 1];
      maxcontract_stream(G.pair_tables + (size_t)G.ptab[p] * G.XX, X, G.texp[p], G.pl.pav[2 * p] != v, bv, G.raw);
      z.e += rescale(G.raw, X, G.scratch);
      for (int j = t; j < X; j += WG) {
        if (up) up[(size_t)v * Xp + j] = G.raw[j];
        G.bel[(size_t)par * Xp + j] *= G.raw[j];
      }
      __syncthreads();
    }
  }
  return z;
}

// ---- any X: the workgroup walks a chunk's configurations ---------------------------------------------------
template <bool MM>
__global__ __launch_bounds__(WG) void exactmap_generic_kernel(ExactDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X, Xp = (X + 1) & ~1;
  const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  const int n_vars = d.n_vars, n_free = d.n_free, n_cut = d.n_cut;
  Generic G;
  generic_open(G, d, g);

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
  G.scratch = lds;
  lds += 8;
  G.texp = reinterpret_cast<int*>(lds);
  G.st = G.texp + d.P + d.U;
  const size_t vs = (size_t)n_vars * Xp;
  double* acc = vec;                                           // [n_vars][Xp] max over configurations, mantissas against ref
  G.base = acc + vs;
  G.bel = G.base + vs;
  double* up = G.bel + vs;                                     // a free variable's message to its parent
  double* dn = up + vs;                                        // its parent's message to it
  G.raw = dn + vs;
  double* excl = G.raw + Xp;

  generic_setup(G);
  if (MM)
    for (size_t i = t; i < vs; i += WG) acc[i] = 0.0;

  Best best = {0.0, EMPTY, -1};
  int ref = EMPTY;                                             // the largest exponent of a positive V_c so far
  for (int c = k; c < d.n_configs; c += d.chunks) {
    const Scaled z = generic_up(G, c, MM ? up : nullptr);
    offer(best, z, c);
    if (!MM) continue;
    if (!(z.m > 0.0)) continue;                                // V_c = 0: nothing to record

    if (z.e > ref) {
      const int shift = ref - z.e;
      for (size_t i = t; i < vs; i += WG) acc[i] = shifted(acc[i], shift);
      ref = z.e;
      __syncthreads();
    }
    const int shift = z.e - ref;
    if (t < n_cut) {
      double* a = acc + (size_t)G.pl.cutset[t] * Xp + G.st[t];
      *a = fmax(*a, shifted(z.m, shift));
    }
    // roots to leaves
    for (int i = n_free - 1; i >= 0; --i) {
      const int v = G.pl.order[i], p = G.pl.parent[2 * v];
      double* bv = G.bel + (size_t)v * Xp;
      if (p >= 0) {
        const int par = G.pl.parent[2 * v + 1];
        const bool par_has_parent = G.pl.parent[2 * par] >= 0;
        for (int j = t; j < X; j += WG) {
          double b = generic_local(G, par, j);
          if (par_has_parent) b *= dn[(size_t)par * Xp + j];
          excl[j] = b;
        }
        for (int q = 0; q < n_free; ++q) {                     // the parent's other children
          const int sib = G.pl.order[q];
          if (sib == v || G.pl.parent[2 * sib + 1] != par) continue;
          for (int j = t; j < X; j += WG) excl[j] *= up[(size_t)sib * Xp + j];
        }
        __syncthreads();
        rescale(excl, X, G.scratch);
        maxcontract_stream(G.pair_tables + (size_t)G.ptab[p] * G.XX, X, G.texp[p], G.pl.pav[2 * p] == v, excl, G.raw);
        rescale(G.raw, X, G.scratch);
        for (int j = t; j < X; j += WG) {
          dn[(size_t)v * Xp + j] = G.raw[j];
          bv[j] *= G.raw[j];
        }
      }
      double m = 0.0;
      for (int j = t; j < X; j += WG) m = fmax(m, bv[j]);
      m = block_max(m, G.scratch);
      for (int j = t; j < X; j += WG) {
        double* a = acc + (size_t)v * Xp + j;
        *a = fmax(*a, shifted(z.m * (bv[j] / m), shift));
      }
      __syncthreads();
    }
  }

  __syncthreads();
  double* out = d.partials + ((size_t)g * d.parts + k) * d.per;
  if (t == 0) {
    out[0] = best.m;
    out[1] = (double)best.e;
    out[2] = (double)best.c;
    out[3] = (double)ref;
  }
  if (MM)
    for (int v = 0; v < n_vars; ++v)
      for (int j = t; j < X; j += WG) out[PART + (size_t)v * X + j] = acc[(size_t)v * Xp + j];
}

// ---- X = 64: a wave per configuration ---------------------------------------------------------------------
constexpr int ROW = 65;                     // padded row of an LDS table

// The max-contraction of the padded LDS table with the wave's vector (m: the entry of this lane): lane i returns
// max_j T[i][j] m[j] (tm) or max_i m[i] T[i][lane].  Four chains of 16 multiplies and fmax, joined pairwise.
__device__ __forceinline__ double wave_maxcontract_x64(const double* table, bool tm, double m, int lane) {
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  if (tm) {
    const double* row = table + lane * ROW;
#pragma unroll
    for (int j = 0; j < 64; ++j) a[j & 3] = fmax(a[j & 3], row[j] * read_lane(m, j));
  } else {
    const double* col = table + lane;
#pragma unroll
    for (int i = 0; i < 64; ++i) a[i & 3] = fmax(a[i & 3], read_lane(m, i) * col[i * ROW]);
  }
  return fmax(fmax(a[0], a[1]), fmax(a[2], a[3]));
}

template <bool MM>
__global__ __launch_bounds__(WG) void exactmap_x64_kernel(ExactDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int X = 64;
  const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  PlanSections<const_i32p> pl;
  carve_plan(as_const(d.plan), d.n_vars, d.P, d.U, d.n_cut, d.n_free, d.n_items, d.n_consts, pl);
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const int n_vars = d.n_vars, P = d.P, U = d.U, n_free = d.n_free, n_cut = d.n_cut;

  // LDS: [forest tables, rows of 65] [base] [4 waves x (acc, phi, bel, up, dn)] [scratch] [table exponents]; without MM a wave
  // uses its bel alone
  double* tabs = reinterpret_cast<double*>(smem);
  double* base = tabs + (size_t)d.n_forest * 64 * ROW;         // [n_vars][64] the product of a variable's unary rows
  const size_t vs = (size_t)n_vars * 64;
  double* acc = base + vs + (size_t)wave * 5 * vs;             // this wave's: max over its configurations, mantissas against ref
  double* phi = acc + vs;                                      // a free variable's own factors under the configuration
  double* bel = phi + vs;                                      // its vector on the way up
  double* up = bel + vs;                                       // its message to its parent
  double* dn = up + vs;                                        // its parent's message to it
  double* scratch = base + vs + 20 * vs;
  int* texp = reinterpret_cast<int*>(scratch + 8);

  table_exponents(d.pair_tables, ptab, P, d.unary_tables, utab, U, X, scratch, texp);
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
  if (MM)
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

  Best best = {0.0, EMPTY, -1};
  int ref = EMPTY;                                             // the largest exponent of a positive V_c so far
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
      const double b = local(v, c);
      bel[(size_t)v * 64 + lane] = b;
      if (MM) phi[(size_t)v * 64 + lane] = b;
    }
    // leaves to roots
    for (int i = 0; i < n_free; ++i) {
      const int v = pl.order[i], p = pl.parent[2 * v];
      const double x = wave_rescale(bel[(size_t)v * 64 + lane], z.e);
      if (MM) bel[(size_t)v * 64 + lane] = x;
      if (p < 0) {
        mul(z, wave_max(fmax(x, 0.0)));
      } else {
        const int par = pl.parent[2 * v + 1];
        const double r = wave_rescale(wave_maxcontract_x64(tabs + (size_t)pl.fslot[p] * 64 * ROW, pl.pav[2 * p] != v, x, lane), z.e);
        if (MM) up[(size_t)v * 64 + lane] = r;
        bel[(size_t)par * 64 + lane] *= r;
      }
    }
    offer(best, z, c);
    if (!MM) continue;
    if (!(z.m > 0.0)) continue;                                // V_c = 0: nothing to record

    if (z.e > ref) {
      const int shift = ref - z.e;
      for (int v = 0; v < n_vars; ++v) acc[(size_t)v * 64 + lane] = shifted(acc[(size_t)v * 64 + lane], shift);
      ref = z.e;
    }
    const int shift = z.e - ref;
    const double w = shifted(z.m, shift);
    for (int q = 0; q < n_cut; ++q)
      if (lane == state(q, c)) acc[(size_t)pl.cutset[q] * 64 + lane] = fmax(acc[(size_t)pl.cutset[q] * 64 + lane], w);

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
        const double r = wave_rescale(wave_maxcontract_x64(tabs + (size_t)pl.fslot[p] * 64 * ROW, pl.pav[2 * p] == v, b, lane), unused);
        dn[(size_t)v * 64 + lane] = r;
        x *= r;
      }
      const double top = wave_max(fmax(x, 0.0));
      acc[(size_t)v * 64 + lane] = fmax(acc[(size_t)v * 64 + lane], shifted(z.m * (x / top), shift));
    }
  }

  double* out = d.partials + ((size_t)g * d.parts + 4 * k + wave) * d.per;
  if (lane == 0) {
    out[0] = best.m;
    out[1] = (double)best.e;
    out[2] = (double)best.c;
    out[3] = (double)ref;
  }
  if (MM)
    for (int v = 0; v < n_vars; ++v) out[PART + (size_t)v * 64 + lane] = acc[(size_t)v * 64 + lane];
}

// ---- the partials of a graph's chunks -> its outputs ----------------------------------------------------
__global__ __launch_bounds__(WG) void exactmap_final_kernel(ExactDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int X = d.X, n_vars = d.n_vars;
  int32_t* xs = d.assignment + (size_t)g * n_vars;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) {
    for (int v = t; v < n_vars; v += WG) xs[v] = -1;
    if (t == 0) d.score[g] = __builtin_nan("");
    return;
  }
  const double* ws = d.partials + (size_t)g * d.parts * d.per;

  // the best partial: the larger V, then the lower configuration index
  Best best = {0.0, EMPTY, -1};
  int ref = EMPTY;
  for (int k = 0; k < d.parts; ++k) {
    const double* w = ws + (size_t)k * d.per;
    const double m = w[0];
    const int e = (int)w[1], c = (int)w[2];
    ref = max(ref, (int)w[3]);
    if (c < 0) continue;                                       // a wave without a configuration
    bool take;
    if (best.c < 0) take = true;
    else if ((m > 0.0) != (best.m > 0.0)) take = m > 0.0;
    else if (m > 0.0 && e != best.e) take = e > best.e;
    else if (m > 0.0 && m != best.m) take = m > best.m;
    else take = c < best.c;
    if (take) best = {m, e, c};
  }

  // that configuration once more, leaves to roots; then the states, roots to leaves
  Generic G;
  generic_open(G, d, g);
  double* lds = reinterpret_cast<double*>(smem);
  G.scratch = lds;
  G.texp = reinterpret_cast<int*>(lds + 8);
  G.st = G.texp + d.P + d.U;
  const int Xp = G.Xp;
  G.base = d.fvec + (size_t)g * (2 * n_vars + 1) * Xp;
  G.bel = G.base + (size_t)n_vars * Xp;
  G.raw = G.bel + (size_t)n_vars * Xp;
  const bool positive = best.m > 0.0;                          // else every assignment has potential zero: all of them tie
  if (positive) {
    generic_setup(G);
    generic_up(G, best.c, nullptr);
    if (t < d.n_cut) xs[G.pl.cutset[t]] = G.st[t];
  } else {
    for (int v = t; v < n_vars; v += WG) xs[v] = 0;
  }
  __syncthreads();
  for (int i = positive ? d.n_free - 1 : -1; i >= 0; --i) {
    const int v = G.pl.order[i], p = G.pl.parent[2 * v];
    const double* bv = G.bel + (size_t)v * Xp;
    if (p < 0) {
      for (int j = t; j < X; j += WG) G.raw[j] = bv[j];
    } else {
      const int s = xs[G.pl.parent[2 * v + 1]];                // the parent's state: written above, behind a barrier
      const double* T = G.pair_tables + (size_t)G.ptab[p] * G.XX;
      const int te = G.texp[p];
      if (G.pl.pav[2 * p] != v)
        for (int j = t; j < X; j += WG) G.raw[j] = ldexp(T[(size_t)s * X + j], -te) * bv[j];
      else
        for (int j = t; j < X; j += WG) G.raw[j] = bv[j] * ldexp(T[(size_t)j * X + s], -te);
    }
    double m = 0.0;
    for (int j = t; j < X; j += WG) m = fmax(m, G.raw[j]);
    m = block_max(m, G.scratch);
    unsigned idx = 0xffffffffu;
    for (int j = t; j < X; j += WG)
      if (G.raw[j] == m) { idx = (unsigned)j; break; }
    idx = block_min_index(idx, G.scratch);
    if (t == 0) xs[v] = idx < (unsigned)X ? (int)idx : 0;
    __syncthreads();
  }

  // max-marginals: the partials against the graph's reference exponent
  if (d.max_marginals) {
    const size_t N = (size_t)n_vars * X;
    double* mm = d.max_marginals + (size_t)g * N;
    for (size_t i = t; i < N; i += WG) {
      double a = 0.0;
      for (int k = 0; k < d.parts; ++k) {
        const double* w = ws + (size_t)k * d.per;
        a = fmax(a, shifted(w[PART + i], (int)w[3] - ref));
      }
      mm[i] = a > 0.0 ? fma((double)ref, LN2, log(a)) : -__builtin_huge_val();
    }
  }
  if (wave != 0) return;
  double sc = 0.0;
  for (int p = lane; p < d.P; p += 64) {
    const int i = xs[G.pl.pav[2 * p]], j = xs[G.pl.pav[2 * p + 1]];
    sc += log(d.pair_tables[(size_t)G.ptab[p] * G.XX + (size_t)i * X + j]);
  }
  for (int u = lane; u < d.U; u += 64) sc += log(d.unary_tables[(size_t)G.utab[u] * X + xs[G.pl.uvar[u]]]);
  sc = wave_sum(sc);
  if (lane == 0) d.score[g] = sc;
}

// ---- host ----------------------------------------------------------------------------------------
thread_local int g_last_kernel = MLBP_EXACTMAP_KERNEL_NONE;

int64_t ints_bytes(int64_t P, int64_t U) { return 4 * ((P + U + 16 + 3) / 4 * 4); }
int64_t vector_doubles(int64_t n_vars, int64_t X) { return (5 * n_vars + 2) * ((X + 1) / 2 * 2); }
int64_t x64_lds_bytes(int64_t n_vars, int64_t P, int64_t U, int64_t n_forest) {
  return n_forest * 33280 + 21 * n_vars * 512 + 64 + ints_bytes(P, U);
}
int64_t generic_lds_bytes(int64_t n_vars, int64_t P, int64_t U, int64_t X) { return vector_doubles(n_vars, X) * 8 + 64 + ints_bytes(P, U); }

}  // namespace

extern "C" {

const char* mlbp_exactmap_arch(void) { return "gfx950"; }
const char* mlbp_exactmap_last_error(void) { return g_last_error.c_str(); }
int mlbp_exactmap_last_kernel(void) { return g_last_kernel; }

int mlbp_exactmap_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest) {
  if (X < 2 || n_vars <= 0 || P < 0 || U < 0 || n_forest < 0 || n_forest > P)
    return fail(MLBP_EINVAL, "pick_kernel: X = %d, n_vars = %d, P = %d, U = %d, n_forest = %d", X, n_vars, P, U, n_forest);
  if (X > MLBP_CUTSET_MAX_X) return fail(MLBP_EUNSUPPORTED, "X = %d: at most %d states are supported", X, MLBP_CUTSET_MAX_X);
  if (X == 64 && x64_lds_bytes(n_vars, P, U, n_forest) <= MLBP_CUTSET_X64_LDS_BYTES) return MLBP_EXACTMAP_KERNEL_X64;
  if (64 + ints_bytes(P, U) > MLBP_CUTSET_GENERIC_LDS_BYTES)
    return fail(MLBP_EUNSUPPORTED, "P + U = %lld factors: their exponents do not fit the LDS budget", (long long)P + U);
  return MLBP_EXACTMAP_KERNEL_GENERIC;
}

int mlbp_exactmap_chunks(int32_t B, int32_t n_configs) {
  if (B <= 0 || n_configs <= 0) return fail(MLBP_EINVAL, "chunks: B = %d, n_configs = %d", B, n_configs);
  const int32_t spread = (MLBP_CUTSET_MIN_WORKGROUPS + B - 1) / B;
  return n_configs < spread ? n_configs : spread;
}

int64_t mlbp_exactmap_workspace_bytes(int32_t B, int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t n_cut,
                                      int32_t max_marginals) {
  const int which = mlbp_exactmap_pick_kernel(X, n_vars, P, U, n_forest);
  if (which < 0) return which;
  if (n_cut < 0 || n_cut > n_vars) return fail(MLBP_EINVAL, "workspace: n_cut = %d with %d variables", n_cut, n_vars);
  const int64_t n_configs = count_configs(X, n_cut);
  if (n_configs < 0) return too_many_configs(X, n_cut);
  const int chunks = mlbp_exactmap_chunks(B, (int32_t)n_configs);
  if (chunks < 0) return chunks;
  const int64_t Xp = (X + 1) / 2 * 2;
  int64_t per = PART + (max_marginals ? (int64_t)n_vars * X : 0);
  if (which == MLBP_EXACTMAP_KERNEL_X64) per *= 4;             // a partial per wave
  else if (generic_lds_bytes(n_vars, P, U, X) > MLBP_CUTSET_GENERIC_LDS_BYTES) per += vector_doubles(n_vars, X);
  return ((int64_t)B * chunks * per + (int64_t)B * (2 * (int64_t)n_vars + 1) * Xp) * 8;
}

int mlbp_exactmap_check_plan(const int32_t* plan, int32_t n_words, int32_t X) { return check_packed_plan(plan, n_words, X); }

int mlbp_exactmap_f64(const mlbp_exactmap_args* a, void* stream) {
  g_last_kernel = MLBP_EXACTMAP_KERNEL_NONE;
  if (!a) return fail(MLBP_EINVAL, "args is NULL");
  if (a->B <= 0 || a->n_vars <= 0 || a->P < 0 || a->U < 0 || a->P + a->U <= 0 || a->n_cut < 0 || a->n_free < 0 || a->n_items < 0 ||
      a->n_consts < 0 || (int64_t)a->n_cut + a->n_free != a->n_vars)
    return fail(MLBP_EINVAL, "bad sizes: B %d, n_vars %d, P %d, U %d, n_cut %d, n_free %d, n_items %d, n_consts %d", a->B, a->n_vars, a->P,
                a->U, a->n_cut, a->n_free, a->n_items, a->n_consts);
  if (int e = check_states(a->X)) return e;
  const int which = mlbp_exactmap_pick_kernel(a->X, a->n_vars, a->P, a->U, a->n_forest);
  if (which < 0) return which;
  if (!a->plan || plan_words(a->n_vars, a->P, a->U, a->n_cut, a->n_free, a->n_items, a->n_consts) != a->plan_words)
    return fail(MLBP_EINVAL, "plan is NULL or plan_words = %d disagrees with the sizes", a->plan_words);
  if (int e = check_args_tables(a)) return e;
  if (!a->assignment || !a->score) return fail(MLBP_EINVAL, "assignment or score is NULL");
  const int64_t n_configs = count_configs(a->X, a->n_cut);
  if (n_configs < 0) return too_many_configs(a->X, a->n_cut);
  const int chunks = mlbp_exactmap_chunks(a->B, (int32_t)n_configs);
  if (chunks < 0) return chunks;
  if ((int64_t)a->n_vars * a->X > 0x7fffffff / 16) return fail(MLBP_EUNSUPPORTED, "n_vars * X = %lld too large", (long long)a->n_vars * a->X);
  const bool mm = a->max_marginals != nullptr;
  const int64_t need = mlbp_exactmap_workspace_bytes(a->B, a->X, a->n_vars, a->P, a->U, a->n_forest, a->n_cut, mm);
  if (need < 0) return (int)need;
  if (!a->workspace || a->workspace_bytes < need)
    return fail(MLBP_EINVAL, "workspace is NULL or workspace_bytes = %lld below the %lld the call needs", (long long)a->workspace_bytes, (long long)need);
  if (int e = check_device("libmlbp_exactmap.so")) return e;
  const int64_t Xp = (a->X + 1) / 2 * 2;
  ExactDev d;
  d.plan = a->plan;
  d.pair_tables = a->pair_tables; d.pair_tab = a->pair_tab; d.unary_tables = a->unary_tables; d.unary_tab = a->unary_tab;
  d.assignment = a->assignment; d.score = a->score; d.max_marginals = a->max_marginals;
  d.B = a->B; d.X = a->X; d.n_vars = a->n_vars; d.P = a->P; d.U = a->U; d.n_cut = a->n_cut; d.n_free = a->n_free; d.n_items = a->n_items;
  d.n_consts = a->n_consts; d.n_forest = a->n_forest; d.n_pair_tables = a->n_pair_tables; d.n_unary_tables = a->n_unary_tables;
  d.n_configs = (int32_t)n_configs; d.chunks = chunks; d.parts = which == MLBP_EXACTMAP_KERNEL_X64 ? 4 * chunks : chunks;
  d.per = PART + (mm ? a->n_vars * a->X : 0);
  d.partials = a->workspace;
  d.fvec = d.partials + (int64_t)a->B * d.parts * d.per;
  d.vectors = nullptr;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(a->B, chunks);
  (void)hipGetLastError();
  if (which == MLBP_EXACTMAP_KERNEL_X64) {
    const size_t lds = (size_t)x64_lds_bytes(a->n_vars, a->P, a->U, a->n_forest);
    if (mm) {
      if (int e = grant_x64_lds((const void*)exactmap_x64_kernel<true>, 1, MLBP_CUTSET_X64_LDS_BYTES)) return e;
      hipLaunchKernelGGL(exactmap_x64_kernel<true>, grid, dim3(WG), lds, st, d);
    } else {
      if (int e = grant_x64_lds((const void*)exactmap_x64_kernel<false>, 0, MLBP_CUTSET_X64_LDS_BYTES)) return e;
      hipLaunchKernelGGL(exactmap_x64_kernel<false>, grid, dim3(WG), lds, st, d);
    }
  } else {
    int64_t lds = generic_lds_bytes(a->n_vars, a->P, a->U, a->X);
    if (lds > MLBP_CUTSET_GENERIC_LDS_BYTES) {
      d.vectors = d.fvec + (int64_t)a->B * (2 * (int64_t)a->n_vars + 1) * Xp;
      lds = 64 + ints_bytes(a->P, a->U);
    }
    if (mm) hipLaunchKernelGGL(exactmap_generic_kernel<true>, grid, dim3(WG), (size_t)lds, st, d);
    else hipLaunchKernelGGL(exactmap_generic_kernel<false>, grid, dim3(WG), (size_t)lds, st, d);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MLBP_EHIP, "exactmap launch failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(exactmap_final_kernel, dim3(a->B), dim3(WG), (size_t)(64 + ints_bytes(a->P, a->U)), st, d);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(MLBP_EHIP, "final launch failed: %s", hipGetErrorString(e));
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
