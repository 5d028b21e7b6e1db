// The walk over cutset configurations that libmlbp_cutset.so, libmlbp_exactmap.so, libmlbp_exactgrad.so and their later
// siblings share (gfx950 only, float64; libmlbp_cutsetis.so walks a caller's list with it, see "where a configuration's states
// come from"): for one configuration of the cutset variables, the pass from the leaves of the remaining forest to its roots
// -- which yields Z_c, or V_c in the max form -- and the pass back, which yields every free variable's belief.  Stated once,
// over an algebra (SumAlg, MaxAlg), in the two forms the libraries run: the generic walker (any X, the workgroup one
// configuration at a time, tables streamed) and the X = 64 walker (tables in LDS, a wave per configuration, lane = state).
// What a library does with Z_c and the beliefs -- its accumulators, its partial, its read-out -- stays in its own kernels: the
// generic pass back takes it as two hooks, the X = 64 pass back is a step the kernel's own loop calls.  Helpers only, no kernel.
// Not part of the ABI.
// Include after mlbp_cutset_plan.h.
#ifndef MLBP_CUTSET_WALK_H
#define MLBP_CUTSET_WALK_H

namespace mlbp_graph {

// ---- the algebra: what differs between the sum form and the max form of a walk --------------------------------------
//   mad      a step of a streamed contraction, written as the sum form always was: the compiler contracts it as before
//   fmad     a step of the X = 64 contraction: one fused multiply-add; in the max form the product is rounded, then compared
//   join     two partial results
//   wave     the wave's result of a streamed row;  root: a root's vector -> its factor of Z_c / V_c and of the belief's scale
//   block    the workgroup's result, the same bits in every thread; two barriers, reached by all
//   dead     Z_c / V_c adds nothing: the configuration is passed over
struct SumAlg {
  static __device__ __forceinline__ double mad(double acc, double a, double b) { return acc + a * b; }
  static __device__ __forceinline__ double fmad(double acc, double a, double b) { return fma(a, b, acc); }
  static __device__ __forceinline__ double join(double a, double b) { return a + b; }
  static __device__ __forceinline__ double wave(double x) { return wave_sum(x); }
  static __device__ __forceinline__ double root(double x) { return wave_sum(x); }
  static __device__ __forceinline__ double block(double v, double* scratch) { return block_sum(v, scratch); }
  static __device__ __forceinline__ bool dead(const Scaled& z) { return z.m == 0.0; }
};
struct MaxAlg {
  static __device__ __forceinline__ double mad(double acc, double a, double b) { return fmax(acc, a * b); }
  static __device__ __forceinline__ double fmad(double acc, double a, double b) { return fmax(acc, a * b); }
  static __device__ __forceinline__ double join(double a, double b) { return fmax(a, b); }
  static __device__ __forceinline__ double wave(double x) { return wave_max(x); }
  static __device__ __forceinline__ double root(double x) { return wave_max(fmax(x, 0.0)); }
  static __device__ __forceinline__ double block(double v, double* scratch) { return block_max(v, scratch); }
  static __device__ __forceinline__ bool dead(const Scaled& z) { return !(z.m > 0.0); }
};

// The edge hook of a library that keeps nothing per forest factor.
struct NoEdge {
  template <class... A>
  __device__ __forceinline__ void operator()(A...) const {}
};

// Streamed contraction with the table rescaled as it is read: out[i] = Alg_j T[i][j] m[j] (tm) or out[j] = Alg_i m[i] T[i][j];
// a barrier behind the result.
template <class Alg>
__device__ __forceinline__ void contract_stream(const double* T, int X, int te, bool tm, const double* m, double* out) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (tm) {
    for (int row = wave; row < X; row += WG / 64) {
      const double* Tr = T + (size_t)row * X;
      double acc = 0.0;
      for (int j = lane; j < X; j += 64) acc = Alg::mad(acc, ldexp(Tr[j], -te), m[j]);
      acc = Alg::wave(acc);
      if (lane == 0) out[row] = acc;
    }
  } else {
    for (int j = t; j < X; j += WG) {
      double acc = 0.0;
#pragma unroll 4
      for (int i = 0; i < X; ++i) acc = Alg::mad(acc, m[i], ldexp(T[(size_t)i * X + j], -te));
      out[j] = acc;
    }
  }
  __syncthreads();
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

// ---- any X: the workgroup walks one configuration at a time ---------------------------------------------------------
struct Generic {
  const double* pair_tables; const double* unary_tables;
  PlanSections<const_i32p> pl;
  const_i32p ptab, utab;
  int X, Xp, P, U, n_free, n_cut, n_consts;
  size_t XX;
  double* acc;                               // [n_vars][Xp] the library's accumulator over configurations (generic_carve only)
  double* base;                              // [n_vars][Xp] the product of a free variable's unary rows
  double* bel;                               // [n_vars][Xp] a free variable's vector: upward, then its full belief
  double* up;                                // [n_vars][Xp] its message to its parent (generic_carve only)
  double* dn;                                // [n_vars][Xp] its parent's message to it (generic_carve only)
  double* raw;                               // [Xp]
  double* excl;                              // [Xp] (generic_carve only)
  double* scratch;                           // [8]
  int* texp;                                 // [P + U] exponent of every factor's table
  int* st;                                   // [16] states of the configuration
  int e_fixed;
};

__device__ __forceinline__ void generic_open(Generic& G, const WalkDev& d, int g) {
  G.pair_tables = d.pair_tables; G.unary_tables = d.unary_tables;
  carve_plan(as_const(d.plan), d.n_vars, d.P, d.U, d.n_cut, d.n_free, d.n_items, d.n_consts, G.pl);
  G.ptab = as_const(d.pair_tab) + (size_t)g * d.P;
  G.utab = as_const(d.unary_tab) + (size_t)g * d.U;
  G.X = d.X; G.Xp = (d.X + 1) & ~1; G.P = d.P; G.U = d.U; G.n_free = d.n_free; G.n_cut = d.n_cut; G.n_consts = d.n_consts;
  G.XX = (size_t)d.X * d.X;
}

// The walk kernel's memory, chunk k of graph g.  LDS: [vectors, unless in the workspace] [scratch] [integers]; the vectors are
// [acc, base, bel, up, dn][n_vars][Xp], raw [Xp], excl [Xp].  Returns n_vars * Xp, the doubles of acc.
__device__ __forceinline__ size_t generic_carve(Generic& G, const WalkDev& d, int g, int k, char* smem) {
  double* lds = reinterpret_cast<double*>(smem);
  const size_t n_vec = (size_t)(5 * d.n_vars + 2) * G.Xp;
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
  const size_t vs = (size_t)d.n_vars * G.Xp;
  G.acc = vec;
  G.base = G.acc + vs;
  G.bel = G.base + vs;
  G.up = G.bel + vs;
  G.dn = G.up + vs;
  G.raw = G.dn + vs;
  G.excl = G.raw + G.Xp;
  return vs;
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

// ---- where a configuration's states come from ------------------------------------------------------------------------
// A walk reads the state of cut position q as state(q).  The exact libraries number the configurations, c in [0, X^|C|), and
// decode c's digits (GenericCode, X64Code); libmlbp_cutsetis.so walks a caller's list, a row of n_cut states (ListedStates,
// wave-uniform loads) -- no number, so no 32-bit limit on X^|C|.
struct GenericCode {
  int c, X;
  __device__ __forceinline__ int operator()(int q) const {
    int r = c;
    for (int i = 0; i < q; ++i) r /= X;
    return r % X;
  }
};
struct X64Code {
  int c;
  __device__ __forceinline__ int operator()(int q) const { return (c >> (6 * q)) & 63; }
};
struct ListedStates {
  const_i32p row;                            // [n_cut], checked against [0, X) by the caller
  __device__ __forceinline__ int operator()(int q) const { return row[q]; }
};
// A listed entry in the X = 64 walk: lane q of `packed` holds the state of cut position q -- the entry's row in one coalesced
// load, checked against [0, 64) by a ballot of the caller -- and a position's state is one v_readlane, a scalar as X64Code's.
struct X64Packed {
  int packed;
  __device__ __forceinline__ int operator()(int q) const { return __builtin_amdgcn_readlane(packed, q); }
};

// A configuration, leaves to roots: returns Z_c (V_c); st holds the configuration's states, bel[v] is left holding every free
// variable's rescaled upward vector, up (unless NULL) its rescaled message to its parent.  Reached by every thread; the first
// barrier stands behind the last reads of st and bel of the configuration before; ends behind a barrier.
template <class Alg, class State>
__device__ __forceinline__ Scaled generic_up(const Generic& G, State state, double* up) {
  const int t = threadIdx.x, X = G.X, Xp = G.Xp;
  __syncthreads();
  if (t < G.n_cut) G.st[t] = state(t);
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
      double s = 0.0;
      for (int j = t; j < X; j += WG) s = Alg::join(s, bv[j]);
      mul(z, Alg::block(s, G.scratch));
    } else {
      const int par = G.pl.parent[2 * v + 1];
      contract_stream<Alg>(G.pair_tables + (size_t)G.ptab[p] * G.XX, X, G.texp[p], G.pl.pav[2 * p] != v, bv, G.raw);
      z.e += rescale(G.raw, X, G.scratch);
      for (int j = t; j < X; j += WG) {
        if (up) up[(size_t)v * Xp + j] = G.raw[j];
        G.bel[(size_t)par * Xp + j] *= G.raw[j];
      }
      __syncthreads();                                         // raw is written again, bel[par] read by every thread
    }
  }
  return z;
}

// Configuration number c: its digits base X.
template <class Alg>
__device__ __forceinline__ Scaled generic_up(const Generic& G, int c, double* up) {
  return generic_up<Alg>(G, GenericCode{c, G.X}, up);
}

// The configuration of the last generic_up (with up = G.up), roots to leaves.  Both hooks are reached by every thread of the
// workgroup under uniform control flow:
//   edge(p, v_on_axis0, bv, excl, er)  per forest factor p between v and its parent: bv is v's vector on the way up, excl the
//                                      parent's belief without v's message, G.raw 2^-er times their contraction with the
//                                      table -- all behind a barrier, none written until the hook returns; a hook that
//                                      reads entries of other threads ends with a barrier of its own
//   belief(v, j, x)                    per free variable v and entry j of this thread: x its normalised belief
// Ends behind a barrier.
template <class Alg, class Edge, class Belief>
__device__ __forceinline__ void generic_down(const Generic& G, Edge edge, Belief belief) {
  const int t = threadIdx.x, X = G.X, Xp = G.Xp;
  for (int i = G.n_free - 1; i >= 0; --i) {
    const int v = G.pl.order[i], p = G.pl.parent[2 * v];
    double* bv = G.bel + (size_t)v * Xp;
    if (p >= 0) {
      const int par = G.pl.parent[2 * v + 1];
      const bool par_has_parent = G.pl.parent[2 * par] >= 0;
      for (int j = t; j < X; j += WG) {
        double b = generic_local(G, par, j);
        if (par_has_parent) b *= G.dn[(size_t)par * Xp + j];
        G.excl[j] = b;
      }
      for (int q = 0; q < G.n_free; ++q) {                     // the parent's other children
        const int sib = G.pl.order[q];
        if (sib == v || G.pl.parent[2 * sib + 1] != par) continue;
        for (int j = t; j < X; j += WG) G.excl[j] *= G.up[(size_t)sib * Xp + j];
      }
      __syncthreads();                                         // excl: every thread wrote its own entries, rescale reads all
      rescale(G.excl, X, G.scratch);
      const bool v_on_axis0 = G.pl.pav[2 * p] == v;
      contract_stream<Alg>(G.pair_tables + (size_t)G.ptab[p] * G.XX, X, G.texp[p], v_on_axis0, G.excl, G.raw);
      const int er = rescale(G.raw, X, G.scratch);
      edge(p, v_on_axis0, bv, G.excl, er);
      for (int j = t; j < X; j += WG) {                        // a thread's own entries, as in the total below
        G.dn[(size_t)v * Xp + j] = G.raw[j];
        bv[j] *= G.raw[j];
      }
    }
    double s = 0.0;
    for (int j = t; j < X; j += WG) s = Alg::join(s, bv[j]);
    s = Alg::block(s, G.scratch);
    for (int j = t; j < X; j += WG) belief(v, j, bv[j] / s);
    __syncthreads();                                           // dn[v] and raw: read and written by the next variable's threads
  }
}

// ---- X = 64: a wave per configuration -----------------------------------------------------------------------------
struct X64 {
  const double* pair_tables;
  PlanSections<const_i32p> pl;
  const_i32p ptab;
  int n_vars, n_free, n_cut, n_consts, lane;
  double* tabs;                              // [n_forest][64][ROW] the forest's tables, rescaled
  double* base;                              // [n_vars][64] the product of a variable's unary rows, free or cut
  double* acc;                               // this wave's [n_vars][64]: the library's accumulator over its configurations
  double* phi;                               // a free variable's own factors under the configuration
  double* bel;                               // its vector on the way up
  double* up;                                // its message to its parent
  double* dn;                                // its parent's message to it
  int* texp;                                 // [P + U] exponent of every factor's table
  int e_fixed;
};

// The kernel's LDS -- [forest tables, rows of 65] [base] [4 waves x (acc, phi, bel, up, dn)] [scratch] [table exponents] --
// and its prologue by the whole workgroup: the exponents, the forest's tables into their padded rows, base for every variable,
// e_fixed.  Ends behind a barrier: the tables and base are read by every wave from there on, and a wave's own vectors by it alone.
__device__ __forceinline__ void x64_open(X64& W, const WalkDev& d, int g, char* smem) {
  constexpr int X = 64;
  const int t = threadIdx.x, wave = t >> 6, n_vars = d.n_vars, P = d.P, U = d.U;
  W.pair_tables = d.pair_tables;
  carve_plan(as_const(d.plan), d.n_vars, d.P, d.U, d.n_cut, d.n_free, d.n_items, d.n_consts, W.pl);
  W.ptab = as_const(d.pair_tab) + (size_t)g * P;
  const const_i32p utab = as_const(d.unary_tab) + (size_t)g * U;
  W.n_vars = n_vars; W.n_free = d.n_free; W.n_cut = d.n_cut; W.n_consts = d.n_consts; W.lane = t & 63;
  W.tabs = reinterpret_cast<double*>(smem);
  W.base = W.tabs + (size_t)d.n_forest * 64 * ROW;
  const size_t vs = (size_t)n_vars * 64;
  W.acc = W.base + vs + (size_t)wave * 5 * vs;
  W.phi = W.acc + vs;
  W.bel = W.phi + vs;
  W.up = W.bel + vs;
  W.dn = W.up + vs;
  double* scratch = W.base + vs + 20 * vs;
  W.texp = reinterpret_cast<int*>(scratch + 8);

  table_exponents(d.pair_tables, W.ptab, P, d.unary_tables, utab, U, X, scratch, W.texp);
  int e_fixed = 0;                                             // every factor enters every configuration once
  for (int f = 0; f < P + U; ++f) e_fixed += W.texp[f];
  for (int p = 0; p < P; ++p) {
    const int s = W.pl.fslot[p];
    if (s < 0) continue;
    const double* T = d.pair_tables + (size_t)W.ptab[p] * 4096;
    const int te = W.texp[p];
    for (int i = t; i < 4096; i += WG) W.tabs[(size_t)s * 64 * ROW + (i >> 6) * ROW + (i & 63)] = ldexp(T[i], -te);
  }
  for (int v = 0; v < n_vars; ++v) {                           // the unary rows of every variable, free or cut, multiplied once
    if (t < 64) {
      double b = 1.0;
      for (int u = 0; u < U; ++u)
        if (W.pl.uvar[u] == v) b *= ldexp(d.unary_tables[(size_t)utab[u] * 64 + t], -W.texp[P + u]);
      W.base[(size_t)v * 64 + t] = b;
    }
    __syncthreads();
    e_fixed += rescale(W.base + (size_t)v * 64, X, scratch);
  }
  W.e_fixed = e_fixed;
  __syncthreads();
}

// the state of cut position q under configuration c
__device__ __forceinline__ int x64_state(int q, int c) { return (c >> (6 * q)) & 63; }

// the free variable's configuration-free part times its cutset-incident rows and columns, at state `lane`
template <class State>
__device__ __forceinline__ double x64_local(const X64& W, int v, State state) {
  const int lane = W.lane;
  double b = W.base[(size_t)v * 64 + lane];
  for (int it = W.pl.item_off[v]; it < W.pl.item_off[v + 1]; ++it) {
    const int kind = W.pl.items[3 * it];
    if (kind == MLBP_CUTSET_ITEM_UNARY) continue;
    const int p = W.pl.items[3 * it + 1], s = state(W.pl.items[3 * it + 2]);
    const double* T = W.pair_tables + (size_t)W.ptab[p] * 4096;
    b *= ldexp(kind == MLBP_CUTSET_ITEM_COL ? T[lane * 64 + s] : T[s * 64 + lane], -W.texp[p]);
  }
  return b;
}
__device__ __forceinline__ double x64_local(const X64& W, int v, int c) { return x64_local(W, v, X64Code{c}); }

// The contraction of the padded LDS table with the wave's vector (m: the entry of this lane): lane i returns
// Alg_j T[i][j] m[j] (tm) or Alg_i m[i] T[i][lane].  Four chains of 16 steps, joined pairwise.
template <class Alg>
__device__ __forceinline__ double wave_contract_x64(const double* table, bool tm, double m, int lane) {
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  if (tm) {
    const double* row = table + lane * ROW;
#pragma unroll
    for (int j = 0; j < 64; ++j) a[j & 3] = Alg::fmad(a[j & 3], row[j], read_lane(m, j));
  } else {
    const double* col = table + lane;
#pragma unroll
    for (int i = 0; i < 64; ++i) a[i & 3] = Alg::fmad(a[i & 3], read_lane(m, i), col[i * ROW]);
  }
  return Alg::join(Alg::join(a[0], a[1]), Alg::join(a[2], a[3]));
}

// A configuration by this wave, leaves to roots: returns Z_c (V_c).  With KEEP the wave's phi, bel and up are left holding what
// x64_down_step reads; without, bel alone is used.  No barrier: every slot is written and read by the same lane.
template <class Alg, bool KEEP, class State>
__device__ __forceinline__ Scaled x64_up(const X64& W, State state) {
  const int lane = W.lane;
  Scaled z = {1.0, W.e_fixed};
  for (int q = 0; q < W.n_cut; ++q) mul(z, W.base[(size_t)W.pl.cutset[q] * 64 + state(q)]);
  for (int i = 0; i < W.n_consts; ++i) {
    if (W.pl.consts[4 * i] != MLBP_CUTSET_CONST_PAIR) continue;
    const int f = W.pl.consts[4 * i + 1], s0 = state(W.pl.consts[4 * i + 2]), s1 = state(W.pl.consts[4 * i + 3]);
    mul(z, ldexp(W.pair_tables[(size_t)W.ptab[f] * 4096 + s0 * 64 + s1], -W.texp[f]));
  }
  for (int i = 0; i < W.n_free; ++i) {
    const int v = W.pl.order[i];
    const double b = x64_local(W, v, state);
    W.bel[(size_t)v * 64 + lane] = b;
    if (KEEP) W.phi[(size_t)v * 64 + lane] = b;
  }
  for (int i = 0; i < W.n_free; ++i) {
    const int v = W.pl.order[i], p = W.pl.parent[2 * v];
    const double x = wave_rescale(W.bel[(size_t)v * 64 + lane], z.e);
    if (KEEP) W.bel[(size_t)v * 64 + lane] = x;
    if (p < 0) {
      mul(z, Alg::root(x));
    } else {
      const int par = W.pl.parent[2 * v + 1];
      const double r = wave_rescale(wave_contract_x64<Alg>(W.tabs + (size_t)W.pl.fslot[p] * 64 * ROW, W.pl.pav[2 * p] != v, x, lane), z.e);
      if (KEEP) W.up[(size_t)v * 64 + lane] = r;
      W.bel[(size_t)par * 64 + lane] *= r;
    }
  }
  return z;
}

// Configuration number c: six bits per cut position.
template <class Alg, bool KEEP>
__device__ __forceinline__ Scaled x64_up(const X64& W, int c) {
  return x64_up<Alg, KEEP>(W, X64Code{c});
}

// One free variable of the pass back at X = 64: what x64_down_step leaves to the library.
struct X64Down {
  int v;                                     // the variable
  double x;                                  // its normalised belief at state `lane`
  int p;                                     // its forest factor, -1 at a root; slot .. er are the factor's, for p >= 0 alone:
  int slot; bool v_on_axis0;                 // its table's LDS slot; v is on its axis 0
  double a, b;                               // v's vector on the way up; the parent's belief without v's message
  int er;                                    // 2^er total = a^T T~ b
  double total;                              // the belief's scale, at a root too
};

// The configuration of the last x64_up<Alg, true>, roots to leaves, by this wave: the step of order[i], to be called for
// i = n_free - 1 .. 0 by all 64 lanes.  A step and not a pass with hooks: a hook that picks a row of a register array by `slot`
// is optimised on its own before it is inlined, with the array behind a pointer, and the two rows' updates are merged into one
// indexed access -- the array's entries then live in scratch.  With the loop in the kernel the array is indexed by constants.
// FUSED: the scale of a non-root's belief is reduced in the block of the product a r, where the compiler contracts the product
// into the reduction's first addition; without, the product is rounded first.  libmlbp_exactgrad.so has always computed the
// former and libmlbp_cutset.so the latter, and both keep their bits; a maximum rounds nothing either way.
template <class Alg, bool FUSED>
__device__ __forceinline__ X64Down x64_down_step(const X64& W, int i) {
  const int lane = W.lane;
  X64Down s = {W.pl.order[i], 0.0, 0, -1, false, 0.0, 0.0, 0, 0.0};
  s.p = W.pl.parent[2 * s.v];
  double x = W.bel[(size_t)s.v * 64 + lane];
  if (s.p >= 0) {
    const int par = W.pl.parent[2 * s.v + 1];
    double b = W.phi[(size_t)par * 64 + lane];
    if (W.pl.parent[2 * par] >= 0) b *= W.dn[(size_t)par * 64 + lane];
    for (int q = 0; q < W.n_free; ++q) {                       // the parent's other children
      const int sib = W.pl.order[q];
      if (sib != s.v && W.pl.parent[2 * sib + 1] == par) b *= W.up[(size_t)sib * 64 + lane];
    }
    int unused = 0;
    b = wave_rescale(b, unused);
    s.v_on_axis0 = W.pl.pav[2 * s.p] == s.v;
    s.slot = W.pl.fslot[s.p];
    const double r = wave_rescale(wave_contract_x64<Alg>(W.tabs + (size_t)s.slot * 64 * ROW, s.v_on_axis0, b, lane), s.er);
    W.dn[(size_t)s.v * 64 + lane] = r;
    s.a = x;
    s.b = b;
    x *= r;
    if (FUSED) s.total = Alg::root(x);
  }
  if (!FUSED || s.p < 0) s.total = Alg::root(x);
  s.x = x / s.total;
  return s;
}

// ---- the sum form's running sum, and its partials read back by a combine kernel ----------------------------------------
// Z_c joins the running sum of a walker (a workgroup or a wave; z and sum have the same bits in all of its threads): the larger
// exponent is kept, rescale_acc(shift, first) brings the walker's accumulators under it -- first: they hold nothing yet.
// Returns the weight of Z_c under the sum's exponent.
template <class RescaleAcc>
__device__ __forceinline__ double join_sum(Scaled& sum, const Scaled& z, RescaleAcc rescale_acc) {
  if (z.e > sum.e) {
    const int shift = max(sum.e - z.e, MIN_SHIFT);
    rescale_acc(shift, sum.e == EMPTY);
    sum.m = ldexp(sum.m, shift);
    sum.e = z.e;
  }
  const double w = ldexp(z.m, max(z.e - sum.e, MIN_SHIFT));
  sum.m += w;
  return w;
}

// A partial: {sum mantissa, its exponent, entries ...}; `parts` of them, `stride` doubles apart.
struct SumParts {
  const double* ws; size_t stride; int parts;
  int emax;                                  // the largest exponent of a partial
  double Z;                                  // the sum of the partials' Z, a mantissa under emax
};

__device__ __forceinline__ SumParts read_sum_parts(const double* ws, size_t stride, int parts) {
  SumParts s = {ws, stride, parts, EMPTY, 0.0};
  for (int k = 0; k < parts; ++k) s.emax = max(s.emax, (int)ws[k * stride + 1]);
  for (int k = 0; k < parts; ++k) s.Z += ldexp(ws[k * stride], max((int)ws[k * stride + 1] - s.emax, MIN_SHIFT));
  return s;
}

// Entry `at` of the partials (behind the two header words), summed in index order under emax.  SKIP_EMPTY: an empty partial
// holds nothing behind its header and is passed over; without it an empty partial holds zeros.
template <bool SKIP_EMPTY>
__device__ __forceinline__ double summed(const SumParts& s, size_t at) {
  double v = 0.0;
  for (int k = 0; k < s.parts; ++k) {
    const int e = (int)s.ws[k * s.stride + 1];
    if (!SKIP_EMPTY || e != EMPTY) v += ldexp(s.ws[k * s.stride + 2 + at], max(e - s.emax, MIN_SHIFT));
  }
  return v;
}

}  // namespace mlbp_graph

#endif
