// libmlbp_exactmap.so: the exact MAP assignment and the max-marginals by cutset conditioning (include/mlbp_exactmap.h),
// gfx950 only, float64.  The max form of libmlbp_cutset.so's walk: max where that one sums, compared as (mantissa, exponent)
// pairs, decoded by back-pointers.  The walk itself is csrc/mlbp_cutset_walk.h over MaxAlg; this file holds what the library does
// with V_c and the beliefs -- the best configuration, the max-marginal accumulators, the final solve.
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
// A LISTED call (N > 0, never with MM) runs the same three kernels over the caller's list of cutset states: a walker's c is
// then the index of a list entry and the states come from the entry's row of configs -- the generic kernel in a loop of its
// own (ListedStates), the X = 64 kernel likewise (X64Packed), the final kernel re-solving the winning entry from its row.
// Without MM a walk is the pass from the leaves to the roots alone.  Every scalar a workgroup or wave branches on comes out of a
// reduction and has the same bits in every thread of it.  No sum is formed: a result does not depend on the launch at all.
// No device-side mutable globals: everything comes through ExactDev.
#include <hip/hip_runtime.h>

#include "../../include/mlbp_exactmap.h"
#define MLBP_GRAPH_NO_SWEEPS                // this library runs no sweep program
#include "../csrc/mlbp_graph_device.h"
#include "../csrc/mlbp_graph_host.h"
#include "../csrc/mlbp_cutset_plan.h"
#include "../csrc/mlbp_cutset_walk.h"

namespace {

using namespace mlbp_graph;

constexpr int PART = MLBP_EXACTMAP_PARTIAL_HEADER;
constexpr double LN2 = 0.693147180559945309417232121458;

struct ExactDev : WalkDev {                  // partials: [B][parts][per], per = PART (+ n_vars * X with max-marginals)
  double* fvec;                              // the final kernel's vectors: [B][2 n_vars + 1][round_up(X, 2)]
  int32_t* assignment; double* score; double* max_marginals;
  int32_t per;
  const int32_t* configs;                    // a listed call with cutset variables: [B][n_configs][n_cut]; else NULL
  int32_t* entry;                            // optional [B]
};

// A listed call (the header's listed mode): n_configs is N, a walker's c the index of a list entry, and the entry's states are
// its row of configs (ListedStates) where the exact call decodes c.  Without cutset variables configs is NULL and the N entries
// are the one empty configuration: the exact loop walks them as they are.  A walker that meets a row with a state outside
// [0, X) stops there and marks its partial; the final kernel then refuses the graph.
constexpr int BAD_ENTRY = -2;                // word 2 of such a partial

__device__ __forceinline__ const_i32p listed_row(const ExactDev& d, int g, int i) {
  return as_const(d.configs) + ((size_t)g * d.n_configs + i) * d.n_cut;
}

// the row's address is the same in every thread of the walker, and so is the answer
__device__ __forceinline__ bool row_in_range(const_i32p row, int n_cut, int X) {
  bool ok = true;
  for (int q = 0; q < n_cut; ++q) ok &= (unsigned)row[q] < (unsigned)X;
  return ok;
}

// The states of a listed entry in the X = 64 walk: X64Packed of csrc/mlbp_cutset_walk.h.  The listed loop is a call site of its
// own: with the exact loop's source as it was, exact_map() keeps its time (one call site for both cost it 1 to 4 %).  With
// ListedStates (scalar loads of the row) the second call site cost the instance a wave of occupancy: 106 scalar registers.

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

// A partial's header: the best configuration of the walker and the reference exponent of its max-marginals.
__device__ __forceinline__ void write_partial_header(double* out, const Best& best, int ref) {
  out[0] = best.m;
  out[1] = (double)best.e;
  out[2] = (double)best.c;
  out[3] = (double)ref;
}

// ---- any X: the workgroup walks a chunk's configurations ---------------------------------------------------
template <bool MM>
__global__ __launch_bounds__(WG) void exactmap_generic_kernel(ExactDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X, g = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  Generic G;
  generic_open(G, d, g);
  const size_t vs = generic_carve(G, d, g, k, smem);
  const int Xp = G.Xp;
  double* acc = G.acc;                                         // [n_vars][Xp] max over configurations, mantissas against ref
  generic_setup(G);
  if (MM)
    for (size_t i = t; i < vs; i += WG) acc[i] = 0.0;

  Best best = {0.0, EMPTY, -1};
  int ref = EMPTY;                                             // the largest exponent of a positive V_c so far
  if constexpr (!MM) {
    if (d.configs) {                                           // a listed call: its own loop, the exact one below is as it was
      for (int i = k; i < d.n_configs; i += d.chunks) {
        const const_i32p row = listed_row(d, g, i);
        if (!row_in_range(row, d.n_cut, X)) {
          best.c = BAD_ENTRY;                                  // the graph is refused: nothing more to walk
          break;
        }
        offer(best, generic_up<MaxAlg>(G, ListedStates{row}, nullptr), i);
      }
      if (t == 0) write_partial_header(d.partials + ((size_t)g * d.parts + k) * d.per, best, ref);
      return;
    }
  }
  for (int c = k; c < d.n_configs; c += d.chunks) {
    const Scaled z = generic_up<MaxAlg>(G, c, MM ? G.up : nullptr);
    offer(best, z, c);
    if (!MM) continue;
    if (MaxAlg::dead(z)) continue;                             // V_c = 0: nothing to record

    if (z.e > ref) {
      const int shift = ref - z.e;
      for (size_t i = t; i < vs; i += WG) acc[i] = shifted(acc[i], shift);
      ref = z.e;
      __syncthreads();
    }
    const int shift = z.e - ref;
    if (t < d.n_cut) {
      double* a = acc + (size_t)G.pl.cutset[t] * Xp + G.st[t];
      *a = fmax(*a, shifted(z.m, shift));
    }
    generic_down<MaxAlg>(G, NoEdge(), [&](int v, int j, double x) {
      double* a = acc + (size_t)v * Xp + j;
      *a = fmax(*a, shifted(z.m * x, shift));
    });
  }

  __syncthreads();
  double* out = d.partials + ((size_t)g * d.parts + k) * d.per;
  if (t == 0) write_partial_header(out, best, ref);
  if (MM)
    for (int v = 0; v < d.n_vars; ++v)
      for (int j = t; j < X; j += WG) out[PART + (size_t)v * X + j] = acc[(size_t)v * Xp + j];
}

// ---- X = 64: a wave per configuration ---------------------------------------------------------------------
// Without MM a wave uses its bel alone.
template <bool MM>
__global__ __launch_bounds__(WG) void exactmap_x64_kernel(ExactDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  X64 W;
  x64_open(W, d, g, smem);
  const int n_vars = d.n_vars;
  double* acc = W.acc;                                         // this wave's: max over its configurations, mantissas against ref
  if (MM)
    for (int v = 0; v < n_vars; ++v) acc[(size_t)v * 64 + lane] = 0.0;

  Best best = {0.0, EMPTY, -1};
  int ref = EMPTY;                                             // the largest exponent of a positive V_c so far
  if constexpr (!MM) {
    if (d.configs) {                                           // a listed call: its own loop, the exact one below is as it was
      for (int i = 4 * k + wave; i < d.n_configs; i += 4 * d.chunks) {
        const int packed = lane < d.n_cut ? listed_row(d, g, i)[lane] : 0;
        if (__any((unsigned)packed >= 64u)) {
          best.c = BAD_ENTRY;                                  // the graph is refused: nothing more to walk
          break;
        }
        offer(best, x64_up<MaxAlg, false>(W, X64Packed{packed}), i);
      }
      if (lane == 0) write_partial_header(d.partials + ((size_t)g * d.parts + 4 * k + wave) * d.per, best, ref);
      return;
    }
  }
  for (int c = 4 * k + wave; c < d.n_configs; c += 4 * d.chunks) {
    const Scaled z = x64_up<MaxAlg, MM>(W, c);
    offer(best, z, c);
    if (!MM) continue;
    if (MaxAlg::dead(z)) continue;                             // V_c = 0: nothing to record

    if (z.e > ref) {
      const int shift = ref - z.e;
      for (int v = 0; v < n_vars; ++v) acc[(size_t)v * 64 + lane] = shifted(acc[(size_t)v * 64 + lane], shift);
      ref = z.e;
    }
    const int shift = z.e - ref;
    const double w = shifted(z.m, shift);
    for (int q = 0; q < d.n_cut; ++q)
      if (lane == x64_state(q, c)) acc[(size_t)W.pl.cutset[q] * 64 + lane] = fmax(acc[(size_t)W.pl.cutset[q] * 64 + lane], w);
    for (int i = W.n_free - 1; i >= 0; --i) {
      const X64Down s = x64_down_step<MaxAlg, false>(W, i);
      acc[(size_t)s.v * 64 + lane] = fmax(acc[(size_t)s.v * 64 + lane], shifted(z.m * s.x, shift));
    }
  }

  double* out = d.partials + ((size_t)g * d.parts + 4 * k + wave) * d.per;
  if (lane == 0) write_partial_header(out, best, ref);
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
    if (t == 0 && d.entry) d.entry[g] = -1;
    return;
  }
  const double* ws = d.partials + (size_t)g * d.parts * d.per;

  // the best partial: the larger V, then the lower configuration index (of a listed call: the lower entry index)
  Best best = {0.0, EMPTY, -1};
  int ref = EMPTY;
  bool bad = false;                                            // a listed call: a walker met a state outside [0, X)
  if (d.configs)
    for (int k = 0; k < d.parts; ++k) bad |= (int)ws[(size_t)k * d.per + 2] == BAD_ENTRY;
  if (bad) {                                                   // the same in every thread: the graph is not computed
    for (int v = t; v < n_vars; v += WG) xs[v] = -1;
    if (t == 0) d.score[g] = __builtin_nan("");
    if (t == 0 && d.entry) d.entry[g] = -1;
    return;
  }
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
    if (d.configs) generic_up<MaxAlg>(G, ListedStates{listed_row(d, g, best.c)}, nullptr);
    else generic_up<MaxAlg>(G, best.c, nullptr);
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
  if (lane == 0 && d.entry) d.entry[g] = best.c;
}

// ---- host ----------------------------------------------------------------------------------------
thread_local int g_last_kernel = MLBP_EXACTMAP_KERNEL_NONE;
static_assert(MLBP_EXACTMAP_KERNEL_X64 == WALK_X64 && MLBP_EXACTMAP_KERNEL_GENERIC == WALK_GENERIC, "the shared host core numbers the kernels");
static_assert(MLBP_EXACTMAP_MAX_CUT == MAX_LISTED_CUT, "the header states the shared walk's bound");

// The header's workspace formula, exact or listed: `per` doubles in a partial, `chunks` = C of the grid.
int64_t workspace_of(int which, int64_t B, int64_t chunks, int64_t per, int64_t n_vars, int64_t P, int64_t U, int64_t X) {
  const int64_t Xp = (X + 1) / 2 * 2;
  return (B * chunks * chunk_doubles(which, per, n_vars, P, U, X) + B * (2 * n_vars + 1) * Xp) * 8;
}

}  // namespace

extern "C" {

const char* mlbp_exactmap_arch(void) { return "gfx950"; }
const char* mlbp_exactmap_last_error(void) { return g_last_error.c_str(); }
int mlbp_exactmap_last_kernel(void) { return g_last_kernel; }

int mlbp_exactmap_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest) {
  return pick_walk_kernel(X, n_vars, P, U, n_forest);
}

int mlbp_exactmap_chunks(int32_t B, int32_t n_configs) {
  if (B <= 0 || n_configs <= 0) return fail(MLBP_EINVAL, "chunks: B = %d, n_configs = %d", B, n_configs);
  return walk_chunks(B, n_configs, MLBP_CUTSET_MIN_WORKGROUPS);
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
  return workspace_of(which, B, chunks, PART + (max_marginals ? (int64_t)n_vars * X : 0), n_vars, P, U, X);
}

int mlbp_exactmap_check_plan(const int32_t* plan, int32_t n_words, int32_t X) { return check_packed_plan(plan, n_words, X); }

int mlbp_exactmap_f64(const mlbp_exactmap_args* a, void* stream) {
  g_last_kernel = MLBP_EXACTMAP_KERNEL_NONE;
  const bool listed = a && a->N > 0;                           // the header's listed mode: the walk's entries are the list's
  int64_t n_configs = listed ? a->N : 0;
  const int which = check_walk_args(a, mlbp_exactmap_pick_kernel, [](const mlbp_exactmap_args* a) {
    if (!a->assignment || !a->score) return fail(MLBP_EINVAL, "assignment or score is NULL");
    if (a->N < 0 || a->N > MLBP_EXACTMAP_MAX_LISTED)
      return fail(MLBP_EINVAL, "N = %d: a list holds 1 to %d configurations (0: the exact call)", a->N, MLBP_EXACTMAP_MAX_LISTED);
    if (a->N > 0 && a->n_cut > 0 && !a->configs) return fail(MLBP_EINVAL, "configs is NULL in a listed call with cutset variables");
    if (a->N > 0 && a->max_marginals)
      return fail(MLBP_EUNSUPPORTED, "max_marginals with N = %d: the max over a list is no max-marginal", a->N);
    return (int)MLBP_OK;
  }, &n_configs, listed);
  if (which < 0) return which;
  const int chunks = mlbp_exactmap_chunks(a->B, (int32_t)n_configs);
  if (chunks < 0) return chunks;
  const bool mm = a->max_marginals != nullptr;
  const int64_t need = listed ? workspace_of(which, a->B, chunks, PART, a->n_vars, a->P, a->U, a->X)
                              : mlbp_exactmap_workspace_bytes(a->B, a->X, a->n_vars, a->P, a->U, a->n_forest, a->n_cut, mm);
  if (int e = check_walk_workspace(a, need)) return e;
  if (int e = check_device("libmlbp_exactmap.so")) return e;
  const int64_t Xp = (a->X + 1) / 2 * 2;
  ExactDev d;
  fill_walk_dev(d, a, n_configs, chunks, which);
  d.assignment = a->assignment; d.score = a->score; d.max_marginals = a->max_marginals;
  d.configs = listed && a->n_cut > 0 ? a->configs : nullptr;
  d.entry = a->entry;
  d.per = PART + (mm ? a->n_vars * a->X : 0);
  d.fvec = d.partials + (int64_t)a->B * d.parts * d.per;
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
    const size_t lds = generic_walk_lds(d, d.fvec + (int64_t)a->B * (2 * (int64_t)a->n_vars + 1) * Xp);
    if (mm) hipLaunchKernelGGL(exactmap_generic_kernel<true>, grid, dim3(WG), lds, st, d);
    else hipLaunchKernelGGL(exactmap_generic_kernel<false>, grid, dim3(WG), lds, st, d);
  }
  if (int e = launched("exactmap")) return e;
  hipLaunchKernelGGL(exactmap_final_kernel, dim3(a->B), dim3(WG), (size_t)(64 + ints_bytes(a->P, a->U)), st, d);
  if (int e = launched("final")) return e;
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
