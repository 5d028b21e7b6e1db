// libmlbp_cutsetis.so: an estimate of log Z and the marginals by cutset importance sampling (include/mlbp_cutsetis.h), gfx950
// only, float64.  The sum form of the walk of csrc/mlbp_cutset_walk.h over a caller's LIST of configurations: the states of an
// entry are read from the list (ListedStates) where the exact libraries decode a configuration number.  This file holds what
// the library does with Z_c and the beliefs -- the weight Z_c / q(c) as a (mantissa, exponent) pair, the accumulation of
// w m_c and of w and w^2 under a running exponent, the partials, the read-out.
//
// Three kernels; the first two are chosen from (X, n_vars, P, U, n_forest) by mlbp_cutsetis_pick_kernel:
//   cutsetis_x64_kernel      X = 64: the forest's tables in LDS (x64_open); every WAVE walks list entries of its own, no
//                            workgroup barrier inside the walk; a wave writes its own partial: four per workgroup.
//   cutsetis_generic_kernel  any X in [2, 1024]: the whole workgroup walks one entry at a time, tables streamed, the vectors in
//                            LDS when they fit, else in the caller's workspace.
//   cutsetis_combine_kernel  one workgroup per graph: adds the partials in index order, divides by S1, takes the one logarithm,
//                            ess, and the score at the labels.
// Workgroup (g, k) of the generic kernel walks entries k, k + chunks, ... of graph g; wave w of workgroup (g, k) of the X = 64
// kernel walks 4 k + w, 4 k + w + 4 chunks, ...  An entry's states and log_q are read at a wave-uniform address, so every
// scalar a workgroup or wave branches on has the same bits in every thread of it.  An entry that cannot be walked (a state
// outside [0, X), a log_q out of range) is passed over and marks the walker's partial; the combine kernel then refuses the graph.
// No device-side mutable globals: everything comes through CutsetisDev.
#include <hip/hip_runtime.h>

#include "../../include/mlbp_cutset.h"      // the plan's layout and constants
#include "../../include/mlbp_cutsetis.h"
#define MLBP_GRAPH_NO_SWEEPS                // this library runs no sweep program
#include "../csrc/mlbp_graph_device.h"
#include "../csrc/mlbp_graph_host.h"
#include "../csrc/mlbp_cutset_plan.h"
#include "../csrc/mlbp_cutset_walk.h"

namespace {

using namespace mlbp_graph;

struct CutsetisDev : WalkDev {               // n_configs: N, the entries listed per graph; partials: [B][parts][n_vars * X + 3]
  const int32_t* configs; const double* log_q; const int32_t* labels;
  double* log_z_hat; double* marginals; double* ess; double* log_w; double* score; double* joint_logp;
};

constexpr double LN2 = 0.693147180559945309417232121458;
constexpr int BAD = 1 << 29;                 // the exponent of a partial whose walker met an entry it could not walk

// The states of an entry are inside [0, X) and its log_q is a finite number within the header's range (the same in every thread).
__device__ __forceinline__ bool entry_ok(const_i32p row, int n_cut, int X, double lq) {
  bool ok = fabs(lq) <= MLBP_CUTSETIS_MAX_ABS_LOG_Q;           // false for a NaN
  for (int q = 0; q < n_cut; ++q) ok &= (unsigned)row[q] < (unsigned)X;
  return ok;
}

// Z_c exp(-log_q) by the header's formula: weighted() of csrc/mlbp_cutset_plan.h.
__device__ __forceinline__ double log_of(const Scaled& w) { return fma((double)w.e, LN2, log(w.m)); }

// A graph whose table indices are out of range is not walked: its log_w reads NaN.
__device__ __forceinline__ void refuse_log_w(const CutsetisDev& d, int g, int first, int step) {
  if (!d.log_w) return;
  for (int i = first; i < d.n_configs; i += step) d.log_w[(size_t)g * d.n_configs + i] = __builtin_nan("");
}

// ---- any X: the workgroup walks a chunk's entries ------------------------------------------------------------
__global__ __launch_bounds__(WG) void cutsetis_generic_kernel(CutsetisDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X, g = blockIdx.x, k = blockIdx.y, t = threadIdx.x, N = d.n_configs;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) {
    refuse_log_w(d, g, k + t * d.chunks, WG * d.chunks);
    return;
  }
  Generic G;
  generic_open(G, d, g);
  const size_t vs = generic_carve(G, d, g, k, smem);
  const int Xp = G.Xp;
  double* acc = G.acc;                                         // [n_vars][Xp] sum over entries of w m_c, mantissas
  generic_setup(G);
  for (size_t i = t; i < vs; i += WG) acc[i] = 0.0;

  const size_t gN = (size_t)g * N;
  const const_f64p log_q = as_const_f64(d.log_q);
  Scaled sum = {0.0, EMPTY};                                   // S1 over this chunk
  double s2 = 0.0;                                             // S2 over this chunk, under twice S1's exponent
  bool bad = false;
  for (int i = k; i < N; i += d.chunks) {
    const const_i32p row = as_const(d.configs) + (gN + i) * d.n_cut;
    const double lq = log_q[gN + i];
    if (!entry_ok(row, d.n_cut, X, lq)) {
      bad = true;
      if (d.log_w && t == 0) d.log_w[gN + i] = __builtin_nan("");
      continue;
    }
    const Scaled z = generic_up<SumAlg>(G, ListedStates{row}, G.up);
    if (SumAlg::dead(z)) {                                     // Z_c = 0: nothing to add
      if (d.log_w && t == 0) d.log_w[gN + i] = -__builtin_huge_val();
      continue;
    }
    const Scaled zw = weighted(z, lq);
    if (d.log_w && t == 0) d.log_w[gN + i] = log_of(zw);
    const double w = join_sum(sum, zw, [&](int shift, bool) {
      for (size_t j = t; j < vs; j += WG) acc[j] = ldexp(acc[j], shift);
      s2 = ldexp(s2, 2 * shift);
      __syncthreads();
    });
    s2 = fma(w, w, s2);
    if (t < d.n_cut) acc[(size_t)G.pl.cutset[t] * Xp + G.st[t]] += w;
    generic_down<SumAlg>(G, NoEdge(), [&](int v, int j, double x) { acc[(size_t)v * Xp + j] += w * x; });
  }

  __syncthreads();
  const size_t nvx = (size_t)d.n_vars * X;
  double* out = d.partials + ((size_t)g * d.parts + k) * (nvx + 3);
  if (t == 0) {
    out[0] = sum.m;
    out[1] = (double)(bad ? BAD : sum.e);
    out[2 + nvx] = s2;
  }
  for (int v = 0; v < d.n_vars; ++v)
    for (int j = t; j < X; j += WG) out[2 + (size_t)v * X + j] = acc[(size_t)v * Xp + j];
}

// ---- X = 64: a wave per entry ---------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void cutsetis_x64_kernel(CutsetisDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x, lane = t & 63, N = d.n_configs;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);     // the entry's address is wave-uniform: scalar loads
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) {
    refuse_log_w(d, g, 4 * k + wave + 4 * d.chunks * lane, 4 * d.chunks * 64);
    return;
  }
  X64 W;
  x64_open(W, d, g, smem);
  const int n_vars = d.n_vars, n_cut = d.n_cut;
  double* acc = W.acc;                                         // this wave's: sum over its entries of w m_c, mantissas
  for (int v = 0; v < n_vars; ++v) acc[(size_t)v * 64 + lane] = 0.0;

  const size_t gN = (size_t)g * N;
  const const_f64p log_q = as_const_f64(d.log_q);
  Scaled sum = {0.0, EMPTY};                                   // S1 over this wave's entries
  double s2 = 0.0;                                             // S2 over them, under twice S1's exponent
  bool bad = false;
  for (int i = 4 * k + wave; i < N; i += 4 * d.chunks) {
    const const_i32p row = as_const(d.configs) + (gN + i) * n_cut;
    const double lq = log_q[gN + i];
    if (!entry_ok(row, n_cut, 64, lq)) {
      bad = true;
      if (d.log_w && lane == 0) d.log_w[gN + i] = __builtin_nan("");
      continue;
    }
    const ListedStates state = {row};
    const Scaled z = x64_up<SumAlg, true>(W, state);
    if (SumAlg::dead(z)) {                                     // Z_c = 0: nothing to add
      if (d.log_w && lane == 0) d.log_w[gN + i] = -__builtin_huge_val();
      continue;
    }
    const Scaled zw = weighted(z, lq);
    if (d.log_w && lane == 0) d.log_w[gN + i] = log_of(zw);
    const double w = join_sum(sum, zw, [&](int shift, bool) {
      for (int v = 0; v < n_vars; ++v) acc[(size_t)v * 64 + lane] = ldexp(acc[(size_t)v * 64 + lane], shift);
      s2 = ldexp(s2, 2 * shift);
    });
    s2 = fma(w, w, s2);
    for (int q = 0; q < n_cut; ++q)
      if (lane == state(q)) acc[(size_t)W.pl.cutset[q] * 64 + lane] += w;
    for (int j = W.n_free - 1; j >= 0; --j) {
      const X64Down s = x64_down_step<SumAlg, false>(W, j);
      acc[(size_t)s.v * 64 + lane] = fma(w, s.x, acc[(size_t)s.v * 64 + lane]);
    }
  }

  const size_t nvx = (size_t)n_vars * 64;
  double* out = d.partials + ((size_t)g * d.parts + 4 * k + wave) * (nvx + 3);
  if (lane == 0) {
    out[0] = sum.m;
    out[1] = (double)(bad ? BAD : sum.e);
    out[2 + nvx] = s2;
  }
  for (int v = 0; v < n_vars; ++v) out[2 + (size_t)v * 64 + lane] = acc[(size_t)v * 64 + lane];
}

// score at the labels of graph g, by one wave (every lane returns it): NaN when a label is outside [0, X).
__device__ __forceinline__ double wave_score(const CutsetisDev& d, const_i32p pav, const_i32p uvar, int g, int lane) {
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

// ---- the partials of a graph's chunks -> its outputs ------------------------------------------------------------
__global__ __launch_bounds__(WG) void cutsetis_combine_kernel(CutsetisDev d) {
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool want = d.labels && (d.score || d.joint_logp);
  const double nan = __builtin_nan("");
  const size_t nvx = (size_t)d.n_vars * d.X, stride = nvx + 3;
  const double* ws = d.partials + (size_t)g * d.parts * stride;
  bool ok = tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g);
  if (ok)                                                      // the partials of a graph with a bad table index were not written
    for (int k = 0; k < d.parts; ++k) ok &= (int)ws[k * stride + 1] != BAD;
  if (!ok) {
    if (t == 0) {
      d.log_z_hat[g] = nan;
      d.ess[g] = nan;
      if (want && d.score) d.score[g] = nan;
      if (want && d.joint_logp) d.joint_logp[g] = nan;
    }
    return;
  }
  const SumParts parts = read_sum_parts(ws, stride, d.parts);
  const double S1 = parts.Z;
  const double uniform = 1.0 / (double)d.X;
  double* marg = d.marginals + (size_t)g * nvx;
  for (size_t i = t; i < nvx; i += WG) {
    const double s = summed<false>(parts, i);                  // an empty partial holds zeros
    marg[i] = S1 == 0.0 ? uniform : s / S1;
  }
  if (wave != 0) return;
  double S2 = 0.0;                                             // under twice emax
  for (int k = 0; k < d.parts; ++k)
    S2 += ldexp(ws[k * stride + 2 + nvx], 2 * max((int)ws[k * stride + 1] - parts.emax, MIN_SHIFT));
  const double lz = S1 == 0.0 ? -__builtin_huge_val() : fma((double)parts.emax, LN2, log(S1 / (double)d.n_configs));
  double sc = nan;
  if (want) {
    PlanSections<const_i32p> pl;
    carve_plan(as_const(d.plan), d.n_vars, d.P, d.U, d.n_cut, d.n_free, d.n_items, d.n_consts, pl);
    sc = wave_score(d, pl.pav, pl.uvar, g, lane);
  }
  if (lane == 0) {
    d.log_z_hat[g] = lz;
    d.ess[g] = S1 == 0.0 ? 0.0 : S1 * S1 / S2;
    if (want && d.score) d.score[g] = sc;
    if (want && d.joint_logp) d.joint_logp[g] = sc - lz;
  }
}

// ---- host ----------------------------------------------------------------------------------------
thread_local int g_last_kernel = MLBP_CUTSETIS_KERNEL_NONE;
static_assert(MLBP_CUTSETIS_KERNEL_X64 == WALK_X64 && MLBP_CUTSETIS_KERNEL_GENERIC == WALK_GENERIC, "the shared host core numbers the kernels");
static_assert(MLBP_CUTSETIS_MAX_CUT == MAX_LISTED_CUT, "the header states the shared walk's bound");

}  // namespace

extern "C" {

const char* mlbp_cutsetis_arch(void) { return "gfx950"; }
const char* mlbp_cutsetis_last_error(void) { return g_last_error.c_str(); }
int mlbp_cutsetis_last_kernel(void) { return g_last_kernel; }

int mlbp_cutsetis_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest) {
  return pick_walk_kernel(X, n_vars, P, U, n_forest);
}

int mlbp_cutsetis_chunks(int32_t B, int32_t N) {
  if (B <= 0 || N <= 0 || N > MLBP_CUTSETIS_MAX_LISTED)
    return fail(MLBP_EINVAL, "chunks: B = %d, N = %d (N in [1, %d])", B, N, MLBP_CUTSETIS_MAX_LISTED);
  return walk_chunks(B, N, MLBP_CUTSETIS_MIN_WORKGROUPS);
}

int64_t mlbp_cutsetis_workspace_bytes(int32_t B, int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t N) {
  const int which = mlbp_cutsetis_pick_kernel(X, n_vars, P, U, n_forest);
  if (which < 0) return which;
  const int chunks = mlbp_cutsetis_chunks(B, N);
  if (chunks < 0) return chunks;
  return (int64_t)B * chunks * chunk_doubles(which, (int64_t)n_vars * X + 3, n_vars, P, U, X) * 8;
}

int mlbp_cutsetis_check_plan(const int32_t* plan, int32_t n_words, int32_t X) { return check_packed_plan(plan, n_words, X, true); }

int mlbp_cutsetis_f64(const mlbp_cutsetis_args* a, void* stream) {
  g_last_kernel = MLBP_CUTSETIS_KERNEL_NONE;
  int64_t unused = 0;
  const int which = check_walk_args(a, mlbp_cutsetis_pick_kernel, [](const mlbp_cutsetis_args* a) {
    if (a->N <= 0 || a->N > MLBP_CUTSETIS_MAX_LISTED) return fail(MLBP_EINVAL, "N = %d: a list holds 1 to %d configurations", a->N, MLBP_CUTSETIS_MAX_LISTED);
    if (!a->log_q || (a->n_cut > 0 && !a->configs)) return fail(MLBP_EINVAL, "configs or log_q is NULL");
    if (!a->log_z_hat || !a->marginals || !a->ess) return fail(MLBP_EINVAL, "log_z_hat, marginals or ess is NULL");
    if ((a->score || a->joint_logp) && !a->labels) return fail(MLBP_EINVAL, "score and joint_logp need labels");
    return (int)MLBP_OK;
  }, &unused, true);
  if (which < 0) return which;
  const int chunks = mlbp_cutsetis_chunks(a->B, a->N);
  if (chunks < 0) return chunks;
  if (int e = check_walk_workspace(a, mlbp_cutsetis_workspace_bytes(a->B, a->X, a->n_vars, a->P, a->U, a->n_forest, a->N))) return e;
  if (int e = check_device("libmlbp_cutsetis.so")) return e;
  CutsetisDev d;
  fill_walk_dev(d, a, a->N, chunks, which);
  d.configs = a->configs; d.log_q = a->log_q; d.labels = a->labels;
  d.log_z_hat = a->log_z_hat; d.marginals = a->marginals; d.ess = a->ess; d.log_w = a->log_w; d.score = a->score; d.joint_logp = a->joint_logp;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(a->B, chunks);
  (void)hipGetLastError();
  if (which == MLBP_CUTSETIS_KERNEL_X64) {
    if (int e = grant_x64_lds((const void*)cutsetis_x64_kernel, 0, MLBP_CUTSET_X64_LDS_BYTES)) return e;
    hipLaunchKernelGGL(cutsetis_x64_kernel, grid, dim3(WG), (size_t)x64_lds_bytes(a->n_vars, a->P, a->U, a->n_forest), st, d);
  } else {
    const size_t lds = generic_walk_lds(d, a->workspace + (int64_t)a->B * chunks * ((int64_t)a->n_vars * a->X + 3));
    hipLaunchKernelGGL(cutsetis_generic_kernel, grid, dim3(WG), lds, st, d);
  }
  if (int e = launched("cutsetis")) return e;
  hipLaunchKernelGGL(cutsetis_combine_kernel, dim3(a->B), dim3(WG), 0, st, d);
  if (int e = launched("combine")) return e;
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
