// libmlbp_cutset.so: the model's true marginals and log Z by cutset conditioning (include/mlbp_cutset.h), gfx950 only,
// float64.  The sum form of the walk of csrc/mlbp_cutset_walk.h: this file holds what the library does with Z_c and the
// beliefs -- the accumulation of Z_c m_c under a running exponent, the partials, the read-out.
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

#include "../../include/mlbp_cutset.h"
#define MLBP_GRAPH_NO_SWEEPS                // this library runs no sweep program: mlbp_cutset.h has no op kinds
#include "../csrc/mlbp_graph_device.h"
#include "../csrc/mlbp_graph_host.h"
#include "../csrc/mlbp_cutset_plan.h"       // the plan, the power-of-two helpers, the host core: shared with the two exact* libraries
#include "../csrc/mlbp_cutset_walk.h"       // the walk

namespace {

using namespace mlbp_graph;

struct CutsetDev : WalkDev {                 // partials: [B][parts][n_vars * X + 2]
  const int32_t* labels;
  double* log_z; double* marginals; double* score; double* joint_logp;
};

// ---- any X: the workgroup walks a chunk's configurations ---------------------------------------------------
__global__ __launch_bounds__(WG) void cutset_generic_kernel(CutsetDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X, g = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  Generic G;
  generic_open(G, d, g);
  const size_t vs = generic_carve(G, d, g, k, smem);
  const int Xp = G.Xp;
  double* acc = G.acc;                                         // [n_vars][Xp] sum over configurations of Z_c m_c, mantissas
  generic_setup(G);
  for (size_t i = t; i < vs; i += WG) acc[i] = 0.0;

  Scaled sum = {0.0, EMPTY};                                   // sum of Z_c over this chunk
  for (int c = k; c < d.n_configs; c += d.chunks) {
    const Scaled z = generic_up<SumAlg>(G, c, G.up);
    if (SumAlg::dead(z)) continue;                             // Z_c = 0: nothing to add
    const double w = join_sum(sum, z, [&](int shift, bool) {
      for (size_t i = t; i < vs; i += WG) acc[i] = ldexp(acc[i], shift);
      __syncthreads();
    });
    if (t < d.n_cut) acc[(size_t)G.pl.cutset[t] * Xp + G.st[t]] += w;
    generic_down<SumAlg>(G, NoEdge(), [&](int v, int j, double x) { acc[(size_t)v * Xp + j] += w * x; });
  }

  __syncthreads();
  double* out = d.partials + ((size_t)g * d.parts + k) * ((size_t)d.n_vars * X + 2);
  if (t == 0) {
    out[0] = sum.m;
    out[1] = (double)sum.e;
  }
  for (int v = 0; v < d.n_vars; ++v)
    for (int j = t; j < X; j += WG) out[2 + (size_t)v * X + j] = acc[(size_t)v * Xp + j];
}

// ---- X = 64: a wave per configuration ---------------------------------------------------------------------
__global__ __launch_bounds__(WG) void cutset_x64_kernel(CutsetDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  X64 W;
  x64_open(W, d, g, smem);
  const int n_vars = d.n_vars;
  double* acc = W.acc;                                         // this wave's: sum over its configurations of Z_c m_c, mantissas
  for (int v = 0; v < n_vars; ++v) acc[(size_t)v * 64 + lane] = 0.0;

  Scaled sum = {0.0, EMPTY};                                   // sum of Z_c over this wave's configurations
  for (int c = 4 * k + wave; c < d.n_configs; c += 4 * d.chunks) {
    const Scaled z = x64_up<SumAlg, true>(W, c);
    if (SumAlg::dead(z)) continue;                             // Z_c = 0: nothing to add
    const double w = join_sum(sum, z, [&](int shift, bool) {
      for (int v = 0; v < n_vars; ++v) acc[(size_t)v * 64 + lane] = ldexp(acc[(size_t)v * 64 + lane], shift);
    });
    for (int q = 0; q < d.n_cut; ++q)
      if (lane == x64_state(q, c)) acc[(size_t)W.pl.cutset[q] * 64 + lane] += w;
    for (int i = W.n_free - 1; i >= 0; --i) {
      const X64Down s = x64_down_step<SumAlg, false>(W, i);
      acc[(size_t)s.v * 64 + lane] = fma(w, s.x, acc[(size_t)s.v * 64 + lane]);       // fused, as the compiler always contracted it
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
  const SumParts parts = read_sum_parts(d.partials + (size_t)g * d.parts * stride, stride, d.parts);
  const double Z = parts.Z;
  const double uniform = 1.0 / (double)d.X;
  double* marg = d.marginals + (size_t)g * N;
  for (size_t i = t; i < N; i += WG) {
    const double s = summed<false>(parts, i);                  // an empty partial holds zeros
    marg[i] = Z == 0.0 ? uniform : s / Z;
  }
  if (wave != 0) return;
  const double lz = Z == 0.0 ? -__builtin_huge_val() : fma((double)parts.emax, 0.693147180559945309417232121458, log(Z));
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
static_assert(MLBP_CUTSET_KERNEL_X64 == WALK_X64 && MLBP_CUTSET_KERNEL_GENERIC == WALK_GENERIC, "the shared host core numbers the kernels");

}  // namespace

extern "C" {

const char* mlbp_cutset_arch(void) { return "gfx950"; }
const char* mlbp_cutset_last_error(void) { return g_last_error.c_str(); }
int mlbp_cutset_last_kernel(void) { return g_last_kernel; }

int mlbp_cutset_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest) {
  return pick_walk_kernel(X, n_vars, P, U, n_forest);
}

int mlbp_cutset_chunks(int32_t B, int32_t n_configs) {
  if (B <= 0 || n_configs <= 0) return fail(MLBP_EINVAL, "chunks: B = %d, n_configs = %d", B, n_configs);
  return walk_chunks(B, n_configs, MLBP_CUTSET_MIN_WORKGROUPS);
}

int64_t mlbp_cutset_workspace_bytes(int32_t B, int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t n_cut) {
  const int which = mlbp_cutset_pick_kernel(X, n_vars, P, U, n_forest);
  if (which < 0) return which;
  if (n_cut < 0 || n_cut > n_vars) return fail(MLBP_EINVAL, "workspace: n_cut = %d with %d variables", n_cut, n_vars);
  const int64_t n_configs = count_configs(X, n_cut);
  if (n_configs < 0) return too_many_configs(X, n_cut);
  const int chunks = mlbp_cutset_chunks(B, (int32_t)n_configs);
  if (chunks < 0) return chunks;
  return (int64_t)B * chunks * chunk_doubles(which, (int64_t)n_vars * X + 2, n_vars, P, U, X) * 8;
}

int mlbp_cutset_check_plan(const int32_t* plan, int32_t n_words, int32_t X) { return check_packed_plan(plan, n_words, X); }

int mlbp_cutset_f64(const mlbp_cutset_args* a, void* stream) {
  g_last_kernel = MLBP_CUTSET_KERNEL_NONE;
  int64_t n_configs = 0;
  const int which = check_walk_args(a, mlbp_cutset_pick_kernel, [](const mlbp_cutset_args* a) {
    if (!a->log_z || !a->marginals) return fail(MLBP_EINVAL, "log_z or marginals is NULL");
    if ((a->score || a->joint_logp) && !a->labels) return fail(MLBP_EINVAL, "score and joint_logp need labels");
    return (int)MLBP_OK;
  }, &n_configs);
  if (which < 0) return which;
  const int chunks = mlbp_cutset_chunks(a->B, (int32_t)n_configs);
  if (chunks < 0) return chunks;
  if (int e = check_walk_workspace(a, mlbp_cutset_workspace_bytes(a->B, a->X, a->n_vars, a->P, a->U, a->n_forest, a->n_cut))) return e;
  if (int e = check_device("libmlbp_cutset.so")) return e;
  CutsetDev d;
  fill_walk_dev(d, a, n_configs, chunks, which);
  d.labels = a->labels;
  d.log_z = a->log_z; d.marginals = a->marginals; d.score = a->score; d.joint_logp = a->joint_logp;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(a->B, chunks);
  (void)hipGetLastError();
  if (which == MLBP_CUTSET_KERNEL_X64) {
    if (int e = grant_x64_lds((const void*)cutset_x64_kernel, 0, MLBP_CUTSET_X64_LDS_BYTES)) return e;
    hipLaunchKernelGGL(cutset_x64_kernel, grid, dim3(WG), (size_t)x64_lds_bytes(a->n_vars, a->P, a->U, a->n_forest), st, d);
  } else {
    const size_t lds = generic_walk_lds(d, a->workspace + (int64_t)a->B * chunks * ((int64_t)a->n_vars * a->X + 2));
    hipLaunchKernelGGL(cutset_generic_kernel, grid, dim3(WG), lds, st, d);
  }
  if (int e = launched("cutset")) return e;
  hipLaunchKernelGGL(cutset_combine_kernel, dim3(a->B), dim3(WG), 0, st, d);
  if (int e = launched("combine")) return e;
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
