// libmlbp_exactsample.so: whole assignments drawn from the model itself by cutset conditioning (include/mlbp_exactsample.h),
// gfx950 only, float64.  The sum form of the walk of csrc/mlbp_cutset_walk.h without its pass back; this file holds what the
// library does around it -- every Z_c kept apart, their scan, the draw of a configuration and of the free variables from the
// roots down.
//
// Five kernels, three launches per call; the form of the first and the third is chosen from (X, n_vars, P, U, n_forest) by
// mlbp_exactsample_pick_kernel:
//   exactsample_weights_x64_kernel      X = 64: the forest's tables in LDS (x64_open); every WAVE walks configurations of its own
//                                       (x64_up<SumAlg, false>) and writes Z_c as a (mantissa, exponent) pair.
//   exactsample_weights_generic_kernel  any X in [2, 1024]: the workgroup walks one configuration at a time (generic_up<SumAlg>).
//   exactsample_scan_kernel             one workgroup per graph: the Z_c under the graph's largest exponent, their SEGMENTED
//                                       prefix sums, log Z, and whether the graph can be drawn from at all.
//   exactsample_draw_x64_kernel         X = 64: the tables in LDS for the whole launch; every WAVE draws samples of its own,
//                                       lane = state, no workgroup barrier: binary search for the configuration, one pass up,
//                                       then per free variable a DPP scan, a ballot and a readlane.
//   exactsample_draw_generic_kernel     any X: one workgroup per (graph, sample chunk), tables streamed, block-wide scans.
// No Z_c is merged with another before the scan and a sample is drawn by one wave or one workgroup, so the bits of a result are
// a function of the graph, the cutset and the sample's uniforms alone.  Every scalar a workgroup or wave branches on comes out
// of a reduction, a ballot or wave-uniform memory and has the same bits in every thread of it.
// A LISTED call (N > 0, the header's listed mode) runs the same five kernels over the caller's list of cutset states: a walker's
// c is then the index of a list entry, its weight Z_c exp(-log_q) (weighted() of csrc/mlbp_cutset_plan.h) and its states the
// entry's row of configs -- the weights kernels in a loop of their own (ListedStates, X64Packed), the scan with n = N and the
// sum of squares for ess, the draw kernels reading the drawn entry's row.
// No device-side mutable globals: everything comes through SampleDev.
#include <hip/hip_runtime.h>

#include "../../include/mlbp_exactsample.h"
#include "../../include/mlbp_cutsetis.h"    // MLBP_CUTSETIS_MAX_ABS_LOG_Q: the range of a list's log_q
#define MLBP_GRAPH_NO_SWEEPS                // this library runs no sweep program
#include "../csrc/mlbp_graph_device.h"
#include "../csrc/mlbp_graph_host.h"
#include "../csrc/mlbp_cutset_plan.h"
#include "../csrc/mlbp_cutset_walk.h"
#include "../csrc/mlbp_draw_device.h"

namespace {

using namespace mlbp_graph;

constexpr int HEAD = MLBP_EXACTSAMPLE_HEAD;
constexpr double LN2 = 0.693147180559945309417232121458;

struct SampleDev : WalkDev {                 // chunks: of the pass the copy is handed to
  const double* uniforms;
  double* zc;                                // [B][n_configs][2] Z_c as (mantissa, exponent)
  double* scan;                              // [B][n_configs] W_c
  double* head;                              // [B][HEAD] {E, W_last, usable, listed: the sum of w^2 under E}
  int32_t* samples; double* logp; double* log_z; double* score;
  int32_t S;
  int32_t listed;                            // a listed call: n_configs is N, and the four below are the caller's; else 0 and NULL
  const int32_t* configs;                    // [B][N][n_cut], NULL without cutset variables
  const double* log_q;                       // [B][N]
  int32_t* entry; double* ess;               // optional [S][B], [B]
};

// The row of list entry i of graph g (a listed call with cutset variables).
__device__ __forceinline__ const_i32p listed_row(const SampleDev& d, int g, int i) {
  return as_const(d.configs) + ((size_t)g * d.n_configs + i) * d.n_cut;
}

// The states of the drawn configuration in the generic draw kernel: the row of the drawn entry (a listed call), else c's digits.
// One call site of the walk for both: a second one cost the kernel a wave of occupancy (98 vector registers against 96).
struct DrawnStates {
  const_i32p row; int c, X;
  __device__ __forceinline__ int operator()(int q) const { return row ? row[q] : GenericCode{c, X}(q); }
};

// An entry that cannot be walked -- a state outside [0, X), a log_q out of range -- is never walked: its weight has a NaN
// mantissa, which the scan passes on to the whole graph.
__device__ __forceinline__ Scaled unwalked() { return {__builtin_nan(""), 0}; }

__device__ __forceinline__ bool log_q_ok(double lq) { return fabs(lq) <= MLBP_CUTSETIS_MAX_ABS_LOG_Q; }     // false for a NaN

// w_c: the mantissa of Z_c under the graph's exponent E.
__device__ __forceinline__ double weight_of(const double* zc, int c, int E) {
  return ldexp(zc[2 * c], max((int)zc[2 * c + 1] - E, MIN_SHIFT));
}

// The draw rule on the scanned weights (they never decrease): the lowest c with W_c > thr; when there is none, the lowest c
// with W_c = W_last, which is the highest c of positive weight.  Always in [0, n).
__device__ __forceinline__ int find_config(const double* W, int n, double thr, double last) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (W[mid] > thr) hi = mid; else lo = mid + 1;
  }
  if (lo < n) return lo;
  lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (W[mid] >= last) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The configuration of sample `u` -- of a listed call: the index of the list entry -- and its log-probability; with
// n_cut == 0 the one empty configuration (entry 0 of a list).
__device__ __forceinline__ int draw_config(const SampleDev& d, int g, double u0, double& logp) {
  logp = 0.0;
  if (d.n_cut == 0) return 0;
  const double* head = d.head + (size_t)g * HEAD;
  const double last = head[1];
  const int c = find_config(d.scan + (size_t)g * d.n_configs, d.n_configs, u0 * last, last);
  logp = log(weight_of(d.zc + (size_t)g * d.n_configs * 2, c, (int)head[0]) / last);
  return c;
}

// A graph that cannot be drawn from: -1 / NaN for sample s.  By one wave (X = 64) or the workgroup; `first`, `step`: its threads.
__device__ __forceinline__ void refuse_sample(const SampleDev& d, int g, int s, int first, int step) {
  const size_t at = (size_t)s * d.B + g;
  for (int v = first; v < d.n_vars; v += step) d.samples[at * d.n_vars + v] = -1;
  if (first == 0) {
    d.logp[at] = __builtin_nan("");
    if (d.score) d.score[at] = __builtin_nan("");
    if (d.entry) d.entry[at] = -1;
  }
}

// The log-potential of the assignment xs (LDS or memory, visible to this wave), by one wave: every lane returns it.
__device__ __forceinline__ double wave_score(const SampleDev& d, const_i32p pav, const_i32p uvar, int g, const int* xs, int lane) {
  const size_t X = (size_t)d.X;
  double sc = 0.0;
  for (int p = lane; p < d.P; p += 64) {
    const int i = xs[pav[2 * p]], j = xs[pav[2 * p + 1]];
    sc += log(d.pair_tables[(size_t)d.pair_tab[(size_t)g * d.P + p] * X * X + (size_t)i * X + j]);
  }
  for (int u = lane; u < d.U; u += 64) sc += log(d.unary_tables[(size_t)d.unary_tab[(size_t)g * d.U + u] * X + xs[uvar[u]]]);
  return wave_sum(sc);
}

// ---- the weights pass: every Z_c of a chunk's configurations --------------------------------------------------
__global__ __launch_bounds__(WG) void exactsample_weights_generic_kernel(SampleDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  Generic G;
  generic_open(G, d, g);
  generic_carve(G, d, g, k, smem);
  generic_setup(G);
  double* out = d.zc + (size_t)g * d.n_configs * 2;
  if (d.listed) {                                              // a listed call: its own loop, the exact one below is as it was
    const double* log_q = d.log_q + (size_t)g * d.n_configs;
    for (int i = k; i < d.n_configs; i += d.chunks) {
      const const_i32p row = listed_row(d, g, i);              // not read without cutset variables
      const double lq = log_q[i];
      bool ok = log_q_ok(lq);                                  // the same in every thread: the row's address is
      for (int q = 0; q < d.n_cut; ++q) ok &= (unsigned)row[q] < (unsigned)d.X;
      const Scaled z = ok ? weighted(generic_up<SumAlg>(G, ListedStates{row}, nullptr), lq) : unwalked();
      if (t == 0) {
        out[2 * i] = z.m;
        out[2 * i + 1] = (double)z.e;
      }
    }
    return;
  }
  for (int c = k; c < d.n_configs; c += d.chunks) {
    const Scaled z = generic_up<SumAlg>(G, c, nullptr);
    if (t == 0) {
      out[2 * c] = z.m;
      out[2 * c + 1] = (double)z.e;
    }
  }
}

__global__ __launch_bounds__(WG) void exactsample_weights_x64_kernel(SampleDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  X64 W;
  x64_open(W, d, g, smem);
  double* out = d.zc + (size_t)g * d.n_configs * 2;
  if (d.listed) {                                              // a listed call: its own loop, the exact one below is as it was
    const double* log_q = d.log_q + (size_t)g * d.n_configs;
    for (int i = 4 * k + wave; i < d.n_configs; i += 4 * d.chunks) {
      const int packed = lane < d.n_cut ? listed_row(d, g, i)[lane] : 0;       // lane q: the state of cut position q
      const double lq = log_q[i];
      const bool ok = !__any((unsigned)packed >= 64u) && log_q_ok(lq);         // the same in every lane
      const Scaled z = ok ? weighted(x64_up<SumAlg, false>(W, X64Packed{packed}), lq) : unwalked();
      if (lane == 0) {
        out[2 * i] = z.m;
        out[2 * i + 1] = (double)z.e;
      }
    }
    return;
  }
  for (int c = 4 * k + wave; c < d.n_configs; c += 4 * d.chunks) {
    const Scaled z = x64_up<SumAlg, false>(W, c);
    if (lane == 0) {
      out[2 * c] = z.m;
      out[2 * c + 1] = (double)z.e;
    }
  }
}

// ---- the scan: a graph's Z_c -> E, W_c, log Z ------------------------------------------------------------------
// SEGMENTED, as the header states it: thread t owns configurations [t L, (t + 1) L).  Of a listed call: the entries' weights,
// n = N, and ess from the sum of their squares under the same E -- a thread's segment left to right, the segments in order.
__global__ __launch_bounds__(WG) void exactsample_scan_kernel(SampleDev d) {
  __shared__ double seg[WG];
  __shared__ double scratch[8];
  const int g = blockIdx.x, t = threadIdx.x, n = d.n_configs;
  double* head = d.head + (size_t)g * HEAD;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) {
    if (t == 0) {
      head[0] = 0.0; head[1] = __builtin_nan(""); head[2] = 0.0; head[3] = 0.0;
      if (d.log_z) d.log_z[g] = __builtin_nan("");
      if (d.ess) d.ess[g] = __builtin_nan("");
    }
    return;
  }
  const double* zc = d.zc + (size_t)g * n * 2;
  double* W = d.scan + (size_t)g * n;
  constexpr double NONE = -1e300;
  double em = NONE;                                            // the largest exponent of a positive Z_c
  for (int c = t; c < n; c += WG)
    if (zc[2 * c] > 0.0) em = fmax(em, zc[2 * c + 1]);
  em = block_max(em, scratch);
  const int E = em > NONE ? (int)em : 0;
  const int L = (n + WG - 1) / WG, lo = min(n, t * L), hi = min(n, lo + L);
  double tot = 0.0;
  for (int c = lo; c < hi; ++c) tot += weight_of(zc, c, E);
  seg[t] = tot;
  __syncthreads();
  double off = 0.0;
  for (int s = 0; s < t; ++s) off += seg[s];
  double local = 0.0;
  for (int c = lo; c < hi; ++c) {
    local += weight_of(zc, c, E);
    W[c] = off + local;
  }
  double s2 = 0.0;
  if (d.listed) {                                              // the same in every thread: the barriers are reached by all
    double sq = 0.0;
    for (int c = lo; c < hi; ++c) {
      const double w = weight_of(zc, c, E);
      sq = fma(w, w, sq);
    }
    __syncthreads();                                           // seg: read above by every thread
    seg[t] = sq;
    __syncthreads();
    if (t == WG - 1)
      for (int s = 0; s < WG; ++s) s2 += seg[s];
  }
  if (t != WG - 1) return;
  const double last = off + tot;                               // = W[n - 1]: the empty segments behind it add nothing
  head[0] = (double)E;
  head[1] = last;
  head[2] = (last > 0.0 && last < __builtin_huge_val()) ? 1.0 : 0.0;
  head[3] = s2;
  if (d.listed) {                                              // log_z_hat: the mean weight; a NaN weight has made `last` a NaN
    if (d.log_z) d.log_z[g] = last == 0.0 ? -__builtin_huge_val() : fma((double)E, LN2, log(last / (double)n));
    if (d.ess) d.ess[g] = last == 0.0 ? 0.0 : last * last / s2;
    return;
  }
  if (d.log_z) d.log_z[g] = last == 0.0 ? -__builtin_huge_val() : fma((double)E, LN2, log(last));
}

// ---- X = 64: a wave per sample -------------------------------------------------------------------------------
// The wave scan and the draw rule on a wave's vector: wave_scan, wave_draw of csrc/mlbp_draw_device.h.
__global__ __launch_bounds__(WG) void exactsample_draw_x64_kernel(SampleDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n_vars = d.n_vars, step = 4 * d.chunks;
  if (d.head[(size_t)g * HEAD + 2] == 0.0) {                   // Z is zero or no finite number, or a table index is out of range
    for (int s = 4 * k + wave; s < d.S; s += step) refuse_sample(d, g, s, lane, 64);
    return;
  }
  X64 W;
  x64_open(W, d, g, smem);
  int* xi = reinterpret_cast<int*>(W.dn);                      // this wave's: the drawn states, for the score
  for (int s = 4 * k + wave; s < d.S; s += step) {
    const size_t at = (size_t)s * d.B + g;
    const double* u = d.uniforms + at * n_vars;
    double logp;
    const int c = draw_config(d, g, u[0], logp);
    if (lane == 0 && d.entry) d.entry[at] = c;
    int xs = 0;                                                // lane v: the state of variable v (n_vars <= 12 on this kernel)
    if (d.configs) {                                           // a listed call: the entry's row, lane q the state of position q;
      const int packed = lane < d.n_cut ? listed_row(d, g, c)[lane] : 0;       // a drawn entry has a weight, so a row in range
      x64_up<SumAlg, true>(W, X64Packed{packed});
      for (int q = 0; q < d.n_cut; ++q) {
        const int sq = __builtin_amdgcn_readlane(packed, q);
        if (lane == W.pl.cutset[q]) xs = sq;
      }
    } else {
      x64_up<SumAlg, true>(W, c);                              // bel: every free variable's vector on the way up
      for (int q = 0; q < d.n_cut; ++q)
        if (lane == W.pl.cutset[q]) xs = x64_state(q, c);
    }
    for (int i = W.n_free - 1; i >= 0; --i) {
      const int v = W.pl.order[i], p = W.pl.parent[2 * v];
      double b = W.bel[(size_t)v * 64 + lane];
      if (p >= 0) {
        const int sp = __builtin_amdgcn_readlane(xs, W.pl.parent[2 * v + 1]);
        const double* tab = W.tabs + (size_t)W.pl.fslot[p] * 64 * ROW;
        b *= W.pl.pav[2 * p] == v ? tab[lane * ROW + sp] : tab[sp * ROW + lane];
      }
      double num, total;
      const int x = wave_draw(b, u[d.n_cut + (W.n_free - 1 - i)], lane, num, total);
      logp += log(num / total);
      if (lane == v) xs = x;
    }
    if (lane < n_vars) {
      d.samples[at * n_vars + lane] = xs;
      xi[lane] = xs;
    }
    if (lane == 0) d.logp[at] = logp;
    if (d.score) {
      const double sc = wave_score(d, W.pl.pav, W.pl.uvar, g, xi, lane);
      if (lane == 0) d.score[at] = sc;
    }
  }
}

// ---- any X: a workgroup per sample -----------------------------------------------------------------------------
// The segmented block scan and the draw rule on a vector in LDS: block_min_max, block_draw of csrc/mlbp_draw_device.h.
__global__ __launch_bounds__(WG) void exactsample_draw_generic_kernel(SampleDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X, g = blockIdx.x, k = blockIdx.y, t = threadIdx.x, n_vars = d.n_vars;
  if (d.head[(size_t)g * HEAD + 2] == 0.0) {                   // Z is zero or no finite number, or a table index is out of range
    for (int s = k; s < d.S; s += d.chunks) refuse_sample(d, g, s, t, WG);
    return;
  }
  Generic G;
  generic_open(G, d, g);
  generic_carve(G, d, g, k, smem);
  const int Xp = G.Xp;
  generic_setup(G);
  int* xs = reinterpret_cast<int*>(G.acc);                     // [n_vars] the drawn states: the walk without its pass back leaves
  double* seg = G.excl;                                        // acc and excl to the library
  for (int s = k; s < d.S; s += d.chunks) {
    const size_t at = (size_t)s * d.B + g;
    const double* u = d.uniforms + at * n_vars;
    double logp;
    const int c = draw_config(d, g, u[0], logp);
    if (t == 0 && d.entry) d.entry[at] = c;
    generic_up<SumAlg>(G, DrawnStates{d.configs ? listed_row(d, g, c) : nullptr, c, X}, nullptr);   // bel: every free
                                                               // variable's vector on the way up; st: c's digits or the entry's row
    if (t < d.n_cut) xs[G.pl.cutset[t]] = G.st[t];
    __syncthreads();
    for (int i = d.n_free - 1; i >= 0; --i) {
      const int v = G.pl.order[i], p = G.pl.parent[2 * v];
      const double* bv = G.bel + (size_t)v * Xp;
      if (p < 0) {
        for (int j = t; j < X; j += WG) G.raw[j] = bv[j];
      } else {
        const int sp = xs[G.pl.parent[2 * v + 1]];
        const double* T = G.pair_tables + (size_t)G.ptab[p] * G.XX;
        const int te = G.texp[p];
        if (G.pl.pav[2 * p] == v)
          for (int j = t; j < X; j += WG) G.raw[j] = bv[j] * ldexp(T[(size_t)j * X + sp], -te);
        else
          for (int j = t; j < X; j += WG) G.raw[j] = bv[j] * ldexp(T[(size_t)sp * X + j], -te);
      }
      __syncthreads();
      double num, total;
      const int x = block_draw(G.raw, X, u[d.n_cut + (d.n_free - 1 - i)], seg, G.scratch, num, total);
      logp += log(num / total);
      if (t == 0) xs[v] = x;
      __syncthreads();
    }
    for (int v = t; v < n_vars; v += WG) d.samples[at * n_vars + v] = xs[v];
    if (t == 0) d.logp[at] = logp;
    if (d.score && t < 64) {
      const double sc = wave_score(d, G.pl.pav, G.pl.uvar, g, xs, t);
      if (t == 0) d.score[at] = sc;
    }
    __syncthreads();                                           // xs is written again by the next sample
  }
}

// ---- host ----------------------------------------------------------------------------------------
thread_local int g_last_kernel = MLBP_EXACTSAMPLE_KERNEL_NONE;
static_assert(MLBP_EXACTSAMPLE_KERNEL_X64 == WALK_X64 && MLBP_EXACTSAMPLE_KERNEL_GENERIC == WALK_GENERIC, "the shared host core numbers the kernels");

// Cd of the draw pass: the X = 64 kernel's four waves take a sample each.
int draw_chunks(int which, int32_t B, int32_t S) {
  return walk_chunks(B, which == WALK_X64 ? (S + 3) / 4 : S, MLBP_CUTSET_MIN_WORKGROUPS);
}

// The header's workspace formula over n walked entries: the configurations of the exact call, the list's of a listed one.
int64_t workspace_of(int which, int32_t B, int32_t S, int64_t n, int32_t X, int32_t n_vars, int32_t P, int32_t U) {
  if (B <= 0) return fail(MLBP_EINVAL, "chunks: B = %d, n = %lld", B, (long long)n);
  const int cw = walk_chunks(B, (int32_t)n, MLBP_CUTSET_MIN_WORKGROUPS);
  const int cd = draw_chunks(which, B, S);
  const bool spill = which == WALK_GENERIC && generic_lds_bytes(n_vars, P, U, X) > MLBP_CUTSET_GENERIC_LDS_BYTES;
  return ((int64_t)B * n * 3 + (int64_t)B * HEAD + (spill ? (int64_t)B * (cw > cd ? cw : cd) * vector_doubles(n_vars, X) : 0)) * 8;
}

}  // namespace

extern "C" {

const char* mlbp_exactsample_arch(void) { return "gfx950"; }
const char* mlbp_exactsample_last_error(void) { return g_last_error.c_str(); }
int mlbp_exactsample_last_kernel(void) { return g_last_kernel; }

int mlbp_exactsample_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest) {
  return pick_walk_kernel(X, n_vars, P, U, n_forest);
}

int mlbp_exactsample_chunks(int32_t B, int32_t n) {
  if (B <= 0 || n <= 0) return fail(MLBP_EINVAL, "chunks: B = %d, n = %d", B, n);
  return walk_chunks(B, n, MLBP_CUTSET_MIN_WORKGROUPS);
}

int64_t mlbp_exactsample_workspace_bytes(int32_t B, int32_t S, int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest,
                                         int32_t n_cut) {
  const int which = mlbp_exactsample_pick_kernel(X, n_vars, P, U, n_forest);
  if (which < 0) return which;
  if (n_cut < 0 || n_cut > n_vars) return fail(MLBP_EINVAL, "workspace: n_cut = %d with %d variables", n_cut, n_vars);
  if (S <= 0) return fail(MLBP_EINVAL, "workspace: S = %d samples", S);
  const int64_t n_configs = count_configs(X, n_cut);
  if (n_configs < 0) return too_many_configs(X, n_cut);
  return workspace_of(which, B, S, n_configs, X, n_vars, P, U);
}

int mlbp_exactsample_check_plan(const int32_t* plan, int32_t n_words, int32_t X) { return check_packed_plan(plan, n_words, X); }

int mlbp_exactsample_f64(const mlbp_exactsample_args* a, void* stream) {
  g_last_kernel = MLBP_EXACTSAMPLE_KERNEL_NONE;
  const bool listed = a && a->N > 0;                           // the header's listed mode: the walk's entries are the list's
  int64_t n_configs = listed ? a->N : 0;
  const int which = check_walk_args(a, mlbp_exactsample_pick_kernel, [](const mlbp_exactsample_args* a) {
    if (a->S <= 0) return fail(MLBP_EINVAL, "bad sizes: S = %d samples", a->S);
    if (!a->uniforms) return fail(MLBP_EINVAL, "uniforms is NULL");
    if (!a->samples || !a->logp) return fail(MLBP_EINVAL, "samples or logp is NULL");
    if (a->N < 0 || a->N > MLBP_EXACTSAMPLE_MAX_LISTED)
      return fail(MLBP_EINVAL, "N = %d: a list holds 1 to %d configurations (0: the exact call)", a->N, MLBP_EXACTSAMPLE_MAX_LISTED);
    if (a->N > 0 && a->n_cut > 0 && !a->configs) return fail(MLBP_EINVAL, "configs is NULL in a listed call with cutset variables");
    if (a->N > 0 && !a->log_q) return fail(MLBP_EINVAL, "log_q is NULL in a listed call");
    return (int)MLBP_OK;
  }, &n_configs, listed);
  if (which < 0) return which;
  const int cw = mlbp_exactsample_chunks(a->B, (int32_t)n_configs);
  if (cw < 0) return cw;
  const int cd = draw_chunks(which, a->B, a->S);
  const int64_t need = listed ? workspace_of(which, a->B, a->S, n_configs, a->X, a->n_vars, a->P, a->U)
                              : mlbp_exactsample_workspace_bytes(a->B, a->S, a->X, a->n_vars, a->P, a->U, a->n_forest, a->n_cut);
  if (int e = check_walk_workspace(a, need)) return e;
  if (int e = check_device("libmlbp_exactsample.so")) return e;
  SampleDev d;
  fill_walk_dev(d, a, n_configs, cw, which);
  d.uniforms = a->uniforms;
  d.zc = a->workspace;
  d.scan = d.zc + (int64_t)a->B * n_configs * 2;
  d.head = d.scan + (int64_t)a->B * n_configs;
  d.samples = a->samples; d.logp = a->logp; d.log_z = a->log_z; d.score = a->score;
  d.S = a->S;
  d.listed = listed;                                           // N == 0: the four fields are not looked at, whatever they hold
  d.configs = listed && a->n_cut > 0 ? a->configs : nullptr;
  d.log_q = listed ? a->log_q : nullptr;
  d.entry = listed ? a->entry : nullptr;
  d.ess = listed ? a->ess : nullptr;
  double* spill = d.head + (int64_t)a->B * HEAD;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  SampleDev dd = d;                                            // the draw pass: its own number of chunks
  dd.chunks = cd;
  if (which == MLBP_EXACTSAMPLE_KERNEL_X64) {
    const size_t lds = (size_t)x64_lds_bytes(a->n_vars, a->P, a->U, a->n_forest);
    if (int e = grant_x64_lds((const void*)exactsample_weights_x64_kernel, 0, MLBP_CUTSET_X64_LDS_BYTES)) return e;
    if (int e = grant_x64_lds((const void*)exactsample_draw_x64_kernel, 1, MLBP_CUTSET_X64_LDS_BYTES)) return e;
    hipLaunchKernelGGL(exactsample_weights_x64_kernel, dim3(a->B, cw), dim3(WG), lds, st, d);
    if (int e = launched("weights")) return e;
    hipLaunchKernelGGL(exactsample_scan_kernel, dim3(a->B), dim3(WG), 0, st, d);
    if (int e = launched("scan")) return e;
    hipLaunchKernelGGL(exactsample_draw_x64_kernel, dim3(a->B, cd), dim3(WG), lds, st, dd);
  } else {
    const size_t lds = generic_walk_lds(d, spill);
    dd.vectors = d.vectors;
    hipLaunchKernelGGL(exactsample_weights_generic_kernel, dim3(a->B, cw), dim3(WG), lds, st, d);
    if (int e = launched("weights")) return e;
    hipLaunchKernelGGL(exactsample_scan_kernel, dim3(a->B), dim3(WG), 0, st, d);
    if (int e = launched("scan")) return e;
    hipLaunchKernelGGL(exactsample_draw_generic_kernel, dim3(a->B, cd), dim3(WG), lds, st, dd);
  }
  if (int e = launched("draw")) return e;
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
