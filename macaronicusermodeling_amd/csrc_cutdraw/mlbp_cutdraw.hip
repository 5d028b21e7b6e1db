// libmlbp_cutdraw.so: a proposal for cutset importance sampling drawn from held BP messages (include/mlbp_cutdraw.h), gfx950
// only, float64.  Per entry and cut position: the product of the position's base messages, times the row or column of every
// pairwise table that reaches an earlier position at the state drawn there, rescaled by a power of two after every
// multiplication, then the draw rule of csrc/mlbp_draw_device.h.  No sweep, no contraction, no workspace.
//
// Two kernels, chosen from X by mlbp_cutdraw_pick_kernel:
//   cutdraw_x64_kernel      X = 64, lane = state: the workgroup forms every position's base product once (wave w those of
//                           positions w, w + 4, ...) into static LDS, one barrier; then every WAVE draws entries of its own.
//                           The drawn states of an entry live in one register, lane q the state of position q.
//   cutdraw_generic_kernel  any X in [2, 1024]: the workgroup draws one entry at a time, v in static LDS, thread t the
//                           states t, t + 256, ...; base messages and table rows are streamed.
// Workgroup (g, k) of the generic kernel takes entries k, k + chunks, ... of graph g; wave w of workgroup (g, k) of the X = 64
// kernel takes 4 k + w, 4 k + w + 4 chunks, ...  Every scalar a workgroup or wave branches on comes out of a reduction, a
// ballot, LDS behind a barrier or wave-uniform memory and has the same bits in every thread of it.  An entry is drawn by one
// wave or one workgroup from its own uniforms, so its bits do not depend on B, N or the grid.
// No device-side mutable globals: everything comes through DrawDev.
#include <hip/hip_runtime.h>

#include "../../include/mlbp_cutdraw.h"
#define MLBP_GRAPH_NO_SWEEPS                // this library runs no sweep program
#include "../csrc/mlbp_graph_device.h"
#include "../csrc/mlbp_graph_host.h"
#include "../csrc/mlbp_draw_device.h"

namespace {

using namespace mlbp_graph;

constexpr int HEADER = MLBP_CUTDRAW_PLAN_HEADER;
constexpr int MAX_CUT = MLBP_CUTDRAW_MAX_CUT;
constexpr int MAX_X = MLBP_CUTDRAW_MAX_X;
constexpr int BATCH = 8;                     // rows or columns of one position in flight together (X = 64 kernel)

struct DrawDev {
  const int32_t* plan;
  const double* pair_tables; const int32_t* pair_tab;
  const double* msgs; const double* uniforms; const int32_t* configs_in;
  int32_t* configs; double* log_q;
  int32_t B, X, n_msgs, P, n_cut, n_pair_tables, N, chunks;
};

// The sections of the packed plan behind its header; n_base is base_off[n_cut].
struct Sections { const_i32p cutset, base_off, base_slots, row_off, rows; };

__device__ __forceinline__ Sections carve(const int32_t* plan, int n_cut) {
  Sections s;
  const const_i32p w = as_const(plan);
  s.cutset = w + HEADER;
  s.base_off = s.cutset + n_cut;
  s.base_slots = s.base_off + n_cut + 1;
  s.row_off = s.base_slots + s.base_off[n_cut];
  s.rows = s.row_off + n_cut + 1;
  return s;
}

// The exponent e that brings a positive normal x to x * 2^-e in [1, 2) (-1023 for a subnormal x); 0 for zero, a negative
// number, NaN and +inf: the scaling is then skipped.
__device__ __forceinline__ int exp_of(double x) {
  if (!(x > 0.0) || x == __builtin_huge_val()) return 0;
  return ((__double2hiint(x) >> 20) & 0x7ff) - 1023;
}

// ln(num / total) of one position; -inf from an empty vector.
__device__ __forceinline__ double log_term(double num, double total) {
  return total == 0.0 ? -__builtin_huge_val() : log(num / total);
}

// A graph whose table indices are out of range: -1 / NaN for its entries first, first + step, ...; `lead`: writes log_q.
__device__ __forceinline__ void refuse_graph(const DrawDev& d, int g, int first, int step, int sub, int n_sub, bool lead) {
  for (int i = first; i < d.N; i += step) {
    const size_t at = (size_t)g * d.N + i;
    if (!d.configs_in)
      for (int q = sub; q < d.n_cut; q += n_sub) d.configs[at * d.n_cut + q] = -1;
    if (lead) d.log_q[at] = __builtin_nan("");
  }
}

// v times 2^-e, e the exponent of the wave's largest entry (lane = state).
__device__ __forceinline__ double wave_rescale(double v) {
  const int e = exp_of(wave_max(v));
  return e != 0 ? ldexp(v, -e) : v;
}

// ---- X = 64: a wave per entry ---------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void cutdraw_x64_kernel(DrawDev d) {
  __shared__ double base[MAX_CUT][64];
  const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x, lane = t & 63, N = d.N, n_cut = d.n_cut;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);     // the entry's address is wave-uniform: scalar loads
  const int step = 4 * d.chunks;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, nullptr, 0, 0, g)) {
    refuse_graph(d, g, 4 * k + wave, step, lane, 64, lane == 0);
    return;
  }
  const Sections pl = carve(d.plan, n_cut);
  const double* msg = d.msgs + (size_t)g * d.n_msgs * 64;
  for (int q = wave; q < n_cut; q += 4) {                      // the prologue: every position's base product, once
    const int lo = pl.base_off[q], hi = pl.base_off[q + 1];
    double v = lo < hi ? msg[(size_t)pl.base_slots[lo] * 64 + lane] : 1.0;
    for (int b = lo + 1; b < hi; ++b) v = wave_rescale(v * msg[(size_t)pl.base_slots[b] * 64 + lane]);
    base[q][lane] = v;
  }
  __syncthreads();                                             // the only workgroup barrier

  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P;
  const const_f64p uni = as_const_f64(d.uniforms);
  const bool given = d.configs_in != nullptr;
  const size_t gN = (size_t)g * N;
  for (int i = 4 * k + wave; i < N; i += step) {
    const size_t at = (gN + i) * n_cut;
    int xs = 0;                                                // lane q: the state of position q
    if (given) {
      if (lane < n_cut) xs = d.configs_in[at + lane];
      if (__any((unsigned)xs >= 64u)) {                        // a state outside [0, X): the entry is not computed
        if (lane == 0) d.log_q[gN + i] = __builtin_nan("");
        continue;
      }
    }
    double lq = 0.0;
    for (int q = 0; q < n_cut; ++q) {
      double v = base[q][lane];
      const int lo = pl.row_off[q], hi = pl.row_off[q + 1];
      for (int r = lo; r < hi; r += BATCH) {
        double f[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {                      // the loads of a batch are independent: issued together
          if (r + u < hi) {
            const int p = pl.rows[3 * (r + u)], c = __builtin_amdgcn_readlane(xs, pl.rows[3 * (r + u) + 1]);
            const double* T = d.pair_tables + (size_t)ptab[p] * 4096;
            f[u] = pl.rows[3 * (r + u) + 2] ? T[c * 64 + lane] : T[lane * 64 + c];
          }
        }
#pragma unroll
        for (int u = 0; u < BATCH; ++u)
          if (r + u < hi) v = wave_rescale(v * f[u]);
      }
      double num, total;
      const int x = wave_draw(v, given ? 0.0 : uni[at + q], lane, num, total);
      if (given) num = read_lane(v, __builtin_amdgcn_readlane(xs, q));
      else if (lane == q) xs = x;
      lq += log_term(num, total);
    }
    if (!given && lane < n_cut) d.configs[at + lane] = xs;
    if (lane == 0) d.log_q[gN + i] = lq;
  }
}

// ---- any X: a workgroup per entry ------------------------------------------------------------------------------
// Max over the workgroup of the threads' values, the same bits in every thread (a NaN is passed over); two barriers.
__device__ __forceinline__ double block_max(double v, double* scratch /*[4]*/) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(scratch[0], scratch[1]), fmax(scratch[2], scratch[3]));
}

// v[j] *= factor(j) for the states of this thread, then v times 2^-e, e the exponent of the largest entry.  A thread touches
// its own states only; reached by every thread.
template <class Factor>
__device__ __forceinline__ void block_multiply(double* v, int X, double* scratch, Factor factor) {
  double m = 0.0;
  for (int j = threadIdx.x; j < X; j += WG) {
    const double x = v[j] * factor(j);
    v[j] = x;
    m = fmax(m, x);
  }
  const int e = exp_of(block_max(m, scratch));
  if (e != 0)
    for (int j = threadIdx.x; j < X; j += WG) v[j] = ldexp(v[j], -e);
}

__global__ __launch_bounds__(WG) void cutdraw_generic_kernel(DrawDev d) {
  __shared__ double v[MAX_X];
  __shared__ double seg[WG];
  __shared__ double scratch[8];
  __shared__ int st[MAX_CUT];                                  // the entry's states, by position
  const int X = d.X, g = blockIdx.x, k = blockIdx.y, t = threadIdx.x, N = d.N, n_cut = d.n_cut;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, nullptr, 0, 0, g)) {
    refuse_graph(d, g, k, d.chunks, t, WG, t == 0);
    return;
  }
  const Sections pl = carve(d.plan, n_cut);
  const double* msg = d.msgs + (size_t)g * d.n_msgs * X;
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P;
  const const_f64p uni = as_const_f64(d.uniforms);
  const bool given = d.configs_in != nullptr;
  const size_t gN = (size_t)g * N, XX = (size_t)X * X;
  for (int i = k; i < N; i += d.chunks) {
    const size_t at = (gN + i) * n_cut;
    if (given) {
      if (t < n_cut) st[t] = d.configs_in[at + t];
      __syncthreads();
      bool ok = true;
      for (int q = 0; q < n_cut; ++q) ok &= (unsigned)st[q] < (unsigned)X;
      if (!ok) {                                               // a state outside [0, X): the entry is not computed
        if (t == 0) d.log_q[gN + i] = __builtin_nan("");
        __syncthreads();                                       // st is written again by the next entry
        continue;
      }
    }
    double lq = 0.0;
    for (int q = 0; q < n_cut; ++q) {
      const int blo = pl.base_off[q], bhi = pl.base_off[q + 1];
      const double* first = msg + (size_t)(blo < bhi ? pl.base_slots[blo] : 0) * X;
      for (int j = t; j < X; j += WG) v[j] = blo < bhi ? first[j] : 1.0;
      for (int b = blo + 1; b < bhi; ++b) {
        const double* m = msg + (size_t)pl.base_slots[b] * X;
        block_multiply(v, X, scratch, [&](int j) { return m[j]; });
      }
      for (int r = pl.row_off[q]; r < pl.row_off[q + 1]; ++r) {
        const size_t c = (size_t)st[pl.rows[3 * r + 1]];
        const double* T = d.pair_tables + (size_t)ptab[pl.rows[3 * r]] * XX;
        if (pl.rows[3 * r + 2]) block_multiply(v, X, scratch, [&](int j) { return T[c * X + j]; });
        else block_multiply(v, X, scratch, [&](int j) { return T[(size_t)j * X + c]; });
      }
      __syncthreads();                                         // v is read across the threads
      double num, total;
      const int x = block_draw(v, X, given ? 0.0 : uni[at + q], seg, scratch, num, total);
      if (given) num = v[st[q]];
      else if (t == 0) st[q] = x;
      lq += log_term(num, total);
      __syncthreads();                                         // st[q] before the next position reads it, v before it is written
    }
    if (!given && t < n_cut) d.configs[at + t] = st[t];
    if (t == 0) d.log_q[gN + i] = lq;
    __syncthreads();                                           // st is written again by the next entry
  }
}

// ---- host ----------------------------------------------------------------------------------------
thread_local int g_last_kernel = MLBP_CUTDRAW_KERNEL_NONE;

// Behind a launch: `what` names the kernel in the message.
int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MLBP_OK : fail(MLBP_EHIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

int check_x(int32_t X) {
  if (int e = check_states(X)) return e;
  if (X > MAX_X) return fail(MLBP_EUNSUPPORTED, "X = %d: at most %d states are supported", X, MAX_X);
  return MLBP_OK;
}

int too_many_cut(int32_t n_cut) {
  return fail(MLBP_EUNSUPPORTED, "n_cut = %d: at most %d cutset variables are supported", n_cut, MAX_CUT);
}

}  // namespace

extern "C" {

const char* mlbp_cutdraw_arch(void) { return "gfx950"; }
const char* mlbp_cutdraw_last_error(void) { return g_last_error.c_str(); }
int mlbp_cutdraw_last_kernel(void) { return g_last_kernel; }

int mlbp_cutdraw_pick_kernel(int32_t X) {
  if (int e = check_x(X)) return e;
  return X == 64 ? MLBP_CUTDRAW_KERNEL_X64 : MLBP_CUTDRAW_KERNEL_GENERIC;
}

int mlbp_cutdraw_chunks(int32_t B, int32_t N) {
  if (B <= 0 || N <= 0 || N > MLBP_CUTDRAW_MAX_LISTED)
    return fail(MLBP_EINVAL, "chunks: B = %d, N = %d (N in [1, %d])", B, N, MLBP_CUTDRAW_MAX_LISTED);
  const int32_t spread = (MLBP_CUTDRAW_MIN_WORKGROUPS + B - 1) / B;
  return N < spread ? N : spread;
}

int mlbp_cutdraw_check_plan(const int32_t* plan, int32_t n_words, int32_t X, int32_t n_msgs) {
  if (!plan) return fail(MLBP_EINVAL, "plan is NULL");
  if (int e = check_x(X)) return e;
  if (n_words < HEADER) return fail(MLBP_EINVAL, "plan: %d words, the header alone has %d", n_words, HEADER);
  const int n_vars = plan[0], P = plan[1], n_cut = plan[3], n_base = plan[4], n_rows = plan[5];
  if (n_vars <= 0 || P < 0 || plan[2] <= 0 || n_cut < 0 || n_base < 0 || n_rows < 0)
    return fail(MLBP_EINVAL, "plan: bad sizes (n_vars %d, P %d, n_msgs %d, n_cut %d, n_base %d, n_rows %d)", n_vars, P, plan[2], n_cut, n_base, n_rows);
  if (plan[2] != n_msgs) return fail(MLBP_EINVAL, "plan: made for %d message slots, the call has %d", plan[2], n_msgs);
  if (n_cut > MAX_CUT) return too_many_cut(n_cut);
  if (n_cut > n_vars) return fail(MLBP_EINVAL, "plan: n_cut = %d with %d variables", n_cut, n_vars);
  const int64_t want = (int64_t)HEADER + n_cut + 2 * ((int64_t)n_cut + 1) + n_base + 3 * (int64_t)n_rows;
  if (want != n_words) return fail(MLBP_EINVAL, "plan: %d words, but its sizes give %lld", n_words, (long long)want);
  const int32_t* cutset = plan + HEADER;
  const int32_t* base_off = cutset + n_cut;
  const int32_t* base_slots = base_off + n_cut + 1;
  const int32_t* row_off = base_slots + n_base;
  const int32_t* rows = row_off + n_cut + 1;
  for (int k = 0; k < n_cut; ++k) {
    if (cutset[k] < 0 || cutset[k] >= n_vars) return fail(MLBP_EINVAL, "plan: cutset[%d] = %d out of [0,%d)", k, cutset[k], n_vars);
    for (int j = 0; j < k; ++j)
      if (cutset[j] == cutset[k]) return fail(MLBP_EINVAL, "plan: variable %d is in the cutset twice", cutset[k]);
  }
  if (base_off[0] != 0 || row_off[0] != 0) return fail(MLBP_EINVAL, "plan: base_off[0] and row_off[0] must be 0");
  for (int k = 0; k < n_cut; ++k) {
    if (base_off[k + 1] < base_off[k] || base_off[k + 1] > n_base)
      return fail(MLBP_EINVAL, "plan: base_off not monotone or beyond the %d base slots at position %d", n_base, k);
    if (row_off[k + 1] < row_off[k] || row_off[k + 1] > n_rows)
      return fail(MLBP_EINVAL, "plan: row_off not monotone or beyond the %d rows at position %d", n_rows, k);
    for (int b = base_off[k]; b < base_off[k + 1]; ++b)
      if (base_slots[b] < 0 || base_slots[b] >= n_msgs)
        return fail(MLBP_EINVAL, "plan: position %d: message slot %d out of [0,%d)", k, base_slots[b], n_msgs);
    for (int r = row_off[k]; r < row_off[k + 1]; ++r) {
      const int p = rows[3 * r], j = rows[3 * r + 1], axis = rows[3 * r + 2];
      if (p < 0 || p >= P) return fail(MLBP_EINVAL, "plan: row %d: pair slot %d out of [0,%d)", r, p, P);
      if (j < 0 || j >= k) return fail(MLBP_EINVAL, "plan: row %d of position %d reads position %d: not an earlier one", r, k, j);
      if (axis != 0 && axis != 1) return fail(MLBP_EINVAL, "plan: row %d: axis %d is neither 0 nor 1", r, axis);
    }
  }
  if (base_off[n_cut] != n_base || row_off[n_cut] != n_rows)
    return fail(MLBP_EINVAL, "plan: base_off / row_off end at %d / %d, but %d base slots and %d rows", base_off[n_cut], row_off[n_cut], n_base, n_rows);
  return MLBP_OK;
}

int mlbp_cutdraw_f64(const mlbp_cutdraw_args* a, void* stream) {
  g_last_kernel = MLBP_CUTDRAW_KERNEL_NONE;
  if (!a) return fail(MLBP_EINVAL, "args is NULL");
  if (a->B <= 0 || a->n_msgs <= 0 || a->P < 0 || a->n_cut < 0)
    return fail(MLBP_EINVAL, "bad sizes: B %d, n_msgs %d, P %d, n_cut %d", a->B, a->n_msgs, a->P, a->n_cut);
  const int which = mlbp_cutdraw_pick_kernel(a->X);
  if (which < 0) return which;
  if (a->n_cut > MAX_CUT) return too_many_cut(a->n_cut);
  if (a->N <= 0 || a->N > MLBP_CUTDRAW_MAX_LISTED)
    return fail(MLBP_EINVAL, "N = %d: a list holds 1 to %d entries", a->N, MLBP_CUTDRAW_MAX_LISTED);
  if (!a->plan || a->plan_words < HEADER + 3 * (int64_t)a->n_cut + 2)
    return fail(MLBP_EINVAL, "plan is NULL or plan_words = %d below what n_cut = %d needs", a->plan_words, a->n_cut);
  if (a->P > 0 && (!a->pair_tables || !a->pair_tab || a->n_pair_tables <= 0))
    return fail(MLBP_EINVAL, "P = %d but pair_tables or pair_tab is NULL (or n_pair_tables <= 0)", a->P);
  if (!a->msgs) return fail(MLBP_EINVAL, "msgs is NULL");
  if (!a->log_q) return fail(MLBP_EINVAL, "log_q is NULL");
  if (a->n_cut > 0 && !a->configs_in && (!a->uniforms || !a->configs))
    return fail(MLBP_EINVAL, "uniforms or configs is NULL and no configs_in is given");
  if (int e = check_args_extent(a)) return e;
  const int chunks = mlbp_cutdraw_chunks(a->B, a->N);
  if (chunks < 0) return chunks;
  if (int e = check_device("libmlbp_cutdraw.so")) return e;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  if (a->n_cut == 0) {                                         // the one empty configuration: no kernel, log_q = 0
    const hipError_t e = hipMemsetAsync(a->log_q, 0, (size_t)a->B * a->N * sizeof(double), st);
    return e == hipSuccess ? MLBP_OK : fail(MLBP_EHIP, "clearing log_q failed: %s", hipGetErrorString(e));
  }
  DrawDev d;
  d.plan = a->plan; d.pair_tables = a->pair_tables; d.pair_tab = a->pair_tab;
  d.msgs = a->msgs; d.uniforms = a->uniforms; d.configs_in = a->configs_in; d.configs = a->configs; d.log_q = a->log_q;
  d.B = a->B; d.X = a->X; d.n_msgs = a->n_msgs; d.P = a->P; d.n_cut = a->n_cut; d.n_pair_tables = a->n_pair_tables; d.N = a->N;
  d.chunks = chunks;
  const dim3 grid(a->B, chunks);
  if (which == MLBP_CUTDRAW_KERNEL_X64) hipLaunchKernelGGL(cutdraw_x64_kernel, grid, dim3(WG), 0, st, d);
  else hipLaunchKernelGGL(cutdraw_generic_kernel, grid, dim3(WG), 0, st, d);
  if (int e = launched("cutdraw")) return e;
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
