// libmlbp_converge.so: sum-product sweeps to convergence with a per-graph residual and early exit (include/mlbp_converge.h),
// gfx950 only, float64.
//
// Two kernels, chosen from (X, n_msgs) by mlbp_converge_pick_kernel, both one workgroup of 256 threads per graph:
//   converge_x64_kernel<RESIDENT>  X = 64, four waves, messages in LDS for the whole launch -- the layout of sample_x64_kernel
//                                  (csrc_sample/mlbp_sample.hip) without the clamp and the draw: a pairwise table is split
//                                  over the 256 threads as 16 entries each, wave w owns rows 16w .. 16w+15, lane l holds, for
//                                  k = 0..7, the two entries of row 16w + 2k + (l >> 5) in columns 2(l & 31), +1.  RESIDENT
//                                  (P <= 3): all tables are loaded once per workgroup and stay in registers over every round;
//                                  otherwise the 16 entries are loaded per update (streamed).  The two contractions:
//                                    out = m^T.T : running sum over the thread's 8 rows for its two columns, the 8 partial
//                                                  vectors (4 waves x 2 row halves) meet in LDS and are added in a fixed order;
//                                    out = T.m   : per row the two products, then a sum over the 32 lanes of the row half on
//                                                  DPP and through scalar registers.
//                                  Wave 0 (lane = state) finishes every update: it has the old and the new message in hand and
//                                  keeps the running per-lane maximum of |new - old| in a register.
//   converge_generic_kernel        any X in [2, 1024]: messages in the caller's `msgs` in place, tables streamed, every thread
//                                  keeps the maximum over the entries it writes.  Correct first: the path nobody times.
// The stop decision is workgroup-uniform in both: at the end of a round the maximum is reduced and published through one LDS
// word, and EVERY thread reads that word behind a barrier before it decides to leave the round loop or to run the next round.
// No thread reaches a barrier that another thread of its workgroup has left behind.
// After the first round the X = 64 kernel skips the UNARY ops whose destination nothing else writes (unary_once_mask below): the
// bits and the residuals are those of running them.  The generic kernel runs every op of every round.
// No device-side mutable globals: everything comes through ConvergeDev.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mlbp_converge.h"
#include "../csrc/mlbp_device.h"

namespace {

using namespace mlbp_dev;

constexpr int WG = 256;

struct ConvergeDev {
  const double* pair_tables; const int32_t* pair_tab;
  const double* unary_tables; const int32_t* unary_tab;
  const int32_t* ops; const int32_t* srcs; const int32_t* sweeps;
  const int32_t* in_off; const int32_t* in_slots;
  double* msgs;
  int32_t* rounds; double* residual; double* marginals; double* history;
  double tol;
  int32_t n_sweeps, n_msgs, P, U, X, n_vars, n_pair_tables, n_unary_tables;
  int32_t init, max_rounds, n_ops;
};

// Sum over each row of 16 lanes, the same bits in every lane of the row (the first four steps of mlbp_dev::wave_sum).
__device__ __forceinline__ double row16_sum(double v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x141>(v);
  v += dpp_mov<0x140>(v);
  return v;
}

// Maximum over the 64 lanes of non-negative numbers (or +inf), the same bits in every lane: wave_sum's steps with fmax.
__device__ __forceinline__ double wave_max(double v) {
  v = fmax(v, dpp_mov<0xB1>(v));
  v = fmax(v, dpp_mov<0x4E>(v));
  v = fmax(v, dpp_mov<0x141>(v));
  v = fmax(v, dpp_mov<0x140>(v));
  return fmax(fmax(read_lane(v, 0), read_lane(v, 16)), fmax(read_lane(v, 32), read_lane(v, 48)));
}

// |new - old| of one entry (mlbp_converge.h step 2): an entry that is NaN before and after has not moved (0); NaN on one side
// only counts as +inf.
__device__ __forceinline__ double entry_delta(double fresh, double old) {
  const double d = fabs(fresh - old);
  if (d == d) return d;
  return (fresh != fresh && old != old) ? 0.0 : __builtin_huge_val();
}

// Which UNARY ops may be skipped after the first round (X = 64 kernel).  A UNARY op writes renorm(row u), a function of the
// launch's constant tables alone; if EVERY op of the program that names its destination slot is a UNARY op of the same unary
// slot u, the slot holds exactly that value from the first round's write on, and running the op again would store the same bits
// with delta 0.  The kernel derives this from the op list itself (the host check admits programs in which another op writes the
// slot, so nothing else could be trusted), in one pass: every op leaves its key -- u for a UNARY op, INT_MAX for any other kind --
// in the minimum and the maximum of its destination slot (LDS atomics on 2 n_msgs words of `scratch`, which the updates use
// only later); a slot qualifies when the two agree below INT_MAX.  Lane l of every wave then keeps bit k for op l + 64 k.  Every
// wave reads the same words, so the skip is workgroup-uniform.  Programs beyond 2048 ops skip nothing.  Three barriers, all of
// them reached by every thread.
constexpr int SKIP_MAX_OPS = 64 * 32;
__device__ __forceinline__ unsigned unary_once_mask(const ConvergeDev& d, int32_t* scratch /* LDS [2 n_msgs] */, int lane) {
  if (d.n_ops > SKIP_MAX_OPS || d.max_rounds < 2) return 0u;   // (uniform; a single round skips nothing)
  int32_t* lo = scratch;
  int32_t* hi = scratch + d.n_msgs;
  for (int s = threadIdx.x; s < d.n_msgs; s += WG) {
    lo[s] = 0x7fffffff;
    hi[s] = -1;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < d.n_ops; o += WG) {
    const int key = d.ops[4 * o] == MLBP_OP_UNARY ? d.ops[4 * o + 1] : 0x7fffffff;
    const int c = d.ops[4 * o + 3];
    atomicMin(&lo[c], key);
    atomicMax(&hi[c], key);
  }
  __syncthreads();
  unsigned mask = 0u;
  for (int k = 0; 64 * k < d.n_ops; ++k) {
    const int o = lane + 64 * k;
    if (o < d.n_ops && d.ops[4 * o] == MLBP_OP_UNARY) {
      const int c = d.ops[4 * o + 3];
      if (lo[c] == hi[c] && hi[c] != 0x7fffffff) mask |= 1u << k;
    }
  }
  __syncthreads();                                             // the words are free again
  return mask;
}

// Is op o (wave-uniform) marked in the masks?
__device__ __forceinline__ bool unary_once(unsigned mask, int o) {
  if (o >= SKIP_MAX_OPS) return false;
  return ((unsigned)__builtin_amdgcn_readlane((int)mask, o & 63) >> (o >> 6)) & 1u;
}

// Every table index of graph g is inside its table array (wave-uniform: scalar loads).
__device__ __forceinline__ bool graph_in_range(const ConvergeDev& d, int g) {
  bool ok = true;
  const const_i32p pt = as_const(d.pair_tab), ut = as_const(d.unary_tab);
  for (int p = 0; p < d.P; ++p) ok &= (unsigned)pt[(size_t)g * d.P + p] < (unsigned)d.n_pair_tables;
  for (int u = 0; u < d.U; ++u) ok &= (unsigned)ut[(size_t)g * d.U + u] < (unsigned)d.n_unary_tables;
  return ok;
}

// What a refused graph returns (mlbp_converge.h): rounds -1, residual NaN, its history row NaN; messages and marginals untouched.
__device__ __forceinline__ void refuse_graph(const ConvergeDev& d, int g) {
  if (threadIdx.x == 0) {
    d.rounds[g] = -1;
    d.residual[g] = __builtin_nan("");
  }
  if (d.history)
    for (int r = threadIdx.x; r < d.max_rounds; r += WG) d.history[(size_t)g * d.max_rounds + r] = __builtin_nan("");
}

// rounds, residual and the unused tail of the history row (the rounds run were written as they ended).
__device__ __forceinline__ void write_result(const ConvergeDev& d, int g, int rounds, double res) {
  if (threadIdx.x == 0) {
    d.rounds[g] = rounds;
    d.residual[g] = res;
  }
  if (d.history)
    for (int r = rounds + threadIdx.x; r < d.max_rounds; r += WG) d.history[(size_t)g * d.max_rounds + r] = -1.0;
}

// The 16 entries of a 64 x 64 table this thread owns: entry 2k + e = T[16 wave + 2k + (lane >> 5)][2 (lane & 31) + e].
__device__ __forceinline__ void load_fragment(const double* table, int wave, int lane, double (&T)[16]) {
  const double2* src = reinterpret_cast<const double2*>(table) + (size_t)(16 * wave) * 32 + lane;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double2 v = src[(size_t)(2 * k) * 32];
    T[2 * k] = v.x;
    T[2 * k + 1] = v.y;
  }
}

// out[j] = sum_i m[i] * T[i][j]: the thread's two columns over its 8 rows -> part[2 wave + half][column].
__device__ __forceinline__ void pair_mt_partial(const double (&T)[16], const double* m, double* part, int wave, int lane) {
  const int h = lane >> 5;
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double mi = m[16 * wave + 2 * k + h];          // two addresses per wave: LDS broadcast
    a0 += mi * T[2 * k];
    a1 += mi * T[2 * k + 1];
  }
  reinterpret_cast<double2*>(part)[(2 * wave + h) * 32 + (lane & 31)] = make_double2(a0, a1);
}

// out[i] = sum_j T[i][j] * m[j]: the wave's 16 rows -> raw[16 wave .. 16 wave + 15].
__device__ __forceinline__ void pair_tm_rows(const double (&T)[16], const double* m, double* raw, int wave, int lane) {
  const double2 mm = reinterpret_cast<const double2*>(m)[lane & 31];
  double2 mine = make_double2(0.0, 0.0);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double p = row16_sum(T[2 * k] * mm.x + T[2 * k + 1] * mm.y);
    const double lo = read_lane(p, 0) + read_lane(p, 16);           // row 16 wave + 2k     (lanes 0..31)
    const double hi = read_lane(p, 32) + read_lane(p, 48);          // row 16 wave + 2k + 1 (lanes 32..63)
    if (lane == k) mine = make_double2(lo, hi);
  }
  if (lane < 8) reinterpret_cast<double2*>(raw)[8 * wave + lane] = mine;
}

template <bool RESIDENT>
__global__ __launch_bounds__(WG) void converge_x64_kernel(ConvergeDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* msg = reinterpret_cast<double*>(smem);               // [n_msgs][64]
  double* part = msg + (size_t)d.n_msgs * 64;                  // [8][64] partial sums of an m^T.T update
  double* raw = part + 512;                                    // [64] un-normalised result of a T.m update
  double* res_word = raw + 64;                                 // [1] the round's residual, read by every thread
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!graph_in_range(d, g)) {                                 // (block-uniform: the whole workgroup leaves)
    refuse_graph(d, g);
    return;
  }
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const const_i32p c_ops = as_const(d.ops), c_srcs = as_const(d.srcs), c_sweeps = as_const(d.sweeps);
  const const_i32p in_off = as_const(d.in_off), in_slots = as_const(d.in_slots);
  const double uniform = 1.0 / 64.0;

  double R[3][16];                                             // RESIDENT: the graph's tables, once per workgroup
  if (RESIDENT) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
      if (p < d.P) load_fragment(d.pair_tables + (size_t)ptab[p] * 4096, wave, lane, R[p]);
  }
  // (2 n_msgs words of `part`: n_msgs <= 150 by the LDS rule, part holds 1024)
  const unsigned once_mask = unary_once_mask(d, reinterpret_cast<int32_t*>(part), lane);
  double2* msg2 = reinterpret_cast<double2*>(msg);
  double2* gmsg2 = reinterpret_cast<double2*>(d.msgs + (size_t)g * d.n_msgs * 64);
  if (d.init) {
    for (int i = t; i < d.n_msgs * 32; i += WG) msg2[i] = make_double2(uniform, uniform);
  } else {
    for (int i = t; i < d.n_msgs * 32; i += WG) msg2[i] = gmsg2[i];
  }
  __syncthreads();

  double rmax = 0.0;                                           // wave 0: this lane's largest |new - old| of the round
  // wave 0, lane = state: normalise and store a finished message, keep the residual
  auto finish = [&](double v, int dst) {
    const double total = wave_sum(v);
    const double fresh = renorm(v, total, uniform, true);
    rmax = fmax(rmax, entry_delta(fresh, msg[dst * 64 + lane]));
    msg[dst * 64 + lane] = fresh;
  };

  int rounds = 0;
  double res = 0.0;
  while (true) {                                               // every thread takes the same number of turns: see below
    rmax = 0.0;
    for (int sw = 0; sw < d.n_sweeps; ++sw) {
      const int op0 = c_sweeps[2 * sw], nop = c_sweeps[2 * sw + 1];
      for (int o = op0; o < op0 + nop; ++o) {
        const int kind = c_ops[4 * o], a = c_ops[4 * o + 1], b = c_ops[4 * o + 2], c = c_ops[4 * o + 3];
        if (kind == MLBP_OP_UNARY && rounds > 0 && unary_once(once_mask, o)) continue;      // (uniform: no barrier is skipped by some)
        if (kind == MLBP_OP_PAIR_TM || kind == MLBP_OP_PAIR_MT) {
          const double* m = msg + b * 64;
          const bool tm = kind == MLBP_OP_PAIR_TM;
          if (RESIDENT) {
            if (a == 0) { if (tm) pair_tm_rows(R[0], m, raw, wave, lane); else pair_mt_partial(R[0], m, part, wave, lane); }
            else if (a == 1) { if (tm) pair_tm_rows(R[1], m, raw, wave, lane); else pair_mt_partial(R[1], m, part, wave, lane); }
            else { if (tm) pair_tm_rows(R[2], m, raw, wave, lane); else pair_mt_partial(R[2], m, part, wave, lane); }
          } else {
            double T[16];
            load_fragment(d.pair_tables + (size_t)ptab[a] * 4096, wave, lane, T);
            if (tm) pair_tm_rows(T, m, raw, wave, lane); else pair_mt_partial(T, m, part, wave, lane);
          }
          __syncthreads();
          if (wave == 0) {
            double acc;
            if (tm) {
              acc = raw[lane];
            } else {
              acc = part[lane];
#pragma unroll
              for (int q = 1; q < 8; ++q) acc += part[q * 64 + lane];
            }
            finish(acc, c);
          }
        } else if (wave == 0) {
          if (kind == MLBP_OP_VAR) {
            double acc = uniform;
            for (int q = 0; q < b; ++q) acc = mul_nan_to_num(msg[c_srcs[a + q] * 64 + lane], acc);
            finish(acc, c);
          } else {
            finish(d.unary_tables[(size_t)utab[a] * 64 + lane], c);
          }
        }
        __syncthreads();
      }
    }
    // The round's residual: wave 0 reduces and publishes it, EVERY thread reads it behind the barrier, so `rounds`, `res` and
    // the decision below are the same in all 256 threads.  The word is written again only behind the next round's first
    // barrier, which no thread passes before it has read this round's value.
    if (wave == 0) {
      const double r = wave_max(rmax);
      if (lane == 0) {
        res_word[0] = r;
        if (d.history) d.history[(size_t)g * d.max_rounds + rounds] = r;
      }
    }
    __syncthreads();
    res = res_word[0];
    ++rounds;
    if (res <= d.tol || rounds >= d.max_rounds) break;
    __syncthreads();                                           // nobody is still reading the word when wave 0 may write it
  }
  write_result(d, g, rounds, res);
  for (int i = t; i < d.n_msgs * 32; i += WG) gmsg2[i] = msg2[i];
  if (d.marginals) {
    for (int v = wave; v < d.n_vars; v += WG / 64) {           // one variable per wave, lane = state
      double acc = uniform;
      for (int q = in_off[v]; q < in_off[v + 1]; ++q) acc = mul_nan_to_num(msg[in_slots[q] * 64 + lane], acc);
      const double total = wave_sum(acc);
      d.marginals[((size_t)g * d.n_vars + v) * 64 + lane] = total > 0.0 ? acc / total : uniform;
    }
  }
}

// ---- any X ---------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double* scratch /*[4]*/) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
}

__global__ __launch_bounds__(WG) void converge_generic_kernel(ConvergeDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X;
  double* raw = reinterpret_cast<double*>(smem);               // [X] (X rounded up to even)
  double* scratch = raw + ((X + 1) & ~1);                      // [4] block sums
  double* wave_res = scratch + 4;                              // [4] the waves' maxima of the round
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!graph_in_range(d, g)) {
    refuse_graph(d, g);
    return;
  }
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const const_i32p c_ops = as_const(d.ops), c_srcs = as_const(d.srcs), c_sweeps = as_const(d.sweeps);
  const const_i32p in_off = as_const(d.in_off), in_slots = as_const(d.in_slots);
  const double uniform = 1.0 / (double)X;
  // only this workgroup touches its messages
  double* msg = d.msgs + (size_t)g * d.n_msgs * X;
  if (d.init)
    for (int i = t; i < d.n_msgs * X; i += WG) msg[i] = uniform;
  __syncthreads();
  int rounds = 0;
  double res = 0.0;
  while (true) {
    double rmax = 0.0;                                         // over the entries this thread writes
    for (int sw = 0; sw < d.n_sweeps; ++sw) {
      const int op0 = c_sweeps[2 * sw], nop = c_sweeps[2 * sw + 1];
      for (int o = op0; o < op0 + nop; ++o) {
        const int kind = c_ops[4 * o], a = c_ops[4 * o + 1], b = c_ops[4 * o + 2], c = c_ops[4 * o + 3];
        if (kind == MLBP_OP_PAIR_TM) {
          const double* T = d.pair_tables + (size_t)ptab[a] * X * X;
          const double* m = msg + (size_t)b * X;
          for (int row = wave; row < X; row += WG / 64) {
            const double* Tr = T + (size_t)row * X;
            double acc = 0.0;
            for (int j = lane; j < X; j += 64) acc += Tr[j] * m[j];
            acc = wave_sum(acc);
            if (lane == 0) raw[row] = acc;
          }
        } else if (kind == MLBP_OP_PAIR_MT) {
          const double* T = d.pair_tables + (size_t)ptab[a] * X * X;
          const double* m = msg + (size_t)b * X;
          for (int j = t; j < X; j += WG) {
            double acc = 0.0;
#pragma unroll 8
            for (int i = 0; i < X; ++i) acc += m[i] * T[(size_t)i * X + j];
            raw[j] = acc;
          }
        } else if (kind == MLBP_OP_VAR) {
          for (int j = t; j < X; j += WG) {
            double acc = uniform;
            for (int q = 0; q < b; ++q) acc = nan_to_num(msg[(size_t)c_srcs[a + q] * X + j] * acc);
            raw[j] = acc;
          }
        } else {
          const double* u = d.unary_tables + (size_t)utab[a] * X;
          for (int j = t; j < X; j += WG) raw[j] = u[j];
        }
        __syncthreads();
        double part = 0.0;
        for (int j = t; j < X; j += WG) part += raw[j];
        const double total = block_sum(part, scratch);
        double* out = msg + (size_t)c * X;
        for (int j = t; j < X; j += WG) {
          const double fresh = renorm(raw[j], total, uniform, true);
          rmax = fmax(rmax, entry_delta(fresh, out[j]));
          out[j] = fresh;
        }
        __syncthreads();
      }
    }
    // block-uniform stop: four wave maxima through LDS, every thread reads all four behind the barrier
    rmax = wave_max(rmax);
    if (lane == 0) wave_res[wave] = rmax;
    __syncthreads();
    res = fmax(fmax(wave_res[0], wave_res[1]), fmax(wave_res[2], wave_res[3]));
    if (t == 0 && d.history) d.history[(size_t)g * d.max_rounds + rounds] = res;
    ++rounds;
    if (res <= d.tol || rounds >= d.max_rounds) break;
    __syncthreads();                                           // nobody is still reading the maxima when they are written again
  }
  write_result(d, g, rounds, res);
  if (d.marginals) {
    for (int v = 0; v < d.n_vars; ++v) {
      double part = 0.0;
      for (int j = t; j < X; j += WG) {
        double acc = uniform;
        for (int q = in_off[v]; q < in_off[v + 1]; ++q) acc = nan_to_num(msg[(size_t)in_slots[q] * X + j] * acc);
        raw[j] = acc;
        part += acc;
      }
      const double total = block_sum(part, scratch);
      for (int j = t; j < X; j += WG) d.marginals[((size_t)g * d.n_vars + v) * X + j] = total > 0.0 ? raw[j] / total : uniform;
      __syncthreads();
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------
thread_local std::string g_last_error = "";
thread_local int g_last_kernel = MLBP_CONVERGE_KERNEL_NONE;

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

int64_t x64_lds_bytes(int32_t n_msgs) { return (int64_t)n_msgs * 512 + 4608 + 8; }

size_t generic_lds_bytes(int32_t X) { return (size_t)((X + 1) & ~1) * 8 + 8 * 8; }

// The X = 64 kernel asks for more than the default 64 KiB of dynamic LDS: its limit is raised once per device and instance
// (a host-side attribute call, on the first -- eager -- call).
int grant_x64_lds(const void* kernel, int instance) {
  enum { MAX_DEVICES = 64 };
  static std::atomic<bool> granted[MAX_DEVICES][2];
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(MLBP_EHIP, "hipGetDevice failed");
  if (dev < 0 || dev >= MAX_DEVICES) return fail(MLBP_EUNSUPPORTED, "device index %d beyond %d", dev, (int)MAX_DEVICES);
  if (granted[dev][instance].load(std::memory_order_acquire)) return MLBP_OK;
  std::lock_guard<std::mutex> lock(mu);
  if (granted[dev][instance].load(std::memory_order_relaxed)) return MLBP_OK;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MLBP_CONVERGE_X64_LDS_BYTES);
  if (e != hipSuccess) return fail(MLBP_EHIP, "raising the X = 64 kernel's LDS limit failed: %s", hipGetErrorString(e));
  granted[dev][instance].store(true, std::memory_order_release);
  return MLBP_OK;
}

}  // namespace

extern "C" {

const char* mlbp_converge_arch(void) { return "gfx950"; }
const char* mlbp_converge_last_error(void) { return g_last_error.c_str(); }
int mlbp_converge_last_kernel(void) { return g_last_kernel; }

int mlbp_converge_pick_kernel(int32_t X, int32_t n_msgs, int32_t n_vars) {
  if (X < 2 || n_msgs <= 0 || n_vars <= 0) return fail(MLBP_EINVAL, "pick_kernel: X = %d, n_msgs = %d, n_vars = %d", X, n_msgs, n_vars);
  if (X > MLBP_CONVERGE_MAX_X) return fail(MLBP_EUNSUPPORTED, "X = %d: at most %d states are supported", X, MLBP_CONVERGE_MAX_X);
  return X == 64 && x64_lds_bytes(n_msgs) <= MLBP_CONVERGE_X64_LDS_BYTES ? MLBP_CONVERGE_KERNEL_X64 : MLBP_CONVERGE_KERNEL_GENERIC;
}

int mlbp_converge_check_program(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs, const int32_t* sweeps,
                                int32_t n_sweeps, int32_t n_msgs, int32_t P, int32_t U) {
  if (!ops || !sweeps) return fail(MLBP_EINVAL, "program: ops or sweeps is NULL");
  if (n_ops <= 0 || n_sweeps <= 0 || n_msgs <= 0 || P < 0 || U < 0 || n_srcs < 0 || (n_srcs > 0 && !srcs))
    return fail(MLBP_EINVAL, "program: bad sizes (n_ops %d, n_sweeps %d, n_msgs %d, P %d, U %d, n_srcs %d) or srcs is NULL", n_ops,
                n_sweeps, n_msgs, P, U, n_srcs);
  for (int o = 0; o < n_ops; ++o) {
    const int kind = ops[4 * o], a = ops[4 * o + 1], b = ops[4 * o + 2], c = ops[4 * o + 3];
    if (c < 0 || c >= n_msgs) return fail(MLBP_EINVAL, "op %d: destination slot %d out of [0,%d)", o, c, n_msgs);
    switch (kind) {
      case MLBP_OP_UNARY:
        if (a < 0 || a >= U) return fail(MLBP_EINVAL, "op %d: unary slot %d out of [0,%d)", o, a, U);
        break;
      case MLBP_OP_PAIR_TM:
      case MLBP_OP_PAIR_MT:
        if (a < 0 || a >= P) return fail(MLBP_EINVAL, "op %d: pair slot %d out of [0,%d)", o, a, P);
        if (b < 0 || b >= n_msgs) return fail(MLBP_EINVAL, "op %d: source slot %d out of [0,%d)", o, b, n_msgs);
        if (b == c) return fail(MLBP_EINVAL, "op %d: source and destination slot coincide", o);
        break;
      case MLBP_OP_VAR:
        if (a < 0 || b < 0 || (int64_t)a + b > n_srcs) return fail(MLBP_EINVAL, "op %d: srcs range [%d,%d) out of [0,%d)", o, a, a + b, n_srcs);
        for (int q = a; q < a + b; ++q)
          if (srcs[q] < 0 || srcs[q] >= n_msgs) return fail(MLBP_EINVAL, "op %d: source slot %d out of [0,%d)", o, srcs[q], n_msgs);
        break;
      default:
        return fail(MLBP_EINVAL, "op %d: unknown kind %d", o, kind);
    }
  }
  std::vector<char> covered((size_t)n_msgs, 0);
  for (int s = 0; s < n_sweeps; ++s) {
    const int first = sweeps[2 * s], cnt = sweeps[2 * s + 1];
    if (first < 0 || cnt < 0 || (int64_t)first + cnt > n_ops)
      return fail(MLBP_EINVAL, "sweep %d: op range [%d,%d) out of [0,%d)", s, first, first + cnt, n_ops);
    for (int o = first; o < first + cnt; ++o) covered[ops[4 * o + 3]] = 1;
  }
  for (int k = 0; k < n_msgs; ++k)
    if (!covered[k])
      return fail(MLBP_EINVAL, "coverage: message slot %d is the destination of no op of the round: the residual would say nothing about it", k);
  return MLBP_OK;
}

int mlbp_converge_check_readout(int32_t n_vars, const int32_t* in_off, const int32_t* in_slots, int32_t n_msgs) {
  if (!in_off || !in_slots) return fail(MLBP_EINVAL, "read-out: in_off or in_slots is NULL");
  if (n_vars <= 0 || n_msgs <= 0) return fail(MLBP_EINVAL, "read-out: bad sizes (n_vars %d, n_msgs %d)", n_vars, n_msgs);
  if (in_off[0] != 0) return fail(MLBP_EINVAL, "read-out: in_off[0] must be 0");
  for (int v = 0; v < n_vars; ++v) {
    if (in_off[v + 1] < in_off[v]) return fail(MLBP_EINVAL, "read-out: in_off not monotone at variable %d", v);
    for (int q = in_off[v]; q < in_off[v + 1]; ++q)
      if (in_slots[q] < 0 || in_slots[q] >= n_msgs) return fail(MLBP_EINVAL, "read-out: variable %d: slot %d out of [0,%d)", v, in_slots[q], n_msgs);
  }
  return MLBP_OK;
}

int mlbp_converge_f64(const mlbp_converge_args* a, void* stream) {
  g_last_kernel = MLBP_CONVERGE_KERNEL_NONE;
  if (!a) return fail(MLBP_EINVAL, "args is NULL");
  if (a->B <= 0 || a->n_msgs <= 0 || a->n_vars <= 0 || a->P < 0 || a->U < 0 || a->n_ops <= 0 || a->n_sweeps <= 0 || a->n_srcs < 0)
    return fail(MLBP_EINVAL, "bad sizes: B %d, n_msgs %d, n_vars %d, P %d, U %d, n_ops %d, n_sweeps %d, n_srcs %d", a->B, a->n_msgs,
                a->n_vars, a->P, a->U, a->n_ops, a->n_sweeps, a->n_srcs);
  if (a->X < 2) return fail(MLBP_EINVAL, "X = %d: a variable needs at least two states", a->X);
  if (!a->normalize_messages)
    return fail(MLBP_EINVAL, "normalize_messages = 0: a residual on unnormalised messages has no scale");
  if (!std::isfinite(a->tol) || a->tol < 0.0) return fail(MLBP_EINVAL, "tol = %g: must be finite and at least 0", a->tol);
  if (a->max_rounds < 1 || a->max_rounds > MLBP_CONVERGE_MAX_ROUNDS)
    return fail(MLBP_EINVAL, "max_rounds = %d out of [1, %d]", a->max_rounds, MLBP_CONVERGE_MAX_ROUNDS);
  const int which = mlbp_converge_pick_kernel(a->X, a->n_msgs, a->n_vars);
  if (which < 0) return which;
  if (!a->ops || !a->sweeps || (a->n_srcs > 0 && !a->srcs)) return fail(MLBP_EINVAL, "ops, srcs or sweeps is NULL");
  if (!a->in_off || !a->in_slots) return fail(MLBP_EINVAL, "in_off or in_slots is NULL");
  if (!a->msgs) return fail(MLBP_EINVAL, "msgs is NULL");
  if (!a->rounds || !a->residual) return fail(MLBP_EINVAL, "rounds or residual is NULL");
  if (a->P > 0 && (!a->pair_tables || !a->pair_tab || a->n_pair_tables <= 0))
    return fail(MLBP_EINVAL, "P = %d but pair_tables or pair_tab is NULL (or n_pair_tables <= 0)", a->P);
  if (a->U > 0 && (!a->unary_tables || !a->unary_tab || a->n_unary_tables <= 0))
    return fail(MLBP_EINVAL, "U = %d but unary_tables or unary_tab is NULL (or n_unary_tables <= 0)", a->U);
  if ((int64_t)a->n_msgs * a->X > 0x7fffffff / 2) return fail(MLBP_EUNSUPPORTED, "n_msgs * X = %lld too large", (long long)a->n_msgs * a->X);
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    (void)hipGetLastError();
    return fail(MLBP_ENODEVICE, "no HIP device visible: libmlbp_converge.so has no CPU fallback");
  }
  ConvergeDev d;
  d.pair_tables = a->pair_tables; d.pair_tab = a->pair_tab; d.unary_tables = a->unary_tables; d.unary_tab = a->unary_tab;
  d.ops = a->ops; d.srcs = a->srcs; d.sweeps = a->sweeps;
  d.in_off = a->in_off; d.in_slots = a->in_slots;
  d.msgs = a->msgs; d.rounds = a->rounds; d.residual = a->residual; d.marginals = a->marginals; d.history = a->history;
  d.tol = a->tol;
  d.n_sweeps = a->n_sweeps; d.n_msgs = a->n_msgs; d.P = a->P; d.U = a->U; d.X = a->X; d.n_vars = a->n_vars;
  d.n_pair_tables = a->n_pair_tables; d.n_unary_tables = a->n_unary_tables;
  d.init = a->init_messages != 0; d.max_rounds = a->max_rounds; d.n_ops = a->n_ops;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  if (which == MLBP_CONVERGE_KERNEL_X64) {
    const bool resident = a->P <= 3;
    auto k = resident ? converge_x64_kernel<true> : converge_x64_kernel<false>;
    if (int e = grant_x64_lds((const void*)k, resident ? 1 : 0)) return e;
    hipLaunchKernelGGL(k, dim3(a->B), dim3(WG), (size_t)x64_lds_bytes(a->n_msgs), st, d);
  } else {
    hipLaunchKernelGGL(converge_generic_kernel, dim3(a->B), dim3(WG), generic_lds_bytes(a->X), st, d);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MLBP_EHIP, "converge launch failed: %s", hipGetErrorString(e));
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
