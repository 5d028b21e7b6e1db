// libmlbp_sample.so: posterior sampling of whole assignments by sequential conditioning (include/mlbp_sample.h), gfx950 only,
// float64.
//
// Two kernels, chosen from (X, n_msgs, n_vars) by mlbp_sample_pick_kernel, both on a grid of (B, C) workgroups: workgroup
// (g, c) serves graph g and draws its samples c, c + C, ...
//   sample_x64_kernel<RESIDENT>  X = 64, four waves, messages in LDS for the whole launch -- the layout of
//                                map_sweep_x64_kernel (csrc_map/mlbp_map.hip): a pairwise table is split over the 256 threads
//                                as 16 entries each, wave w owns rows 16w .. 16w+15, lane l holds, for k = 0..7, the two entries
//                                of row 16w + 2k + (l >> 5) in columns 2(l & 31), +1.  RESIDENT (P <= 3): all tables are loaded
//                                once per workgroup and stay in registers over every step of every sample; otherwise the 16
//                                entries are loaded per update (streamed).  The two contractions are sums:
//                                  out = m^T.T : running sum over the thread's 8 rows for its two columns, the 8 partial vectors
//                                                (4 waves x 2 row halves) meet in LDS and are added in a fixed order;
//                                  out = T.m   : per row the two products, then a sum over the 32 lanes of the row half on DPP
//                                                and through scalar registers.
//                                A clamped variable is an int in LDS, applied to its outgoing messages as lane == x ? acc : 0.
//                                The draw runs in wave 0 with lane = state: inclusive scan, total from lane 63, ballot of c > t.
//                                The marginal of step 0 (no variable clamped yet: the same for every sample) is computed for the
//                                workgroup's first sample and kept in LDS.
//   sample_generic_kernel        any X in [2, 1024]: messages in the caller's workspace, tables streamed, the draw a serial
//                                scan by one thread over the LDS copy of the marginal.  Correct first: the path for shapes
//                                nobody times.
// No device-side mutable globals: everything comes through SampleDev.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mlbp_sample.h"
#include "../csrc/mlbp_device.h"

namespace {

using namespace mlbp_dev;

constexpr int WG = 256;

struct SampleDev {
  const double* pair_tables; const int32_t* pair_tab;
  const double* unary_tables; const int32_t* unary_tab;
  const int32_t* ops; const int32_t* srcs; const int32_t* sweeps;
  const int32_t* in_off; const int32_t* in_slots; const int32_t* slot_var; const int32_t* order;
  const double* uniforms; const int32_t* given;
  double* workspace;
  int32_t* samples; double* logq; double* cond_marginals;
  int32_t n_sweeps, n_msgs, P, U, X, n_vars, n_pair_tables, n_unary_tables;
  int32_t normalize, B, S;
};

// Sum over each row of 16 lanes, the same bits in every lane of the row (the first four steps of mlbp_dev::wave_sum).
__device__ __forceinline__ double row16_sum(double v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x141>(v);
  v += dpp_mov<0x140>(v);
  return v;
}

// Inclusive prefix sum over the 64 lanes in lane order (Hillis-Steele, six steps).
__device__ __forceinline__ double wave_inclusive_scan(double v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double up = __shfl_up(v, d, 64);
    if (lane >= d) v += up;
  }
  return v;
}

// Every table index of graph g is inside its table array and every given state is -1 or a state (wave-uniform: scalar loads).
__device__ __forceinline__ bool graph_in_range(const SampleDev& d, int g) {
  bool ok = true;
  const const_i32p pt = as_const(d.pair_tab), ut = as_const(d.unary_tab);
  for (int p = 0; p < d.P; ++p) ok &= (unsigned)pt[(size_t)g * d.P + p] < (unsigned)d.n_pair_tables;
  for (int u = 0; u < d.U; ++u) ok &= (unsigned)ut[(size_t)g * d.U + u] < (unsigned)d.n_unary_tables;
  if (d.given) {
    const const_i32p gv = as_const(d.given) + (size_t)g * d.n_vars;
    for (int v = 0; v < d.n_vars; ++v) ok &= gv[v] >= -1 && gv[v] < d.X;
  }
  return ok;
}

// What a refused graph returns (mlbp_sample.h): samples -1, logq NaN, for the samples of this workgroup.
__device__ __forceinline__ void refuse_graph(const SampleDev& d, int g) {
  for (int s = blockIdx.y; s < d.S; s += gridDim.y) {
    int32_t* out = d.samples + ((size_t)s * d.B + g) * d.n_vars;
    for (int v = threadIdx.x; v < d.n_vars; v += WG) out[v] = -1;
    if (threadIdx.x == 0) d.logq[(size_t)s * d.B + g] = __builtin_nan("");
  }
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
__global__ __launch_bounds__(WG) void sample_x64_kernel(SampleDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* msg = reinterpret_cast<double*>(smem);               // [n_msgs][64]
  double* part = msg + (size_t)d.n_msgs * 64;                  // [8][64] partial sums of an m^T.T update
  double* raw = part + 512;                                    // [64] un-normalised result of a T.m update
  double* m0 = raw + 64;                                       // [64] the marginal of step 0
  int32_t* clamp = reinterpret_cast<int32_t*>(m0 + 64);        // [n_vars] the state a variable is clamped to, -1 while free
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!graph_in_range(d, g)) {
    refuse_graph(d, g);
    return;
  }
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const const_i32p c_ops = as_const(d.ops), c_srcs = as_const(d.srcs), c_sweeps = as_const(d.sweeps);
  const const_i32p in_off = as_const(d.in_off), in_slots = as_const(d.in_slots);
  const const_i32p slot_var = as_const(d.slot_var), order = as_const(d.order);
  const double uniform = 1.0 / 64.0;
  const bool norm = d.normalize != 0;

  double R[3][16];                                             // RESIDENT: the graph's tables, once per workgroup
  if (RESIDENT) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
      if (p < d.P) load_fragment(d.pair_tables + (size_t)ptab[p] * 4096, wave, lane, R[p]);
  }
  double2* msg2 = reinterpret_cast<double2*>(msg);

  // wave 0, lane = state: normalise and store a finished message
  auto finish = [&](double v, int dst) {
    const double total = norm ? wave_sum(v) : 0.0;
    msg[dst * 64 + lane] = renorm(v, total, uniform, norm);
  };

  bool have_m0 = false;
  for (int s = blockIdx.y; s < d.S; s += gridDim.y) {
    for (int v = t; v < d.n_vars; v += WG) clamp[v] = -1;
    __syncthreads();
    double logq = 0.0;                                         // wave 0, the same in every lane
    const size_t sg = (size_t)s * d.B + g;
    for (int k = 0; k < d.n_vars; ++k) {
      const int v = order[k];
      if (k > 0 || !have_m0) {
        for (int i = t; i < d.n_msgs * 32; i += WG) msg2[i] = make_double2(uniform, uniform);
        __syncthreads();                                       // (also publishes the clamp states)
        for (int sw = 0; sw < d.n_sweeps; ++sw) {
          const int op0 = c_sweeps[2 * sw], nop = c_sweeps[2 * sw + 1];
          for (int o = op0; o < op0 + nop; ++o) {
            const int kind = c_ops[4 * o], a = c_ops[4 * o + 1], b = c_ops[4 * o + 2], c = c_ops[4 * o + 3];
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
                const int x = clamp[slot_var[c]];
                if (x >= 0) acc = lane == x ? acc : 0.0;
                finish(acc, c);
              } else {
                finish(d.unary_tables[(size_t)utab[a] * 64 + lane], c);
              }
            }
            __syncthreads();
          }
        }
      }
      // the marginal of v, the draw and the clamp: wave 0, lane = state
      if (wave == 0) {
        double m;
        if (k == 0 && have_m0) {
          m = m0[lane];
        } else {
          double acc = uniform;
          for (int q = in_off[v]; q < in_off[v + 1]; ++q) acc = mul_nan_to_num(msg[in_slots[q] * 64 + lane], acc);
          const double total = wave_sum(acc);
          m = total > 0.0 ? acc / total : uniform;
          if (k == 0) m0[lane] = m;
        }
        if (d.cond_marginals) d.cond_marginals[(sg * d.n_vars + v) * 64 + lane] = m;
        int x = d.given ? d.given[(size_t)g * d.n_vars + v] : -1;
        if (x < 0) {
          const double c = wave_inclusive_scan(m, lane);
          const double thr = d.uniforms[sg * d.n_vars + k] * read_lane(c, 63);
          const unsigned long long pos = __ballot(m > 0.0);
          const unsigned long long above = __ballot(c > thr && m > 0.0);   // (m > 0: a rounding of the scan never picks an empty state)
          x = above ? __builtin_ctzll(above) : (pos ? 63 - __builtin_clzll(pos) : 0);
        }
        logq += log(__shfl(m, x, 64));
        if (lane == 0) {
          clamp[v] = x;
          d.samples[sg * d.n_vars + v] = x;
        }
      }
      if (k == 0) have_m0 = true;
      __syncthreads();
    }
    if (t == 0) d.logq[sg] = logq;
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

__global__ __launch_bounds__(WG) void sample_generic_kernel(SampleDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X;
  double* raw = reinterpret_cast<double*>(smem);               // [X] (X rounded up to even)
  double* scratch = raw + ((X + 1) & ~1);                      // [4] block sums
  double* logq_s = scratch + 4;                                // [1] thread 0's running log q
  int32_t* clamp = reinterpret_cast<int32_t*>(logq_s + 1);     // [n_vars]
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!graph_in_range(d, g)) {
    refuse_graph(d, g);
    return;
  }
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const const_i32p c_ops = as_const(d.ops), c_srcs = as_const(d.srcs), c_sweeps = as_const(d.sweeps);
  const const_i32p in_off = as_const(d.in_off), in_slots = as_const(d.in_slots);
  const const_i32p slot_var = as_const(d.slot_var), order = as_const(d.order);
  const double uniform = 1.0 / (double)X;
  const bool norm = d.normalize != 0;
  // only this workgroup touches its messages
  double* msg = d.workspace + ((size_t)g * gridDim.y + blockIdx.y) * (size_t)d.n_msgs * X;
  for (int s = blockIdx.y; s < d.S; s += gridDim.y) {
    for (int v = t; v < d.n_vars; v += WG) clamp[v] = -1;
    if (t == 0) logq_s[0] = 0.0;
    const size_t sg = (size_t)s * d.B + g;
    for (int k = 0; k < d.n_vars; ++k) {
      const int v = order[k];
      for (int i = t; i < d.n_msgs * X; i += WG) msg[i] = uniform;
      __syncthreads();
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
            const int x = clamp[slot_var[c]];
            for (int j = t; j < X; j += WG) {
              double acc = uniform;
              for (int q = 0; q < b; ++q) acc = nan_to_num(msg[(size_t)c_srcs[a + q] * X + j] * acc);
              raw[j] = (x >= 0 && j != x) ? 0.0 : acc;
            }
          } else {
            const double* u = d.unary_tables + (size_t)utab[a] * X;
            for (int j = t; j < X; j += WG) raw[j] = u[j];
          }
          __syncthreads();
          double part = 0.0;
          for (int j = t; j < X; j += WG) part += raw[j];
          const double total = norm ? block_sum(part, scratch) : 0.0;
          double* out = msg + (size_t)c * X;
          for (int j = t; j < X; j += WG) out[j] = renorm(raw[j], total, uniform, norm);
          __syncthreads();
        }
      }
      // the marginal of v -> raw, the draw by thread 0
      double part = 0.0;
      for (int j = t; j < X; j += WG) {
        double acc = uniform;
        for (int q = in_off[v]; q < in_off[v + 1]; ++q) acc = nan_to_num(msg[(size_t)in_slots[q] * X + j] * acc);
        raw[j] = acc;
        part += acc;
      }
      const double total = block_sum(part, scratch);
      for (int j = t; j < X; j += WG) {
        const double mm = total > 0.0 ? raw[j] / total : uniform;
        raw[j] = mm;
        if (d.cond_marginals) d.cond_marginals[(sg * d.n_vars + v) * X + j] = mm;
      }
      __syncthreads();
      if (t == 0) {
        int x = d.given ? d.given[(size_t)g * d.n_vars + v] : -1;
        if (x < 0) {
          double c = 0.0;
          for (int i = 0; i < X; ++i) c += raw[i];
          const double thr = d.uniforms[sg * d.n_vars + k] * c;
          c = 0.0;
          int last = 0;
          for (int i = 0; i < X; ++i) {
            c += raw[i];
            if (raw[i] > 0.0) {
              last = i;
              if (c > thr) { x = i; break; }
            }
          }
          if (x < 0) x = last;
        }
        logq_s[0] += log(raw[x]);
        clamp[v] = x;
        d.samples[sg * d.n_vars + v] = x;
      }
      __syncthreads();
    }
    if (t == 0) d.logq[sg] = logq_s[0];
  }
}

// ---- host ----------------------------------------------------------------------------------------
thread_local std::string g_last_error = "";
thread_local int g_last_kernel = MLBP_SAMPLE_KERNEL_NONE;

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

int64_t x64_lds_bytes(int32_t n_msgs, int32_t n_vars) {
  return (int64_t)n_msgs * 512 + 4608 + 512 + 4 * (((int64_t)n_vars + 3) & ~(int64_t)3);
}

size_t generic_lds_bytes(int32_t X, int32_t n_vars) {
  return (size_t)((X + 1) & ~1) * 8 + 5 * 8 + 4 * (size_t)n_vars;
}

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
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MLBP_SAMPLE_X64_LDS_BYTES);
  if (e != hipSuccess) return fail(MLBP_EHIP, "raising the X = 64 kernel's LDS limit failed: %s", hipGetErrorString(e));
  granted[dev][instance].store(true, std::memory_order_release);
  return MLBP_OK;
}

}  // namespace

extern "C" {

const char* mlbp_sample_arch(void) { return "gfx950"; }
const char* mlbp_sample_last_error(void) { return g_last_error.c_str(); }
int mlbp_sample_last_kernel(void) { return g_last_kernel; }

int mlbp_sample_pick_kernel(int32_t X, int32_t n_msgs, int32_t n_vars) {
  if (X < 2 || n_msgs <= 0 || n_vars <= 0) return fail(MLBP_EINVAL, "pick_kernel: X = %d, n_msgs = %d, n_vars = %d", X, n_msgs, n_vars);
  if (X > MLBP_SAMPLE_MAX_X) return fail(MLBP_EUNSUPPORTED, "X = %d: at most %d states are supported", X, MLBP_SAMPLE_MAX_X);
  return X == 64 && x64_lds_bytes(n_msgs, n_vars) <= MLBP_SAMPLE_X64_LDS_BYTES ? MLBP_SAMPLE_KERNEL_X64 : MLBP_SAMPLE_KERNEL_GENERIC;
}

int mlbp_sample_chunks(int32_t B, int32_t S) {
  if (B <= 0 || S <= 0) return fail(MLBP_EINVAL, "chunks: B = %d, S = %d", B, S);
  const int32_t want = (MLBP_SAMPLE_MIN_WORKGROUPS + B - 1) / B;          // >= 1
  return S < want ? S : want;
}

int64_t mlbp_sample_workspace_bytes(int32_t B, int32_t S, int32_t X, int32_t n_msgs, int32_t n_vars) {
  const int which = mlbp_sample_pick_kernel(X, n_msgs, n_vars);
  if (which < 0) return which;
  const int C = mlbp_sample_chunks(B, S);
  if (C < 0) return C;
  if (which == MLBP_SAMPLE_KERNEL_X64) return 0;
  return (int64_t)B * C * n_msgs * X * 8;
}

int mlbp_sample_check_program(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs, const int32_t* sweeps,
                              int32_t n_sweeps, int32_t n_msgs, int32_t P, int32_t U, int32_t n_vars, const int32_t* slot_var,
                              const int32_t* order) {
  if (!ops || !sweeps) return fail(MLBP_EINVAL, "program: ops or sweeps is NULL");
  if (!slot_var || !order) return fail(MLBP_EINVAL, "program: slot_var or order is NULL");
  if (n_ops <= 0 || n_sweeps <= 0 || n_msgs <= 0 || n_vars <= 0 || P < 0 || U < 0 || n_srcs < 0 || (n_srcs > 0 && !srcs))
    return fail(MLBP_EINVAL, "program: bad sizes (n_ops %d, n_sweeps %d, n_msgs %d, n_vars %d, P %d, U %d, n_srcs %d) or srcs is NULL",
                n_ops, n_sweeps, n_msgs, n_vars, P, U, n_srcs);
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
    if (kind == MLBP_OP_VAR) {
      if (slot_var[c] < 0 || slot_var[c] >= n_vars)
        return fail(MLBP_EINVAL, "op %d: destination slot %d of a variable update has no source variable (slot_var %d, n_vars %d)", o, c, slot_var[c], n_vars);
    } else if (slot_var[c] != -1) {
      return fail(MLBP_EINVAL, "op %d: destination slot %d of a factor update has slot_var %d, not -1", o, c, slot_var[c]);
    }
  }
  for (int s = 0; s < n_sweeps; ++s) {
    const int first = sweeps[2 * s], cnt = sweeps[2 * s + 1];
    if (first < 0 || cnt < 0 || (int64_t)first + cnt > n_ops)
      return fail(MLBP_EINVAL, "sweep %d: op range [%d,%d) out of [0,%d)", s, first, first + cnt, n_ops);
  }
  std::vector<char> seen((size_t)n_vars, 0);
  for (int k = 0; k < n_vars; ++k) {
    if (order[k] < 0 || order[k] >= n_vars || seen[order[k]])
      return fail(MLBP_EINVAL, "order is not a permutation: order[%d] = %d (n_vars %d)", k, order[k], n_vars);
    seen[order[k]] = 1;
  }
  return MLBP_OK;
}

int mlbp_sample_check_readout(int32_t n_vars, const int32_t* in_off, const int32_t* in_slots, int32_t n_msgs) {
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

int mlbp_sample_f64(const mlbp_sample_args* a, void* stream) {
  g_last_kernel = MLBP_SAMPLE_KERNEL_NONE;
  if (!a) return fail(MLBP_EINVAL, "args is NULL");
  if (a->B <= 0 || a->n_msgs <= 0 || a->n_vars <= 0 || a->P < 0 || a->U < 0 || a->n_ops <= 0 || a->n_sweeps <= 0 || a->n_srcs < 0)
    return fail(MLBP_EINVAL, "bad sizes: B %d, n_msgs %d, n_vars %d, P %d, U %d, n_ops %d, n_sweeps %d, n_srcs %d", a->B, a->n_msgs,
                a->n_vars, a->P, a->U, a->n_ops, a->n_sweeps, a->n_srcs);
  if (a->S <= 0) return fail(MLBP_EINVAL, "S = %d: at least one sample per graph", a->S);
  if (a->X < 2) return fail(MLBP_EINVAL, "X = %d: a variable needs at least two states", a->X);
  const int which = mlbp_sample_pick_kernel(a->X, a->n_msgs, a->n_vars);
  if (which < 0) return which;
  if (!a->ops || !a->sweeps || (a->n_srcs > 0 && !a->srcs)) return fail(MLBP_EINVAL, "ops, srcs or sweeps is NULL");
  if (!a->in_off || !a->in_slots) return fail(MLBP_EINVAL, "in_off or in_slots is NULL");
  if (!a->slot_var || !a->order) return fail(MLBP_EINVAL, "slot_var or order is NULL");
  if (!a->uniforms) return fail(MLBP_EINVAL, "uniforms is NULL");
  if (!a->samples || !a->logq) return fail(MLBP_EINVAL, "samples or logq is NULL");
  if (a->P > 0 && (!a->pair_tables || !a->pair_tab || a->n_pair_tables <= 0))
    return fail(MLBP_EINVAL, "P = %d but pair_tables or pair_tab is NULL (or n_pair_tables <= 0)", a->P);
  if (a->U > 0 && (!a->unary_tables || !a->unary_tab || a->n_unary_tables <= 0))
    return fail(MLBP_EINVAL, "U = %d but unary_tables or unary_tab is NULL (or n_unary_tables <= 0)", a->U);
  if ((int64_t)a->n_msgs * a->X > 0x7fffffff / 2) return fail(MLBP_EUNSUPPORTED, "n_msgs * X = %lld too large", (long long)a->n_msgs * a->X);
  const int C = mlbp_sample_chunks(a->B, a->S);
  if (C < 0) return C;
  if (C > 65535) return fail(MLBP_EUNSUPPORTED, "chunks = %d beyond the grid's second dimension", C);
  if (which == MLBP_SAMPLE_KERNEL_GENERIC) {
    const int64_t need = (int64_t)a->B * C * a->n_msgs * a->X * 8;
    if (!a->workspace || a->workspace_bytes < need)
      return fail(MLBP_EINVAL, "workspace: the generic kernel needs %lld bytes, got %lld%s", (long long)need, (long long)a->workspace_bytes,
                  a->workspace ? "" : " (NULL)");
    if (generic_lds_bytes(a->X, a->n_vars) > 65536)
      return fail(MLBP_EUNSUPPORTED, "n_vars = %d: the generic kernel's clamp states do not fit LDS", a->n_vars);
  }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    (void)hipGetLastError();
    return fail(MLBP_ENODEVICE, "no HIP device visible: libmlbp_sample.so has no CPU fallback");
  }
  SampleDev d;
  d.pair_tables = a->pair_tables; d.pair_tab = a->pair_tab; d.unary_tables = a->unary_tables; d.unary_tab = a->unary_tab;
  d.ops = a->ops; d.srcs = a->srcs; d.sweeps = a->sweeps;
  d.in_off = a->in_off; d.in_slots = a->in_slots; d.slot_var = a->slot_var; d.order = a->order;
  d.uniforms = a->uniforms; d.given = a->given; d.workspace = a->workspace;
  d.samples = a->samples; d.logq = a->logq; d.cond_marginals = a->cond_marginals;
  d.n_sweeps = a->n_sweeps; d.n_msgs = a->n_msgs; d.P = a->P; d.U = a->U; d.X = a->X; d.n_vars = a->n_vars;
  d.n_pair_tables = a->n_pair_tables; d.n_unary_tables = a->n_unary_tables;
  d.normalize = a->normalize_messages != 0; d.B = a->B; d.S = a->S;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  if (which == MLBP_SAMPLE_KERNEL_X64) {
    const bool resident = a->P <= 3;
    auto k = resident ? sample_x64_kernel<true> : sample_x64_kernel<false>;
    if (int e = grant_x64_lds((const void*)k, resident ? 1 : 0)) return e;
    hipLaunchKernelGGL(k, dim3(a->B, C), dim3(WG), (size_t)x64_lds_bytes(a->n_msgs, a->n_vars), st, d);
  } else {
    hipLaunchKernelGGL(sample_generic_kernel, dim3(a->B, C), dim3(WG), generic_lds_bytes(a->X, a->n_vars), st, d);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MLBP_EHIP, "sampling launch failed: %s", hipGetErrorString(e));
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
