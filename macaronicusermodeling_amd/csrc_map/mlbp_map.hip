// libmlbp_map.so: max-product sweeps and MAP decoding (include/mlbp_map.h), gfx950 only, float64.
//
// Two kernels, chosen from (X, n_msgs, n_vars) by mlbp_map_pick_kernel:
//   map_sweep_x64_kernel<RESIDENT>  X = 64, one workgroup of four waves per graph, messages in LDS for the whole launch.
//                                   A pairwise table is split over the 256 threads as 16 entries each: wave w owns rows
//                                   16w .. 16w+15; lane l holds, for k = 0..7, the two entries of row 16w + 2k + (l >> 5) in
//                                   columns 2(l & 31), +1 -- so a wave loads two consecutive rows (1 KiB) per instruction,
//                                   16 bytes per lane.  RESIDENT (P <= 3): all tables are loaded once at the start and stay in
//                                   registers (96 VGPRs) -- each is used twice per sweep, HBM sees it once per launch.
//                                   Otherwise the 16 entries are loaded per update (streamed).
//                                     out = m^T.T : running fmax over the thread's 8 rows for its two columns, the 8 partial
//                                                   vectors (4 waves x 2 row halves) meet in LDS;
//                                     out = T.m   : per row max of the two products, then a max over the 32 lanes of the
//                                                   row half on DPP (row16_max) and through scalar registers.
//                                   Init, max-marginals, argmax and score run in the same launch from the on-chip messages.
//   map_sweep_generic_kernel        any X in [2, 1024]: messages in global memory, tables streamed, read-out in the same launch.
//                                   Correct first: the path for shapes nobody times.
// Bytes per graph on the resident form: P tables of 32 KiB and U rows of 512 B in, n_vars assignments and one score out
// (plus max-marginals / messages when asked for).  No device-side mutable globals: everything comes through MapDev.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <string>

#include "../../include/mlbp_map.h"
#include "../csrc/mlbp_device.h"

namespace {

using namespace mlbp_dev;

constexpr int WG = 256;

struct MapDev {
  const double* pair_tables; const int32_t* pair_tab;
  const double* unary_tables; const int32_t* unary_tab;
  double* msgs;
  const int32_t* ops; const int32_t* srcs; const int32_t* sweeps;
  const int32_t* in_off; const int32_t* in_slots; const int32_t* pair_axis_var; const int32_t* unary_var;
  double* max_marginals; int32_t* assignment; double* score;
  int32_t n_sweeps, n_msgs, P, U, X, n_vars, n_pair_tables, n_unary_tables;
  int32_t init_messages, normalize, write_messages;
};

// Maximum over each row of 16 lanes, the same bits in every lane of the row (wave_sum's pairing, with fmax).
__device__ __forceinline__ double row16_max(double v) {
  v = fmax(v, dpp_mov<0xB1>(v));
  v = fmax(v, dpp_mov<0x4E>(v));
  v = fmax(v, dpp_mov<0x141>(v));
  v = fmax(v, dpp_mov<0x140>(v));
  return v;
}

// Maximum over the 64 lanes, the same bits in every lane (written beside mlbp_dev::wave_sum).
__device__ __forceinline__ double wave_max(double v) {
  v = row16_max(v);
  return fmax(fmax(read_lane(v, 0), read_lane(v, 16)), fmax(read_lane(v, 32), read_lane(v, 48)));
}

// Every table index of graph g is inside its table array (wave-uniform: scalar loads).
__device__ __forceinline__ bool tables_in_range(const MapDev& d, int g) {
  bool ok = true;
  const const_i32p pt = as_const(d.pair_tab), ut = as_const(d.unary_tab);
  for (int p = 0; p < d.P; ++p) ok &= (unsigned)pt[(size_t)g * d.P + p] < (unsigned)d.n_pair_tables;
  for (int u = 0; u < d.U; ++u) ok &= (unsigned)ut[(size_t)g * d.U + u] < (unsigned)d.n_unary_tables;
  return ok;
}

// What a graph with a bad table index returns (mlbp_map.h): assignment -1, score NaN.
__device__ __forceinline__ void refuse_graph(const MapDev& d, int g) {
  if (d.assignment)
    for (int v = threadIdx.x; v < d.n_vars; v += WG) d.assignment[(size_t)g * d.n_vars + v] = -1;
  if (d.score && threadIdx.x == 0) d.score[g] = __builtin_nan("");
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

// out[j] = max_i m[i] * T[i][j]: the thread's two columns over its 8 rows -> part[2 wave + half][column].
__device__ __forceinline__ void pair_mt_partial(const double (&T)[16], const double* m, double* part, int wave, int lane) {
  const int h = lane >> 5;
  double a0 = -__builtin_huge_val(), a1 = -__builtin_huge_val();
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double mi = m[16 * wave + 2 * k + h];          // two addresses per wave: LDS broadcast
    a0 = fmax(a0, mi * T[2 * k]);
    a1 = fmax(a1, mi * T[2 * k + 1]);
  }
  reinterpret_cast<double2*>(part)[(2 * wave + h) * 32 + (lane & 31)] = make_double2(a0, a1);
}

// out[i] = max_j T[i][j] * m[j]: the wave's 16 rows -> raw[16 wave .. 16 wave + 15].
__device__ __forceinline__ void pair_tm_rows(const double (&T)[16], const double* m, double* raw, int wave, int lane) {
  const double2 mm = reinterpret_cast<const double2*>(m)[lane & 31];
  double2 mine = make_double2(0.0, 0.0);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double p = row16_max(fmax(T[2 * k] * mm.x, T[2 * k + 1] * mm.y));
    const double lo = fmax(read_lane(p, 0), read_lane(p, 16));      // row 16 wave + 2k     (lanes 0..31)
    const double hi = fmax(read_lane(p, 32), read_lane(p, 48));     // row 16 wave + 2k + 1 (lanes 32..63)
    if (lane == k) mine = make_double2(lo, hi);
  }
  if (lane < 8) reinterpret_cast<double2*>(raw)[8 * wave + lane] = mine;
}

template <bool RESIDENT>
__global__ __launch_bounds__(WG) void map_sweep_x64_kernel(MapDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* msg = reinterpret_cast<double*>(smem);               // [n_msgs][64]
  double* part = msg + (size_t)d.n_msgs * 64;                  // [8][64] partial maxima of an m^T.T update
  double* raw = part + 512;                                    // [64] un-normalised result of a T.m update
  int32_t* xs = reinterpret_cast<int32_t*>(raw + 64);          // [n_vars] the assignment
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d, g)) {
    refuse_graph(d, g);
    return;
  }
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const const_i32p c_ops = as_const(d.ops), c_srcs = as_const(d.srcs), c_sweeps = as_const(d.sweeps);
  const double uniform = 1.0 / 64.0;
  const bool norm = d.normalize != 0;

  double R[3][16];                                             // RESIDENT: the graph's tables, once per launch
  if (RESIDENT) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
      if (p < d.P) load_fragment(d.pair_tables + (size_t)ptab[p] * 4096, wave, lane, R[p]);
  }
  double2* msg2 = reinterpret_cast<double2*>(msg);
  double2* gm2 = d.msgs ? reinterpret_cast<double2*>(d.msgs + (size_t)g * d.n_msgs * 64) : nullptr;
  if (d.init_messages) {
    for (int i = t; i < d.n_msgs * 32; i += WG) msg2[i] = make_double2(uniform, uniform);
  } else {
    for (int i = t; i < d.n_msgs * 32; i += WG) msg2[i] = gm2[i];
  }
  __syncthreads();

  // wave 0, lane = state: normalise and store a finished message
  auto finish = [&](double v, int dst) {
    const double total = norm ? wave_sum(v) : 0.0;
    msg[dst * 64 + lane] = renorm(v, total, uniform, norm);
  };

  for (int s = 0; s < d.n_sweeps; ++s) {
    const int op0 = c_sweeps[2 * s], nop = c_sweeps[2 * s + 1];
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
          double v;
          if (tm) {
            v = raw[lane];
          } else {
            v = part[lane];
#pragma unroll
            for (int q = 1; q < 8; ++q) v = fmax(v, part[q * 64 + lane]);
          }
          finish(v, c);
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

  // read-out: wave w takes variables w, w + 4, ...; lane = state
  const const_i32p in_off = as_const(d.in_off), in_slots = as_const(d.in_slots);
  for (int v = wave; v < d.n_vars; v += WG / 64) {
    double acc = uniform;
    for (int q = in_off[v]; q < in_off[v + 1]; ++q) acc = mul_nan_to_num(msg[in_slots[q] * 64 + lane], acc);
    const double total = wave_sum(acc);
    const double mm = total > 0.0 ? acc / total : uniform;
    if (d.max_marginals) d.max_marginals[((size_t)g * d.n_vars + v) * 64 + lane] = mm;
    const unsigned long long at_max = __ballot(mm == wave_max(mm));
    if (lane == 0) xs[v] = at_max ? __builtin_ctzll(at_max) : 0;           // ties go to the lowest index
  }
  __syncthreads();
  if (d.assignment)
    for (int v = t; v < d.n_vars; v += WG) d.assignment[(size_t)g * d.n_vars + v] = xs[v];
  if (d.score && wave == 0) {
    double sc = 0.0;
    for (int p = lane; p < d.P; p += 64) {
      const int i = xs[d.pair_axis_var[2 * p]], j = xs[d.pair_axis_var[2 * p + 1]];
      sc += log(d.pair_tables[(size_t)ptab[p] * 4096 + i * 64 + j]);
    }
    for (int u = lane; u < d.U; u += 64) sc += log(d.unary_tables[(size_t)utab[u] * 64 + xs[d.unary_var[u]]]);
    sc = wave_sum(sc);
    if (lane == 0) d.score[g] = sc;
  }
  if (d.write_messages)
    for (int i = t; i < d.n_msgs * 32; i += WG) gm2[i] = msg2[i];
}

// ---- any X ---------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double* scratch /*[4]*/) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
}

__global__ __launch_bounds__(WG) void map_sweep_generic_kernel(MapDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X;
  double* raw = reinterpret_cast<double*>(smem);               // [X] (X rounded up to even)
  double* scratch = raw + ((X + 1) & ~1);                      // [4] block sums
  double* best_v = scratch + 4;                                // [4] per-wave maxima
  int32_t* best_i = reinterpret_cast<int32_t*>(best_v + 4);    // [4] per-wave lowest index at the maximum
  int32_t* xs = best_i + 4;                                    // [n_vars]
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d, g)) {
    refuse_graph(d, g);
    return;
  }
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const const_i32p c_ops = as_const(d.ops), c_srcs = as_const(d.srcs), c_sweeps = as_const(d.sweeps);
  const double uniform = 1.0 / (double)X;
  const bool norm = d.normalize != 0;
  const double ninf = -__builtin_huge_val();
  double* msg = d.msgs + (size_t)g * d.n_msgs * X;             // only this workgroup touches its graph's messages
  if (d.init_messages)
    for (int i = t; i < d.n_msgs * X; i += WG) msg[i] = uniform;
  __syncthreads();
  for (int s = 0; s < d.n_sweeps; ++s) {
    const int op0 = c_sweeps[2 * s], nop = c_sweeps[2 * s + 1];
    for (int o = op0; o < op0 + nop; ++o) {
      const int kind = c_ops[4 * o], a = c_ops[4 * o + 1], b = c_ops[4 * o + 2], c = c_ops[4 * o + 3];
      if (kind == MLBP_OP_PAIR_TM) {
        const double* T = d.pair_tables + (size_t)ptab[a] * X * X;
        const double* m = msg + (size_t)b * X;
        for (int row = wave; row < X; row += WG / 64) {
          const double* Tr = T + (size_t)row * X;
          double acc = ninf;
          for (int j = lane; j < X; j += 64) acc = fmax(acc, Tr[j] * m[j]);
          acc = wave_max(acc);
          if (lane == 0) raw[row] = acc;
        }
      } else if (kind == MLBP_OP_PAIR_MT) {
        const double* T = d.pair_tables + (size_t)ptab[a] * X * X;
        const double* m = msg + (size_t)b * X;
        for (int j = t; j < X; j += WG) {
          double acc = ninf;
#pragma unroll 8
          for (int i = 0; i < X; ++i) acc = fmax(acc, m[i] * T[(size_t)i * X + j]);
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
      const double total = norm ? block_sum(part, scratch) : 0.0;
      double* out = msg + (size_t)c * X;
      for (int j = t; j < X; j += WG) out[j] = renorm(raw[j], total, uniform, norm);
      __syncthreads();
    }
  }
  // read-out
  const const_i32p in_off = as_const(d.in_off), in_slots = as_const(d.in_slots);
  for (int v = 0; v < d.n_vars; ++v) {
    double part = 0.0;
    for (int j = t; j < X; j += WG) {
      double acc = uniform;
      for (int q = in_off[v]; q < in_off[v + 1]; ++q) acc = nan_to_num(msg[(size_t)in_slots[q] * X + j] * acc);
      raw[j] = acc;
      part += acc;
    }
    const double total = block_sum(part, scratch);
    double best = ninf;
    int at = 0x7fffffff;
    for (int j = t; j < X; j += WG) {                          // ascending j and a strict compare: the lowest index wins
      const double mm = total > 0.0 ? raw[j] / total : uniform;
      if (d.max_marginals) d.max_marginals[((size_t)g * d.n_vars + v) * X + j] = mm;
      if (mm > best) { best = mm; at = j; }
    }
    const double wbest = wave_max(best);
    int cand = best == wbest ? at : 0x7fffffff;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cand = min(cand, __shfl_xor(cand, m, 64));
    if (lane == 0) { best_v[wave] = wbest; best_i[wave] = cand; }
    __syncthreads();
    if (t == 0) {
      double bv = best_v[0];
      int bi = best_i[0];
      for (int w = 1; w < WG / 64; ++w)
        if (best_v[w] > bv || (best_v[w] == bv && best_i[w] < bi)) { bv = best_v[w]; bi = best_i[w]; }
      xs[v] = bi < X ? bi : 0;
    }
    __syncthreads();
  }
  if (d.assignment)
    for (int v = t; v < d.n_vars; v += WG) d.assignment[(size_t)g * d.n_vars + v] = xs[v];
  if (d.score) {
    double sc = 0.0;
    for (int p = t; p < d.P; p += WG) {
      const int i = xs[d.pair_axis_var[2 * p]], j = xs[d.pair_axis_var[2 * p + 1]];
      sc += log(d.pair_tables[(size_t)ptab[p] * X * X + (size_t)i * X + j]);
    }
    for (int u = t; u < d.U; u += WG) sc += log(d.unary_tables[(size_t)utab[u] * X + xs[d.unary_var[u]]]);
    sc = block_sum(sc, scratch);
    if (t == 0) d.score[g] = sc;
  }
}

// ---- host ----------------------------------------------------------------------------------------
thread_local std::string g_last_error = "";
thread_local int g_last_kernel = MLBP_MAP_KERNEL_NONE;

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
  return (int64_t)n_msgs * 512 + 4608 + 4 * (((int64_t)n_vars + 3) & ~(int64_t)3);
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
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MLBP_MAP_X64_LDS_BYTES);
  if (e != hipSuccess) return fail(MLBP_EHIP, "raising the X = 64 kernel's LDS limit failed: %s", hipGetErrorString(e));
  granted[dev][instance].store(true, std::memory_order_release);
  return MLBP_OK;
}

}  // namespace

extern "C" {

const char* mlbp_map_arch(void) { return "gfx950"; }
const char* mlbp_map_last_error(void) { return g_last_error.c_str(); }
int mlbp_map_last_kernel(void) { return g_last_kernel; }

int mlbp_map_pick_kernel(int32_t X, int32_t n_msgs, int32_t n_vars) {
  if (X < 2 || n_msgs <= 0 || n_vars <= 0) return fail(MLBP_EINVAL, "pick_kernel: X = %d, n_msgs = %d, n_vars = %d", X, n_msgs, n_vars);
  if (X > MLBP_MAP_MAX_X) return fail(MLBP_EUNSUPPORTED, "X = %d: at most %d states are supported", X, MLBP_MAP_MAX_X);
  return X == 64 && x64_lds_bytes(n_msgs, n_vars) <= MLBP_MAP_X64_LDS_BYTES ? MLBP_MAP_KERNEL_X64 : MLBP_MAP_KERNEL_GENERIC;
}

int mlbp_map_check_program(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs, const int32_t* sweeps,
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
  for (int s = 0; s < n_sweeps; ++s) {
    const int first = sweeps[2 * s], cnt = sweeps[2 * s + 1];
    if (first < 0 || cnt < 0 || (int64_t)first + cnt > n_ops)
      return fail(MLBP_EINVAL, "sweep %d: op range [%d,%d) out of [0,%d)", s, first, first + cnt, n_ops);
  }
  return MLBP_OK;
}

int mlbp_map_check_readout(int32_t n_vars, const int32_t* in_off, const int32_t* in_slots, int32_t n_msgs, int32_t P,
                           const int32_t* pair_axis_var, int32_t U, const int32_t* unary_var) {
  if (!in_off || !in_slots) return fail(MLBP_EINVAL, "read-out: in_off or in_slots is NULL");
  if (n_vars <= 0 || n_msgs <= 0 || P < 0 || U < 0 || (P > 0 && !pair_axis_var) || (U > 0 && !unary_var))
    return fail(MLBP_EINVAL, "read-out: bad sizes (n_vars %d, n_msgs %d, P %d, U %d) or a NULL array", n_vars, n_msgs, P, U);
  if (in_off[0] != 0) return fail(MLBP_EINVAL, "read-out: in_off[0] must be 0");
  for (int v = 0; v < n_vars; ++v) {
    if (in_off[v + 1] < in_off[v]) return fail(MLBP_EINVAL, "read-out: in_off not monotone at variable %d", v);
    for (int q = in_off[v]; q < in_off[v + 1]; ++q)
      if (in_slots[q] < 0 || in_slots[q] >= n_msgs) return fail(MLBP_EINVAL, "read-out: variable %d: slot %d out of [0,%d)", v, in_slots[q], n_msgs);
  }
  for (int i = 0; i < 2 * P; ++i)
    if (pair_axis_var[i] < 0 || pair_axis_var[i] >= n_vars) return fail(MLBP_EINVAL, "read-out: pair factor %d: variable %d out of [0,%d)", i / 2, pair_axis_var[i], n_vars);
  for (int u = 0; u < U; ++u)
    if (unary_var[u] < 0 || unary_var[u] >= n_vars) return fail(MLBP_EINVAL, "read-out: unary factor %d: variable %d out of [0,%d)", u, unary_var[u], n_vars);
  return MLBP_OK;
}

int mlbp_map_sweep_f64(const mlbp_map_args* a, void* stream) {
  g_last_kernel = MLBP_MAP_KERNEL_NONE;
  if (!a) return fail(MLBP_EINVAL, "args is NULL");
  if (a->B <= 0 || a->n_msgs <= 0 || a->n_vars <= 0 || a->P < 0 || a->U < 0 || a->n_ops <= 0 || a->n_sweeps <= 0 || a->n_srcs < 0)
    return fail(MLBP_EINVAL, "bad sizes: B %d, n_msgs %d, n_vars %d, P %d, U %d, n_ops %d, n_sweeps %d, n_srcs %d", a->B, a->n_msgs,
                a->n_vars, a->P, a->U, a->n_ops, a->n_sweeps, a->n_srcs);
  if (a->X < 2) return fail(MLBP_EINVAL, "X = %d: a variable needs at least two states", a->X);
  const int which = mlbp_map_pick_kernel(a->X, a->n_msgs, a->n_vars);
  if (which < 0) return which;
  if (!a->ops || !a->sweeps || (a->n_srcs > 0 && !a->srcs)) return fail(MLBP_EINVAL, "ops, srcs or sweeps is NULL");
  if (!a->in_off || !a->in_slots) return fail(MLBP_EINVAL, "in_off or in_slots is NULL");
  if (a->P > 0 && (!a->pair_tables || !a->pair_tab || !a->pair_axis_var || a->n_pair_tables <= 0))
    return fail(MLBP_EINVAL, "P = %d but pair_tables, pair_tab or pair_axis_var is NULL (or n_pair_tables <= 0)", a->P);
  if (a->U > 0 && (!a->unary_tables || !a->unary_tab || !a->unary_var || a->n_unary_tables <= 0))
    return fail(MLBP_EINVAL, "U = %d but unary_tables, unary_tab or unary_var is NULL (or n_unary_tables <= 0)", a->U);
  if (!a->msgs && (which != MLBP_MAP_KERNEL_X64 || !a->init_messages || a->write_messages))
    return fail(MLBP_EINVAL, "msgs is NULL: allowed only on the X = 64 kernel with init_messages and without write_messages");
  if (!a->max_marginals && !a->assignment && !a->score && !a->write_messages)
    return fail(MLBP_EINVAL, "nothing to compute: max_marginals, assignment and score are NULL and write_messages is 0");
  if ((int64_t)a->n_msgs * a->X > 0x7fffffff / 2) return fail(MLBP_EUNSUPPORTED, "n_msgs * X = %lld too large", (long long)a->n_msgs * a->X);
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    (void)hipGetLastError();
    return fail(MLBP_ENODEVICE, "no HIP device visible: libmlbp_map.so has no CPU fallback");
  }
  MapDev d;
  d.pair_tables = a->pair_tables; d.pair_tab = a->pair_tab; d.unary_tables = a->unary_tables; d.unary_tab = a->unary_tab;
  d.msgs = a->msgs; d.ops = a->ops; d.srcs = a->srcs; d.sweeps = a->sweeps;
  d.in_off = a->in_off; d.in_slots = a->in_slots; d.pair_axis_var = a->pair_axis_var; d.unary_var = a->unary_var;
  d.max_marginals = a->max_marginals; d.assignment = a->assignment; d.score = a->score;
  d.n_sweeps = a->n_sweeps; d.n_msgs = a->n_msgs; d.P = a->P; d.U = a->U; d.X = a->X; d.n_vars = a->n_vars;
  d.n_pair_tables = a->n_pair_tables; d.n_unary_tables = a->n_unary_tables;
  d.init_messages = a->init_messages != 0; d.normalize = a->normalize_messages != 0; d.write_messages = a->write_messages != 0;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  if (which == MLBP_MAP_KERNEL_X64) {
    const bool resident = a->P <= 3;
    auto k = resident ? map_sweep_x64_kernel<true> : map_sweep_x64_kernel<false>;
    if (int e = grant_x64_lds((const void*)k, resident ? 1 : 0)) return e;
    hipLaunchKernelGGL(k, dim3(a->B), dim3(WG), (size_t)x64_lds_bytes(a->n_msgs, a->n_vars), st, d);
  } else {
    const size_t lds = (size_t)((a->X + 1) & ~1) * 8 + 8 * 8 + 4 * 4 + 4 * (size_t)a->n_vars;
    if (lds > 65536) return fail(MLBP_EUNSUPPORTED, "n_vars = %d: the generic kernel's assignment does not fit LDS", a->n_vars);
    hipLaunchKernelGGL(map_sweep_generic_kernel, dim3(a->B), dim3(WG), lds, st, d);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MLBP_EHIP, "max-product sweep launch failed: %s", hipGetErrorString(e));
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
