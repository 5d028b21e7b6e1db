// libmlbp_map.so: max-product sweeps and MAP decoding (include/mlbp_map.h), gfx950 only, float64.
//
// Two kernels, chosen from (X, n_msgs, n_vars) by mlbp_map_pick_kernel:
//   map_sweep_x64_kernel<RESIDENT>  X = 64, one workgroup of four waves per graph, messages in LDS for the whole launch.
//                                   A pairwise table is split over the 256 threads as 16 entries each (load_fragment of
//                                   csrc/mlbp_graph_device.h, which also holds the two contractions and the per-op step; here
//                                   they run with MaxOp: a maximum where the sum-product libraries add).  RESIDENT (P <= 3): all
//                                   tables are loaded once at the start and stay in registers (96 VGPRs) -- each is used twice
//                                   per sweep, HBM sees it once per launch.  Otherwise the 16 entries are loaded per update
//                                   (streamed).  Init, max-marginals, argmax and score run in the same launch from the on-chip
//                                   messages.
//   map_sweep_generic_kernel        any X in [2, 1024]: messages in global memory, tables streamed, read-out in the same launch.
//                                   Correct first: the path for shapes nobody times.
// Bytes per graph on the resident form: P tables of 32 KiB and U rows of 512 B in, n_vars assignments and one score out
// (plus max-marginals / messages when asked for).  No device-side mutable globals: everything comes through MapDev.
// The host checks shared with the other side libraries are in csrc/mlbp_graph_host.h.
#include <hip/hip_runtime.h>

#include "../../include/mlbp_map.h"
#include "../csrc/mlbp_graph_device.h"
#include "../csrc/mlbp_graph_host.h"

namespace {

using namespace mlbp_graph;

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

// What a graph with a bad table index returns (mlbp_map.h): assignment -1, score NaN.
__device__ __forceinline__ void refuse_graph(const MapDev& d, int g) {
  if (d.assignment)
    for (int v = threadIdx.x; v < d.n_vars; v += WG) d.assignment[(size_t)g * d.n_vars + v] = -1;
  if (d.score && threadIdx.x == 0) d.score[g] = __builtin_nan("");
}

template <bool RESIDENT>
__global__ __launch_bounds__(WG) void map_sweep_x64_kernel(MapDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* msg = reinterpret_cast<double*>(smem);               // [n_msgs][64]
  double* part = msg + (size_t)d.n_msgs * 64;                  // [8][64] partial maxima of an m^T.T update
  double* raw = part + 512;                                    // [64] un-normalised result of a T.m update
  int32_t* xs = reinterpret_cast<int32_t*>(raw + 64);          // [n_vars] the assignment
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) {
    refuse_graph(d, g);
    return;
  }
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const const_i32p c_ops = as_const(d.ops), c_sweeps = as_const(d.sweeps);
  const StepGraph G = {d.pair_tables, ptab, d.unary_tables, utab, as_const(d.srcs), msg, part, raw};
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
      x64_step<MaxOp, RESIDENT>(G, R, kind, a, b, c, wave, lane, FreeState(), finish);
    }
  }

  // read-out: wave w takes variables w, w + 4, ...; lane = state
  const const_i32p in_off = as_const(d.in_off), in_slots = as_const(d.in_slots);
  for (int v = wave; v < d.n_vars; v += WG / 64) {
    const double mm = x64_marginal(msg, in_off, in_slots, v, lane);
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
__global__ __launch_bounds__(WG) void map_sweep_generic_kernel(MapDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X;
  double* raw = reinterpret_cast<double*>(smem);               // [X] (X rounded up to even)
  double* scratch = raw + ((X + 1) & ~1);                      // [4] block sums
  double* best_v = scratch + 4;                                // [4] per-wave maxima
  int32_t* best_i = reinterpret_cast<int32_t*>(best_v + 4);    // [4] per-wave lowest index at the maximum
  int32_t* xs = best_i + 4;                                    // [n_vars]
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) {
    refuse_graph(d, g);
    return;
  }
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const const_i32p c_ops = as_const(d.ops), c_sweeps = as_const(d.sweeps);
  const double uniform = 1.0 / (double)X;
  const bool norm = d.normalize != 0;
  const double ninf = -__builtin_huge_val();
  double* msg = d.msgs + (size_t)g * d.n_msgs * X;             // only this workgroup touches its graph's messages
  const StepGraph G = {d.pair_tables, ptab, d.unary_tables, utab, as_const(d.srcs), msg, nullptr, raw};
  if (d.init_messages)
    for (int i = t; i < d.n_msgs * X; i += WG) msg[i] = uniform;
  __syncthreads();
  for (int s = 0; s < d.n_sweeps; ++s) {
    const int op0 = c_sweeps[2 * s], nop = c_sweeps[2 * s + 1];
    for (int o = op0; o < op0 + nop; ++o) {
      const int kind = c_ops[4 * o], a = c_ops[4 * o + 1], b = c_ops[4 * o + 2], c = c_ops[4 * o + 3];
      generic_step<MaxOp>(G, X, uniform, kind, a, b, c, FreeState());
      double* out = msg + (size_t)c * X;
      generic_finish(raw, X, uniform, norm, scratch, [&](int j, double fresh) { out[j] = fresh; });
    }
  }
  // read-out
  const const_i32p in_off = as_const(d.in_off), in_slots = as_const(d.in_slots);
  for (int v = 0; v < d.n_vars; ++v) {
    double best = ninf;
    int at = 0x7fffffff;
    generic_marginal(msg, in_off, in_slots, v, X, uniform, raw, scratch, [&](int j, double mm) {
      if (d.max_marginals) d.max_marginals[((size_t)g * d.n_vars + v) * X + j] = mm;
      if (mm > best) { best = mm; at = j; }                    // ascending j and a strict compare: the lowest index wins
    });
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
thread_local int g_last_kernel = MLBP_MAP_KERNEL_NONE;

int64_t x64_lds_bytes(int32_t n_msgs, int32_t n_vars) {
  return (int64_t)n_msgs * 512 + 4608 + 4 * (((int64_t)n_vars + 3) & ~(int64_t)3);
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
  if (int e = check_program_sizes(ops, n_ops, srcs, n_srcs, sweeps, n_sweeps, n_msgs, P, U)) return e;
  return check_program_indices(ops, n_ops, srcs, n_srcs, sweeps, n_sweeps, n_msgs, P, U, NoMoreChecks());
}

int mlbp_map_check_readout(int32_t n_vars, const int32_t* in_off, const int32_t* in_slots, int32_t n_msgs, int32_t P,
                           const int32_t* pair_axis_var, int32_t U, const int32_t* unary_var) {
  if (int e = check_in_slots_present(in_off, in_slots)) return e;
  if (n_vars <= 0 || n_msgs <= 0 || P < 0 || U < 0 || (P > 0 && !pair_axis_var) || (U > 0 && !unary_var))
    return fail(MLBP_EINVAL, "read-out: bad sizes (n_vars %d, n_msgs %d, P %d, U %d) or a NULL array", n_vars, n_msgs, P, U);
  if (int e = check_in_slots(n_vars, in_off, in_slots, n_msgs, NoMoreChecks())) return e;
  for (int i = 0; i < 2 * P; ++i)
    if (pair_axis_var[i] < 0 || pair_axis_var[i] >= n_vars) return fail(MLBP_EINVAL, "read-out: pair factor %d: variable %d out of [0,%d)", i / 2, pair_axis_var[i], n_vars);
  for (int u = 0; u < U; ++u)
    if (unary_var[u] < 0 || unary_var[u] >= n_vars) return fail(MLBP_EINVAL, "read-out: unary factor %d: variable %d out of [0,%d)", u, unary_var[u], n_vars);
  return MLBP_OK;
}

int mlbp_map_sweep_f64(const mlbp_map_args* a, void* stream) {
  g_last_kernel = MLBP_MAP_KERNEL_NONE;
  if (int e = check_args_sizes(a)) return e;
  if (int e = check_states(a->X)) return e;
  const int which = mlbp_map_pick_kernel(a->X, a->n_msgs, a->n_vars);
  if (which < 0) return which;
  if (int e = check_args_program(a)) return e;
  if (int e = check_args_tables(a, !a->pair_axis_var, "pair_tables, pair_tab or pair_axis_var", !a->unary_var, "unary_tables, unary_tab or unary_var")) return e;
  if (!a->msgs && (which != MLBP_MAP_KERNEL_X64 || !a->init_messages || a->write_messages))
    return fail(MLBP_EINVAL, "msgs is NULL: allowed only on the X = 64 kernel with init_messages and without write_messages");
  if (!a->max_marginals && !a->assignment && !a->score && !a->write_messages)
    return fail(MLBP_EINVAL, "nothing to compute: max_marginals, assignment and score are NULL and write_messages is 0");
  if (int e = check_args_extent(a)) return e;
  if (int e = check_device("libmlbp_map.so")) return e;
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
    if (int e = grant_x64_lds((const void*)k, resident ? 1 : 0, MLBP_MAP_X64_LDS_BYTES)) return e;
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
