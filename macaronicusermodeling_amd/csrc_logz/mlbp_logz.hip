// libmlbp_logz.so: log Z and the joint log-likelihood from the factor->variable messages (include/mlbp_logz.h), gfx950
// only, float64.
//
// Four kernels; the first three are chosen from (X, n_in_slots, n_vars, flags) by mlbp_logz_pick_kernel:
//   logz_x64_kernel         X = 64, one workgroup of four waves per graph.  The graph's 2P + U in-slot messages are staged
//                           in LDS once (in in_slots order: LDS row q = message in_slots[q]).  The workgroup's waves then
//                           take the terms of log Z round-robin, a whole term per wave, so nothing but the final add
//                           crosses waves: a pairwise factor (leave-one-out vectors of its two variables into the wave's
//                           own 1 KiB of LDS, then the 32 KiB table streamed once, 16 bytes per lane and non-temporal: one
//                           load instruction covers two rows), a unary factor, or a variable.  Leave-one-out products are
//                           recomputed from the staged messages (d_v is small), never divided out: messages hold zeros.
//   logz_x64_shared_kernel  X = 64 and the caller claims shared tables: 16 graphs per workgroup.  Per pairwise factor the
//                           workgroup checks that its graphs name ONE table; if so the table is read once as the 16-entry
//                           register fragment of the sweep libraries (load_fragment of csrc/mlbp_graph_device.h: wave w owns
//                           rows 16w .. 16w+15) and contracted
//                           with the group's 16 pairs of leave-one-out vectors from LDS by vector FMAs; if not, every wave
//                           walks its four graphs' own tables as logz_x64_kernel does.  Messages are read from global memory
//                           (a variable's d_v messages are re-read d_v times within a few hundred cycles: L1 hits).
//   logz_generic_kernel     any X in [2, 1024]: one workgroup per graph, messages in global memory, tables streamed row by
//                           row with masked tails.  Correct first: the path for shapes nobody times.
//   logz_sum_kernel         the two batch sums, one workgroup, a fixed order.
// Every sum is float64; every cross-lane sum is mlbp_dev::wave_sum, so a result does not depend on the launch.
// No device-side mutable globals: everything comes through LogzDev.
// The device helpers and host checks shared with the other side libraries are in csrc/mlbp_graph_device.h and
// csrc/mlbp_graph_host.h.
#include <hip/hip_runtime.h>

#include "../../include/mlbp_logz.h"
#define MLBP_GRAPH_NO_SWEEPS                // this library reads finished messages: mlbp_logz.h has no op kinds
#include "../csrc/mlbp_graph_device.h"
#include "../csrc/mlbp_graph_host.h"

namespace {

using namespace mlbp_graph;

constexpr int GROUP = MLBP_LOGZ_GROUP;

struct LogzDev {
  const double* pair_tables; const int32_t* pair_tab;
  const double* unary_tables; const int32_t* unary_tab;
  const double* msgs;
  const int32_t* in_off; const int32_t* in_slots; const int32_t* pair_axis_var; const int32_t* unary_var;
  const int32_t* pair_in_slot; const int32_t* unary_in_slot; const int32_t* labels;
  double* log_z; double* score; double* joint_logp;
  int32_t B, X, n_msgs, P, U, n_vars, n_in, n_pair_tables, n_unary_tables;
};

typedef double nt_d2 __attribute__((ext_vector_type(2)));

// LDS written by some lanes of a wave and read by others of the SAME wave: LDS operations of one wave complete in order,
// so only the compiler has to be kept from moving them across this point.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// score at the labels of graph g, by one wave (every lane returns it): NaN when a label is outside [0, X).
__device__ __forceinline__ double wave_score(const LogzDev& d, int g, int lane) {
  const int32_t* lab = d.labels + (size_t)g * d.n_vars;
  const size_t X = (size_t)d.X;
  bool bad = false;
  for (int v = lane; v < d.n_vars; v += 64) bad |= (unsigned)lab[v] >= (unsigned)d.X;
  if (__any(bad)) return __builtin_nan("");
  double sc = 0.0;
  for (int p = lane; p < d.P; p += 64) {
    const int i = lab[d.pair_axis_var[2 * p]], j = lab[d.pair_axis_var[2 * p + 1]];
    sc += log(d.pair_tables[(size_t)d.pair_tab[(size_t)g * d.P + p] * X * X + (size_t)i * X + j]);
  }
  for (int u = lane; u < d.U; u += 64)
    sc += log(d.unary_tables[(size_t)d.unary_tab[(size_t)g * d.U + u] * X + lab[d.unary_var[u]]]);
  return wave_sum(sc);
}

// The outputs of graph g, by one whole wave; ok = its table indices are in range (else everything is NaN).
__device__ __forceinline__ void write_outputs(const LogzDev& d, int g, double lz, bool ok, int lane) {
  const bool want = d.labels && (d.score || d.joint_logp);
  double sc = __builtin_nan("");
  if (!ok) lz = sc;
  else if (want) sc = wave_score(d, g, lane);
  if (lane == 0) {
    if (d.log_z) d.log_z[g] = lz;
    if (want) {
      if (d.score) d.score[g] = sc;
      if (d.joint_logp) d.joint_logp[g] = sc - lz;
    }
  }
}

// prod over the in-slots of variable v, without slot `skip` (-1: none), at state `lane`; LDS row q holds message in_slots[q].
__device__ __forceinline__ double loo_lds(const double* msg, const_i32p in_off, const_i32p in_slots, int v, int skip, int lane) {
  double acc = 1.0;
  for (int q = in_off[v]; q < in_off[v + 1]; ++q)
    if (in_slots[q] != skip) acc *= msg[q * 64 + lane];
  return acc;
}

// The same from the graph's messages in global memory, X states, at state j.
__device__ __forceinline__ double loo_global(const double* gm, const_i32p in_off, const_i32p in_slots, int v, int skip, int X, int j) {
  double acc = 1.0;
  for (int q = in_off[v]; q < in_off[v + 1]; ++q) {
    const int s = in_slots[q];
    if (s != skip) acc *= gm[(size_t)s * X + j];
  }
  return acc;
}

// na^T . T . nb for one 64 x 64 table, by one wave, the table read once and past the caches: load k covers rows 2k and 2k + 1
// (1 KiB), lane l holds T[2k + (l >> 5)][2 (l & 31)], [.. + 1].  na, nb: LDS.
__device__ __forceinline__ double wave_bilinear_x64(const double* table, const double* na, const double* nb, int lane) {
  const double2 b = reinterpret_cast<const double2*>(nb)[lane & 31];
  const nt_d2* src = reinterpret_cast<const nt_d2*>(table) + lane;
  const double* a = na + (lane >> 5);
  double acc = 0.0;
#pragma unroll 8
  for (int k = 0; k < 32; ++k) {
    const nt_d2 v = __builtin_nontemporal_load(src + 64 * k);
    acc += a[2 * k] * (v.x * b.x + v.y * b.y);
  }
  return wave_sum(acc);
}

// ---- X = 64, one graph per workgroup ---------------------------------------------------------------
__global__ __launch_bounds__(WG) void logz_x64_kernel(LogzDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* msg = reinterpret_cast<double*>(smem);               // [n_in][64]
  double* vec = msg + (size_t)d.n_in * 64;                     // [4 waves][2][64] leave-one-out vectors of a pairwise factor
  double* part = vec + 512;                                    // [4] (+ padding) per-wave sums of log terms
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) {
    if (wave == 0) write_outputs(d, g, 0.0, false, lane);
    return;
  }
  const const_i32p in_off = as_const(d.in_off), in_slots = as_const(d.in_slots);
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const const_i32p pav = as_const(d.pair_axis_var), pis = as_const(d.pair_in_slot);
  const const_i32p uv = as_const(d.unary_var), uis = as_const(d.unary_in_slot);
  const double* gm = d.msgs + (size_t)g * d.n_msgs * 64;
  double2* msg2 = reinterpret_cast<double2*>(msg);
  for (int i = t; i < d.n_in * 32; i += WG)
    msg2[i] = reinterpret_cast<const double2*>(gm + (size_t)d.in_slots[i >> 5] * 64)[i & 31];
  __syncthreads();

  double* na = vec + wave * 128;
  double* nb = na + 64;
  double acc = 0.0;                                            // the same in every lane of the wave
  const int n_terms = d.P + d.U + d.n_vars;
  for (int term = wave; term < n_terms; term += WG / 64) {
    if (term < d.P) {
      const int p = term;
      na[lane] = loo_lds(msg, in_off, in_slots, pav[2 * p], pis[2 * p], lane);
      nb[lane] = loo_lds(msg, in_off, in_slots, pav[2 * p + 1], pis[2 * p + 1], lane);
      wave_lds_fence();
      acc += log(wave_bilinear_x64(d.pair_tables + (size_t)ptab[p] * 4096, na, nb, lane));
      wave_lds_fence();
    } else if (term < d.P + d.U) {
      const int u = term - d.P;
      const double n = loo_lds(msg, in_off, in_slots, uv[u], uis[u], lane);
      acc += log(wave_sum(d.unary_tables[(size_t)utab[u] * 64 + lane] * n));
    } else {
      const int v = term - d.P - d.U, dv = in_off[v + 1] - in_off[v];
      if (dv != 1) acc -= (double)(dv - 1) * log(wave_sum(loo_lds(msg, in_off, in_slots, v, -1, lane)));
    }
  }
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (wave == 0) write_outputs(d, g, (part[0] + part[1]) + (part[2] + part[3]), true, lane);
}

// ---- X = 64, 16 graphs per workgroup, tables shared -------------------------------------------------
__global__ __launch_bounds__(WG) void logz_x64_shared_kernel(LogzDev d) {
  __shared__ __attribute__((aligned(16))) double NA[GROUP * 64];      // [graph][state] leave-one-out vector on table axis 0
  __shared__ __attribute__((aligned(16))) double NB[GROUP * 64];      // ... on axis 1
  __shared__ double part[WG / 64][GROUP];                             // per-wave partial Z_f of the group's graphs
  __shared__ double sums[GROUP];                                      // per-graph sums of log terms
  const int g0 = blockIdx.x * GROUP, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const const_i32p in_off = as_const(d.in_off), in_slots = as_const(d.in_slots);
  const const_i32p pav = as_const(d.pair_axis_var), pis = as_const(d.pair_in_slot);
  const const_i32p uv = as_const(d.unary_var), uis = as_const(d.unary_in_slot);

  // lane l (and l + 16, ...) looks at graph g0 + (l & 15): inside the batch, table indices in range
  const int gl = g0 + (lane & 15);
  bool ok = gl < d.B;
  if (ok) {
    for (int p = 0; p < d.P; ++p) ok &= (unsigned)d.pair_tab[(size_t)gl * d.P + p] < (unsigned)d.n_pair_tables;
    for (int u = 0; u < d.U; ++u) ok &= (unsigned)d.unary_tab[(size_t)gl * d.U + u] < (unsigned)d.n_unary_tables;
  }
  const unsigned okmask = (unsigned)(__ballot(ok) & 0xFFFFull);        // wave-uniform, the same in all four waves

  // unary factors and variables: wave w walks graphs 4w .. 4w + 3
  double accw[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gi = 4 * wave + i;
    if (!((okmask >> gi) & 1)) continue;
    const int g = g0 + gi;
    const double* gm = d.msgs + (size_t)g * d.n_msgs * 64;
    const const_i32p utab = as_const(d.unary_tab) + (size_t)g * d.U;
    double acc = 0.0;
    for (int u = 0; u < d.U; ++u) {
      const double n = loo_global(gm, in_off, in_slots, uv[u], uis[u], 64, lane);
      acc += log(wave_sum(d.unary_tables[(size_t)utab[u] * 64 + lane] * n));
    }
    for (int v = 0; v < d.n_vars; ++v) {
      const int dv = in_off[v + 1] - in_off[v];
      if (dv != 1) acc -= (double)(dv - 1) * log(wave_sum(loo_global(gm, in_off, in_slots, v, -1, 64, lane)));
    }
    accw[i] = acc;
  }

  // pairwise factors
  double accB = 0.0;                                                   // wave 0, lane l < 16: graph g0 + l
  const int first = okmask ? __builtin_ctz(okmask) : 0;
  for (int p = 0; p < d.P && okmask; ++p) {
    const int tp = ok ? d.pair_tab[(size_t)gl * d.P + p] : -1;
    const int tfirst = __builtin_amdgcn_readlane(tp, first);
    const bool uniform = !__any(ok && tp != tfirst);
    double T[16];
    if (uniform) load_fragment(d.pair_tables + (size_t)tfirst * 4096, wave, lane, T);     // read once per workgroup
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gi = 4 * wave + i;
      double a = 0.0, b = 0.0;
      if ((okmask >> gi) & 1) {
        const double* gm = d.msgs + (size_t)(g0 + gi) * d.n_msgs * 64;
        a = loo_global(gm, in_off, in_slots, pav[2 * p], pis[2 * p], 64, lane);
        b = loo_global(gm, in_off, in_slots, pav[2 * p + 1], pis[2 * p + 1], 64, lane);
      }
      NA[gi * 64 + lane] = a;
      NB[gi * 64 + lane] = b;
    }
    __syncthreads();
    if (uniform) {
      double mine = 0.0;
      const int row0 = 16 * wave + (lane >> 5);
#pragma unroll
      for (int gg = 0; gg < GROUP; ++gg) {
        const double2 b = reinterpret_cast<const double2*>(NB)[gg * 32 + (lane & 31)];
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += NA[gg * 64 + row0 + 2 * k] * (T[2 * k] * b.x + T[2 * k + 1] * b.y);
        s = wave_sum(s);
        if (lane == gg) mine = s;
      }
      if (lane < GROUP) part[wave][lane] = mine;
      __syncthreads();
      if (wave == 0 && lane < GROUP && ok) accB += log((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]));
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int gi = 4 * wave + i;
        if (!((okmask >> gi) & 1)) continue;
        const int tg = as_const(d.pair_tab)[(size_t)(g0 + gi) * d.P + p];
        accw[i] += log(wave_bilinear_x64(d.pair_tables + (size_t)tg * 4096, NA + gi * 64, NB + gi * 64, lane));
      }
    }
    __syncthreads();                                                   // NA, NB and part are rewritten by the next factor
  }

  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) sums[4 * wave + i] = accw[i];
  }
  __syncthreads();
  if (wave == 0 && lane < GROUP) sums[lane] += accB;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gi = 4 * wave + i;
    if (g0 + gi < d.B) write_outputs(d, g0 + gi, sums[gi], (okmask >> gi) & 1, lane);
  }
}

// ---- any X -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void logz_generic_kernel(LogzDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X, Xp = (X + 1) & ~1;
  double* na = reinterpret_cast<double*>(smem);                // [Xp]
  double* nb = na + Xp;                                        // [Xp]
  double* scratch = nb + Xp;                                   // [4]
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) {
    if (wave == 0) write_outputs(d, g, 0.0, false, lane);
    return;
  }
  const const_i32p in_off = as_const(d.in_off), in_slots = as_const(d.in_slots);
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const const_i32p pav = as_const(d.pair_axis_var), pis = as_const(d.pair_in_slot);
  const const_i32p uv = as_const(d.unary_var), uis = as_const(d.unary_in_slot);
  const double* gm = d.msgs + (size_t)g * d.n_msgs * X;
  double acc = 0.0;                                            // the same in every thread
  for (int p = 0; p < d.P; ++p) {
    for (int j = t; j < X; j += WG) {
      na[j] = loo_global(gm, in_off, in_slots, pav[2 * p], pis[2 * p], X, j);
      nb[j] = loo_global(gm, in_off, in_slots, pav[2 * p + 1], pis[2 * p + 1], X, j);
    }
    __syncthreads();
    const double* T = d.pair_tables + (size_t)ptab[p] * X * X;
    double part = 0.0;
    for (int row = wave; row < X; row += WG / 64) {
      const double* Tr = T + (size_t)row * X;
      double s = 0.0;
      for (int j = lane; j < X; j += 64) s += __builtin_nontemporal_load(Tr + j) * nb[j];
      part += na[row] * s;
    }
    acc += log(block_sum(part, scratch));                      // (its barriers also fence na / nb before the next factor)
  }
  for (int u = 0; u < d.U; ++u) {
    const double* row = d.unary_tables + (size_t)utab[u] * X;
    double part = 0.0;
    for (int j = t; j < X; j += WG) part += row[j] * loo_global(gm, in_off, in_slots, uv[u], uis[u], X, j);
    acc += log(block_sum(part, scratch));
  }
  for (int v = 0; v < d.n_vars; ++v) {
    const int dv = in_off[v + 1] - in_off[v];
    if (dv == 1) continue;
    double part = 0.0;
    for (int j = t; j < X; j += WG) part += loo_global(gm, in_off, in_slots, v, -1, X, j);
    acc -= (double)(dv - 1) * log(block_sum(part, scratch));
  }
  if (wave == 0) write_outputs(d, g, acc, true, lane);
}

// ---- the batch sums ----------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void logz_sum_kernel(const double* log_z, const double* joint_logp, int B, double* out) {
  __shared__ double scratch[4];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < B; i += WG) {
    a += log_z[i];
    if (joint_logp) b += joint_logp[i];
  }
  a = block_sum(a, scratch);
  b = block_sum(b, scratch);
  if (threadIdx.x == 0) {
    out[0] = a;
    out[1] = b;
  }
}

// ---- host ----------------------------------------------------------------------------------------
thread_local int g_last_kernel = MLBP_LOGZ_KERNEL_NONE;

int64_t x64_lds_bytes(int64_t n_in) { return n_in * 512 + 4096 + 64; }

// slot is one of the in-slots of variable v
bool is_in_slot_of(const int32_t* in_off, const int32_t* in_slots, int v, int slot) {
  for (int q = in_off[v]; q < in_off[v + 1]; ++q)
    if (in_slots[q] == slot) return true;
  return false;
}

}  // namespace

extern "C" {

const char* mlbp_logz_arch(void) { return "gfx950"; }
const char* mlbp_logz_last_error(void) { return g_last_error.c_str(); }
int mlbp_logz_last_kernel(void) { return g_last_kernel; }

int mlbp_logz_pick_kernel(int32_t X, int32_t n_in_slots, int32_t n_vars, int32_t flags) {
  if (X < 2 || n_in_slots <= 0 || n_vars <= 0)
    return fail(MLBP_EINVAL, "pick_kernel: X = %d, n_in_slots = %d, n_vars = %d", X, n_in_slots, n_vars);
  if (flags & ~MLBP_LOGZ_SHARED_PAIR_TABLES) return fail(MLBP_EINVAL, "pick_kernel: unknown flags 0x%x", flags);
  if (X > MLBP_LOGZ_MAX_X) return fail(MLBP_EUNSUPPORTED, "X = %d: at most %d states are supported", X, MLBP_LOGZ_MAX_X);
  if (X == 64 && (flags & MLBP_LOGZ_SHARED_PAIR_TABLES)) return MLBP_LOGZ_KERNEL_X64_SHARED;
  if (X == 64 && x64_lds_bytes(n_in_slots) <= MLBP_LOGZ_X64_LDS_BYTES) return MLBP_LOGZ_KERNEL_X64;
  return MLBP_LOGZ_KERNEL_GENERIC;
}

int mlbp_logz_check_readout(int32_t n_vars, const int32_t* in_off, const int32_t* in_slots, int32_t n_msgs, int32_t P,
                            const int32_t* pair_axis_var, const int32_t* pair_in_slot, int32_t U, const int32_t* unary_var,
                            const int32_t* unary_in_slot) {
  if (int e = check_in_slots_present(in_off, in_slots)) return e;
  if (n_vars <= 0 || n_msgs <= 0 || P < 0 || U < 0 || P + U <= 0 || (P > 0 && (!pair_axis_var || !pair_in_slot)) ||
      (U > 0 && (!unary_var || !unary_in_slot)))
    return fail(MLBP_EINVAL, "read-out: bad sizes (n_vars %d, n_msgs %d, P %d, U %d) or a NULL array", n_vars, n_msgs, P, U);
  const int rc = check_in_slots(n_vars, in_off, in_slots, n_msgs, [&](int v) -> int {
    if ((int64_t)in_off[v + 1] > 2 * (int64_t)P + U)
      return fail(MLBP_EINVAL, "read-out: in_off[%d] = %d beyond the 2 P + U = %d in-slots", v + 1, in_off[v + 1], 2 * P + U);
    return MLBP_OK;
  });
  if (rc) return rc;
  if (in_off[n_vars] != 2 * P + U)
    return fail(MLBP_EINVAL, "read-out: in_off[n_vars] = %d, but 2 P + U = %d in-slots", in_off[n_vars], 2 * P + U);
  for (int i = 0; i < 2 * P; ++i) {
    const int v = pair_axis_var[i];
    if (v < 0 || v >= n_vars) return fail(MLBP_EINVAL, "read-out: pair factor %d: variable %d out of [0,%d)", i / 2, v, n_vars);
    if (!is_in_slot_of(in_off, in_slots, v, pair_in_slot[i]))
      return fail(MLBP_EINVAL, "read-out: pair factor %d: slot %d is no in-slot of variable %d", i / 2, pair_in_slot[i], v);
  }
  for (int u = 0; u < U; ++u) {
    const int v = unary_var[u];
    if (v < 0 || v >= n_vars) return fail(MLBP_EINVAL, "read-out: unary factor %d: variable %d out of [0,%d)", u, v, n_vars);
    if (!is_in_slot_of(in_off, in_slots, v, unary_in_slot[u]))
      return fail(MLBP_EINVAL, "read-out: unary factor %d: slot %d is no in-slot of variable %d", u, unary_in_slot[u], v);
  }
  return MLBP_OK;
}

int mlbp_logz_f64(const mlbp_logz_args* a, void* stream) {
  g_last_kernel = MLBP_LOGZ_KERNEL_NONE;
  if (!a) return fail(MLBP_EINVAL, "args is NULL");
  if (a->B <= 0 || a->n_msgs <= 0 || a->n_vars <= 0 || a->P < 0 || a->U < 0 || a->P + a->U <= 0)
    return fail(MLBP_EINVAL, "bad sizes: B %d, n_msgs %d, n_vars %d, P %d, U %d", a->B, a->n_msgs, a->n_vars, a->P, a->U);
  if (int e = check_states(a->X)) return e;
  const int64_t n_in = 2 * (int64_t)a->P + a->U;
  if (n_in > 0x7fffffff / 64) return fail(MLBP_EUNSUPPORTED, "2 P + U = %lld in-slots: too many", (long long)n_in);
  const int which = mlbp_logz_pick_kernel(a->X, (int32_t)n_in, a->n_vars, a->flags);
  if (which < 0) return which;
  if (!a->msgs) return fail(MLBP_EINVAL, "msgs is NULL");
  if (int e = check_args_in_slots(a)) return e;
  if (int e = check_args_tables(a, !a->pair_axis_var || !a->pair_in_slot, "pair_tables, pair_tab, pair_axis_var or pair_in_slot",
                                !a->unary_var || !a->unary_in_slot, "unary_tables, unary_tab, unary_var or unary_in_slot")) return e;
  if (!a->log_z && !a->score && !a->joint_logp) return fail(MLBP_EINVAL, "nothing to compute: log_z, score and joint_logp are NULL");
  if ((a->score || a->joint_logp) && !a->labels) return fail(MLBP_EINVAL, "score and joint_logp need labels");
  if (a->sum_out && !a->log_z) return fail(MLBP_EINVAL, "sum_out needs log_z");
  if (int e = check_args_extent(a)) return e;
  if (int e = check_device("libmlbp_logz.so")) return e;
  LogzDev d;
  d.pair_tables = a->pair_tables; d.pair_tab = a->pair_tab; d.unary_tables = a->unary_tables; d.unary_tab = a->unary_tab;
  d.msgs = a->msgs; d.in_off = a->in_off; d.in_slots = a->in_slots; d.pair_axis_var = a->pair_axis_var; d.unary_var = a->unary_var;
  d.pair_in_slot = a->pair_in_slot; d.unary_in_slot = a->unary_in_slot; d.labels = a->labels;
  d.log_z = a->log_z; d.score = a->score; d.joint_logp = a->joint_logp;
  d.B = a->B; d.X = a->X; d.n_msgs = a->n_msgs; d.P = a->P; d.U = a->U; d.n_vars = a->n_vars; d.n_in = (int32_t)n_in;
  d.n_pair_tables = a->n_pair_tables; d.n_unary_tables = a->n_unary_tables;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  if (which == MLBP_LOGZ_KERNEL_X64_SHARED) {
    hipLaunchKernelGGL(logz_x64_shared_kernel, dim3((a->B + GROUP - 1) / GROUP), dim3(WG), 0, st, d);
  } else if (which == MLBP_LOGZ_KERNEL_X64) {
    hipLaunchKernelGGL(logz_x64_kernel, dim3(a->B), dim3(WG), (size_t)x64_lds_bytes(n_in), st, d);
  } else {
    const size_t lds = (size_t)((a->X + 1) & ~1) * 16 + 32;
    hipLaunchKernelGGL(logz_generic_kernel, dim3(a->B), dim3(WG), lds, st, d);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MLBP_EHIP, "log-partition launch failed: %s", hipGetErrorString(e));
  if (a->sum_out) {
    hipLaunchKernelGGL(logz_sum_kernel, dim3(1), dim3(WG), 0, st, (const double*)a->log_z, (const double*)a->joint_logp, a->B, a->sum_out);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(MLBP_EHIP, "batch-sum launch failed: %s", hipGetErrorString(e));
  }
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
