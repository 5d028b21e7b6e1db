// libmlbp_sample.so: posterior sampling of whole assignments by sequential conditioning (include/mlbp_sample.h), gfx950 only,
// float64.
//
// Two kernels, chosen from (X, n_msgs, n_vars) by mlbp_sample_pick_kernel, both on a grid of (B, C) workgroups: workgroup
// (g, c) serves graph g and draws its samples c, c + C, ...
//   sample_x64_kernel<RESIDENT>  X = 64, four waves, messages in LDS for the whole launch.  A pairwise table is split over the
//                                256 threads as 16 entries each (load_fragment of csrc/mlbp_graph_device.h, which also holds the
//                                two contractions; here they run with SumOp).  RESIDENT (P <= 3): all tables are loaded once
//                                per workgroup and stay in registers over every step of every sample; otherwise the 16 entries
//                                are loaded per update (streamed).  A clamped variable is an int in LDS: a VAR op keeps
//                                lane == x ? acc : 0 of its outgoing message (the generic kernel hands the shared step the same
//                                int as its state_of).
//                                The draw runs in wave 0 with lane = state: inclusive scan, total from lane 63, ballot of c > t.
//                                The marginal of step 0 (no variable clamped yet: the same for every sample) is computed for the
//                                workgroup's first sample and kept in LDS.
//   sample_generic_kernel        any X in [2, 1024]: messages in the caller's workspace, tables streamed, the draw a serial
//                                scan by one thread over the LDS copy of the marginal.  Correct first: the path for shapes
//                                nobody times.
// No device-side mutable globals: everything comes through SampleDev.
// The host checks shared with the other side libraries are in csrc/mlbp_graph_host.h.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/mlbp_sample.h"
#include "../csrc/mlbp_graph_device.h"
#include "../csrc/mlbp_graph_host.h"

namespace {

using namespace mlbp_graph;

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
  bool ok = tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g);
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
            // x64_step of mlbp_graph_device.h with the clamp, written out: through the helper this kernel alone ran 1.3 % slower
            // (LAB_NOTES R14.4)
            if (kind == MLBP_OP_PAIR_TM || kind == MLBP_OP_PAIR_MT) {
              const double* m = msg + b * 64;
              const bool tm = kind == MLBP_OP_PAIR_TM;
              if (RESIDENT) {
                if (a == 0) pair_contract<SumOp>(R[0], tm, m, part, raw, wave, lane);
                else if (a == 1) pair_contract<SumOp>(R[1], tm, m, part, raw, wave, lane);
                else pair_contract<SumOp>(R[2], tm, m, part, raw, wave, lane);
              } else {
                double T[16];
                load_fragment(d.pair_tables + (size_t)ptab[a] * 4096, wave, lane, T);
                pair_contract<SumOp>(T, tm, m, part, raw, wave, lane);
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
          m = x64_marginal(msg, in_off, in_slots, v, lane);
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
__global__ __launch_bounds__(WG) void sample_generic_kernel(SampleDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X;
  double* raw = reinterpret_cast<double*>(smem);               // [X] (X rounded up to even)
  double* scratch = raw + ((X + 1) & ~1);                      // [4] block sums
  double* logq_s = scratch + 4;                                // [1] thread 0's running log q
  int32_t* clamp = reinterpret_cast<int32_t*>(logq_s + 1);     // [n_vars]
  const int g = blockIdx.x, t = threadIdx.x;
  if (!graph_in_range(d, g)) {
    refuse_graph(d, g);
    return;
  }
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const const_i32p c_ops = as_const(d.ops), c_sweeps = as_const(d.sweeps);
  const const_i32p in_off = as_const(d.in_off), in_slots = as_const(d.in_slots);
  const const_i32p slot_var = as_const(d.slot_var), order = as_const(d.order);
  const double uniform = 1.0 / (double)X;
  const bool norm = d.normalize != 0;
  // only this workgroup touches its messages
  double* msg = d.workspace + ((size_t)g * gridDim.y + blockIdx.y) * (size_t)d.n_msgs * X;
  const StepGraph G = {d.pair_tables, ptab, d.unary_tables, utab, as_const(d.srcs), msg, nullptr, raw};
  auto state_of = [&](int slot) { return clamp[slot_var[slot]]; };
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
          generic_step<SumOp>(G, X, uniform, kind, a, b, c, state_of);
          double* out = msg + (size_t)c * X;
          generic_finish(raw, X, uniform, norm, scratch, [&](int j, double fresh) { out[j] = fresh; });
        }
      }
      // the marginal of v -> raw, the draw by thread 0
      generic_marginal(msg, in_off, in_slots, v, X, uniform, raw, scratch, [&](int j, double mm) {
        raw[j] = mm;
        if (d.cond_marginals) d.cond_marginals[(sg * d.n_vars + v) * X + j] = mm;
      });
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
thread_local int g_last_kernel = MLBP_SAMPLE_KERNEL_NONE;

int64_t x64_lds_bytes(int32_t n_msgs, int32_t n_vars) {
  return (int64_t)n_msgs * 512 + 4608 + 512 + 4 * (((int64_t)n_vars + 3) & ~(int64_t)3);
}

size_t generic_lds_bytes(int32_t X, int32_t n_vars) {
  return (size_t)((X + 1) & ~1) * 8 + 5 * 8 + 4 * (size_t)n_vars;
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
  const int rc = check_program_indices(ops, n_ops, srcs, n_srcs, sweeps, n_sweeps, n_msgs, P, U, [&](int o, int kind, int c) -> int {
    if (kind == MLBP_OP_VAR) {
      if (slot_var[c] < 0 || slot_var[c] >= n_vars)
        return fail(MLBP_EINVAL, "op %d: destination slot %d of a variable update has no source variable (slot_var %d, n_vars %d)", o, c, slot_var[c], n_vars);
    } else if (slot_var[c] != -1) {
      return fail(MLBP_EINVAL, "op %d: destination slot %d of a factor update has slot_var %d, not -1", o, c, slot_var[c]);
    }
    return MLBP_OK;
  });
  if (rc) return rc;
  std::vector<char> seen((size_t)n_vars, 0);
  for (int k = 0; k < n_vars; ++k) {
    if (order[k] < 0 || order[k] >= n_vars || seen[order[k]])
      return fail(MLBP_EINVAL, "order is not a permutation: order[%d] = %d (n_vars %d)", k, order[k], n_vars);
    seen[order[k]] = 1;
  }
  return MLBP_OK;
}

int mlbp_sample_check_readout(int32_t n_vars, const int32_t* in_off, const int32_t* in_slots, int32_t n_msgs) {
  return check_readout_in_slots(n_vars, in_off, in_slots, n_msgs);
}

int mlbp_sample_f64(const mlbp_sample_args* a, void* stream) {
  g_last_kernel = MLBP_SAMPLE_KERNEL_NONE;
  if (int e = check_args_sizes(a)) return e;
  if (a->S <= 0) return fail(MLBP_EINVAL, "S = %d: at least one sample per graph", a->S);
  if (int e = check_states(a->X)) return e;
  const int which = mlbp_sample_pick_kernel(a->X, a->n_msgs, a->n_vars);
  if (which < 0) return which;
  if (int e = check_args_program(a)) return e;
  if (!a->slot_var || !a->order) return fail(MLBP_EINVAL, "slot_var or order is NULL");
  if (!a->uniforms) return fail(MLBP_EINVAL, "uniforms is NULL");
  if (!a->samples || !a->logq) return fail(MLBP_EINVAL, "samples or logq is NULL");
  if (int e = check_args_tables(a)) return e;
  if (int e = check_args_extent(a)) return e;
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
  if (int e = check_device("libmlbp_sample.so")) return e;
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
    if (int e = grant_x64_lds((const void*)k, resident ? 1 : 0, MLBP_SAMPLE_X64_LDS_BYTES)) return e;
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
