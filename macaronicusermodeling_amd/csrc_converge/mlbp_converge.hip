// libmlbp_converge.so: sum-product sweeps to convergence with a per-graph residual and early exit (include/mlbp_converge.h),
// gfx950 only, float64.
//
// Two kernels, chosen from (X, n_msgs) by mlbp_converge_pick_kernel, both one workgroup of 256 threads per graph:
//   converge_x64_kernel<RESIDENT>  X = 64, four waves, messages in LDS for the whole launch.  A pairwise table is split over the
//                                  256 threads as 16 entries each (load_fragment of csrc/mlbp_graph_device.h, which also holds
//                                  the two contractions and the per-op step; here they run with SumOp, as in the sampler).
//                                  RESIDENT (P <= 3): all tables are loaded once per workgroup and stay in registers over every
//                                  round; otherwise the 16 entries are loaded per update (streamed).
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
// The host checks shared with the other side libraries are in csrc/mlbp_graph_host.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/mlbp_converge.h"
#include "../csrc/mlbp_graph_device.h"
#include "../csrc/mlbp_graph_host.h"

namespace {

using namespace mlbp_graph;

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
  // max-product mode: the tag of the round loop, and the decode of mlbp_map.h from the final messages (assignment and score come
  // together, and only with max_product)
  int32_t max_product;
  const int32_t* pair_axis_var; const int32_t* unary_var;
  int32_t* assignment; double* score;
};

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

// The variables the decode's index arrays name are variables of the graph (device data, like the table indices; wave-uniform:
// scalar loads).  Without a decode nothing is read.
__device__ __forceinline__ bool decode_in_range(const ConvergeDev& d) {
  if (!d.assignment) return true;
  bool ok = true;
  const const_i32p pav = as_const(d.pair_axis_var), uv = as_const(d.unary_var);
  for (int i = 0; i < 2 * d.P; ++i) ok &= (unsigned)pav[i] < (unsigned)d.n_vars;
  for (int u = 0; u < d.U; ++u) ok &= (unsigned)uv[u] < (unsigned)d.n_vars;
  return ok;
}

// What a refused graph returns (mlbp_converge.h): rounds -1, residual NaN, its history row NaN, assignment -1 and score NaN;
// messages and marginals untouched.
__device__ __forceinline__ void refuse_graph(const ConvergeDev& d, int g) {
  if (threadIdx.x == 0) {
    d.rounds[g] = -1;
    d.residual[g] = __builtin_nan("");
    if (d.score) d.score[g] = __builtin_nan("");
  }
  if (d.assignment)
    for (int v = threadIdx.x; v < d.n_vars; v += WG) d.assignment[(size_t)g * d.n_vars + v] = -1;
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

template <bool RESIDENT>
__global__ __launch_bounds__(WG) void converge_x64_kernel(ConvergeDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* msg = reinterpret_cast<double*>(smem);               // [n_msgs][64]
  double* part = msg + (size_t)d.n_msgs * 64;                  // [8][64] partial sums of an m^T.T update
  double* raw = part + 512;                                    // [64] un-normalised result of a T.m update
  double* res_word = raw + 64;                                 // [1] the round's residual, read by every thread
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g) || !decode_in_range(d)) {
    refuse_graph(d, g);
    return;                                                    // (block-uniform: the whole workgroup leaves)
  }
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const const_i32p c_ops = as_const(d.ops), c_sweeps = as_const(d.sweeps);
  const const_i32p in_off = as_const(d.in_off), in_slots = as_const(d.in_slots);
  const double uniform = 1.0 / 64.0;
  const StepGraph G = {d.pair_tables, ptab, d.unary_tables, utab, as_const(d.srcs), msg, part, raw};

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
  if (d.max_product) {                                         // (workgroup-uniform) the same rounds over MaxOp, a loop of its own
    while (true) {
      rmax = 0.0;
      for (int sw = 0; sw < d.n_sweeps; ++sw) {
        const int op0 = c_sweeps[2 * sw], nop = c_sweeps[2 * sw + 1];
        for (int o = op0; o < op0 + nop; ++o) {
          const int kind = c_ops[4 * o], a = c_ops[4 * o + 1], b = c_ops[4 * o + 2], c = c_ops[4 * o + 3];
          if (kind == MLBP_OP_UNARY && rounds > 0 && unary_once(once_mask, o)) continue;
          x64_step<MaxOp, RESIDENT>(G, R, kind, a, b, c, wave, lane, FreeState(), finish);
        }
      }
      if (wave == 0) {                                         // the residual and the stop: as in the sum loop below
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
      __syncthreads();
    }
  } else
  while (true) {                                               // every thread takes the same number of turns: see below
    rmax = 0.0;
    for (int sw = 0; sw < d.n_sweeps; ++sw) {
      const int op0 = c_sweeps[2 * sw], nop = c_sweeps[2 * sw + 1];
      for (int o = op0; o < op0 + nop; ++o) {
        const int kind = c_ops[4 * o], a = c_ops[4 * o + 1], b = c_ops[4 * o + 2], c = c_ops[4 * o + 3];
        if (kind == MLBP_OP_UNARY && rounds > 0 && unary_once(once_mask, o)) continue;      // (uniform: no barrier is skipped by some)
        x64_step<SumOp, RESIDENT>(G, R, kind, a, b, c, wave, lane, FreeState(), finish);
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
    for (int v = wave; v < d.n_vars; v += WG / 64)             // one variable per wave, lane = state
      d.marginals[((size_t)g * d.n_vars + v) * 64 + lane] = x64_marginal(msg, in_off, in_slots, v, lane);
  }
  if (d.assignment) {
    // The decode of map_sweep_x64_kernel, op for op, so that the same messages give the same bits: one variable per wave, lane =
    // state, the lowest lane at the wave's maximum; then wave 0 adds the log table entries.  The assignment lives in `part`, free
    // since the last round (the host admits n_vars <= 1024 here: part holds 1024 words).
    int32_t* xs = reinterpret_cast<int32_t*>(part);
    for (int v = wave; v < d.n_vars; v += WG / 64) {
      const double mm = x64_marginal(msg, in_off, in_slots, v, lane);
      const unsigned long long at_max = __ballot(mm == wave_max(mm));
      if (lane == 0) xs[v] = at_max ? __builtin_ctzll(at_max) : 0;           // ties go to the lowest index
    }
    __syncthreads();
    for (int v = t; v < d.n_vars; v += WG) d.assignment[(size_t)g * d.n_vars + v] = xs[v];
    if (wave == 0) {
      double sc = 0.0;
      for (int p = lane; p < d.P; p += 64) {
        const int i = xs[d.pair_axis_var[2 * p]], j = xs[d.pair_axis_var[2 * p + 1]];
        sc += log(d.pair_tables[(size_t)ptab[p] * 4096 + i * 64 + j]);
      }
      for (int u = lane; u < d.U; u += 64) sc += log(d.unary_tables[(size_t)utab[u] * 64 + xs[d.unary_var[u]]]);
      sc = wave_sum(sc);
      if (lane == 0) d.score[g] = sc;
    }
  }
}

// ---- any X ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void converge_generic_kernel(ConvergeDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X;
  double* raw = reinterpret_cast<double*>(smem);               // [X] (X rounded up to even)
  double* scratch = raw + ((X + 1) & ~1);                      // [4] block sums
  double* wave_res = scratch + 4;                              // [4] the waves' maxima of the round
  int32_t* best_i = reinterpret_cast<int32_t*>(wave_res + 4);  // the decode only: [4] per-wave lowest index at the maximum
  int32_t* xs = best_i + 4;                                    //                  [n_vars] the assignment
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g) || !decode_in_range(d)) {
    refuse_graph(d, g);
    return;
  }
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const const_i32p c_ops = as_const(d.ops), c_sweeps = as_const(d.sweeps);
  const const_i32p in_off = as_const(d.in_off), in_slots = as_const(d.in_slots);
  const double uniform = 1.0 / (double)X;
  // only this workgroup touches its messages
  double* msg = d.msgs + (size_t)g * d.n_msgs * X;
  const StepGraph G = {d.pair_tables, ptab, d.unary_tables, utab, as_const(d.srcs), msg, nullptr, raw};
  if (d.init)
    for (int i = t; i < d.n_msgs * X; i += WG) msg[i] = uniform;
  __syncthreads();
  int rounds = 0;
  double res = 0.0;
  if (d.max_product) {                                         // (workgroup-uniform) the same rounds over MaxOp, a loop of its own
    while (true) {
      double rmax = 0.0;
      for (int sw = 0; sw < d.n_sweeps; ++sw) {
        const int op0 = c_sweeps[2 * sw], nop = c_sweeps[2 * sw + 1];
        for (int o = op0; o < op0 + nop; ++o) {
          const int kind = c_ops[4 * o], a = c_ops[4 * o + 1], b = c_ops[4 * o + 2], c = c_ops[4 * o + 3];
          generic_step<MaxOp>(G, X, uniform, kind, a, b, c, FreeState());
          double* out = msg + (size_t)c * X;
          generic_finish(raw, X, uniform, true, scratch, [&](int j, double fresh) {
            rmax = fmax(rmax, entry_delta(fresh, out[j]));
            out[j] = fresh;
          });
        }
      }
      rmax = wave_max(rmax);                                   // the residual and the stop: as in the sum loop below
      if (lane == 0) wave_res[wave] = rmax;
      __syncthreads();
      res = fmax(fmax(wave_res[0], wave_res[1]), fmax(wave_res[2], wave_res[3]));
      if (t == 0 && d.history) d.history[(size_t)g * d.max_rounds + rounds] = res;
      ++rounds;
      if (res <= d.tol || rounds >= d.max_rounds) break;
      __syncthreads();
    }
  } else
  while (true) {
    double rmax = 0.0;                                         // over the entries this thread writes
    for (int sw = 0; sw < d.n_sweeps; ++sw) {
      const int op0 = c_sweeps[2 * sw], nop = c_sweeps[2 * sw + 1];
      for (int o = op0; o < op0 + nop; ++o) {
        const int kind = c_ops[4 * o], a = c_ops[4 * o + 1], b = c_ops[4 * o + 2], c = c_ops[4 * o + 3];
        generic_step<SumOp>(G, X, uniform, kind, a, b, c, FreeState());
        double* out = msg + (size_t)c * X;
        generic_finish(raw, X, uniform, true, scratch, [&](int j, double fresh) {
          rmax = fmax(rmax, entry_delta(fresh, out[j]));
          out[j] = fresh;
        });
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
      generic_marginal(msg, in_off, in_slots, v, X, uniform, raw, scratch,
                       [&](int j, double m) { d.marginals[((size_t)g * d.n_vars + v) * X + j] = m; });
      __syncthreads();
    }
  }
  if (d.assignment) {
    // The decode of map_sweep_generic_kernel, op for op.  wave_res is free since the last round: the waves' maxima go there.
    __syncthreads();                                           // (every thread has read wave_res)
    const double ninf = -__builtin_huge_val();
    for (int v = 0; v < d.n_vars; ++v) {
      double best = ninf;
      int at = 0x7fffffff;
      generic_marginal(msg, in_off, in_slots, v, X, uniform, raw, scratch, [&](int j, double mm) {
        if (mm > best) { best = mm; at = j; }                  // ascending j and a strict compare: the lowest index wins
      });
      const double wbest = wave_max(best);
      int cand = best == wbest ? at : 0x7fffffff;
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) cand = min(cand, __shfl_xor(cand, m, 64));
      if (lane == 0) { wave_res[wave] = wbest; best_i[wave] = cand; }
      __syncthreads();
      if (t == 0) {
        double bv = wave_res[0];
        int bi = best_i[0];
        for (int w = 1; w < WG / 64; ++w)
          if (wave_res[w] > bv || (wave_res[w] == bv && best_i[w] < bi)) { bv = wave_res[w]; bi = best_i[w]; }
        xs[v] = bi < X ? bi : 0;
      }
      __syncthreads();
    }
    for (int v = t; v < d.n_vars; v += WG) d.assignment[(size_t)g * d.n_vars + v] = xs[v];
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
thread_local int g_last_kernel = MLBP_CONVERGE_KERNEL_NONE;

int64_t x64_lds_bytes(int32_t n_msgs) { return (int64_t)n_msgs * 512 + 4608 + 8; }

size_t generic_lds_bytes(int32_t X) { return (size_t)((X + 1) & ~1) * 8 + 8 * 8; }

// What the generic kernel's decode adds behind that: four candidate indices and the assignment.
size_t generic_decode_lds_bytes(int32_t n_vars) { return 4 * 4 + 4 * (size_t)n_vars; }

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
  if (int e = check_program_sizes(ops, n_ops, srcs, n_srcs, sweeps, n_sweeps, n_msgs, P, U)) return e;
  if (int e = check_program_indices(ops, n_ops, srcs, n_srcs, sweeps, n_sweeps, n_msgs, P, U, NoMoreChecks())) return e;
  std::vector<char> covered((size_t)n_msgs, 0);
  for (int s = 0; s < n_sweeps; ++s)
    for (int o = sweeps[2 * s]; o < sweeps[2 * s] + sweeps[2 * s + 1]; ++o) covered[ops[4 * o + 3]] = 1;
  for (int k = 0; k < n_msgs; ++k)
    if (!covered[k])
      return fail(MLBP_EINVAL, "coverage: message slot %d is the destination of no op of the round: the residual would say nothing about it", k);
  return MLBP_OK;
}

int mlbp_converge_check_readout(int32_t n_vars, const int32_t* in_off, const int32_t* in_slots, int32_t n_msgs) {
  return check_readout_in_slots(n_vars, in_off, in_slots, n_msgs);
}

int mlbp_converge_f64(const mlbp_converge_args* a, void* stream) {
  g_last_kernel = MLBP_CONVERGE_KERNEL_NONE;
  if (int e = check_args_sizes(a)) return e;
  if (int e = check_states(a->X)) return e;
  if (!a->normalize_messages)
    return fail(MLBP_EINVAL, "normalize_messages = 0: a residual on unnormalised messages has no scale");
  if (!std::isfinite(a->tol) || a->tol < 0.0) return fail(MLBP_EINVAL, "tol = %g: must be finite and at least 0", a->tol);
  if (a->max_rounds < 1 || a->max_rounds > MLBP_CONVERGE_MAX_ROUNDS)
    return fail(MLBP_EINVAL, "max_rounds = %d out of [1, %d]", a->max_rounds, MLBP_CONVERGE_MAX_ROUNDS);
  const int which = mlbp_converge_pick_kernel(a->X, a->n_msgs, a->n_vars);
  if (which < 0) return which;
  if (int e = check_args_program(a)) return e;
  if (!a->msgs) return fail(MLBP_EINVAL, "msgs is NULL");
  if (!a->rounds || !a->residual) return fail(MLBP_EINVAL, "rounds or residual is NULL");
  if (int e = check_args_tables(a)) return e;
  if (int e = check_args_extent(a)) return e;
  const bool decode = a->assignment || a->score;
  if (a->max_product && decode) {
    if (!a->assignment) return fail(MLBP_EINVAL, "score without assignment: the decode returns both");
    if (!a->score) return fail(MLBP_EINVAL, "assignment without score: the decode returns both");
    if (a->P > 0 && !a->pair_axis_var) return fail(MLBP_EINVAL, "P = %d and assignment given but pair_axis_var is NULL", a->P);
    if (a->U > 0 && !a->unary_var) return fail(MLBP_EINVAL, "U = %d and assignment given but unary_var is NULL", a->U);
    if (which == MLBP_CONVERGE_KERNEL_X64 && a->n_vars > 1024)
      return fail(MLBP_EUNSUPPORTED, "n_vars = %d: the X = 64 kernel's assignment holds at most 1024 variables", a->n_vars);
    if (which == MLBP_CONVERGE_KERNEL_GENERIC && generic_lds_bytes(a->X) + generic_decode_lds_bytes(a->n_vars) > 65536)
      return fail(MLBP_EUNSUPPORTED, "n_vars = %d: the generic kernel's assignment does not fit LDS", a->n_vars);
  }
  if (int e = check_device("libmlbp_converge.so")) return e;
  // (behind the device check: a call that sets every pointer and no mode has always reached it)
  if (!a->max_product && decode) return fail(MLBP_EINVAL, "assignment or score without max_product: the sum-product rounds decode nothing");
  ConvergeDev d;
  d.pair_tables = a->pair_tables; d.pair_tab = a->pair_tab; d.unary_tables = a->unary_tables; d.unary_tab = a->unary_tab;
  d.ops = a->ops; d.srcs = a->srcs; d.sweeps = a->sweeps;
  d.in_off = a->in_off; d.in_slots = a->in_slots;
  d.msgs = a->msgs; d.rounds = a->rounds; d.residual = a->residual; d.marginals = a->marginals; d.history = a->history;
  d.tol = a->tol;
  d.n_sweeps = a->n_sweeps; d.n_msgs = a->n_msgs; d.P = a->P; d.U = a->U; d.X = a->X; d.n_vars = a->n_vars;
  d.n_pair_tables = a->n_pair_tables; d.n_unary_tables = a->n_unary_tables;
  d.init = a->init_messages != 0; d.max_rounds = a->max_rounds; d.n_ops = a->n_ops;
  d.max_product = a->max_product != 0;
  d.pair_axis_var = a->pair_axis_var; d.unary_var = a->unary_var; d.assignment = a->assignment; d.score = a->score;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  if (which == MLBP_CONVERGE_KERNEL_X64) {
    const bool resident = a->P <= 3;
    auto k = resident ? converge_x64_kernel<true> : converge_x64_kernel<false>;
    if (int e = grant_x64_lds((const void*)k, resident ? 1 : 0, MLBP_CONVERGE_X64_LDS_BYTES)) return e;
    hipLaunchKernelGGL(k, dim3(a->B), dim3(WG), (size_t)x64_lds_bytes(a->n_msgs), st, d);
  } else {
    const size_t lds = generic_lds_bytes(a->X) + (decode ? generic_decode_lds_bytes(a->n_vars) : 0);
    hipLaunchKernelGGL(converge_generic_kernel, dim3(a->B), dim3(WG), lds, st, d);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MLBP_EHIP, "converge launch failed: %s", hipGetErrorString(e));
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
