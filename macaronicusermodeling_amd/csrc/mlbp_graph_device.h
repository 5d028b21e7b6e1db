// Device helpers shared by the side libraries (libmlbp_map.so, libmlbp_logz.so, libmlbp_sample.so, libmlbp_converge.so,
// libmlbp_cutset.so, libmlbp_exactmap.so; gfx950 only): the reductions, the X = 64 table fragment and its two contractions, one sweep op in the X = 64 and in the generic
// form, and a variable's marginal from its in-slots.  The contractions and the steps take the combining operation as a tag:
// SumOp for sum-product, MaxOp for max-product.  Helpers only, no __global__ function: every library keeps its own kernels,
// which own the round / sample loops, the read-out, the refusal and the LDS carve-up.  Not part of the ABI.
// Include after the library's public header (the MLBP_OP_* kinds come from there).  A library that runs no sweep program, whose
// header has no op kinds, defines MLBP_GRAPH_NO_SWEEPS first and gets everything but the two steps.
#ifndef MLBP_GRAPH_DEVICE_H
#define MLBP_GRAPH_DEVICE_H

#include "mlbp_device.h"

namespace mlbp_graph {

using namespace mlbp_dev;

constexpr int WG = 256;                                        // every kernel: one workgroup of four waves

struct SumOp {
  static __device__ __forceinline__ double identity() { return 0.0; }
  static __device__ __forceinline__ double combine(double a, double b) { return a + b; }
};
struct MaxOp {
  static __device__ __forceinline__ double identity() { return -__builtin_huge_val(); }
  static __device__ __forceinline__ double combine(double a, double b) { return fmax(a, b); }
};

// Op over each row of 16 lanes, the same bits in every lane of the row (the first four steps of mlbp_dev::wave_sum).
template <class Op>
__device__ __forceinline__ double row16_reduce(double v) {
  v = Op::combine(v, dpp_mov<0xB1>(v));
  v = Op::combine(v, dpp_mov<0x4E>(v));
  v = Op::combine(v, dpp_mov<0x141>(v));
  v = Op::combine(v, dpp_mov<0x140>(v));
  return v;
}

// Op over the 64 lanes, the same bits in every lane: wave_reduce<SumOp> is mlbp_dev::wave_sum, step for step.
template <class Op>
__device__ __forceinline__ double wave_reduce(double v) {
  v = row16_reduce<Op>(v);
  return Op::combine(Op::combine(read_lane(v, 0), read_lane(v, 16)), Op::combine(read_lane(v, 32), read_lane(v, 48)));
}

__device__ __forceinline__ double wave_max(double v) { return wave_reduce<MaxOp>(v); }

// Sum over the workgroup, the same bits in every thread; two barriers, reached by all.
__device__ __forceinline__ double block_sum(double v, double* scratch /*[4]*/) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
}

// Every table index of graph g is inside its table array (wave-uniform: scalar loads).
__device__ __forceinline__ bool tables_in_range(const int32_t* pair_tab, int P, int n_pair_tables, const int32_t* unary_tab, int U,
                                                int n_unary_tables, int g) {
  bool ok = true;
  const const_i32p pt = as_const(pair_tab), ut = as_const(unary_tab);
  for (int p = 0; p < P; ++p) ok &= (unsigned)pt[(size_t)g * P + p] < (unsigned)n_pair_tables;
  for (int u = 0; u < U; ++u) ok &= (unsigned)ut[(size_t)g * U + u] < (unsigned)n_unary_tables;
  return ok;
}

// ---- X = 64: a pairwise table split over the 256 threads --------------------------------------------
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

// out[j] = Op_i m[i] * T[i][j]: the thread's two columns over its 8 rows -> part[2 wave + half][column].
template <class Op>
__device__ __forceinline__ void pair_mt_partial(const double (&T)[16], const double* m, double* part, int wave, int lane) {
  const int h = lane >> 5;
  double a0 = Op::identity(), a1 = Op::identity();
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double mi = m[16 * wave + 2 * k + h];          // two addresses per wave: LDS broadcast
    a0 = Op::combine(a0, mi * T[2 * k]);
    a1 = Op::combine(a1, mi * T[2 * k + 1]);
  }
  reinterpret_cast<double2*>(part)[(2 * wave + h) * 32 + (lane & 31)] = make_double2(a0, a1);
}

// out[i] = Op_j T[i][j] * m[j]: the wave's 16 rows -> raw[16 wave .. 16 wave + 15].  Per row the two products, then Op over the
// 32 lanes of the row half on DPP and through scalar registers.
template <class Op>
__device__ __forceinline__ void pair_tm_rows(const double (&T)[16], const double* m, double* raw, int wave, int lane) {
  const double2 mm = reinterpret_cast<const double2*>(m)[lane & 31];
  double2 mine = make_double2(0.0, 0.0);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double p = row16_reduce<Op>(Op::combine(T[2 * k] * mm.x, T[2 * k + 1] * mm.y));
    const double lo = Op::combine(read_lane(p, 0), read_lane(p, 16));      // row 16 wave + 2k     (lanes 0..31)
    const double hi = Op::combine(read_lane(p, 32), read_lane(p, 48));     // row 16 wave + 2k + 1 (lanes 32..63)
    if (lane == k) mine = make_double2(lo, hi);
  }
  if (lane < 8) reinterpret_cast<double2*>(raw)[8 * wave + lane] = mine;
}

template <class Op>
__device__ __forceinline__ void pair_contract(const double (&T)[16], bool tm, const double* m, double* part, double* raw, int wave, int lane) {
  if (tm) pair_tm_rows<Op>(T, m, raw, wave, lane); else pair_mt_partial<Op>(T, m, part, wave, lane);
}

// No variable is clamped: the `state_of` of every step but the sampler's.
struct FreeState {
  __device__ __forceinline__ int operator()(int) const { return -1; }
};

// What one graph's steps read and write.  X = 64: msg [n_msgs][64], part [8][64] and raw [64] in LDS.  Generic: msg in global
// memory, raw [X] in LDS, part unused.
struct StepGraph {
  const double* pair_tables; const_i32p ptab;                  // ptab, utab: this graph's rows of pair_tab / unary_tab
  const double* unary_tables; const_i32p utab;
  const_i32p srcs;
  double* msg; double* part; double* raw;
};

#ifndef MLBP_GRAPH_NO_SWEEPS
// One op (kind, a, b, c) of a sweep at X = 64, by the whole workgroup; both barriers are reached by every thread.  A pairwise
// update contracts the table -- fragment R[a] when RESIDENT (P <= 3), else loaded here -- with message b; wave 0 (lane = state)
// gathers the result and hands finish(value, c) the un-normalised message.  VAR and UNARY ops run in wave 0 alone.
// state_of(c): the state the source variable of slot c is clamped to, -1 while free; asked for VAR ops only.
template <class Op, bool RESIDENT, class StateOf, class Finish>
__device__ __forceinline__ void x64_step(const StepGraph& G, const double (&R)[3][16], int kind, int a, int b, int c, int wave, int lane,
                                         StateOf state_of, Finish finish) {
  if (kind == MLBP_OP_PAIR_TM || kind == MLBP_OP_PAIR_MT) {
    const double* m = G.msg + b * 64;
    const bool tm = kind == MLBP_OP_PAIR_TM;
    if (RESIDENT) {
      if (a == 0) pair_contract<Op>(R[0], tm, m, G.part, G.raw, wave, lane);
      else if (a == 1) pair_contract<Op>(R[1], tm, m, G.part, G.raw, wave, lane);
      else pair_contract<Op>(R[2], tm, m, G.part, G.raw, wave, lane);
    } else {
      double T[16];
      load_fragment(G.pair_tables + (size_t)G.ptab[a] * 4096, wave, lane, T);
      pair_contract<Op>(T, tm, m, G.part, G.raw, wave, lane);
    }
    __syncthreads();
    if (wave == 0) {
      double v;
      if (tm) {
        v = G.raw[lane];
      } else {
        v = G.part[lane];
#pragma unroll
        for (int q = 1; q < 8; ++q) v = Op::combine(v, G.part[q * 64 + lane]);
      }
      finish(v, c);
    }
  } else if (wave == 0) {
    if (kind == MLBP_OP_VAR) {
      double acc = 1.0 / 64.0;
      for (int q = 0; q < b; ++q) acc = mul_nan_to_num(G.msg[G.srcs[a + q] * 64 + lane], acc);
      const int x = state_of(c);
      if (x >= 0) acc = lane == x ? acc : 0.0;
      finish(acc, c);
    } else {
      finish(G.unary_tables[(size_t)G.utab[a] * 64 + lane], c);
    }
  }
  __syncthreads();
}
#endif

// The marginal of variable v at state `lane` from the LDS messages, by one wave.
__device__ __forceinline__ double x64_marginal(const double* msg, const_i32p in_off, const_i32p in_slots, int v, int lane) {
  const double uniform = 1.0 / 64.0;
  double acc = uniform;
  for (int q = in_off[v]; q < in_off[v + 1]; ++q) acc = mul_nan_to_num(msg[in_slots[q] * 64 + lane], acc);
  const double total = wave_sum(acc);
  return total > 0.0 ? acc / total : uniform;
}

// ---- any X ---------------------------------------------------------------------------------------
#ifndef MLBP_GRAPH_NO_SWEEPS
// One op of a sweep: its un-normalised result into raw[0 .. X), by the whole workgroup, then a barrier.  uniform = 1 / X.
template <class Op, class StateOf>
__device__ __forceinline__ void generic_step(const StepGraph& G, int X, double uniform, int kind, int a, int b, int c, StateOf state_of) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double* raw = G.raw;
  if (kind == MLBP_OP_PAIR_TM) {
    const double* T = G.pair_tables + (size_t)G.ptab[a] * X * X;
    const double* m = G.msg + (size_t)b * X;
    for (int row = wave; row < X; row += WG / 64) {
      const double* Tr = T + (size_t)row * X;
      double acc = Op::identity();
      for (int j = lane; j < X; j += 64) acc = Op::combine(acc, Tr[j] * m[j]);
      acc = wave_reduce<Op>(acc);
      if (lane == 0) raw[row] = acc;
    }
  } else if (kind == MLBP_OP_PAIR_MT) {
    const double* T = G.pair_tables + (size_t)G.ptab[a] * X * X;
    const double* m = G.msg + (size_t)b * X;
    for (int j = t; j < X; j += WG) {
      double acc = Op::identity();
#pragma unroll 8
      for (int i = 0; i < X; ++i) acc = Op::combine(acc, m[i] * T[(size_t)i * X + j]);
      raw[j] = acc;
    }
  } else if (kind == MLBP_OP_VAR) {
    const int x = state_of(c);
    for (int j = t; j < X; j += WG) {
      double acc = uniform;
      for (int q = 0; q < b; ++q) acc = nan_to_num(G.msg[(size_t)G.srcs[a + q] * X + j] * acc);
      raw[j] = (x >= 0 && j != x) ? 0.0 : acc;
    }
  } else {
    const double* u = G.unary_tables + (size_t)G.utab[a] * X;
    for (int j = t; j < X; j += WG) raw[j] = u[j];
  }
  __syncthreads();
}
#endif

// raw[] -> a finished message: the total (when normalising), then store(j, value) for the entries of this thread, then a barrier.
template <class Store>
__device__ __forceinline__ void generic_finish(const double* raw, int X, double uniform, bool norm, double* scratch, Store store) {
  const int t = threadIdx.x;
  double part = 0.0;
  for (int j = t; j < X; j += WG) part += raw[j];
  const double total = norm ? block_sum(part, scratch) : 0.0;
  for (int j = t; j < X; j += WG) store(j, renorm(raw[j], total, uniform, norm));
  __syncthreads();
}

// The marginal of variable v from the messages in global memory, by the whole workgroup: emit(j, value) for the entries of this
// thread.  raw[] is left holding the un-normalised products; the caller fences it before it is written again.
template <class Emit>
__device__ __forceinline__ void generic_marginal(const double* msg, const_i32p in_off, const_i32p in_slots, int v, int X, double uniform,
                                                 double* raw, double* scratch, Emit emit) {
  const int t = threadIdx.x;
  double part = 0.0;
  for (int j = t; j < X; j += WG) {
    double acc = uniform;
    for (int q = in_off[v]; q < in_off[v + 1]; ++q) acc = nan_to_num(msg[(size_t)in_slots[q] * X + j] * acc);
    raw[j] = acc;
    part += acc;
  }
  const double total = block_sum(part, scratch);
  for (int j = t; j < X; j += WG) emit(j, total > 0.0 ? raw[j] / total : uniform);
}

}  // namespace mlbp_graph

#endif
