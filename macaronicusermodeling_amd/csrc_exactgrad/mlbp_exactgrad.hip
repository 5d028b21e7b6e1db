// libmlbp_exactgrad.so: the model's true pairwise marginals, expected features and likelihood gradient by cutset conditioning
// (include/mlbp_exactgrad.h), gfx950 only, float64.
//
// Three kernels; the walk kernel is chosen from (X, n_vars, P, U, n_forest) by mlbp_exactgrad_pick_kernel:
//   exactgrad_x64_kernel<NF>   X = 64, n_forest <= 2, NF = max(n_forest, 1): the X = 64 walk of csrc/mlbp_cutset_walk.h in its sum
//                              form -- the forest's tables in LDS, rows of 65, every WAVE its own configurations, lane = state,
//                              no workgroup barrier inside the walk -- and around its steps the wave's pair accumulators: the
//                              64 x 64 sum of rank-1 updates of every forest factor in registers (lane = column, 64 doubles per
//                              lane, 64 FMAs on v_readlane broadcasts per configuration), the rows of the cutset-incident
//                              factors and the cells of the cutset-internal ones in the wave's own partial in the workspace.
//   exactgrad_generic_kernel   any X in [2, 1024]: the generic walk of csrc/mlbp_cutset_walk.h in its sum form, the workgroup one
//                              configuration at a time; every pair accumulator in the workgroup's partial.
//   exactgrad_combine_kernel   one workgroup per graph: adds the partials in index order, applies the rescaled table to the
//                              forest factors, divides by Z, writes the requested tensors, contracts with phi eight features
//                              at a time, forms the observed features at the labels and takes the one logarithm.
// A global accumulator entry is only ever touched by one lane (X = 64: entry [row][lane] by `lane`), or by threads of one
// workgroup with a barrier between two touches (generic); there is no atomic.  Every scalar a wave or workgroup branches on comes
// out of a reduction and has the same bits in every thread of it.
// A LISTED call (mlbp_exactgrad_listed_args with N > 0: the header's listed mode) runs the same three kernels over the caller's list of cutset states: a walker's
// c is then the index of a list entry, its weight Z_c exp(-log_q) (weighted() of csrc/mlbp_cutset_plan.h) and its states the
// entry's row of configs, checked before they index anything; the combine kernel divides the sum by N for log_z_hat.
// No device-side mutable globals: everything comes through GradDev.
#include <hip/hip_runtime.h>

#include "../../include/mlbp_exactgrad.h"
#include "../../include/mlbp_cutsetis.h"    // MLBP_CUTSETIS_MAX_ABS_LOG_Q: the range of a list's log_q
#define MLBP_GRAPH_NO_SWEEPS                // this library runs no sweep program
#include "../csrc/mlbp_graph_device.h"
#include "../csrc/mlbp_graph_host.h"
#include "../csrc/mlbp_cutset_plan.h"       // the plan's layout and check, the power-of-two helpers, the host core
#include "../csrc/mlbp_cutset_walk.h"       // the walk

namespace {

using namespace mlbp_graph;

constexpr int MAXF = MLBP_EXACTGRAD_MAX_FEATURES;
constexpr int FG = 8;                       // features contracted per pass of the combine kernel

struct GradDev : WalkDev {                   // partials: [B][parts][stride]: {sum mantissa, exponent, [n_vars][X], [P][X][X]}
  const double* phi_en_en; const double* phi_en_en_w1; const double* phi_en_de;
  const int32_t* pair_phi; const int32_t* unary_kind; const int32_t* unary_obs; const int32_t* labels;
  double* log_z; double* marginals; double* pair_marginals; double* expect_ee; double* expect_ed; double* grad_ee; double* grad_ed;
  int64_t stride;
  int32_t F_ee, F_ed, Vde;
  int32_t listed;                            // a listed call: n_configs is N, and the two below are the caller's; else 0 and NULL
  const int32_t* configs;                    // [B][N][n_cut], NULL without cutset variables
  const double* log_q;                       // [B][N]
};

// ---- a listed call: where an entry's states and weight come from ----------------------------------------------
// An entry of a list is checked before anything is indexed by it.  The generic kernel reads the state of cut position q through
// ONE functor in both modes (EntryStates), so its walk has one call site.  The X = 64 kernel has a loop for each mode, the exact
// one the text it always was: with one loop over a shared functor -- a scalar select between the digits of c and a v_readlane, or
// the digits of c laid out one per lane -- the exact call at K4 ran 2.6 % and 3.1 % slower than before, with two it does not.
__device__ __forceinline__ const_i32p listed_row(const GradDev& d, int g, int i) {
  return as_const(d.configs) + ((size_t)g * d.n_configs + i) * d.n_cut;
}

__device__ __forceinline__ bool log_q_ok(double lq) { return fabs(lq) <= MLBP_CUTSETIS_MAX_ABS_LOG_Q; }     // false for a NaN

// The generic kernel takes an entry's factor exp(-log_q) = r 2^k OUT OF LINE.  Inlined into its loop, the nine coefficients of the
// exponential's polynomial are hoisted out of the loop and held in 18 vector registers across the whole walk: 90 registers and
// five waves per SIMD against the 61 and seven of the exact-only kernel.  Behind a call they live in the callee alone (72, seven
// waves, no scratch).  The X = 64 kernels have the room and take it inline: a call there would have to save the accumulators.
__device__ __attribute__((noinline)) ProposalFactor generic_entry_factor(double lq) { return proposal_factor(lq); }

// Generic kernel: the row of the entry (a listed call with cutset variables), else c's digits.
struct EntryStates {
  const_i32p row; int c, X;
  __device__ __forceinline__ int operator()(int q) const { return row ? row[q] : GenericCode{c, X}(q); }
};

// The partial of a walker that met an entry it may not walk: a NaN sum under exponent 0, which makes the graph's Z a NaN in the
// combine kernel -- its sign of a refused list.
__device__ __forceinline__ Scaled refused() { return {__builtin_nan(""), 0}; }

// ---- any X: the workgroup walks a chunk's configurations ---------------------------------------------------
__global__ __launch_bounds__(WG) void exactgrad_generic_kernel(GradDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X, g = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  Generic G;
  generic_open(G, d, g);
  const size_t vs = generic_carve(G, d, g, k, smem), XX = G.XX;
  const int Xp = G.Xp;
  double* acc = G.acc;                                         // [n_vars][Xp] sum over configurations of Z_c m_c, mantissas
  double* out = d.partials + ((size_t)g * d.parts + k) * d.stride;
  double* pacc = out + 2 + (size_t)d.n_vars * X;               // [P][X][X] pair accumulators, mantissas under the sum's exponent
  generic_setup(G);
  for (size_t i = t; i < vs; i += WG) acc[i] = 0.0;

  Scaled sum = {0.0, EMPTY};                                   // sum of Z_c over this chunk
  for (int c = k; c < d.n_configs; c += d.chunks) {            // a listed call: c is the index of an entry
    EntryStates states = {nullptr, c, X};
    ProposalFactor pf = {1.0, 0};
    if (d.listed) {                                            // the same in every thread: the entry's address is
      const double lq = d.log_q[(size_t)g * d.n_configs + c];
      bool ok = log_q_ok(lq);
      if (d.n_cut > 0) {
        states.row = listed_row(d, g, c);
        for (int q = 0; q < d.n_cut; ++q) ok &= (unsigned)states.row[q] < (unsigned)X;
      }
      if (!ok) {                                               // before st holds a state of it: st indexes the pair accumulators
        sum = refused();
        break;
      }
      pf = generic_entry_factor(lq);
    }
    Scaled z = generic_up<SumAlg>(G, states, G.up);
    if (d.listed) z = weighted(z, pf);
    if (SumAlg::dead(z)) continue;                             // Z_c = 0: nothing to add
    const double w = join_sum(sum, z, [&](int shift, bool first) {           // the first Z_c clears the pair accumulators
      for (size_t i = t; i < vs; i += WG) acc[i] = ldexp(acc[i], shift);
      for (size_t i = t; i < (size_t)d.P * XX; i += WG) pacc[i] = first ? 0.0 : ldexp(pacc[i], shift);
      __syncthreads();
    });
    if (t < d.n_cut) acc[(size_t)G.pl.cutset[t] * Xp + G.st[t]] += w;
    if (t == 0)
      for (int i = 0; i < d.n_consts; ++i)
        if (G.pl.consts[4 * i] == MLBP_CUTSET_CONST_PAIR)        // a factor inside the cutset: its cell gains Z_c
          pacc[(size_t)G.pl.consts[4 * i + 1] * XX + (size_t)G.st[G.pl.consts[4 * i + 2]] * X + G.st[G.pl.consts[4 * i + 3]]] += w;
    generic_down<SumAlg>(
        G,
        // the forest factor's rank-1 update: a = bv (v's vector on the way up), b = excl, a^T T~ b = 2^er sum_i a[i] raw[i]
        [&](int p, bool v_on_axis0, const double* bv, const double* excl, int er) {
          double s = 0.0;
          for (int j = t; j < X; j += WG) s += bv[j] * G.raw[j];
          const double coef = ldexp(w / block_sum(s, G.scratch), -er);
          const double* v0 = v_on_axis0 ? bv : excl;
          const double* v1 = v_on_axis0 ? excl : bv;
          double* A = pacc + (size_t)p * XX;
          for (int r = 0; r < X; ++r) {
            const double ar = coef * v0[r];
            for (int j = t; j < X; j += WG) A[(size_t)r * X + j] = fma(ar, v1[j], A[(size_t)r * X + j]);
          }
          __syncthreads();                                     // every thread has read all of bv before its entries change
        },
        [&](int v, int j, double x) {
          const double wm = w * x;
          acc[(size_t)v * Xp + j] += wm;
          for (int it = G.pl.item_off[v]; it < G.pl.item_off[v + 1]; ++it)       // row s_q of every cutset-incident factor, [s_q][state of v]
            if (G.pl.items[3 * it] != MLBP_CUTSET_ITEM_UNARY)
              pacc[(size_t)G.pl.items[3 * it + 1] * XX + (size_t)G.st[G.pl.items[3 * it + 2]] * X + j] += wm;
        });
  }

  __syncthreads();
  if (t == 0) {
    out[0] = sum.m;
    out[1] = (double)sum.e;
  }
  if (sum.e == EMPTY) return;
  for (int v = 0; v < d.n_vars; ++v)
    for (int j = t; j < X; j += WG) out[2 + (size_t)v * X + j] = acc[(size_t)v * Xp + j];
}

// ---- X = 64: a wave per configuration ---------------------------------------------------------------------
// R[i] += v0[i] * v1[lane]: the rank-1 update of a 64 x 64 accumulator held as 64 registers per lane (lane = column).
__device__ __forceinline__ void rank1_x64(double (&R)[64], double v0, double v1) {
#pragma unroll
  for (int i = 0; i < 64; ++i) R[i] = fma(read_lane(v0, i), v1, R[i]);
}

template <int NF>
__global__ __launch_bounds__(WG) void exactgrad_x64_kernel(GradDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  X64 W;
  x64_open(W, d, g, smem);
  const int n_vars = d.n_vars, P = d.P;
  double* acc = W.acc;                                         // this wave's: sum over its configurations of Z_c m_c, mantissas
  double* out = d.partials + ((size_t)g * d.parts + 4 * k + wave) * d.stride;
  double* pacc = out + 2 + (size_t)n_vars * 64;                // [P][64][64] this wave's pair accumulators in its partial
  for (int v = 0; v < n_vars; ++v) acc[(size_t)v * 64 + lane] = 0.0;
  double R[NF][64];                                            // the forest factors' accumulators, [row][lane = column] in table axes
#pragma unroll
  for (int s = 0; s < NF; ++s)
#pragma unroll
    for (int i = 0; i < 64; ++i) R[s][i] = 0.0;

  Scaled sum = {0.0, EMPTY};                                   // sum of Z_c over this wave's configurations
  if (d.listed) {                                              // a listed call: a loop of its own, the exact one below is as it was
    for (int c = 4 * k + wave; c < d.n_configs; c += 4 * d.chunks) {         // c: the index of an entry; its weight where Z_c stands
      const X64Packed state = {lane < d.n_cut ? listed_row(d, g, c)[lane] : 0};   // lane q: the state of cut position q
      ProposalFactor pf = {1.0, 0};
      {                                                          // (in this form the <2> instance allocates without a spill copy)
        const double lq = d.log_q[(size_t)g * d.n_configs + c];
        if (__any((unsigned)state.packed >= 64u) || !log_q_ok(lq)) {           // before a state of it selects a row or a cell
          sum = refused();
          break;
        }
        pf = proposal_factor(lq);                                // here, not behind the walk: fewer registers are live there
      }
      Scaled z = x64_up<SumAlg, true>(W, state);
      z = weighted(z, pf);
      if (SumAlg::dead(z)) continue;                             // Z_c = 0: nothing to add
      const double w = join_sum(sum, z, [&](int shift, bool first) {           // the first Z_c clears the accumulators in the partial
        for (int v = 0; v < n_vars; ++v) acc[(size_t)v * 64 + lane] = ldexp(acc[(size_t)v * 64 + lane], shift);
        for (int p = 0; p < P; ++p) {
          if (W.pl.fslot[p] >= 0) continue;
          double* A = pacc + (size_t)p * 4096;
          for (int i = lane; i < 4096; i += 64) A[i] = first ? 0.0 : ldexp(A[i], shift);
        }
#pragma unroll
        for (int s = 0; s < NF; ++s)
#pragma unroll
          for (int i = 0; i < 64; ++i) R[s][i] = ldexp(R[s][i], shift);
      });
      for (int q = 0; q < d.n_cut; ++q)
        if (lane == state(q)) acc[(size_t)W.pl.cutset[q] * 64 + lane] += w;
      for (int i = 0; i < d.n_consts; ++i) {                     // a factor inside the cutset: its cell gains Z_c
        if (W.pl.consts[4 * i] != MLBP_CUTSET_CONST_PAIR) continue;
        const int s0 = state(W.pl.consts[4 * i + 2]), s1 = state(W.pl.consts[4 * i + 3]);
        if (lane == s1) pacc[(size_t)W.pl.consts[4 * i + 1] * 4096 + s0 * 64 + lane] += w;
      }
      for (int i = W.n_free - 1; i >= 0; --i) {
        const X64Down s = x64_down_step<SumAlg, true>(W, i);
        if (s.p >= 0) {                                          // the forest factor's rank-1 update
          const double coef = ldexp(w / s.total, -s.er);
          const double v0 = s.v_on_axis0 ? s.a : s.b, v1 = coef * (s.v_on_axis0 ? s.b : s.a);
#pragma unroll
          for (int f = 0; f < NF; ++f)                           // R is indexed by constants alone: it stays in registers
            if (s.slot == f) rank1_x64(R[f], v0, v1);
        }
        const double wm = w * s.x;
        acc[(size_t)s.v * 64 + lane] += wm;
        for (int it = W.pl.item_off[s.v]; it < W.pl.item_off[s.v + 1]; ++it)   // row s_q of every cutset-incident factor, [s_q][state of v]
          if (W.pl.items[3 * it] != MLBP_CUTSET_ITEM_UNARY)
            pacc[(size_t)W.pl.items[3 * it + 1] * 4096 + state(W.pl.items[3 * it + 2]) * 64 + lane] += wm;
      }
    }
  } else                                                       // the exact call: the loop it has always run
  for (int c = 4 * k + wave; c < d.n_configs; c += 4 * d.chunks) {
    const Scaled z = x64_up<SumAlg, true>(W, c);
    if (SumAlg::dead(z)) continue;                             // Z_c = 0: nothing to add
    const double w = join_sum(sum, z, [&](int shift, bool first) {           // the first Z_c clears the accumulators in the partial
      for (int v = 0; v < n_vars; ++v) acc[(size_t)v * 64 + lane] = ldexp(acc[(size_t)v * 64 + lane], shift);
      for (int p = 0; p < P; ++p) {
        if (W.pl.fslot[p] >= 0) continue;
        double* A = pacc + (size_t)p * 4096;
        for (int i = lane; i < 4096; i += 64) A[i] = first ? 0.0 : ldexp(A[i], shift);
      }
#pragma unroll
      for (int s = 0; s < NF; ++s)
#pragma unroll
        for (int i = 0; i < 64; ++i) R[s][i] = ldexp(R[s][i], shift);
    });
    for (int q = 0; q < d.n_cut; ++q)
      if (lane == x64_state(q, c)) acc[(size_t)W.pl.cutset[q] * 64 + lane] += w;
    for (int i = 0; i < d.n_consts; ++i) {                     // a factor inside the cutset: its cell gains Z_c
      if (W.pl.consts[4 * i] != MLBP_CUTSET_CONST_PAIR) continue;
      const int s0 = x64_state(W.pl.consts[4 * i + 2], c), s1 = x64_state(W.pl.consts[4 * i + 3], c);
      if (lane == s1) pacc[(size_t)W.pl.consts[4 * i + 1] * 4096 + s0 * 64 + lane] += w;
    }
    for (int i = W.n_free - 1; i >= 0; --i) {
      const X64Down s = x64_down_step<SumAlg, true>(W, i);
      if (s.p >= 0) {                                          // the forest factor's rank-1 update
        const double coef = ldexp(w / s.total, -s.er);
        const double v0 = s.v_on_axis0 ? s.a : s.b, v1 = coef * (s.v_on_axis0 ? s.b : s.a);
#pragma unroll
        for (int f = 0; f < NF; ++f)                           // R is indexed by constants alone: it stays in registers
          if (s.slot == f) rank1_x64(R[f], v0, v1);
      }
      const double wm = w * s.x;
      acc[(size_t)s.v * 64 + lane] += wm;
      for (int it = W.pl.item_off[s.v]; it < W.pl.item_off[s.v + 1]; ++it)   // row s_q of every cutset-incident factor, [s_q][state of v]
        if (W.pl.items[3 * it] != MLBP_CUTSET_ITEM_UNARY)
          pacc[(size_t)W.pl.items[3 * it + 1] * 4096 + x64_state(W.pl.items[3 * it + 2], c) * 64 + lane] += wm;
    }
  }

  if (lane == 0) {
    out[0] = sum.m;
    out[1] = (double)sum.e;
  }
  if (sum.e == EMPTY) return;                                  // an empty partial holds nothing else
  for (int v = 0; v < n_vars; ++v) out[2 + (size_t)v * 64 + lane] = acc[(size_t)v * 64 + lane];
  for (int p = 0; p < P; ++p) {
    const int slot = W.pl.fslot[p];
    if (slot < 0) continue;
    double* A = pacc + (size_t)p * 4096 + lane;
#pragma unroll
    for (int f = 0; f < NF; ++f)
      if (slot == f) {
#pragma unroll
        for (int i = 0; i < 64; ++i) A[i * 64] = R[f][i];
      }
  }
}

// ---- the partials of a graph's chunks -> its outputs ----------------------------------------------------
__global__ __launch_bounds__(WG) void exactgrad_combine_kernel(GradDev d) {
  __shared__ double scratch[8];
  __shared__ double ex_ee[MAXF], ex_ed[MAXF], ob_ee[MAXF], ob_ed[MAXF];
  const int g = blockIdx.x, t = threadIdx.x;
  const int X = d.X, P = d.P, U = d.U, F_ee = d.F_ee, F_ed = d.F_ed;
  const bool want_expect = d.expect_ee || d.expect_ed || d.grad_ee || d.grad_ed;
  const bool want_grad = d.grad_ee || d.grad_ed;
  const double nan = __builtin_nan("");
  auto refuse = [&]() {                                        // the graph is not computed: NaN, its tensors left as they were
    if (t == 0) {
      d.log_z[g] = nan;
      for (int f = 0; f < F_ee; ++f) {
        if (d.expect_ee) d.expect_ee[(size_t)g * F_ee + f] = nan;
        if (d.grad_ee) d.grad_ee[(size_t)g * F_ee + f] = nan;
      }
      for (int f = 0; f < F_ed; ++f) {
        if (d.expect_ed) d.expect_ed[(size_t)g * F_ed + f] = nan;
        if (d.grad_ed) d.grad_ed[(size_t)g * F_ed + f] = nan;
      }
    }
  };
  if (!tables_in_range(d.pair_tab, P, d.n_pair_tables, d.unary_tab, U, d.n_unary_tables, g)) {
    refuse();
    return;
  }
  PlanSections<const_i32p> pl;
  carve_plan(as_const(d.plan), d.n_vars, P, U, d.n_cut, d.n_free, d.n_items, d.n_consts, pl);
  const size_t XX = (size_t)X * X, stride = (size_t)d.stride;
  const SumParts parts = read_sum_parts(d.partials + (size_t)g * d.parts * stride, stride, d.parts);
  const double Z = parts.Z;
  if (d.listed && Z != Z) {                                    // a walker refused an entry of the list (the same in every thread)
    refuse();
    return;
  }
  // entry `at` of the partials (behind the two header words), summed in index order; an empty partial holds nothing
  auto summed = [&](size_t at) { return mlbp_graph::summed<true>(parts, at); };
  const size_t N = (size_t)d.n_vars * X;
  const double uniform = 1.0 / (double)X;
  if (d.marginals)
    for (size_t i = t; i < N; i += WG) d.marginals[(size_t)g * N + i] = Z == 0.0 ? uniform : summed(i) / Z;
  if (t < MAXF) ex_ee[t] = ex_ed[t] = ob_ee[t] = ob_ed[t] = 0.0;
  __syncthreads();

  // ---- pairwise factors: M_p, then its contraction with phi_p ----
  if (d.pair_marginals || want_expect) {
    for (int p = 0; p < P; ++p) {
      // where the factor was accumulated: a forest factor in table axes (T~ still to be applied), a factor inside the cutset in
      // table axes, a cutset-incident one as [s_q][state of the free variable]: transposed when that variable is on axis 0
      const bool forest = pl.fslot[p] >= 0;
      bool transposed = false;
      for (int it = 0; it < d.n_items; ++it)
        if (pl.items[3 * it] == MLBP_CUTSET_ITEM_COL && pl.items[3 * it + 1] == p) transposed = true;
      const double* T = d.pair_tables + (size_t)d.pair_tab[(size_t)g * P + p] * XX;
      int te = 0;
      if (forest) {
        double m = 0.0;
        for (size_t i = t; i < XX; i += WG) m = fmax(m, T[i]);
        te = exp_of(block_max(m, scratch));
      }
      const double* phi = want_expect ? (d.pair_phi[p] == 0 ? d.phi_en_en : d.phi_en_en_w1) : nullptr;
      double* pm = d.pair_marginals ? d.pair_marginals + ((size_t)g * P + p) * XX : nullptr;
      const int n_pass = want_expect ? (F_ee + FG - 1) / FG : 1;
      for (int pass = 0; pass < n_pass; ++pass) {
        const int f0 = pass * FG;
        double fs[FG];
#pragma unroll
        for (int q = 0; q < FG; ++q) fs[q] = 0.0;
        for (size_t src = t; src < XX; src += WG) {            // in the accumulator's order: the partials are read in whole lines
          const size_t hi = src / X, lo = src - hi * X;
          const size_t idx = transposed ? lo * X + hi : src;   // the entry's place in table axes
          double m = uniform * uniform;
          if (Z != 0.0) {
            m = summed(N + (size_t)p * XX + src) / Z;
            if (forest) m *= ldexp(T[idx], -te);
          }
          if (pm && pass == 0) pm[idx] = m;
          if (want_expect) {
#pragma unroll
            for (int q = 0; q < FG; ++q)
              if (f0 + q < F_ee) fs[q] = fma(m, phi[idx * F_ee + f0 + q], fs[q]);
          }
        }
        if (want_expect) {
#pragma unroll
          for (int q = 0; q < FG; ++q) {
            if (f0 + q >= F_ee) continue;                      // (uniform)
            const double total = block_sum(fs[q], scratch);
            if (t == 0) ex_ee[f0 + q] += total;
          }
        }
      }
    }
  }

  // ---- unary factors: the variable's marginal against phi_u at the observed column ----
  bool bad = false;                                            // a column or selector out of range: no gradient
  if (want_expect) {
    for (int u = 0; u < U; ++u) {
      const int kind = d.unary_kind[u], obs = d.unary_obs[(size_t)g * U + u], v = pl.uvar[u];
      const int cols = kind == 2 ? d.Vde : X;
      if ((unsigned)kind > 2u || (unsigned)obs >= (unsigned)cols) {
        bad = true;
        continue;
      }
      const double* phi = kind == 0 ? d.phi_en_en : kind == 1 ? d.phi_en_en_w1 : d.phi_en_de;
      const int F = kind == 2 ? F_ed : F_ee;
      double* ex = kind == 2 ? ex_ed : ex_ee;
      for (int f0 = 0; f0 < F; f0 += FG) {
        double fs[FG];
#pragma unroll
        for (int q = 0; q < FG; ++q) fs[q] = 0.0;
        for (int i = t; i < X; i += WG) {
          const double m = Z == 0.0 ? uniform : summed((size_t)v * X + i) / Z;
#pragma unroll
          for (int q = 0; q < FG; ++q)
            if (f0 + q < F) fs[q] = fma(m, phi[((size_t)i * cols + obs) * F + f0 + q], fs[q]);
        }
#pragma unroll
        for (int q = 0; q < FG; ++q) {
          if (f0 + q >= F) continue;
          const double total = block_sum(fs[q], scratch);
          if (t == 0) ex[f0 + q] += total;
        }
      }
    }
  }
  if (t != 0) return;

  // ---- thread 0: the observed features at the labels, the outputs ----
  if (want_grad) {
    const int32_t* lab = d.labels + (size_t)g * d.n_vars;
    for (int v = 0; v < d.n_vars; ++v) bad |= (unsigned)lab[v] >= (unsigned)X;
    if (!bad) {
      for (int p = 0; p < P; ++p) {
        const double* phi = (d.pair_phi[p] == 0 ? d.phi_en_en : d.phi_en_en_w1) + ((size_t)lab[pl.pav[2 * p]] * X + lab[pl.pav[2 * p + 1]]) * F_ee;
        for (int f = 0; f < F_ee; ++f) ob_ee[f] += phi[f];
      }
      for (int u = 0; u < U; ++u) {
        const int kind = d.unary_kind[u], obs = d.unary_obs[(size_t)g * U + u];
        const int cols = kind == 2 ? d.Vde : X, F = kind == 2 ? F_ed : F_ee;
        const double* phi = (kind == 0 ? d.phi_en_en : kind == 1 ? d.phi_en_en_w1 : d.phi_en_de) + ((size_t)lab[pl.uvar[u]] * cols + obs) * F;
        double* ob = kind == 2 ? ob_ed : ob_ee;
        for (int f = 0; f < F; ++f) ob[f] += phi[f];
      }
    }
  }
  // a listed call: log_z_hat, the logarithm of the MEAN weight
  d.log_z[g] = Z == 0.0 ? -__builtin_huge_val()
                        : fma((double)parts.emax, 0.693147180559945309417232121458, log(d.listed ? Z / (double)d.n_configs : Z));
  for (int f = 0; f < F_ee; ++f) {
    if (d.expect_ee) d.expect_ee[(size_t)g * F_ee + f] = ex_ee[f];
    if (d.grad_ee) d.grad_ee[(size_t)g * F_ee + f] = bad ? nan : ob_ee[f] - ex_ee[f];
  }
  for (int f = 0; f < F_ed; ++f) {
    if (d.expect_ed) d.expect_ed[(size_t)g * F_ed + f] = ex_ed[f];
    if (d.grad_ed) d.grad_ed[(size_t)g * F_ed + f] = bad ? nan : ob_ed[f] - ex_ed[f];
  }
}

// ---- host ----------------------------------------------------------------------------------------
thread_local int g_last_kernel = MLBP_EXACTGRAD_KERNEL_NONE;
static_assert(MLBP_EXACTGRAD_KERNEL_X64 == WALK_X64 && MLBP_EXACTGRAD_KERNEL_GENERIC == WALK_GENERIC, "the shared host core numbers the kernels");
static_assert(MLBP_EXACTGRAD_MAX_CUT == MAX_LISTED_CUT, "a listed walk's bound on the cutset is the shared one");

}  // namespace

extern "C" {

const char* mlbp_exactgrad_arch(void) { return "gfx950"; }
const char* mlbp_exactgrad_last_error(void) { return g_last_error.c_str(); }
int mlbp_exactgrad_last_kernel(void) { return g_last_kernel; }

int mlbp_exactgrad_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest) {
  return pick_walk_kernel(X, n_vars, P, U, n_forest, MLBP_EXACTGRAD_X64_MAX_FOREST);
}

int mlbp_exactgrad_chunks(int32_t B, int32_t n_configs, int32_t kernel) {
  if (B <= 0 || n_configs <= 0 || (kernel != MLBP_EXACTGRAD_KERNEL_X64 && kernel != MLBP_EXACTGRAD_KERNEL_GENERIC))
    return fail(MLBP_EINVAL, "chunks: B = %d, n_configs = %d, kernel = %d", B, n_configs, kernel);
  return walk_chunks(B, kernel == MLBP_EXACTGRAD_KERNEL_X64 ? (n_configs + 3) / 4 : n_configs, MLBP_EXACTGRAD_MIN_WORKGROUPS);
}

// The header's workspace formula over n walked entries: the configurations of the exact call, the list's of a listed one.
static int64_t workspace_of(int which, int32_t B, int64_t n, int32_t X, int32_t n_vars, int32_t P, int32_t U) {
  const int chunks = mlbp_exactgrad_chunks(B, (int32_t)n, which);
  if (chunks < 0) return chunks;
  return (int64_t)B * chunks * chunk_doubles(which, 2 + (int64_t)n_vars * X + (int64_t)P * X * X, n_vars, P, U, X) * 8;
}

int64_t mlbp_exactgrad_workspace_bytes(int32_t B, int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t n_cut) {
  const int which = mlbp_exactgrad_pick_kernel(X, n_vars, P, U, n_forest);
  if (which < 0) return which;
  if (n_cut < 0 || n_cut > n_vars) return fail(MLBP_EINVAL, "workspace: n_cut = %d with %d variables", n_cut, n_vars);
  const int64_t n_configs = count_configs(X, n_cut);
  if (n_configs < 0) return too_many_configs(X, n_cut);
  return workspace_of(which, B, n_configs, X, n_vars, P, U);
}

int mlbp_exactgrad_check_plan(const int32_t* plan, int32_t n_words, int32_t X) { return check_packed_plan(plan, n_words, X); }

int mlbp_exactgrad_f64(const mlbp_exactgrad_args* a, void* stream) {
  g_last_kernel = MLBP_EXACTGRAD_KERNEL_NONE;
  // a negative plan_words: the struct is the `args` of a mlbp_exactgrad_listed_args and the list lies behind it
  const mlbp_exactgrad_listed_args* list = a && a->plan_words < 0 ? reinterpret_cast<const mlbp_exactgrad_listed_args*>(a) : nullptr;
  mlbp_exactgrad_args plain;
  if (list) {
    plain = *a;
    plain.plan_words = -plain.plan_words;
    a = &plain;
    if (list->N < 0 || list->N > MLBP_EXACTGRAD_MAX_LISTED)
      return fail(MLBP_EINVAL, "N = %d: a list holds 1 to %d configurations (0: the exact call)", list->N, MLBP_EXACTGRAD_MAX_LISTED);
  }
  const bool listed = list && list->N > 0;                     // the header's listed mode: the walk's entries are the list's
  int64_t n_configs = listed ? list->N : 0;
  const int which = check_walk_args(a, mlbp_exactgrad_pick_kernel, [listed, list](const mlbp_exactgrad_args* a) {
    if (!a->log_z) return fail(MLBP_EINVAL, "log_z is NULL");
    if (listed && a->n_cut > 0 && a->n_cut <= MLBP_EXACTGRAD_MAX_CUT && !list->configs)
      return fail(MLBP_EINVAL, "configs is NULL in a listed call with cutset variables");
    if (listed && !list->log_q) return fail(MLBP_EINVAL, "log_q is NULL in a listed call");
    const bool want_grad = a->grad_ee || a->grad_ed;
    if (!want_grad && !a->expect_ee && !a->expect_ed) return (int)MLBP_OK;
    if (!a->phi_en_en || !a->phi_en_en_w1 || !a->phi_en_de || a->F_ee < 1 || a->F_ed < 1 || a->Vde < 1 || (a->P > 0 && !a->pair_phi) ||
        (a->U > 0 && (!a->unary_kind || !a->unary_obs)))
      return fail(MLBP_EINVAL, "expect_* and grad_* need the feature inputs: phi_en_en, phi_en_en_w1, phi_en_de, pair_phi, unary_kind, unary_obs "
                               "and F_ee, F_ed, Vde >= 1 (F_ee %d, F_ed %d, Vde %d)", a->F_ee, a->F_ed, a->Vde);
    if (a->F_ee > MAXF || a->F_ed > MAXF)
      return fail(MLBP_EUNSUPPORTED, "F_ee = %d, F_ed = %d: at most %d features each are supported", a->F_ee, a->F_ed, MAXF);
    if (want_grad && !a->labels) return fail(MLBP_EINVAL, "grad_* needs labels");
    return (int)MLBP_OK;
  }, &n_configs, listed);
  if (which < 0) return which;
  const int chunks = mlbp_exactgrad_chunks(a->B, (int32_t)n_configs, which);
  if (chunks < 0) return chunks;
  if (int e = check_walk_workspace(a, workspace_of(which, a->B, n_configs, a->X, a->n_vars, a->P, a->U))) return e;
  if (int e = check_device("libmlbp_exactgrad.so")) return e;
  const bool want_expect = a->grad_ee || a->grad_ed || a->expect_ee || a->expect_ed;
  GradDev d;
  fill_walk_dev(d, a, n_configs, chunks, which);
  d.phi_en_en = a->phi_en_en; d.phi_en_en_w1 = a->phi_en_en_w1; d.phi_en_de = a->phi_en_de;
  d.pair_phi = a->pair_phi; d.unary_kind = a->unary_kind; d.unary_obs = a->unary_obs; d.labels = a->labels;
  d.log_z = a->log_z; d.marginals = a->marginals; d.pair_marginals = a->pair_marginals;
  d.expect_ee = a->expect_ee; d.expect_ed = a->expect_ed; d.grad_ee = a->grad_ee; d.grad_ed = a->grad_ed;
  d.stride = 2 + (int64_t)a->n_vars * a->X + (int64_t)a->P * a->X * a->X;
  d.F_ee = want_expect ? a->F_ee : 0; d.F_ed = want_expect ? a->F_ed : 0; d.Vde = a->Vde;
  d.listed = listed;                                           // N == 0: the two fields are not looked at, whatever they hold
  d.configs = listed && a->n_cut > 0 ? list->configs : nullptr;
  d.log_q = listed ? list->log_q : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(a->B, chunks);
  (void)hipGetLastError();
  if (which == MLBP_EXACTGRAD_KERNEL_X64) {
    const size_t lds = (size_t)x64_lds_bytes(a->n_vars, a->P, a->U, a->n_forest);
    if (a->n_forest <= 1) {                                     // NF = max(n_forest, 1): the register accumulators of the instance
      if (int e = grant_x64_lds((const void*)exactgrad_x64_kernel<1>, 0, MLBP_CUTSET_X64_LDS_BYTES)) return e;
      hipLaunchKernelGGL(exactgrad_x64_kernel<1>, grid, dim3(WG), lds, st, d);
    } else {
      if (int e = grant_x64_lds((const void*)exactgrad_x64_kernel<2>, 1, MLBP_CUTSET_X64_LDS_BYTES)) return e;
      hipLaunchKernelGGL(exactgrad_x64_kernel<2>, grid, dim3(WG), lds, st, d);
    }
  } else {
    const size_t lds = generic_walk_lds(d, a->workspace + (int64_t)a->B * chunks * d.stride);
    hipLaunchKernelGGL(exactgrad_generic_kernel, grid, dim3(WG), lds, st, d);
  }
  if (int e = launched("exactgrad")) return e;
  hipLaunchKernelGGL(exactgrad_combine_kernel, dim3(a->B), dim3(WG), 0, st, d);
  if (int e = launched("combine")) return e;
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
