// Batched sum-product sweeps for gfx950 (MI355X): the hot path of libmlbp.so.
//
// One 256-thread workgroup (4 wavefronts of 64) owns one factor graph for ALL sweeps of a call:
//   * the graph's messages (n_msgs x X f64) are staged into LDS once, updated there and written
//     back once -- the per-update traffic of the reference's `graph.messages` dict never reaches
//     HBM;
//   * pairwise potential tables are streamed HBM -> VGPR with 16-byte-per-lane loads (8 rows of
//     the 64x64 table = 4 KiB per workgroup load instruction, fully coalesced in BOTH message
//     directions), and the table of the NEXT pairwise update is prefetched into a second register
//     set while the current update reduces/normalises, so every workgroup keeps 32 KiB in flight;
//   * the op list is identical for every graph of the launch (wave-uniform control flow, scalar
//     loads).
// Updates inside a graph are strictly sequential (Gauss-Seidel order of LBP.py:227-243);
// parallelism comes from batch x |X| only.
//
// Algorithmic HBM bytes per pairwise update: (X*X + 2X) * 8.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "mlbp_internal.h"
#include "mlbp_device.h"

using mlbp::fail;
using namespace mlbp_dev;

namespace {

constexpr int WG = 256;

// Uniform check of the graph's table indices; an out-of-range index would be an out-of-bounds
// read, so the whole graph is skipped and the status word raised instead.
__device__ __forceinline__ bool tables_in_range(const SweepDev& d, int g) {
  bool ok = true;
  for (int i = threadIdx.x; i < d.P; i += WG)
    ok &= (unsigned)d.pair_tab[(size_t)g * d.P + i] < (unsigned)d.n_pair_tables;
  for (int i = threadIdx.x; i < d.U; i += WG)
    ok &= (unsigned)d.unary_tab[(size_t)g * d.U + i] < (unsigned)d.n_unary_tables;
  int all_ok = __syncthreads_and(ok ? 1 : 0);
  if (!all_ok && threadIdx.x == 0) atomicExch(d.status, 1);
  return all_ok != 0;
}

// ------------------------------------------------------------------------------------------------
// X = 64, float64, the EXACT kernel ("fused" program form, see build_fused_program in mlbp_compile.cpp): thread t holds rows 8k + (t >> 5),
// columns 2 (t & 31) .. +1 of a resident table (as double2 element k * 256 + t).  It normalises after every update like the
// reference and is the fix-up pass behind the fast kernels (mlbp_lean.hip, mlbp_shared.hip), the kernel for
// normalize_messages = False and for programs whose unary updates cannot be hoisted:
//   * unary factor->variable messages depend on nothing but their table, so when the program
//     allows it (every such slot is written before it is first read) they are all computed once,
//     in parallel over the 4 waves, before the first sweep, and the UNARY ops are dropped -- the
//     values are bit-identical to recomputing them every sweep as the reference does;
//   * a variable->factor update that feeds the next pairwise update is fused into it: every wave
//     forms the product redundantly (lane i = state i), so no barrier separates the two;
//   * every wave finishes every update redundantly (same inputs, same order => same bits) and
//     stores the result itself, so a wave only ever reads back its own LDS writes; the single
//     workgroup barrier per pairwise update orders the exchange of partial sums, which lives in a
//     double-buffered scratch;
//   * NT > 0: the graph's (at most NT) pairwise tables are loaded ONCE into registers and reused
//     by every sweep of the call (16 f64 per thread and table); NT == 0 streams with a one-table
//     register prefetch as before;
//   * init != 0 starts from uniform messages instead of reading them (FactorGraph.initialize fused).
// ------------------------------------------------------------------------------------------------
// VariableNode.get_marginal (LBP.py:392-400) for every variable of the graph, straight from the
// normalised messages in LDS: uniform x incoming messages in facset order, nan_to_num after each
// product, renormalise.  Wave w takes variables w, w+4, ...
__device__ __forceinline__ void marginals_from_lds_x64(const SweepDev& d, const double* msg, int g, int wave, int lane) {
  if (!d.marginals) return;
  const const_i32p off = as_const(d.readout), slots = as_const(d.readout + d.n_vars + 1);
  for (int v = wave; v < d.n_vars; v += 4) {
    double acc = 1.0 / 64.0;
    for (int q = off[v]; q < off[v + 1]; ++q) acc = mul_nan_to_num(msg[slots[q] * 64 + lane], acc);
    d.marginals[((size_t)g * d.n_vars + v) * 64 + lane] = renorm(acc, wave_sum(acc), 1.0 / 64.0, true);
  }
}

using mlbp::FOP_UNARY; using mlbp::FOP_PAIR_TM; using mlbp::FOP_PAIR_MT; using mlbp::FOP_VAR;
using mlbp::FOP_VAR_PAIR_TM; using mlbp::FOP_VAR_PAIR_MT; using mlbp::FOP_BUNDLED;

constexpr int LP_MAX_BLOCKS = 4096;
constexpr int LP_WG = 256;
__device__ double g_lp_partials[LP_MAX_BLOCKS];
__device__ unsigned g_lp_done[2] = {0, 0};

// FactorGraph.get_posterior_probs (LBP.py:247-259) behind the sweeps of the same call (train_mp.py:381-400 calls one after the
// other): the fix-up pass, which walks every graph's flag anyway, also takes the log-posteriors and their batch sum.
struct PosteriorDev {
  const int32_t* labels;   // [B][n_vars] or NULL (off)
  double* out;             // [B]
  double* sum_out;         // [1] or NULL
  unsigned generation;     // of the batch sum's arrival counter (see log_posterior_kernel)
  int32_t pad_;
};

struct FusedDev {
  PosteriorDev post;
  const uint8_t* only;     // when non-NULL: run only graphs with only[g] != 0 (fix-up pass)
  const int32_t* image;    // fused op headers, source lists, hoist list, constant-product lists (one block)
  const int32_t* fsweeps;  // [n_sweeps][2]
  int32_t n_fops, n_psrcs, n_hoist, n_cprod, n_cpw, n_ext, init;
  int32_t n_graphs;        // B
};
constexpr int FIXUP_GRAPHS_PER_WG = 64;

template <bool MT>
__device__ __forceinline__ void pair_partials(const double2 (&T)[8], const double* m, double* red, int rg, int cp,
                                              int lane) {
  if (MT) {
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const double mi = m[8 * k + rg];
      a0 += mi * T[k].x;
      a1 += mi * T[k].y;
    }
    reinterpret_cast<double2*>(red + rg * 64)[cp] = make_double2(a0, a1);
  } else {
    const double2 mj = reinterpret_cast<const double2*>(m)[cp];
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = T[k].x * mj.x + T[k].y * mj.y;
    // transposing butterfly over the 16 lanes of a DPP row: each step pairs lane l with its mirror
    // and halves the live values (8 -> 4 -> 2 -> 1); "up" lanes keep the upper half.
    {
      const bool up = lane & 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double send = up ? v[i] : v[i + 4], keep = up ? v[i + 4] : v[i];
        v[i] = keep + dpp_mov<0x140>(send);
      }
    }
    {
      const bool up = lane & 4;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const double send = up ? v[i] : v[i + 2], keep = up ? v[i + 2] : v[i];
        v[i] = keep + dpp_mov<0x141>(send);
      }
    }
    {
      const bool up = lane & 2;
      const double send = up ? v[0] : v[1], keep = up ? v[1] : v[0];
      v[0] = keep + dpp_mov<0x1B>(send);
    }
    v[0] += dpp_mov<0xB1>(v[0]);
    // lane holds row 8k+rg summed over the 32 columns of its 16-lane row; the other 32 columns
    // sit in the neighbouring row of the same half-wave: both go to LDS, added after the barrier.
    if ((lane & 1) == 0) {
      const int k = ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
      red[((lane >> 4) & 1) * 64 + 8 * k + rg] = v[0];
    }
  }
}

// ---- gradient fused into the sweep epilogue (X = 64, F = (3, 6), tables resident) --------------------
// After the last sweep the workgroup still holds what FactorGraph.get_unregularized_gradeint needs
// (LBP.py:301-320): the pairwise tables in registers, the normalised messages in LDS -- and a unary
// factor's normalised message IS its belief vector au.normalize(table) whenever the table's total is
// positive (LBP.py:540 vs 494-498).  Only the shared feature tensors come from L2.  Saves the
// standalone gradient kernel's second pass over every table in HBM.
// umsg[u] = message slot of unary slot u's factor->variable message, upos[u] = 1 when its table total
// was positive (both filled in the prologue from the hoist list).  scratch: >= 4*24 doubles of LDS.
template <int NT>
__device__ __forceinline__ void gradient_epilogue_x64(const SweepDev& d, const GradFusedDev& gf, const double2 (&tab)[NT][8],
                                                      const double* msg, const int32_t* umsg, const int32_t* upos,
                                                      double* scratch, int g) {
  const int32_t* ukind = upos + d.U;      // staged by the prologue right behind upos: kind, observed
  const int32_t* uobs = ukind + d.U;      // column and label of every unary factor of this graph
  const int32_t* ulab = uobs + d.U;
  constexpr int FEE = 3, FED = 6;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, rg = t >> 5, cp = t & 31;
  double pacc[NT][FEE + 1];
#pragma unroll
  for (int p = 0; p < NT; ++p) {
#pragma unroll
    for (int f = 0; f <= FEE; ++f) pacc[p][f] = 0.0;
    if (p < d.P) {
      const double* c = msg + gf.pair_c_slot[p] * 64;
      const double* r = msg + gf.pair_r_slot[p] * 64;
      // interleaved [64][64][F] features: measured faster here than the planar copies the standalone
      // gradient kernel prefers (0.517 vs 0.55 ms per fused launch, tools/time_train_step.py)
      const double* phi = gf.pair_phi[p] ? gf.phi_en_en_w1 : gf.phi_en_en;
      const double2 rj = reinterpret_cast<const double2*>(r)[cp];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const double ci = c[8 * k + rg];
        const double w0 = (ci * rj.x) * tab[p][k].x, w1 = (ci * rj.y) * tab[p][k].y;
        pacc[p][0] += w0 + w1;
        const double* ph = phi + ((size_t)(8 * k + rg) * 64 + 2 * cp) * FEE;
#pragma unroll
        for (int f = 0; f < FEE; ++f) pacc[p][1 + f] += w0 * ph[f] + w1 * ph[FEE + f];
      }
#pragma unroll
      for (int f = 0; f <= FEE; ++f) pacc[p][f] = wave_sum(pacc[p][f]);
    }
  }
  // unary factors: wave w takes slots w, w+4, ...; belief = normalised message (zero when the table
  // total was <= 0).  kind / observed column / label were staged in LDS by the prologue; the feature
  // slabs of a whole batch of factors are requested before the first reduction.
  double uee[FEE] = {0.0, 0.0, 0.0}, ued[FED] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool bad = false;
  constexpr int UB = 3;
  for (int u0 = wave; u0 < d.U; u0 += 4 * UB) {
    double b[UB], pv[UB][FED];
    int kd[UB], at[UB];                       // kind and scalar offset of the label's feature row
#pragma unroll
    for (int j = 0; j < UB; ++j) {
      const int u = u0 + 4 * j;
      kd[j] = -1;
      if (u < d.U) {
        const int kind = __builtin_amdgcn_readfirstlane(ukind[u]), obs = __builtin_amdgcn_readfirstlane(uobs[u]);
        const int lab = __builtin_amdgcn_readfirstlane(ulab[u]);
        const int cols = kind == 2 ? gf.Vde : 64;
        if ((unsigned)obs >= (unsigned)cols || (unsigned)lab >= 64u) { bad = true; continue; }
        kd[j] = kind;
        b[j] = upos[u] ? msg[umsg[u] * 64 + lane] : 0.0;
        if (kind == 2) {
          const double* ph = gf.phi_en_de_t + ((size_t)obs * 64 + lane) * FED;
          at[j] = (obs * 64 + lab) * FED;
#pragma unroll
          for (int f = 0; f < FED; ++f) pv[j][f] = ph[f];
        } else {
          const double* ph = (kind ? gf.phi_en_en_w1_t : gf.phi_en_en_t) + ((size_t)obs * 64 + lane) * FEE;
          at[j] = (obs * 64 + lab) * FEE;
#pragma unroll
          for (int f = 0; f < FEE; ++f) pv[j][f] = ph[f];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < UB; ++j) {
      if (kd[j] == 2) {
#pragma unroll
        for (int f = 0; f < FED; ++f) ued[f] += gf.phi_en_de_t[at[j] + f] - wave_sum(b[j] * pv[j][f]);
      } else if (kd[j] >= 0) {
        const double* base = kd[j] ? gf.phi_en_en_w1_t : gf.phi_en_en_t;
#pragma unroll
        for (int f = 0; f < FEE; ++f) uee[f] += base[at[j] + f] - wave_sum(b[j] * pv[j][f]);
      }
    }
  }
  if (bad && lane == 0) atomicExch(d.status, 1);
  // combine the four waves: per wave NT*(FEE+1) pair sums + FEE + FED unary sums
  constexpr int PER = NT * (FEE + 1) + FEE + FED;
  if (lane == 0) {
    double* o = scratch + wave * PER;
#pragma unroll
    for (int p = 0; p < NT; ++p)
#pragma unroll
      for (int f = 0; f <= FEE; ++f) o[p * (FEE + 1) + f] = pacc[p][f];
#pragma unroll
    for (int f = 0; f < FEE; ++f) o[NT * (FEE + 1) + f] = uee[f];
#pragma unroll
    for (int f = 0; f < FED; ++f) o[NT * (FEE + 1) + FEE + f] = ued[f];
  }
  lds_barrier();
  if (t == 0) {
    double tot[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) tot[q] = (scratch[q] + scratch[PER + q]) + (scratch[2 * PER + q] + scratch[3 * PER + q]);
    double gee[FEE];
#pragma unroll
    for (int f = 0; f < FEE; ++f) gee[f] = tot[NT * (FEE + 1) + f];
    bool lbad = false;
#pragma unroll
    for (int p = 0; p < NT; ++p) {
      if (p < d.P) {
        const int l0 = gf.pair_label[((size_t)g * d.P + p) * 2], l1 = gf.pair_label[((size_t)g * d.P + p) * 2 + 1];
        if ((unsigned)l0 >= 64u || (unsigned)l1 >= 64u) { lbad = true; continue; }
        const double* phi = gf.pair_phi[p] ? gf.phi_en_en_w1 : gf.phi_en_en;
        const double Z = tot[p * (FEE + 1)];
#pragma unroll
        for (int f = 0; f < FEE; ++f)
          gee[f] += phi[((size_t)l0 * 64 + l1) * FEE + f] - (Z > 0.0 ? tot[p * (FEE + 1) + 1 + f] / Z : 0.0);
      }
    }
    if (lbad) atomicExch(d.status, 1);
#pragma unroll
    for (int f = 0; f < FEE; ++f) gf.grad_en_en[(size_t)g * FEE + f] = gee[f];
#pragma unroll
    for (int f = 0; f < FED; ++f) gf.grad_en_de[(size_t)g * FED + f] = tot[NT * (FEE + 1) + FEE + f];
  }
}

// Register budget: the resident tables take 32 VGPRs each; the waves-per-SIMD floor keeps the
// allocator at 3 workgroups per CU with 3 resident tables (<= 168 VGPRs) and 4 otherwise (<= 128).
//
// LDS image of one workgroup (doubles unless noted):
//   msg   [n_msgs][64]      the graph's messages
//   ext   [n_ext][64]       slot n_msgs = the uniform vector; then one "constant product" per
//                           distinct set of hoisted unary messages a variable multiplies in
//   gin   [64]              input vector of the pairwise update in flight
//   red   [8][64]           partial sums of the contraction
//   prog  int32             fused op headers [n_fops][8], source lists, hoist / constant-product
//                           lists, the graph's table indices
template <bool NORM, int NT, bool GRAD>
__device__ __forceinline__ void sweep_x64_fused_body(const SweepDev& d, const FusedDev& f, const GradFusedDev& gf, const int g) {
  extern __shared__ double lds[];
  double* msg = lds;
  double* gin = lds + (size_t)(d.n_msgs + f.n_ext) * 64;
  double* red = gin + 64;
  int32_t* prog = reinterpret_cast<int32_t*>(red + 512);
  const int32_t* psrcs = prog + f.n_fops * 8;          // [n_psrcs]
  const int32_t* phoist = psrcs + f.n_psrcs;            // [n_hoist][2]
  const int32_t* pcp = phoist + 2 * f.n_hoist;          // [n_cpw] constant-product lists: count, slots...
  int32_t* tabidx = const_cast<int32_t*>(pcp) + f.n_cpw;  // [P + U] this graph's table indices
  int32_t* flags = tabidx + d.P + d.U;                  // [0] = vector wave already stored the v->f message
  int32_t* umsg = flags + 4;                            // [U] message slot of each unary factor's message
  int32_t* upos = umsg + d.U;                           // [U] 1 when that factor's table total was positive

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int rg = t >> 5, cp = t & 31;
  double* gm = d.msgs + (size_t)g * d.n_msgs * 64;
  const double uniform = 1.0 / 64.0;
  const const_i32p c_fsweeps = as_const(f.fsweeps), c_pairseq = as_const(d.pairseq);

  // ---- phase A: table indices (range-checked), program image and messages into LDS ----
  bool ok = true;
  for (int i = t; i < d.P + d.U; i += WG) {
    const int v = i < d.P ? d.pair_tab[(size_t)g * d.P + i] : d.unary_tab[(size_t)g * d.U + (i - d.P)];
    ok &= (unsigned)v < (unsigned)(i < d.P ? d.n_pair_tables : d.n_unary_tables);
    tabidx[i] = v;
  }
  {
    const int n_img = f.n_fops * 8 + f.n_psrcs + 2 * f.n_hoist + f.n_cpw;
    for (int i = t; i < n_img; i += WG) prog[i] = f.image[i];
    double2* dst = reinterpret_cast<double2*>(msg);
    if (f.init) {
      for (int i = t; i < d.n_msgs * 32; i += WG) dst[i] = make_double2(uniform, uniform);
    } else {
      const double2* src = reinterpret_cast<const double2*>(gm);
      for (int i = t; i < d.n_msgs * 32; i += WG) dst[i] = src[i];
    }
    if (t < 32) dst[d.n_msgs * 32 + t] = make_double2(uniform, uniform);    // ext slot 0
    if (t == 0) flags[0] = 0;
    if (GRAD)
      for (int i = t; i < d.U; i += WG) {
        umsg[i] = -1; upos[i] = 0;
        upos[d.U + i] = gf.unary_kind[i];
        upos[2 * d.U + i] = gf.unary_obs[(size_t)g * d.U + i];
        upos[3 * d.U + i] = gf.unary_label[(size_t)g * d.U + i];
      }
  }
  if (!__syncthreads_and(ok ? 1 : 0)) {       // an out-of-range table index: skip the graph, raise the status word
    if (t == 0) atomicExch(d.status, 1);
    return;
  }

  // ---- phase B: every HBM load of the prologue in flight together ----
  constexpr int NR = NT > 0 ? NT : 1;
  double2 tab[NR][8];
  int pair_k = 0;
  if (NT > 0) {
#pragma unroll
    for (int p = 0; p < NT; ++p) {
      if (p < d.P) {
        const int ti = __builtin_amdgcn_readfirstlane(tabidx[p]);
        const double2* T = reinterpret_cast<const double2*>(d.pair_tables + (size_t)ti * 4096);
#pragma unroll
        for (int k = 0; k < 8; ++k) tab[p][k] = T[k * WG + t];
      }
    }
  } else {
    const int s0 = c_pairseq[0];
    if (s0 >= 0) {
      const int ti = __builtin_amdgcn_readfirstlane(tabidx[s0]);
      const double2* T = reinterpret_cast<const double2*>(d.pair_tables + (size_t)ti * 4096);
#pragma unroll
      for (int k = 0; k < 8; ++k) tab[0][k] = T[k * WG + t];
    }
  }
  // hoisted unary messages: wave w takes entries w, w+4, ...; 8 loads in flight per wave
  constexpr int HB = 8;
  for (int h0 = wave; h0 < f.n_hoist; h0 += 4 * HB) {
    double r[HB];
#pragma unroll
    for (int j = 0; j < HB; ++j) {
      const int h = h0 + 4 * j;
      r[j] = (h < f.n_hoist) ? d.unary_tables[(size_t)tabidx[d.P + phoist[2 * h]] * 64 + lane] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < HB; ++j) {
      const int h = h0 + 4 * j;
      if (h < f.n_hoist) {
        const double tot = wave_sum(r[j]);
        msg[phoist[2 * h + 1] * 64 + lane] = renorm(r[j], tot, uniform, NORM);
        if (GRAD && lane == 0) { umsg[phoist[2 * h]] = phoist[2 * h + 1]; upos[phoist[2 * h]] = tot > 0.0 ? 1 : 0; }
      }
    }
  }
  lds_barrier();
  // constant products: uniform times the hoisted messages a variable multiplies in, in facset
  // order with nan_to_num after each product (the constant prefix of LBP.py:381-386)
  {
    int at = 0;
    for (int k = 0; k < f.n_cprod; ++k) {
      const int cnt = pcp[at];
      if ((k & 3) == wave) {
        double acc = uniform;
        bool clean = true;
        for (int q = 0; q < cnt; ++q) {
          acc *= msg[pcp[at + 1 + q] * 64 + lane];
          clean = clean && __all(__builtin_isfinite(acc));
        }
        // a non-finite intermediate means nan_to_num would have acted inside the constant part:
        // poison the product so that every update using it takes the exact-order path
        msg[(d.n_msgs + 1 + k) * 64 + lane] = clean ? acc : __builtin_nan("");
      }
      at += 1 + cnt;
    }
  }
  lds_barrier();

  // Main loop.  Wave 0 is the graph's "vector wave": it alone runs the 64-element work on the
  // critical path of every update (variable product, gathering the partial sums, normalising the
  // factor->variable message); all four waves run the table contraction.  Two LDS-only barriers per
  // pairwise update hand the input vector to the contraction and the partial sums back.
  for (int s = 0; s < d.n_sweeps; ++s) {
    const int op0 = c_fsweeps[2 * s], nop = c_fsweeps[2 * s + 1];
    for (int o = op0; o < op0 + nop; ++o) {
      const int4 h0 = reinterpret_cast<const int4*>(prog)[2 * o];
      const int4 h1 = reinterpret_cast<const int4*>(prog)[2 * o + 1];
      const int kind = __builtin_amdgcn_readfirstlane(h0.x) & 0xFF;
      if (kind == FOP_UNARY) {
        if (wave == 0) {
          const int us = __builtin_amdgcn_readfirstlane(h0.y), c = __builtin_amdgcn_readfirstlane(h0.w);
          const double r = d.unary_tables[(size_t)tabidx[d.P + us] * 64 + lane];
          msg[c * 64 + lane] = renorm(r, wave_sum(r), uniform, NORM);
        }
        continue;
      }
      int pslot, dst;
      const double* m;
      const bool from_var = (kind == FOP_VAR || kind == FOP_VAR_PAIR_TM || kind == FOP_VAR_PAIR_MT);
      const int c = __builtin_amdgcn_readfirstlane(h0.w);
      if (from_var) {
        if (wave == 0) {
          // fast form: (constant product) x (the varying messages), valid while every factor is
          // finite and non-negative and the product is not identically zero; then the product's
          // scale cancels in the normalised pairwise update, so the contraction takes it
          // unnormalised and wave 1 normalises and stores the variable->factor message meanwhile
          const int a = __builtin_amdgcn_readfirstlane(h0.y), n = __builtin_amdgcn_readfirstlane(h0.z);
          const int4 s4 = *reinterpret_cast<const int4*>(psrcs + a);
          double acc = msg[s4.x * 64 + lane];
          if (n > 1) acc *= msg[s4.y * 64 + lane];
          if (n > 2) acc *= msg[s4.z * 64 + lane];
          if (n > 3) acc *= msg[s4.w * 64 + lane];
          for (int q = 4; q < n; ++q) acc *= msg[psrcs[a + q] * 64 + lane];
          const bool fast = __all(acc >= 0.0 && acc < __builtin_huge_val()) && __any(acc > 0.0);
          if (fast && kind != FOP_VAR) {
            gin[lane] = acc;
            if (lane == 0) flags[0] = 0;
          } else {
            // exact reference order (LBP.py:381-389) from the raw messages
            const int ae = __builtin_amdgcn_readfirstlane(h1.z), ne = __builtin_amdgcn_readfirstlane(h1.w);
            double ex = uniform;
            for (int q = 0; q < ne; ++q) ex = mul_nan_to_num(msg[psrcs[ae + q] * 64 + lane], ex);
            const double mn = renorm(ex, wave_sum(ex), uniform, NORM);
            msg[c * 64 + lane] = mn;
            gin[lane] = mn;
            if (lane == 0) flags[0] = 1;
          }
        }
        if (kind == FOP_VAR) continue;
        m = gin;
        pslot = __builtin_amdgcn_readfirstlane(h1.x);
        dst = __builtin_amdgcn_readfirstlane(h1.y);
      } else {
        pslot = __builtin_amdgcn_readfirstlane(h0.y);
        m = msg + __builtin_amdgcn_readfirstlane(h0.z) * 64;
        dst = c;
      }
      const bool mt = (kind == FOP_PAIR_MT || kind == FOP_VAR_PAIR_MT);
      lds_barrier();         // the input vector (and every earlier vector-wave store) is visible
      if (NT > 0) {
#pragma unroll
        for (int p = 0; p < NT; ++p) {
          if (p == pslot) {
            if (mt) pair_partials<true>(tab[p], m, red, rg, cp, lane);
            else pair_partials<false>(tab[p], m, red, rg, cp, lane);
          }
        }
      } else {
        double2 cur[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) cur[k] = tab[0][k];
        ++pair_k;
        const int sn = c_pairseq[pair_k];
        if (sn >= 0) {
          const int ti = __builtin_amdgcn_readfirstlane(tabidx[sn]);
          const double2* T = reinterpret_cast<const double2*>(d.pair_tables + (size_t)ti * 4096);
#pragma unroll
          for (int k = 0; k < 8; ++k) tab[0][k] = T[k * WG + t];
        }
        if (mt) pair_partials<true>(cur, m, red, rg, cp, lane);
        else pair_partials<false>(cur, m, red, rg, cp, lane);
      }
      if (from_var && wave == 1 && flags[0] == 0) {
        // off the critical path: normalise and store the variable->factor message (LBP.py:387-389)
        const double v = gin[lane];
        msg[c * 64 + lane] = renorm(v, wave_sum(v), uniform, NORM);
      }
      lds_barrier();         // partial sums are in LDS
      if (wave == 0) {
        double r;
        if (mt) {
          r = 0.0;
#pragma unroll
          for (int q = 0; q < 8; ++q) r += red[q * 64 + lane];
        } else {
          r = red[lane] + red[64 + lane];
        }
        msg[dst * 64 + lane] = renorm(r, wave_sum(r), uniform, NORM);
      }
    }
  }
  lds_barrier();
  {
    const double2* src = reinterpret_cast<const double2*>(msg);
    double2* dst = reinterpret_cast<double2*>(gm);
    for (int i = t; i < d.n_msgs * 32; i += WG) dst[i] = src[i];
  }
  if (NORM) marginals_from_lds_x64(d, msg, g, wave, lane);
  if (GRAD) gradient_epilogue_x64<(NT > 0 ? NT : 1)>(d, gf, tab, msg, umsg, upos, red, g);       // (NT = 0 with GRAD: no pairwise factor at all -- a single predicted word --, the unary terms only: every pairwise step of the epilogue is behind p < d.P)
}

// Log-posteriors of the block's 64 graphs from the marginals in memory (the fast kernel's, or the ones this workgroup has just
// redone), and -- sum_out given -- their batch sum in a fixed order: lanes, then the blocks' partials by the last block to
// arrive (the two-counter protocol of log_posterior_kernel).
// The label thread t reads when the block's variables fit one wave each (n_vars <= WG / 64: wave v takes variable v of the
// block's 64 graphs), requested by the caller TOGETHER with the flags -- one round of memory latency instead of two; -1: none.
__device__ __forceinline__ int posterior_prefetch_label(const SweepDev& d, const PosteriorDev& p, int base, int n_graphs) {
  const int t = threadIdx.x, v = t >> 6, g = base + (t & 63);
  if (!p.labels || d.n_vars > WG / 64 || v >= d.n_vars || g >= n_graphs) return -1;
  return p.labels[(size_t)g * d.n_vars + v];
}
__device__ __forceinline__ void posterior_of_block(const SweepDev& d, const PosteriorDev& p, int base, int n_graphs, int my_label) {
  __shared__ double part[WG / 64];
  __shared__ double lpv[WG];
  __shared__ bool last;
  __syncthreads();                                   // (the marginals of graphs redone above are this workgroup's own stores)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double total = 0.0;
  const int g = base + t;
  if (d.n_vars <= WG / 64) {
    // thread (variable t >> 6, graph t & 63): label (here already) -> marginal entry -> log, all the block's entries in ONE round
    // of latency; then the graph's terms are added in variable order, as the loop below adds them
    double lp = 0.0;
    if (wave < d.n_vars && base + lane < n_graphs) {
      if ((unsigned)my_label >= 64u) atomicExch(d.status, 1);
      else {
        lp = log(d.marginals[((size_t)(base + lane) * d.n_vars + wave) * 64 + my_label]);
        if (lp == -__builtin_huge_val()) lp = -99.99;        // LBP.py:254-256
      }
    }
    lpv[t] = lp;
    __syncthreads();
    if (t < FIXUP_GRAPHS_PER_WG && g < n_graphs) {
      for (int v = 0; v < d.n_vars; ++v) total += lpv[v * 64 + t];
      p.out[g] = total;
    }
  } else if (t < FIXUP_GRAPHS_PER_WG && g < n_graphs) {
    for (int v = 0; v < d.n_vars; ++v) {
      const int lab = p.labels[(size_t)g * d.n_vars + v];
      if ((unsigned)lab >= 64u) { atomicExch(d.status, 1); continue; }
      const double lp = log(d.marginals[((size_t)g * d.n_vars + v) * 64 + lab]);
      total += (lp == -__builtin_huge_val()) ? -99.99 : lp;  // LBP.py:254-256
    }
    p.out[g] = total;
  }
  if (!p.sum_out) return;
  if (wave == 0) {
    const double ws = wave_sum(total);
    if (lane == 0) {
      g_lp_partials[blockIdx.x] = ws;
      __threadfence();
      if (blockIdx.x == 0) g_lp_done[(p.generation + 1) & 1] = 0;
      last = atomicAdd(&g_lp_done[p.generation & 1], 1u) == gridDim.x - 1;
    }
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  double acc = 0.0;
  for (unsigned q = t; q < gridDim.x; q += WG) acc += __builtin_nontemporal_load(&g_lp_partials[q]);
  const double fs = wave_sum(acc);
  if (lane == 0) part[wave] = fs;
  __syncthreads();
  if (t == 0) {
    double v = part[0];
    for (int w = 1; w < WG / 64; ++w) v += part[w];
    *p.sum_out = v;
    g_lp_done[p.generation & 1] = 0;
  }
}

// One workgroup per graph -- or, as the fix-up pass behind a fast kernel (f.only), one workgroup per 64 graphs that
// walks their flags and redoes the (normally zero) flagged ones: 128 workgroups instead of 8192 that exit at once.
template <bool NORM, int NT, bool GRAD>
__global__ __launch_bounds__(WG, (NT >= 4 ? 2 : (NT == 3 ? 3 : 4))) void sweep_x64_fused_kernel(SweepDev d, FusedDev f, GradFusedDev gf) {
  // fix-up mode: all 64 flags in one load (lane i of every wave reads flag i; the ballot is the same in the four waves)
  int base = blockIdx.x;
  unsigned long long todo = 1;
  int my_label = -1;
  if (f.only) {
    base = blockIdx.x * FIXUP_GRAPHS_PER_WG;
    const int mine = base + (threadIdx.x & 63);
    my_label = posterior_prefetch_label(d, f.post, base, f.n_graphs);      // (requested with the flags)
    todo = __ballot(mine < f.n_graphs && f.only[mine] != 0);
  }
  while (todo) {
    const int i = __builtin_ctzll(todo);
    todo &= todo - 1;
    sweep_x64_fused_body<NORM, NT, GRAD>(d, f, gf, base + i);
    if (todo) __syncthreads();
  }
  if (f.only && f.post.labels) posterior_of_block(d, f.post, base, f.n_graphs, my_label);
}

// The fix-up pass for SEVERAL groups of graphs in one launch (mlbp_sweep_groups_f64 behind the shared-table kernels: a
// minibatch of mixed sentence shapes used to pay one near-empty launch per shape).  groups[k]: the group's descriptions as a
// single-group fix-up launch would get them, and its first workgroup; tables are streamed (NT = 0: any number of pairwise
// factors), the gradient of a redone graph comes from gradient_x64_kernel's flagged-only mode (mlbp_grad.hip).
struct FixupGroup { SweepDev d; FusedDev f; int32_t first_block, per_wg; };      // per_wg: graphs a workgroup looks at (64; 1 for a group that is redone as a whole)
__global__ __launch_bounds__(WG, 4) void sweep_x64_fixup_groups_kernel(const FixupGroup* groups, int n_groups) {
  int lo = 0, hi = n_groups - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (groups[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const FixupGroup& G = groups[lo];
  const int base = ((int)blockIdx.x - G.first_block) * G.per_wg;
  const int mine = base + (threadIdx.x & 63);
  unsigned long long todo = __ballot((int)(threadIdx.x & 63) < G.per_wg && mine < G.f.n_graphs && G.f.only[mine] != 0);
  if (!todo) return;
  const SweepDev d = G.d;
  const FusedDev f = G.f;
  const GradFusedDev gf = {};
  while (todo) {
    const int i = __builtin_ctzll(todo);
    todo &= todo - 1;
    sweep_x64_fused_body<true, 0, false>(d, f, gf, base + i);
    if (todo) __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// Any X: messages in LDS when they fit (LDSMSG) else in place in global memory (only this
// workgroup touches its graph's messages; __syncthreads orders the accesses).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double* scratch /*[4]*/) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return scratch[0] + scratch[1] + scratch[2] + scratch[3];
}

template <bool NORM, bool LDSMSG>
__global__ __launch_bounds__(WG) void sweep_generic_kernel(SweepDev d) {
  extern __shared__ double lds[];
  const int X = d.X;
  double* raw = lds;            // [X]
  double* scratch = lds + X;    // [4]
  double* lmsg = lds + X + 4;   // [n_msgs][X] when LDSMSG
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (d.only && !d.only[g]) return;
  if (!tables_in_range(d, g)) return;
  double* gm = d.msgs + (size_t)g * d.n_msgs * X;
  double* msg = LDSMSG ? lmsg : gm;
  if (d.fill_uniform) {
    for (int i = t; i < d.n_msgs * X; i += WG) msg[i] = 1.0 / (double)X;
  } else if (LDSMSG) {
    for (int i = t; i < d.n_msgs * X; i += WG) lmsg[i] = gm[i];
  }
  const int32_t* ptab = d.pair_tab + (size_t)g * d.P;
  const int32_t* utab = d.unary_tab + (size_t)g * d.U;
  const double uniform = 1.0 / (double)X;
  __syncthreads();
  for (int s = 0; s < d.n_sweeps; ++s) {
    const int op0 = d.sweeps[2 * s], nop = d.sweeps[2 * s + 1];
    for (int o = op0; o < op0 + nop; ++o) {
      const int kind = d.ops[4 * o], a = d.ops[4 * o + 1], b = d.ops[4 * o + 2], c = d.ops[4 * o + 3];
      if (kind == MLBP_OP_PAIR_TM) {
        const double* T = d.pair_tables + (size_t)ptab[a] * X * X;
        const double* m = msg + (size_t)b * X;
        for (int row = wave; row < X; row += 4) {
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
          for (int q = 0; q < b; ++q) acc = nan_to_num(msg[(size_t)d.srcs[a + q] * X + j] * acc);
          raw[j] = acc;
        }
      } else {
        const double* u = d.unary_tables + (size_t)utab[a] * X;
        for (int j = t; j < X; j += WG) raw[j] = u[j];
      }
      __syncthreads();
      double part = 0.0;
      for (int j = t; j < X; j += WG) part += raw[j];
      const double total = NORM ? block_sum(part, scratch) : 0.0;
      double* out = msg + (size_t)c * X;
      for (int j = t; j < X; j += WG) out[j] = renorm(raw[j], total, uniform, NORM);
      __syncthreads();
    }
  }
  if (LDSMSG) {
    for (int i = t; i < d.n_msgs * X; i += WG) gm[i] = lmsg[i];
  }
}

// ------------------------------------------------------------------------------------------------
// X in {128, 256, 512}, float64: every pairwise update streams a 128 KiB .. 2 MiB table, so the
// kernel is organised around that stream.  Wave w of the workgroup owns rows i = w, w+4, ...; a row
// is read by its wave as Q = X/128 fully coalesced 16-byte-per-lane loads (lane l, piece q holds
// columns 128q + 2l, +1), four rows in flight per wave (16 KiB * Q per workgroup).
//   out = T . m   (TM): the lane's 2Q message values stay in registers; per row one dot-product
//                       partial per lane, four rows reduced together by a DPP butterfly.
//   out = m^T . T (MT): the lane accumulates its 2Q columns over the wave's rows (m_i by LDS
//                       broadcast); the four waves' accumulators meet in LDS once at the end.
// Messages stay in global memory (L2 resident; 4 KiB against a 2 MiB table at X = 512).
// Algorithmic bytes per pairwise update (X*X + 2X) * 8 -- HBM-bound.
// ------------------------------------------------------------------------------------------------
// Table element type TT: double (V = 2 columns per lane and piece) or float (V = 4, the optional f32
// table mode of SURVEY.md section 8 / BASELINE config 5: half the bytes per update; products and sums stay
// in float64, so the only difference from the f64 path is the rounding of the table entries themselves).
// PAD: 0 = X is exactly 64 V Q; 1 = any even X <= 64 V Q (pieces of a row that reach past X are masked: a pair of
// columns lies wholly inside or wholly outside the row, and every row starts 16-byte aligned); 2 = any odd X (8-byte
// loads, masked per column).  Real vocabularies (train_mp.py:591-594: X = len(en_domain)) are not powers of two.
template <typename TT, int V, int PAD> struct WidePiece;
template <> struct WidePiece<double, 2, 0> {
  __device__ static __forceinline__ void load(const double* row, int idx, int, double (&o)[2]) {
    const double2 v = reinterpret_cast<const double2*>(row)[idx];
    o[0] = v.x; o[1] = v.y;
  }
};
template <> struct WidePiece<double, 2, 1> {
  __device__ static __forceinline__ void load(const double* row, int idx, int X, double (&o)[2]) {
    o[0] = 0.0; o[1] = 0.0;
    if (2 * idx < X) {
      const double2 v = reinterpret_cast<const double2*>(row)[idx];
      o[0] = v.x; o[1] = v.y;
    }
  }
};
template <> struct WidePiece<double, 2, 2> {
  __device__ static __forceinline__ void load(const double* row, int idx, int X, double (&o)[2]) {
    o[0] = 2 * idx < X ? row[2 * idx] : 0.0;
    o[1] = 2 * idx + 1 < X ? row[2 * idx + 1] : 0.0;
  }
};
template <> struct WidePiece<float, 4, 0> {
  __device__ static __forceinline__ void load(const float* row, int idx, int, double (&o)[4]) {
    const float4 v = reinterpret_cast<const float4*>(row)[idx];
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  }
};

template <bool NORM, int Q, typename TT, int V, int PAD>
__global__ __launch_bounds__(WG) void sweep_wide_kernel(SweepDev d) {
  constexpr int XP = 64 * V * Q;           // padded width
  const int X = PAD ? d.X : XP;
  extern __shared__ double lds[];
  double* vin = lds;             // [XP] input message of the update in flight (zero beyond X)
  double* raw = lds + XP;        // [XP] un-normalised result
  double* part = lds + 2 * XP;   // [4][XP] per-wave column accumulators (MT)
  double* scratch = part + 4 * XP;  // [4]
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d, g)) return;
  double* gm = d.msgs + (size_t)g * d.n_msgs * X;
  const int32_t* ptab = d.pair_tab + (size_t)g * d.P;
  const int32_t* utab = d.unary_tab + (size_t)g * d.U;
  const double uniform = 1.0 / (double)X;
  const const_i32p c_ops = as_const(d.ops), c_sweeps = as_const(d.sweeps), c_srcs = as_const(d.srcs);
  for (int s = 0; s < d.n_sweeps; ++s) {
    const int op0 = c_sweeps[2 * s], nop = c_sweeps[2 * s + 1];
    for (int o = op0; o < op0 + nop; ++o) {
      const int kind = c_ops[4 * o], a = c_ops[4 * o + 1], b = c_ops[4 * o + 2], c = c_ops[4 * o + 3];
      if (kind == MLBP_OP_PAIR_TM || kind == MLBP_OP_PAIR_MT) {
        const TT* T = reinterpret_cast<const TT*>(d.pair_tables) + (size_t)ptab[a] * X * X;
        const double* m = gm + (size_t)b * X;
        for (int j = t; j < XP; j += WG) vin[j] = j < X ? m[j] : 0.0;
        __syncthreads();
        if (d.approx_k > 0) {
          // use_approx_inference: keep the K largest entries of the message (ranks_above: the rule of mlbp_topk_f64, NaN
          // below every number), zero the rest -- sum over the index set, as au.sparse_vec_mat_dot does
          double* keep = part;
          for (int j = t; j < X; j += WG) {
            const double x = vin[j];
            int rank = 0;
            for (int i = 0; i < X; ++i) rank += ranks_above(vin[i], i, x, j);
            keep[j] = rank < d.approx_k ? x : 0.0;
          }
          __syncthreads();
          for (int j = t; j < X; j += WG) vin[j] = keep[j];
          __syncthreads();
        }
        if (kind == MLBP_OP_PAIR_TM) {
          double mj[Q][V];
#pragma unroll
          for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int e = 0; e < V; ++e) mj[q][e] = vin[64 * V * q + V * lane + e];
          for (int i0 = wave; i0 < X; i0 += 16) {          // rows i0, i0+4, i0+8, i0+12 of this wave
            double r[4][Q][V];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int row = PAD ? min(i0 + 4 * u, X - 1) : i0 + 4 * u;     // past the table: re-read the last row, result dropped
#pragma unroll
              for (int q = 0; q < Q; ++q)
                WidePiece<TT, V, PAD>::load(T + (size_t)row * X, 64 * q + lane, X, r[u][q]);
            }
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              double acc = 0.0;
#pragma unroll
              for (int q = 0; q < Q; ++q)
#pragma unroll
                for (int e = 0; e < V; ++e) acc += r[u][q][e] * mj[q][e];
              v[u] = acc;
            }
            // 4 values x 64 lanes -> 4 row sums: transposing butterfly inside each 16-lane row (4 -> 2
            // -> 1 live values), then plain sums inside the row, then the four rows through readlane
            {
              const bool up = lane & 8;
#pragma unroll
              for (int k = 0; k < 2; ++k) {
                const double send = up ? v[k] : v[k + 2], keep = up ? v[k + 2] : v[k];
                v[k] = keep + dpp_mov<0x140>(send);
              }
            }
            {
              const bool up = lane & 4;
              const double send = up ? v[0] : v[1], keep = up ? v[1] : v[0];
              v[0] = keep + dpp_mov<0x141>(send);
            }
            v[0] += dpp_mov<0x1B>(v[0]);
            v[0] += dpp_mov<0xB1>(v[0]);
            // lanes with equal (bit3, bit2) hold the same row u = 2*bit3 + bit2, summed over 16 lanes
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int src = ((u >> 1) << 3) | ((u & 1) << 2);
              const double tot = (read_lane(v[0], src) + read_lane(v[0], 16 + src)) +
                                 (read_lane(v[0], 32 + src) + read_lane(v[0], 48 + src));
              if (lane == 0 && (!PAD || i0 + 4 * u < X)) raw[i0 + 4 * u] = tot;
            }
          }
        } else {
          double acc[Q][V];
#pragma unroll
          for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int e = 0; e < V; ++e) acc[q][e] = 0.0;
          for (int i0 = wave; i0 < X; i0 += 16) {
            double r[4][Q][V];
            double mi[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int row = PAD ? min(i0 + 4 * u, X - 1) : i0 + 4 * u;
              mi[u] = (!PAD || i0 + 4 * u < X) ? vin[i0 + 4 * u] : 0.0;
#pragma unroll
              for (int q = 0; q < Q; ++q)
                WidePiece<TT, V, PAD>::load(T + (size_t)row * X, 64 * q + lane, X, r[u][q]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
              for (int q = 0; q < Q; ++q)
#pragma unroll
                for (int e = 0; e < V; ++e) acc[q][e] += mi[u] * r[u][q][e];
          }
#pragma unroll
          for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int e = 0; e < V; ++e) part[wave * XP + 64 * V * q + V * lane + e] = acc[q][e];
          __syncthreads();
          for (int j = t; j < X; j += WG) raw[j] = (part[j] + part[XP + j]) + (part[2 * XP + j] + part[3 * XP + j]);
        }
      } else if (kind == MLBP_OP_VAR) {
        for (int j = t; j < X; j += WG) {
          double acc = uniform;
          for (int q = 0; q < b; ++q) acc = nan_to_num(gm[(size_t)c_srcs[a + q] * X + j] * acc);
          raw[j] = acc;
        }
      } else {
        const double* u = d.unary_tables + (size_t)utab[a] * X;
        for (int j = t; j < X; j += WG) raw[j] = u[j];
      }
      __syncthreads();
      double psum = 0.0;
      for (int j = t; j < X; j += WG) psum += raw[j];
      const double total = NORM ? block_sum(psum, scratch) : 0.0;
      double* out = gm + (size_t)c * X;
      for (int j = t; j < X; j += WG) out[j] = renorm(raw[j], total, uniform, NORM);
      __syncthreads();
    }
  }
}

__global__ void fill_kernel(double* p, int64_t n, double v) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}

// One workgroup per graph; marginal of every variable (LBP.py:392-400).
__global__ __launch_bounds__(WG) void marginals_kernel(const double* msgs, int n_msgs, int X, int n_vars,
                                                       const int32_t* in_off, const int32_t* in_slots,
                                                       int normalize, double* out) {
  __shared__ double scratch[4];
  const int g = blockIdx.x, t = threadIdx.x;
  const double* gm = msgs + (size_t)g * n_msgs * X;
  const double uniform = 1.0 / (double)X;
  for (int v = 0; v < n_vars; ++v) {
    const int s0 = in_off[v], s1 = in_off[v + 1];
    double part = 0.0;
    double* o = out + ((size_t)g * n_vars + v) * X;
    for (int j = t; j < X; j += WG) {
      double acc = uniform;
      for (int q = s0; q < s1; ++q) acc = nan_to_num(gm[(size_t)in_slots[q] * X + j] * acc);
      o[j] = acc;
      part += acc;
    }
    if (normalize) {
      const double total = block_sum(part, scratch);
      for (int j = t; j < X; j += WG) o[j] = renorm(o[j], total, uniform, true);
    }
    __syncthreads();
  }
}

// FactorGraph.get_posterior_probs for every graph, and (when sum_out is given) their sum over the batch in a fixed
// order: lanes by DPP, the block's waves in order, then the last block to finish adds the block partials in block order.
// "Last" by an arrival counter the last block re-arms itself.  There are TWO counters, taken in turn by the launch's
// generation number, and every launch also zeroes the one it does not use: a launch that was aborted halfway leaves its counter
// dirty, the next launch (other counter) cleans it, so it cannot wedge a later one -- without the memset that used to precede
// every launch (4.6 us of every bench step).

__global__ __launch_bounds__(LP_WG) void log_posterior_kernel(const double* marg, const int32_t* labels, int B, int n_vars, int X,
                                                              double* out, double* sum_out, int32_t* status, unsigned generation) {
  __shared__ double part[LP_WG / 64];
  __shared__ bool last;
  const int g = blockIdx.x * LP_WG + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double total = 0.0;
  if (g < B) {
    for (int v = 0; v < n_vars; ++v) {
      int lab = labels[(size_t)g * n_vars + v];
      if ((unsigned)lab >= (unsigned)X) { atomicExch(status, 1); continue; }
      double lp = log(marg[((size_t)g * n_vars + v) * X + lab]);
      total += (lp == -__builtin_huge_val()) ? -99.99 : lp;  // LBP.py:254-256
    }
    out[g] = total;
  }
  if (!sum_out) return;
  const double ws = wave_sum(total);
  if (lane == 0) part[wave] = ws;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = part[0];
    for (int w = 1; w < LP_WG / 64; ++w) v += part[w];
    g_lp_partials[blockIdx.x] = v;
    __threadfence();
    if (blockIdx.x == 0) g_lp_done[(generation + 1) & 1] = 0;
    last = atomicAdd(&g_lp_done[generation & 1], 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  double acc = 0.0;                                  // block-strided partial sums per thread, then lanes, then waves: fixed order
  for (unsigned q = threadIdx.x; q < gridDim.x; q += LP_WG) acc += __builtin_nontemporal_load(&g_lp_partials[q]);
  const double fs = wave_sum(acc);
  if (lane == 0) part[wave] = fs;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = part[0];
    for (int w = 1; w < LP_WG / 64; ++w) v += part[w];
    *sum_out = v;
    g_lp_done[generation & 1] = 0;                             // ready for the next launch of this parity (a replayed capture keeps its generation)
  }
}

// The same per-graph sum for several groups of graphs (each its own variable count) in one launch: thread i finds its group
// by binary search over the groups' first indices.
__global__ __launch_bounds__(LP_WG) void log_posterior_groups_kernel(const mlbp_posterior_group* groups, int n_groups, long long n_total, int X,
                                                                     double* out, int32_t* status) {
  const long long i = (long long)blockIdx.x * LP_WG + threadIdx.x;
  if (i >= n_total) return;
  int lo = 0, hi = n_groups - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (groups[mid].start <= i) lo = mid; else hi = mid - 1;
  }
  const mlbp_posterior_group g = groups[lo];
  const long long b = i - g.start;
  if (b >= g.B) return;
  double total = 0.0;
  for (int v = 0; v < g.n_vars; ++v) {
    const int lab = g.labels[(size_t)b * g.n_vars + v];
    if ((unsigned)lab >= (unsigned)X) { atomicExch(status, 1); continue; }
    const double lp = log(g.marginals[((size_t)b * g.n_vars + v) * X + lab]);
    total += (lp == -__builtin_huge_val()) ? -99.99 : lp;  // LBP.py:254-256
  }
  out[i] = total;
}

}  // namespace

namespace mlbp {
bool exact_kernel_fuses_gradient(const mlbp_program* prog, const mlbp_sweep_args* a) {
  const mlbp_gradient_args* ga = a->gradient;
  if (!ga || a->X != 64 || !a->normalize_messages) return false;
  if (ga->B != a->B || ga->X != a->X || ga->P != prog->P || ga->U != prog->U || ga->n_msgs != prog->n_msgs || ga->msgs != a->msgs) return false;
  // (P = 0: a single predicted word, unary terms only -- fused for small batches, where the second launch is what costs: at 8192
  // graphs the per-graph gradient kernel behind the sweeps is the faster pair, 0.106 against 0.131 ms per trainer step)
  if (prog->P == 0 && a->B > 1024) return false;
  return ga->F_ee == 3 && ga->F_ed == 6 && prog->P >= 0 && prog->P <= 3 && prog->n_hoist == prog->U && prog->U <= WG &&
         ga->phi_en_en_t && ga->phi_en_en_w1_t && ga->phi_en_de_t && !(ga->flags & MLBP_GRADIENT_APPROX_BELIEFS);
}

void fill_grad_fused(const mlbp_gradient_args* ga, GradFusedDev* gf) {
  *gf = GradFusedDev{};
  gf->pair_c_slot = ga->pair_c_slot; gf->pair_r_slot = ga->pair_r_slot; gf->pair_phi = ga->pair_phi; gf->pair_label = ga->pair_label;
  gf->unary_kind = ga->unary_kind; gf->unary_obs = ga->unary_obs; gf->unary_label = ga->unary_label;
  gf->phi_en_en = ga->phi_en_en; gf->phi_en_en_w1 = ga->phi_en_en_w1;
  gf->phi_en_en_t = ga->phi_en_en_t; gf->phi_en_en_w1_t = ga->phi_en_en_w1_t; gf->phi_en_de_t = ga->phi_en_de_t;
  gf->grad_en_en = ga->grad_en_en; gf->grad_en_de = ga->grad_en_de; gf->Vde = ga->Vde; gf->enabled = 1;
}
}  // namespace mlbp

static unsigned next_lp_generation() {
  static std::atomic<unsigned> generation{0};
  return generation.fetch_add(1u) + 1u;
}

// The per-graph kernels' description of (prog, a): the op list as given, no fused read-out, every graph.  Filled in place over
// zeroed memory (a grouped call compares its descriptors word by word).
static void fill_sweep_dev(const mlbp_program* prog, const mlbp_sweep_args* a, SweepDev* d) {
  memset(d, 0, sizeof(*d));
  d->pair_tables = a->pair_tables; d->pair_tab = a->pair_tab; d->unary_tables = a->unary_tables; d->unary_tab = a->unary_tab;
  d->msgs = a->msgs; d->ops = prog->d_ops; d->srcs = prog->d_srcs; d->sweeps = prog->d_sweeps; d->pairseq = prog->d_pairseq;
  d->status = prog->d_status;
  d->n_sweeps = prog->n_sweeps; d->n_msgs = prog->n_msgs; d->P = prog->P; d->U = prog->U; d->X = a->X;
  d->n_pair_tables = a->n_pair_tables; d->n_unary_tables = a->n_unary_tables;
  d->readout = prog->d_readout; d->n_vars = prog->n_vars;
}

// LDS bytes of the exact X = 64 kernel on prog's graphs: above X64_LDS_MAX it does not apply.
constexpr size_t X64_LDS_MAX = 160 * 1024;
static size_t exact_x64_lds(const mlbp_program* prog) {
  const size_t img_words = (size_t)prog->n_fops * 8 + prog->n_psrcs + 2 * prog->n_hoist + prog->n_cpw + prog->n_written;
  return ((size_t)(prog->n_msgs + 1 + prog->n_cprod) * 64 + 64 + 512) * sizeof(double) + (img_words + prog->P + 6 * prog->U + 8) * sizeof(int32_t);
}

// The exact X = 64 kernel's description of (prog, a) -- the fused program, the marginals as its epilogue when the messages are
// normalised -- for every graph and without a posterior (G->f.only, G->f.post and the grouped launch's block fields are the
// caller's).  Returns the kernel's LDS bytes.
static size_t fill_fixup_group(const mlbp_program* prog, const mlbp_sweep_args* a, FixupGroup* G) {
  memset(G, 0, sizeof(*G));
  fill_sweep_dev(prog, a, &G->d);
  G->d.pairseq = prog->d_fpairseq;
  G->d.marginals = a->normalize_messages ? a->marginals : nullptr;
  FusedDev& f = G->f;
  f.image = prog->d_fops; f.fsweeps = prog->d_fsweeps;
  f.n_fops = prog->n_fops; f.n_psrcs = prog->n_psrcs; f.n_hoist = prog->n_hoist; f.n_cprod = prog->n_cprod; f.n_cpw = prog->n_cpw;
  f.n_ext = 1 + prog->n_cprod; f.init = a->init_messages; f.n_graphs = a->B;
  return exact_x64_lds(prog);
}

namespace mlbp {

bool exact_x64_applies(const mlbp_program* prog, const mlbp_sweep_args* a) { return a->X == 64 && exact_x64_lds(prog) <= X64_LDS_MAX; }

int launch_exact_x64(mlbp_program* prog, const mlbp_sweep_args* a, bool flagged_only, bool fuse_gradient, void* stream, bool* post_done) {
  const bool norm = a->normalize_messages != 0;
  FixupGroup G;
  const size_t lds = fill_fixup_group(prog, a, &G);
  FusedDev& f = G.f;
  f.only = flagged_only ? prog->d_bail.p : nullptr;
  GradFusedDev gf = {};
  if (fuse_gradient) fill_grad_fused(a->gradient, &gf);
  const int fixup_blocks = (a->B + FIXUP_GRAPHS_PER_WG - 1) / FIXUP_GRAPHS_PER_WG;
  const mlbp_posterior_args* pa = a->posterior;
  *post_done = pa && f.only && norm && fixup_blocks <= LP_MAX_BLOCKS;
  if (*post_done) {
    f.post.labels = pa->labels; f.post.out = pa->out; f.post.sum_out = pa->sum_out;
    f.post.generation = pa->sum_out ? next_lp_generation() : 0u;
  }
  // the kernel keeps the tables in registers when the graph has at most 3 of them, else it streams them
  const int nt = (prog->P >= 1 && prog->P <= 3) ? prog->P : 0;
  void (*k)(SweepDev, FusedDev, GradFusedDev) = nullptr;
#define MLBP_PICK(N) k = fuse_gradient ? sweep_x64_fused_kernel<true, N, true> : (norm ? sweep_x64_fused_kernel<true, N, false> : sweep_x64_fused_kernel<false, N, false>)
  switch (nt) {
    case 1: MLBP_PICK(1); break;
    case 2: MLBP_PICK(2); break;
    case 3: MLBP_PICK(3); break;
    default: MLBP_PICK(0); break;
  }
#undef MLBP_PICK
  if (int e = grant_lds((const void*)k, lds)) return e;
  launch_begin();
  MLBP_LAUNCH(k, dim3(f.only ? fixup_blocks : a->B), dim3(WG), lds, (hipStream_t)stream, G.d, f, gf);
  return launch_verdict("exact X = 64 sweep");
}

int launch_exact_x64_groups(mlbp_program* const* progs, const mlbp_sweep_args* args, int n_groups, const std::vector<char>& member,
                            void* stream, bool* launched) {
  *launched = false;
  std::vector<FixupGroup> table;
  size_t lds_max = 0;
  int blocks = 0, n_grads = 0;
  for (int k = 0; k < n_groups; ++k) {
    if (!member[k]) continue;
    const mlbp_program* prog = progs[k];
    const mlbp_sweep_args* a = &args[k];
    if (!exact_x64_applies(prog, a) || !a->normalize_messages || !a->init_messages) return MLBP_OK;
    table.emplace_back();
    FixupGroup& G = table.back();
    lds_max = std::max(lds_max, fill_fixup_group(prog, a, &G));
    // (a group without pairwise factors -- one predicted word -- never ran the shared-table kernels: launch_shared_groups flagged
    // all of its graphs, so this pass and the flagged graphs' gradient behind it ARE its sweep call)
    if (a->gradient && prog->P > 0 && !shared_gradient_fused(prog, a)) return MLBP_OK;
    G.f.only = prog->d_bail;
    G.first_block = blocks;
    G.per_wg = prog->P == 0 ? 1 : FIXUP_GRAPHS_PER_WG;          // (a pairwise-free group is all flagged: one workgroup per graph, not 64 graphs in a row)
    blocks += (a->B + G.per_wg - 1) / G.per_wg;
    n_grads += a->gradient ? 1 : 0;
  }
  const int n_in = (int)table.size();
  if (n_grads != 0 && n_grads != n_in) return MLBP_OK;                        // (all members or none carry a gradient)
  // the table as 32-bit words in the first program's group-table cache (one device copy per distinct contents)
  static_assert(sizeof(FixupGroup) % 4 == 0, "");
  std::vector<int32_t> words(sizeof(FixupGroup) / 4 * (size_t)n_in + 1);
  memcpy(words.data(), table.data(), sizeof(FixupGroup) * (size_t)n_in);
  words.back() = 0x46495855;                                                  // (keeps this table apart from the sweep kernels' own)
  int32_t* d_table = nullptr;
  if (int e = group_table_device(progs[0]->stables, words, stream, &d_table)) return e;
  if (int e = grant_lds((const void*)sweep_x64_fixup_groups_kernel, lds_max)) return e;
  launch_begin();
  MLBP_LAUNCH(sweep_x64_fixup_groups_kernel, dim3(blocks), dim3(WG), lds_max, (hipStream_t)stream,
                     reinterpret_cast<const FixupGroup*>(d_table), n_in);
  if (int e = launch_verdict("grouped exact X = 64 fix-up")) return e;
  *launched = true;
  return MLBP_OK;
}

int launch_wide_sweep(mlbp_program* prog, const mlbp_sweep_args* a, void* stream, bool* launched) {
  *launched = false;
  const bool norm = a->normalize_messages != 0, f32_tables = (a->flags & MLBP_SWEEP_PAIR_TABLES_F32) != 0;
  const bool wide_exact = a->X == 128 || a->X == 256 || a->X == 512;
  const bool wide_padded = !wide_exact && !f32_tables && norm && a->X > 64 && a->X <= 1024;
  if (!wide_exact && !wide_padded) return MLBP_OK;
  SweepDev d;
  fill_sweep_dev(prog, a, &d);
  d.approx_k = (a->flags & MLBP_SWEEP_APPROX_INFERENCE) ? MLBP_APPROX_K : 0;
  void (*kw)(SweepDev) = nullptr;
  int xp = a->X;
  if (f32_tables) {
    d.pair_tables = reinterpret_cast<const double*>(a->pair_tables_f32);
    if (a->X == 256) kw = norm ? sweep_wide_kernel<true, 1, float, 4, 0> : sweep_wide_kernel<false, 1, float, 4, 0>;
    else kw = norm ? sweep_wide_kernel<true, 2, float, 4, 0> : sweep_wide_kernel<false, 2, float, 4, 0>;
  } else if (a->X == 128) kw = norm ? sweep_wide_kernel<true, 1, double, 2, 0> : sweep_wide_kernel<false, 1, double, 2, 0>;
  else if (a->X == 256) kw = norm ? sweep_wide_kernel<true, 2, double, 2, 0> : sweep_wide_kernel<false, 2, double, 2, 0>;
  else if (a->X == 512) kw = norm ? sweep_wide_kernel<true, 4, double, 2, 0> : sweep_wide_kernel<false, 4, double, 2, 0>;
  else {
    const int q = (a->X + 127) / 128;              // 128-column pieces per row
    const bool odd = (a->X & 1) != 0;
#define MLBP_WIDE_PAD(QQ) (kw = odd ? sweep_wide_kernel<true, QQ, double, 2, 2> : sweep_wide_kernel<true, QQ, double, 2, 1>, xp = 128 * QQ)
    if (q <= 1) MLBP_WIDE_PAD(1);
    else if (q <= 2) MLBP_WIDE_PAD(2);
    else if (q <= 3) MLBP_WIDE_PAD(3);
    else if (q <= 4) MLBP_WIDE_PAD(4);
    else if (q <= 6) MLBP_WIDE_PAD(6);
    else MLBP_WIDE_PAD(8);
#undef MLBP_WIDE_PAD
  }
  const size_t ldsw = ((size_t)6 * xp + 4) * sizeof(double);
  launch_begin();
  MLBP_LAUNCH(kw, dim3(a->B), dim3(WG), ldsw, (hipStream_t)stream, d);
  if (int e = launch_verdict("wide sweep")) return e;
  *launched = true;
  return MLBP_OK;
}

int launch_generic_sweep(mlbp_program* prog, const mlbp_sweep_args* a, bool flagged_only, void* stream) {
  const bool norm = a->normalize_messages != 0;
  SweepDev d;
  fill_sweep_dev(prog, a, &d);
  if (flagged_only) {                                // the graphs the padded lean pass flagged; it initialised none of them
    d.only = prog->d_bail;
    d.fill_uniform = a->init_messages;
  }
  // the messages live in LDS when they fit
  const size_t base = ((size_t)a->X + 4) * sizeof(double);
  const size_t with_msgs = base + (size_t)prog->n_msgs * a->X * sizeof(double);
  launch_begin();
  if (with_msgs <= 64 * 1024) {
    auto k = norm ? sweep_generic_kernel<true, true> : sweep_generic_kernel<false, true>;
    MLBP_LAUNCH(k, dim3(a->B), dim3(WG), with_msgs, (hipStream_t)stream, d);
  } else {
    auto k = norm ? sweep_generic_kernel<true, false> : sweep_generic_kernel<false, false>;
    MLBP_LAUNCH(k, dim3(a->B), dim3(WG), base, (hipStream_t)stream, d);
  }
  return launch_verdict("generic sweep");
}

}  // namespace mlbp

extern "C" {

int mlbp_init_messages_f64(double* msgs, int64_t n_rows, int32_t X, void* stream) {
  if (!msgs || n_rows <= 0 || X <= 0) return fail(MLBP_EINVAL, "mlbp_init_messages_f64: bad arguments");
  if (int e = mlbp::check_device()) return e;
  int64_t n = n_rows * X;
  int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  mlbp::launch_begin();
  MLBP_LAUNCH(fill_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, msgs, n, 1.0 / (double)X);
  return mlbp::launch_verdict("message initialisation");
}

int mlbp_marginals_f64(const double* msgs, int32_t B, int32_t n_msgs, int32_t X, int32_t n_vars,
                       const int32_t* in_off, const int32_t* in_slots, int32_t normalize_messages,
                       double* out, void* stream) {
  if (!msgs || !in_off || !in_slots || !out || B <= 0 || n_msgs <= 0 || X <= 0 || n_vars <= 0)
    return fail(MLBP_EINVAL, "mlbp_marginals_f64: bad arguments");
  if (int e = mlbp::check_device()) return e;
  mlbp::launch_begin();
  MLBP_LAUNCH(marginals_kernel, dim3(B), dim3(WG), 0, (hipStream_t)stream, msgs, n_msgs, X, n_vars,
                     in_off, in_slots, normalize_messages, out);
  return mlbp::launch_verdict("marginals");
}

int mlbp_log_posterior_sum_f64(const double* marginals, const int32_t* labels, int32_t B, int32_t n_vars,
                               int32_t X, double* out, double* sum_out, void* stream) {
  if (!marginals || !labels || !out || B <= 0 || n_vars <= 0 || X <= 0)
    return fail(MLBP_EINVAL, "mlbp_log_posterior_f64: bad arguments");
  if (int e = mlbp::check_device()) return e;
  int32_t* status = nullptr;
  if (int e = mlbp::status_word(&status)) return e;
  const int blocks = (B + LP_WG - 1) / LP_WG;
  if (sum_out && blocks > LP_MAX_BLOCKS)
    return fail(MLBP_EUNSUPPORTED, "mlbp_log_posterior_sum_f64: at most %d graphs with sum_out", LP_MAX_BLOCKS * LP_WG);
  // the block partials live in one device-wide scratch array: launches on DIFFERENT streams must not overlap.  Every
  // launch has its own generation number (the arrival word restarts with it: see the kernel)
  const unsigned gen = sum_out ? next_lp_generation() : 0u;
  mlbp::launch_begin();
  MLBP_LAUNCH(log_posterior_kernel, dim3(blocks), dim3(LP_WG), 0, (hipStream_t)stream, marginals, labels, B, n_vars, X, out,
                     sum_out, status, gen);
  return mlbp::launch_verdict("log-posterior");
}

int mlbp_log_posterior_groups_f64(const mlbp_posterior_group* groups, int32_t n_groups, int64_t n_total, int32_t X, double* out,
                                  void* stream) {
  if (!groups || !out || n_groups <= 0 || n_total <= 0 || X <= 0) return fail(MLBP_EINVAL, "mlbp_log_posterior_groups_f64: bad arguments");
  if (int e = mlbp::check_device()) return e;
  int32_t* status = nullptr;
  if (int e = mlbp::status_word(&status)) return e;
  mlbp::launch_begin();
  MLBP_LAUNCH(log_posterior_groups_kernel, dim3((unsigned)((n_total + LP_WG - 1) / LP_WG)), dim3(LP_WG), 0, (hipStream_t)stream, groups,
                     n_groups, (long long)n_total, X, out, status);
  return mlbp::launch_verdict("grouped log-posterior");
}

int mlbp_log_posterior_f64(const double* marginals, const int32_t* labels, int32_t B, int32_t n_vars,
                           int32_t X, double* out, void* stream) {
  return mlbp_log_posterior_sum_f64(marginals, labels, B, n_vars, X, out, nullptr, stream);
}

}  // extern "C"
