// libmlbp_exactmbest.so: the M best whole assignments, ranked, by cutset conditioning (include/mlbp_exactmbest.h), gfx950
// only, float64.  The max form of the walk of csrc/mlbp_cutset_walk.h without exact_map's merge; this file holds what the
// library does around it -- every V_c kept apart, the choice of the M best configurations, the list form of the pass up over
// those, and the merge of their candidates.
//
// Six kernels, four launches per call; the forms of the first and the third are chosen from (X, n_vars, P, U, n_forest, M) by
// mlbp_exactmbest_pick_kernel:
//   exactmbest_values_x64_kernel      X = 64: the forest's tables in LDS (x64_open); every WAVE walks configurations of its own
//                                     (x64_up<MaxAlg, false>) and writes V_c as a (mantissa, exponent) pair.
//   exactmbest_values_generic_kernel  any X in [2, 1024]: the workgroup walks one configuration at a time (generic_up<MaxAlg>).
//   exactmbest_select_kernel          one workgroup per graph: the at most M positive V_c, largest first, ties to the lower c.
//   exactmbest_lists_x64_kernel       X = 64: the tables in LDS once per graph; every WAVE solves selected configurations of its
//                                     own in the list form, lane = state, lists in registers, no workgroup barrier.
//   exactmbest_lists_generic_kernel   one workgroup per (graph, selected configuration): the list form of the pass up, a thread
//                                     per state, tables streamed; the candidates decoded by back-pointers, a thread each.
//   exactmbest_merge_kernel           one workgroup per graph, a thread per candidate: its rank by counting, the rows, the
//                                     logarithms.
// A LISTED call (N > 0, the header's listed mode) runs the same six kernels over the caller's list of cutset states: a
// configuration's number is then the index of a list entry and the states come from the entry's row of configs -- the values
// kernels in loops of their own (ListedStates, X64Packed), the select over the entries with the duplicate rule, the lists
// kernels reading the selected entry's row where they decode c, the merge breaking ties by entry index.
// No sum is formed and nothing is merged before the merge, so the bits of a result are a function of the graph, the cutset and
// M's prefix alone.  Every scalar a workgroup branches on comes out of a reduction or workgroup-uniform memory and has the same
// bits in every thread of it.  No device-side mutable globals: everything comes through MbestDev.
#include <hip/hip_runtime.h>

#include "../../include/mlbp_exactmbest.h"
#define MLBP_GRAPH_NO_SWEEPS                // this library runs no sweep program
#include "../csrc/mlbp_graph_device.h"
#include "../csrc/mlbp_graph_host.h"
#include "../csrc/mlbp_cutset_plan.h"
#include "../csrc/mlbp_cutset_walk.h"

namespace {

using namespace mlbp_graph;

constexpr int MAXM = MLBP_EXACTMBEST_MAX_M;
static_assert(MAXM == 16, "a back-pointer packs a rank into four bits");
static_assert(MLBP_CUTSET_MAX_X <= 4 * WG, "the root list keeps four cursors per thread");
static_assert(MAXM * MAXM <= WG, "the merge gives every candidate a thread");

struct MbestDev : WalkDev {
  double* vc;                                // [B][n_configs][2] V_c as (mantissa, exponent)
  double* sel;                               // [B][M + 1] the selected configurations, best first, then their number
  double* cval;                              // [B][M][M][2] the candidates' values as (mantissa, exponent); mantissa 0: none
  int32_t* cxs;                              // [B][M][M][n_vars] the candidates' assignments
  char* lists;                               // the lists kernel's lists when they are not in LDS: [B][M][lists_bytes]
  int64_t lists_bytes;
  int32_t x64_bytes, wave_bytes;             // the X = 64 lists kernel: x64_open's LDS, and a wave's own behind it
  int32_t* assignments; double* scores; int32_t* n_found;
  int32_t M;
  const int32_t* configs;                    // a listed call with cutset variables: [B][n_configs][n_cut]; else NULL
  int32_t* entries;                          // optional [B][M]
};

// A listed call: n_configs is N, a configuration's number the index of a list entry, and the entry's states are its row of
// configs where the exact call decodes c.  Without cutset variables configs is NULL and the list is the one empty configuration:
// the host hands over n_configs = 1 and every kernel runs as in the exact call.  A values walker that meets a row with a state
// outside [0, X) writes BAD_ENTRY in the place of the pair's exponent, before any state forms an address; the select then
// refuses the graph (REFUSED in the place of the number of selected entries) and no lists task reads a row of it.
constexpr double BAD_ENTRY = 1e300;          // no exponent reads so
constexpr int REFUSED = -1;

__device__ __forceinline__ const_i32p listed_row(const MbestDev& d, int g, int i) {
  return as_const(d.configs) + ((size_t)g * d.n_configs + i) * d.n_cut;
}

// the row's address is the same in every thread of the walker, and so is the answer
__device__ __forceinline__ bool row_in_range(const_i32p row, int n_cut, int X) {
  bool ok = true;
  for (int q = 0; q < n_cut; ++q) ok &= (unsigned)row[q] < (unsigned)X;
  return ok;
}

// Where the X = 64 lists kernel takes the state of cut position q: lane q of `packed` (the selected entry's row, a listed call)
// or the digits of c.  A scalar either way.
struct X64Selected {
  int packed, c;
  bool listed;
  __device__ __forceinline__ int operator()(int q) const { return listed ? __builtin_amdgcn_readlane(packed, q) : x64_state(q, c); }
};

// Does the pair a exceed the pair b?  A pair without a positive mantissa exceeds nothing.
__device__ __forceinline__ bool exceeds(double am, int ae, double bm, int be) {
  return am > 0.0 && (!(bm > 0.0) || ae > be || (ae == be && am > bm));
}

// An ordered list of MAXM values with tags, in registers: every index is a constant.
struct Top {
  double v[MAXM];
  int tag[MAXM];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < MAXM; ++k) { v[k] = 0.0; tag[k] = 0; }
  }
  // y enters behind every entry it does not exceed
  __device__ __forceinline__ void offer(double y, int t) {
#pragma unroll
    for (int k = 0; k < MAXM; ++k) {
      const bool in = y > v[k];
      const double ov = v[k];
      const int ot = tag[k];
      v[k] = in ? y : ov;
      tag[k] = in ? t : ot;
      y = in ? ov : y;
      t = in ? ot : t;
    }
  }
};

// The same over (mantissa, exponent) pairs.
struct TopPairs {
  double m[MAXM];
  int e[MAXM], tag[MAXM];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < MAXM; ++k) { m[k] = 0.0; e[k] = EMPTY; tag[k] = 0; }
  }
  __device__ __forceinline__ void offer(Scaled y, int t) {
    double ym = y.m;
    int ye = y.e;
#pragma unroll
    for (int k = 0; k < MAXM; ++k) {
      const bool in = exceeds(ym, ye, m[k], e[k]);
      const double om = m[k];
      const int oe = e[k], ot = tag[k];
      m[k] = in ? ym : om;
      e[k] = in ? ye : oe;
      tag[k] = in ? t : ot;
      ym = in ? om : ym;
      ye = in ? oe : ye;
      t = in ? ot : t;
    }
  }
};

// vec[0 .. X)[0 .. M) times 2^-e, e the exponent of its largest entry (a rank 0); an entry of rank >= 1 below
// 2^-MLBP_EXACTMBEST_DROP_BELOW becomes 0.  Returns e.  The entries are visible on entry; ends with a barrier.
__device__ __forceinline__ int rescale_lists(double* vec, int X, int M, double* scratch) {
  const int t = threadIdx.x;
  double m = 0.0;
  for (int j = t; j < X; j += WG) m = fmax(m, vec[(size_t)j * M]);
  const int e = exp_of(block_max(m, scratch));
  for (int i = t; i < X * M; i += WG) {
    const double x = vec[i];
    const double y = e != 0 ? ldexp(x, -e) : x;
    vec[i] = (i % M != 0 && y < 0x1p-1000) ? 0.0 : y;
  }
  __syncthreads();
  return e;
}
static_assert(MLBP_EXACTMBEST_DROP_BELOW == 1000, "rescale_lists() states the limit as a literal");

// ---- the values pass: every V_c of a chunk's configurations ---------------------------------------------------
__global__ __launch_bounds__(WG) void exactmbest_values_generic_kernel(MbestDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  Generic G;
  generic_open(G, d, g);
  generic_carve(G, d, g, k, smem);
  generic_setup(G);
  double* out = d.vc + (size_t)g * d.n_configs * 2;
  if (d.configs) {                                             // a listed call: its own loop, the exact one below is as it was
    for (int i = k; i < d.n_configs; i += d.chunks) {
      const const_i32p row = listed_row(d, g, i);
      if (!row_in_range(row, d.n_cut, d.X)) {
        if (t == 0) {
          out[2 * i] = 0.0;
          out[2 * i + 1] = BAD_ENTRY;
        }
        continue;
      }
      const Scaled z = generic_up<MaxAlg>(G, ListedStates{row}, nullptr);
      if (t == 0) {
        out[2 * i] = z.m;
        out[2 * i + 1] = (double)z.e;
      }
    }
    return;
  }
  for (int c = k; c < d.n_configs; c += d.chunks) {
    const Scaled z = generic_up<MaxAlg>(G, c, nullptr);
    if (t == 0) {
      out[2 * c] = z.m;
      out[2 * c + 1] = (double)z.e;
    }
  }
}

__global__ __launch_bounds__(WG) void exactmbest_values_x64_kernel(MbestDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int g = blockIdx.x, k = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  X64 W;
  x64_open(W, d, g, smem);
  double* out = d.vc + (size_t)g * d.n_configs * 2;
  if (d.configs) {                                             // a listed call: its own loop, the exact one below is as it was
    for (int i = 4 * k + wave; i < d.n_configs; i += 4 * d.chunks) {
      const int packed = lane < d.n_cut ? listed_row(d, g, i)[lane] : 0;
      const bool bad = __any((unsigned)packed >= 64u);
      Scaled z = {0.0, 0};
      if (!bad) z = x64_up<MaxAlg, false>(W, X64Packed{packed});
      if (lane == 0) {
        out[2 * i] = bad ? 0.0 : z.m;
        out[2 * i + 1] = bad ? BAD_ENTRY : (double)z.e;
      }
    }
    return;
  }
  for (int c = 4 * k + wave; c < d.n_configs; c += 4 * d.chunks) {
    const Scaled z = x64_up<MaxAlg, false>(W, c);
    if (lane == 0) {
      out[2 * c] = z.m;
      out[2 * c + 1] = (double)z.e;
    }
  }
}

// ---- the select: a graph's V_c -> its at most M best configurations ------------------------------------------------
// Round r takes the best configuration behind the one round r - 1 took: the largest exponent, among those the largest
// mantissa, among those the lowest index.
__global__ __launch_bounds__(WG) void exactmbest_select_kernel(MbestDev d) {
  __shared__ double scratch[8];
  const int g = blockIdx.x, t = threadIdx.x, n = d.n_configs, M = d.M;
  double* sel = d.sel + (size_t)g * (M + 1);
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) {
    if (t == 0) sel[M] = 0.0;
    return;
  }
  const double* vc = d.vc + (size_t)g * n * 2;
  constexpr double NONE = -1e300;
  double pm = 0.0, pe = 0.0;                                   // the configuration taken last
  int pc = -1, found = 0;
  if (d.configs) {                                             // a listed call: its own rounds, the exact ones below are as they were
    // An entry whose row equals the row of an entry of lower index is ignored.  Equal rows have equal V bits and the lower
    // index is taken first, so a duplicate is an open entry whose pair equals the pair taken last and whose row equals the row
    // of one of the entries taken with that pair: taken[same .. r).  Rows are compared nowhere else.
    __shared__ int taken[MAXM];
    int bad = 0;
    for (int c = t; c < n; c += WG) bad |= vc[2 * c + 1] == BAD_ENTRY;
    if (block_max(bad ? 1.0 : 0.0, scratch) > 0.0) {           // a state outside [0, X): the graph is not computed
      if (t == 0) sel[M] = (double)REFUSED;
      return;
    }
    int same = 0;
    for (int r = 0; r < M; ++r) {
      auto open = [&](int c, double m, double e) {
        if (!(m > 0.0)) return false;
        if (pc < 0 || e < pe || (e == pe && m < pm)) return true;
        if (!(e == pe && m == pm && c > pc)) return false;
        const const_i32p row = listed_row(d, g, c);
        for (int k = same; k < r; ++k) {
          const const_i32p other = listed_row(d, g, taken[k]);
          bool equal = true;
          for (int q = 0; q < d.n_cut; ++q) equal &= row[q] == other[q];
          if (equal) return false;
        }
        return true;
      };
      double be = NONE;
      for (int c = t; c < n; c += WG)
        if (open(c, vc[2 * c], vc[2 * c + 1])) be = fmax(be, vc[2 * c + 1]);
      be = block_max(be, scratch);
      if (!(be > NONE)) break;
      double bm = 0.0;
      for (int c = t; c < n; c += WG)
        if (vc[2 * c + 1] == be && open(c, vc[2 * c], be)) bm = fmax(bm, vc[2 * c]);
      bm = block_max(bm, scratch);
      unsigned bc = 0xffffffffu;
      for (int c = t; c < n; c += WG)
        if (vc[2 * c + 1] == be && vc[2 * c] == bm && open(c, bm, be)) { bc = (unsigned)c; break; }
      bc = block_min_index(bc, scratch);
      if (bc == 0xffffffffu) break;
      if (t == 0) {
        sel[r] = (double)bc;
        taken[r] = (int)bc;
      }
      if (!(bm == pm && be == pe)) same = r;
      pm = bm; pe = be; pc = (int)bc;
      ++found;
      __syncthreads();                                         // taken[r]: read by every thread's scans of the next round
    }
    if (t == 0) sel[M] = (double)found;
    return;
  }
  for (int r = 0; r < M; ++r) {
    // is c behind the last one taken?
    auto open = [&](int c, double m, double e) {
      return m > 0.0 && (pc < 0 || e < pe || (e == pe && (m < pm || (m == pm && c > pc))));
    };
    double be = NONE;
    for (int c = t; c < n; c += WG)
      if (open(c, vc[2 * c], vc[2 * c + 1])) be = fmax(be, vc[2 * c + 1]);
    be = block_max(be, scratch);
    if (!(be > NONE)) break;
    double bm = 0.0;
    for (int c = t; c < n; c += WG)
      if (vc[2 * c + 1] == be && open(c, vc[2 * c], be)) bm = fmax(bm, vc[2 * c]);
    bm = block_max(bm, scratch);
    unsigned bc = 0xffffffffu;
    for (int c = t; c < n; c += WG)
      if (vc[2 * c + 1] == be && vc[2 * c] == bm && open(c, bm, be)) { bc = (unsigned)c; break; }
    bc = block_min_index(bc, scratch);
    if (bc == 0xffffffffu) break;
    if (t == 0) sel[r] = (double)bc;
    pm = bm; pe = be; pc = (int)bc;
    ++found;
  }
  if (t == 0) sel[M] = (double)found;
}

// ---- the lists pass: one selected configuration in the list form ---------------------------------------------------
// The kernel's memory.  LDS: [scratch 8] [F mantissas MAXM] [R MAXM] [F exponents MAXM] [table exponents, states]; then, in LDS
// or in the workspace, the task's lists: base [n_vars][Xp], L [n_vars][X][M], C [X][M], the decode's ranks [M][n_vars], and the
// back-pointers bpC, bpF [n_vars][X][M], bpRoot, bpR [n_vars][M].
__global__ __launch_bounds__(WG) void exactmbest_lists_generic_kernel(MbestDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int X = d.X, M = d.M, g = blockIdx.x, r = blockIdx.y, t = threadIdx.x, n_vars = d.n_vars;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  double* cval = d.cval + ((size_t)g * M + r) * M * 2;
  int32_t* cxs = d.cxs + ((size_t)g * M + r) * M * n_vars;
  if (r >= (int)d.sel[(size_t)g * (M + 1) + M]) {                // no such configuration: no candidate
    if (t < M) cval[2 * t] = 0.0;
    return;
  }
  const int c = (int)d.sel[(size_t)g * (M + 1) + r];

  Generic G;
  generic_open(G, d, g);
  double* lds = reinterpret_cast<double*>(smem);
  G.scratch = lds;
  double* Fm = lds + 8;
  double* R = Fm + MAXM;
  int* Fe = reinterpret_cast<int*>(R + MAXM);
  G.texp = Fe + MAXM;
  G.st = G.texp + d.P + d.U;
  char* big = d.lists ? d.lists + ((size_t)g * M + r) * d.lists_bytes
                      : smem + MLBP_EXACTMBEST_LISTS_FIXED + 4 * ((d.P + d.U + 16 + 3) / 4 * 4);
  const int Xp = G.Xp;
  const size_t vl = (size_t)X * M;                             // the entries of one variable's lists
  G.base = reinterpret_cast<double*>(big);
  double* L = G.base + (size_t)n_vars * Xp;
  double* Cl = L + (size_t)n_vars * vl;
  int* rk = reinterpret_cast<int*>(Cl + vl);
  uint16_t* bpC = reinterpret_cast<uint16_t*>(rk + (size_t)M * n_vars);
  uint16_t* bpF = bpC + (size_t)n_vars * vl;
  uint16_t* bpRoot = bpF + (size_t)n_vars * vl;
  uint16_t* bpR = bpRoot + (size_t)n_vars * M;

  generic_setup(G);
  if (t < G.n_cut) {
    int q = c;
    for (int i = 0; i < t; ++i) q /= X;
    G.st[t] = d.configs ? listed_row(d, g, c)[t] : q % X;      // a listed call: the selected entry's row, validated by the values pass
  }
  __syncthreads();
  Scaled z = {1.0, G.e_fixed};                                 // the configuration's constants, as generic_up takes them
  for (int i = 0; i < G.n_consts; ++i) {
    const int f = G.pl.consts[4 * i + 1], s0 = G.st[G.pl.consts[4 * i + 2]];
    if (G.pl.consts[4 * i] == MLBP_CUTSET_CONST_UNARY) {
      mul(z, ldexp(G.unary_tables[(size_t)G.utab[f] * X + s0], -G.texp[G.P + f]));
    } else {
      const int s1 = G.st[G.pl.consts[4 * i + 3]];
      mul(z, ldexp(G.pair_tables[(size_t)G.ptab[f] * G.XX + (size_t)s0 * X + s1], -G.texp[f]));
    }
  }
  for (int i = 0; i < G.n_free; ++i) {
    const int v = G.pl.order[i];
    for (int j = t; j < X; j += WG) {
      double* l = L + (size_t)v * vl + (size_t)j * M;
      l[0] = generic_local(G, v, j);
      for (int k = 1; k < M; ++k) l[k] = 0.0;
    }
  }
  if (t < MAXM) {
    Fm[t] = t == 0 ? z.m : 0.0;
    Fe[t] = t == 0 ? z.e : EMPTY;
  }
  __syncthreads();

  int tally = 0;                                               // the exponents the rescalings took out
  for (int i = 0; i < G.n_free; ++i) {
    const int v = G.pl.order[i], p = G.pl.parent[2 * v];
    double* Lv = L + (size_t)v * vl;
    tally += rescale_lists(Lv, X, M, G.scratch);
    if (p < 0) {
      // R: round k takes the largest entry no round took, the lowest state among equals; a state's entries go in rank order
      if (t < MAXM) R[t] = 0.0;
      __syncthreads();
      int cur[4] = {0, 0, 0, 0};
      for (int k = 0; k < M; ++k) {
        double best = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = t + q * WG;
          if (j < X && cur[q] < M) best = fmax(best, Lv[(size_t)j * M + cur[q]]);
        }
        const double mx = block_max(best, G.scratch);
        unsigned idx = 0xffffffffu;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = t + q * WG;
          if (idx == 0xffffffffu && j < X && cur[q] < M && Lv[(size_t)j * M + cur[q]] == mx) idx = (unsigned)j;
        }
        idx = block_min_index(idx, G.scratch);
        if (!(mx > 0.0) || idx == 0xffffffffu) break;
        if ((int)(idx % WG) == t) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q == (int)(idx / WG)) {
              R[k] = mx;
              bpRoot[(size_t)v * M + k] = (uint16_t)(idx * MAXM + cur[q]);
              ++cur[q];
            }
        }
      }
      __syncthreads();
      if (t == 0) {
        TopPairs out;
        out.clear();
        for (int a = 0; a < M; ++a)
          for (int b = 0; (a + 1) * (b + 1) <= M; ++b) {
            Scaled y = {Fm[a], Fe[a]};
            if (!(y.m > 0.0) || !(R[b] > 0.0)) continue;
            mul(y, R[b]);
            out.offer(y, a * MAXM + b);
          }
#pragma unroll
        for (int k = 0; k < MAXM; ++k) {
          Fm[k] = out.m[k];
          Fe[k] = out.e[k];
          if (k < M) bpR[(size_t)v * M + k] = (uint16_t)out.tag[k];
        }
      }
      __syncthreads();
    } else {
      const int par = G.pl.parent[2 * v + 1], te = G.texp[p];
      const bool tm = G.pl.pav[2 * p] != v;                      // the parent is on axis 0
      const double* T = G.pair_tables + (size_t)G.ptab[p] * G.XX;
      for (int s = t; s < X; s += WG) {
        Top out;
        out.clear();
        for (int j = 0; j < X; ++j) {
          const double tj = ldexp(tm ? T[(size_t)s * X + j] : T[(size_t)j * X + s], -te);
          const double* l = Lv + (size_t)j * M;
          for (int k = 0; k < M; ++k) {
            const double y = tj * l[k];
            if (!(y > out.v[MAXM - 1])) break;                 // the ranks behind it are no larger
            out.offer(y, j * MAXM + k);
          }
        }
#pragma unroll
        for (int k = 0; k < MAXM; ++k)
          if (k < M) {
            Cl[(size_t)s * M + k] = out.v[k];
            bpC[(size_t)v * vl + (size_t)s * M + k] = (uint16_t)out.tag[k];
          }
      }
      __syncthreads();
      tally += rescale_lists(Cl, X, M, G.scratch);
      double* Lp = L + (size_t)par * vl;
      for (int s = t; s < X; s += WG) {
        Top out;
        out.clear();
        for (int a = 0; a < M; ++a) {
          const double la = Lp[(size_t)s * M + a];
          for (int b = 0; (a + 1) * (b + 1) <= M; ++b) out.offer(la * Cl[(size_t)s * M + b], a * MAXM + b);
        }
#pragma unroll
        for (int k = 0; k < MAXM; ++k)
          if (k < M) {
            Lp[(size_t)s * M + k] = out.v[k];
            bpF[(size_t)v * vl + (size_t)s * M + k] = (uint16_t)out.tag[k];
          }
      }
      __syncthreads();
    }
  }

  // candidate k by thread k: its value, and its states from the back-pointers
  if (t >= M) return;
  int32_t* xs = cxs + (size_t)t * n_vars;
  const bool there = Fm[t] > 0.0;
  cval[2 * t] = there ? Fm[t] : 0.0;
  cval[2 * t + 1] = (double)(Fe[t] + tally);
  if (!there) {
    for (int v = 0; v < n_vars; ++v) xs[v] = -1;
    return;
  }
  for (int q = 0; q < G.n_cut; ++q) xs[G.pl.cutset[q]] = G.st[q];
  int* rank = rk + (size_t)t * n_vars;
  int rf = t;                                                  // the rank in F as it stood behind the root at hand
  for (int i = G.n_free - 1; i >= 0; --i) {
    const int v = G.pl.order[i], p = G.pl.parent[2 * v];
    int jk;
    if (p < 0) {
      const int ab = bpR[(size_t)v * M + rf];
      rf = min(ab / MAXM, M - 1);
      jk = bpRoot[(size_t)v * M + min(ab % MAXM, M - 1)];
    } else {
      const int par = G.pl.parent[2 * v + 1];
      const size_t at = (size_t)v * vl + (size_t)xs[par] * M;
      const int ab = bpF[at + rank[par]];
      rank[par] = min(ab / MAXM, M - 1);
      jk = bpC[at + min(ab % MAXM, M - 1)];
    }
    xs[v] = min(jk / MAXM, X - 1);
    rank[v] = min(jk % MAXM, M - 1);
  }
}

// ---- the lists pass at X = 64: a wave per selected configuration, lane = state ---------------------------------------
// A list of MAXM values in a lane's registers times 2^-e, e the exponent of the wave's largest rank 0; ranks >= 1 below the
// limit are dropped; e is added to the tally.  Rank 0 goes through wave_rescale's operations.
__device__ __forceinline__ void wave_rescale_lists(double (&l)[MAXM], int& tally) {
  const int e = exp_of(wave_max(fmax(l[0], 0.0)));
  tally += e;
#pragma unroll
  for (int k = 0; k < MAXM; ++k) {
    const double y = e != 0 ? ldexp(l[k], -e) : l[k];
    l[k] = (k != 0 && y < 0x1p-1000) ? 0.0 : y;
  }
}

// A variable's list into a lane's registers: its slot's in L, or (slot < 0) its local vector alone.  Returns the ranks that may
// hold an entry.
__device__ __forceinline__ int load_list(double (&l)[MAXM], int slot, const double* Lw, const double* local, int M, int lane) {
#pragma unroll
  for (int k = 0; k < MAXM; ++k) l[k] = 0.0;
  if (slot < 0) {
    l[0] = local[lane];
    return 1;
  }
#pragma unroll
  for (int k = 0; k < MAXM; ++k)
    if (k < M) l[k] = Lw[((size_t)slot * M + k) * 64 + lane];
  return M;
}

// The wave's memory beside x64_open's: L [n_forest][M][64] doubles -- the list of a variable that has had a child folded into it,
// in the slot of the first such child's factor --, then bp [n_forest][M][64] words -- per forest factor, the back-pointers of
// its contraction (low half) and of its fold (high half).  Of x64_open's vectors of the wave: bel holds the local vectors, phi
// the list slots [n_vars], up the decode's ranks [MAXM][n_vars], dn the roots' back-pointers [2][n_vars][MAXM].
// Unlike the shared walk, which only ever touches [v * 64 + lane], this kernel hands values from lane to lane of a wave THROUGH
// LDS without a fence: lslot[par] is written by lane 0 and read by all, bpRoot and bpR are written by lane k and read by the
// decoding lanes at other ranks, bp is read at the parent's state, another lane's column.  That is sound because the LDS
// operations of one wave complete in the order they were issued and every such value is re-read from LDS where it is used;
// keeping one of them in a register across a write (a cached lslot, say) would break it.
__global__ __launch_bounds__(WG) void exactmbest_lists_x64_kernel(MbestDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int g = blockIdx.x, kb = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6, M = d.M, n_vars = d.n_vars;
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g)) return;
  const int n_sel = (int)d.sel[(size_t)g * (M + 1) + M];
  for (int r = 4 * kb + wave; r < M; r += 4 * d.chunks)         // no such configuration: no candidate
    if (r >= n_sel && lane < M) d.cval[(((size_t)g * M + r) * M + lane) * 2] = 0.0;
  if (4 * kb >= n_sel) return;                                 // the same in every wave of the workgroup
  X64 W;
  x64_open(W, d, g, smem);
  double* Lw = reinterpret_cast<double*>(smem + d.x64_bytes + (size_t)wave * d.wave_bytes);
  uint32_t* bpw = reinterpret_cast<uint32_t*>(Lw + (size_t)d.n_forest * M * 64);
  int* lslot = reinterpret_cast<int*>(W.phi);
  int* rank = reinterpret_cast<int*>(W.up) + lane * n_vars;
  int* bpRoot = reinterpret_cast<int*>(W.dn);
  int* bpR = bpRoot + n_vars * MAXM;

  for (int r = 4 * kb + wave; r < n_sel; r += 4 * d.chunks) {
    const int c = (int)d.sel[(size_t)g * (M + 1) + r];
    // a listed call: lane q holds the state of cut position q of the selected entry, validated by the values pass
    const X64Selected state = {d.configs && lane < W.n_cut ? listed_row(d, g, c)[lane] : 0, c, d.configs != nullptr};
    Scaled z = {1.0, W.e_fixed};                               // the configuration's constants, as x64_up takes them
    for (int q = 0; q < W.n_cut; ++q) mul(z, W.base[(size_t)W.pl.cutset[q] * 64 + state(q)]);
    for (int i = 0; i < W.n_consts; ++i) {
      if (W.pl.consts[4 * i] != MLBP_CUTSET_CONST_PAIR) continue;
      const int f = W.pl.consts[4 * i + 1], s0 = state(W.pl.consts[4 * i + 2]), s1 = state(W.pl.consts[4 * i + 3]);
      mul(z, ldexp(W.pair_tables[(size_t)W.ptab[f] * 4096 + s0 * 64 + s1], -W.texp[f]));
    }
    for (int i = 0; i < W.n_free; ++i) {
      const int v = W.pl.order[i];
      W.bel[(size_t)v * 64 + lane] = x64_local(W, v, state);
    }
    if (lane < n_vars) lslot[lane] = -1;
    double Fm = lane == 0 ? z.m : 0.0;                         // F: lane k holds entry k
    int Fe = lane == 0 ? z.e : EMPTY, tally = 0;

    for (int i = 0; i < W.n_free; ++i) {
      const int v = W.pl.order[i], p = W.pl.parent[2 * v];
      double lv[MAXM];
      const int nk = load_list(lv, lslot[v], Lw, W.bel + (size_t)v * 64, M, lane);
      wave_rescale_lists(lv, tally);
      if (p < 0) {
        // R: lane k holds entry k.  Round k takes the largest front entry, the lowest state among equals; that lane's list moves up
        double Rv = 0.0;
        int Rtag = 0, popped = 0;
        for (int k = 0; k < M; ++k) {
          const double mx = wave_max(fmax(lv[0], 0.0));
          if (!(mx > 0.0)) break;
          const int j = __ffsll(__ballot(lv[0] == mx)) - 1;
          const int pj = __builtin_amdgcn_readlane(popped, j);
          if (lane == k) { Rv = mx; Rtag = j * MAXM + pj; }
          if (lane == j) {
#pragma unroll
            for (int q = 0; q + 1 < MAXM; ++q) lv[q] = lv[q + 1];
            lv[MAXM - 1] = 0.0;
            ++popped;
          }
        }
        TopPairs out;                                          // wave-uniform: every lane holds the same list
        out.clear();
        for (int a = 0; a < M; ++a)
          for (int b = 0; (a + 1) * (b + 1) <= M; ++b) {
            Scaled y = {read_lane(Fm, a), __builtin_amdgcn_readlane(Fe, a)};
            const double rb = read_lane(Rv, b);
            if (y.m > 0.0 && rb > 0.0) {
              mul(y, rb);
              out.offer(y, a * MAXM + b);
            }
          }
#pragma unroll
        for (int k = 0; k < MAXM; ++k)
          if (lane == k) {
            Fm = out.m[k];
            Fe = out.e[k];
            bpR[v * MAXM + k] = out.tag[k];
            bpRoot[v * MAXM + k] = Rtag;
          }
      } else {
        const int par = W.pl.parent[2 * v + 1], slot = W.pl.fslot[p];
        const double* tab = W.tabs + (size_t)slot * 64 * ROW;
        const bool tm = W.pl.pav[2 * p] != v;                    // the parent is on axis 0
        Top out;
        out.clear();
        for (int j = 0; j < 64; ++j) {
          const double tj = tm ? tab[lane * ROW + j] : tab[j * ROW + lane];
#pragma unroll
          for (int k = 0; k < MAXM; ++k)
            if (k < nk) {
              const double y = tj * read_lane(lv[k], j);
              if (y > out.v[MAXM - 1]) out.offer(y, j * MAXM + k);
            }
        }
        wave_rescale_lists(out.v, tally);
        double pv[MAXM];
        const int nkp = load_list(pv, lslot[par], Lw, W.bel + (size_t)par * 64, M, lane);
        Top nl;
        nl.clear();
#pragma unroll
        for (int a = 0; a < MAXM; ++a)
#pragma unroll
          for (int b = 0; b < MAXM; ++b)                       // a >= nkp: the parent's list holds no such entry
            if ((a + 1) * (b + 1) <= MAXM && (a + 1) * (b + 1) <= M && a < nkp) nl.offer(pv[a] * out.v[b], a * MAXM + b);
        int pslot = lslot[par];
        if (pslot < 0) {
          pslot = slot;
          if (lane == 0) lslot[par] = slot;
        }
#pragma unroll
        for (int k = 0; k < MAXM; ++k)
          if (k < M) {
            Lw[((size_t)pslot * M + k) * 64 + lane] = nl.v[k];
            bpw[((size_t)slot * M + k) * 64 + lane] = (uint32_t)out.tag[k] | (uint32_t)nl.tag[k] << 16;
          }
      }
    }

    // candidate k by lane k: its value, and its states from the back-pointers
    if (lane >= M) continue;
    double* cval = d.cval + (((size_t)g * M + r) * M + lane) * 2;
    int32_t* xs = d.cxs + (((size_t)g * M + r) * M + lane) * n_vars;
    const bool there = Fm > 0.0;
    cval[0] = there ? Fm : 0.0;
    cval[1] = (double)(Fe + tally);
    if (!there) {
      for (int v = 0; v < n_vars; ++v) xs[v] = -1;
      continue;
    }
    for (int q = 0; q < W.n_cut; ++q) xs[W.pl.cutset[q]] = state(q);
    int rf = lane;                                             // the rank in F as it stood behind the root at hand
    for (int i = W.n_free - 1; i >= 0; --i) {
      const int v = W.pl.order[i], p = W.pl.parent[2 * v];
      int jk;
      if (p < 0) {
        const int ab = bpR[v * MAXM + rf];
        rf = min(ab / MAXM, M - 1);
        jk = bpRoot[v * MAXM + min(ab % MAXM, M - 1)];
      } else {
        const int par = W.pl.parent[2 * v + 1], slot = W.pl.fslot[p], s = xs[par];
        const int ab = (int)(bpw[((size_t)slot * M + rank[par]) * 64 + s] >> 16);
        rank[par] = min(ab / MAXM, M - 1);
        jk = (int)(bpw[((size_t)slot * M + min(ab % MAXM, M - 1)) * 64 + s] & 0xffffu);
      }
      xs[v] = min(jk / MAXM, 63);
      rank[v] = min(jk % MAXM, M - 1);
    }
  }
}

// ---- the merge: a graph's candidates -> its rows ----------------------------------------------------------------
__global__ __launch_bounds__(WG) void exactmbest_merge_kernel(MbestDev d) {
  __shared__ double cm[MAXM * MAXM];
  __shared__ int ce[MAXM * MAXM], cc[MAXM * MAXM];
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int X = d.X, M = d.M, n_vars = d.n_vars;
  int32_t* rows = d.assignments + (size_t)g * M * n_vars;
  double* scores = d.scores + (size_t)g * M;
  int32_t* entries = d.entries ? d.entries + (size_t)g * M : nullptr;
  // a table index outside its array, or (a listed call) a state outside [0, X): the graph is not computed
  if (!tables_in_range(d.pair_tab, d.P, d.n_pair_tables, d.unary_tab, d.U, d.n_unary_tables, g) ||
      (int)d.sel[(size_t)g * (M + 1) + M] == REFUSED) {
    for (int i = t; i < M * n_vars; i += WG) rows[i] = -1;
    if (t < M) scores[t] = __builtin_nan("");
    if (t < M && entries) entries[t] = -1;
    if (t == 0) d.n_found[g] = -1;
    return;
  }
  const int n_sel = (int)d.sel[(size_t)g * (M + 1) + M], n = M * M;
  const double* cval = d.cval + (size_t)g * n * 2;
  // candidate t = (r, k): configuration sel[r], rank k inside it
  const bool mine = t < n && t / M < n_sel && cval[2 * t] > 0.0;
  const double m = mine ? cval[2 * t] : 0.0;
  const int e = mine ? (int)cval[2 * t + 1] : EMPTY;
  const int c = mine ? (int)d.sel[(size_t)g * (M + 1) + t / M] : 0;
  if (t < n) { cm[t] = m; ce[t] = e; cc[t] = c; }
  __syncthreads();
  int ahead = 0, positive = 0;                                 // candidates in front of this one; candidates there are
  for (int o = 0; o < n; ++o) {
    positive += cm[o] > 0.0;
    if (!mine || o == t) continue;
    if (exceeds(cm[o], ce[o], m, e)) ++ahead;
    else if (cm[o] == m && ce[o] == e && (cc[o] < c || (cc[o] == c && o < t))) ++ahead;
  }
  const int found = min(positive, M);
  if (mine && ahead < M) {
    const int32_t* xs = d.cxs + ((size_t)g * n + t) * n_vars;
    for (int v = 0; v < n_vars; ++v) rows[(size_t)ahead * n_vars + v] = xs[v];
    if (entries) entries[ahead] = c;
  }
  if (entries && t >= found && t < M) entries[t] = -1;
  for (int i = t; i < (M - found) * n_vars; i += WG) rows[(size_t)found * n_vars + i] = -1;
  if (t == 0) d.n_found[g] = found;
  __syncthreads();

  // the scores: a wave per row, as exactmap_final_kernel takes its score
  PlanSections<const_i32p> pl;
  carve_plan(as_const(d.plan), d.n_vars, d.P, d.U, d.n_cut, d.n_free, d.n_items, d.n_consts, pl);
  const const_i32p ptab = as_const(d.pair_tab) + (size_t)g * d.P, utab = as_const(d.unary_tab) + (size_t)g * d.U;
  const size_t XX = (size_t)X * X;
  for (int r = wave; r < M; r += WG / 64) {
    if (r >= found) {
      if (lane == 0) scores[r] = -__builtin_huge_val();
      continue;
    }
    const int32_t* xs = rows + (size_t)r * n_vars;
    double sc = 0.0;
    for (int p = lane; p < d.P; p += 64) {
      const int i = xs[pl.pav[2 * p]], j = xs[pl.pav[2 * p + 1]];
      sc += log(d.pair_tables[(size_t)ptab[p] * XX + (size_t)i * X + j]);
    }
    for (int u = lane; u < d.U; u += 64) sc += log(d.unary_tables[(size_t)utab[u] * X + xs[pl.uvar[u]]]);
    sc = wave_sum(sc);
    if (lane == 0) scores[r] = sc;
  }
}

// ---- host ----------------------------------------------------------------------------------------
thread_local int g_last_kernel = MLBP_EXACTMBEST_KERNEL_NONE;
static_assert(MLBP_EXACTMBEST_KERNEL_X64 == WALK_X64 && MLBP_EXACTMBEST_KERNEL_GENERIC == WALK_GENERIC, "the shared host core numbers the kernels");

int check_m(int32_t M) {
  if (M < 1 || M > MAXM) return fail(MLBP_EINVAL, "M = %d: between 1 and %d rows may be asked for", M, MAXM);
  return MLBP_OK;
}

int64_t lists_fixed_bytes(int64_t P, int64_t U) { return MLBP_EXACTMBEST_LISTS_FIXED + ints_bytes(P, U); }

// The X = 64 lists kernel: a wave's own LDS, and the rule that picks the kernel.
int64_t x64_wave_bytes(int64_t n_forest, int64_t M) { return n_forest * M * 64 * 12; }
int pick_lists_kernel(int values, int64_t n_vars, int64_t P, int64_t U, int64_t n_forest, int64_t M) {
  return values == WALK_X64 && x64_lds_bytes(n_vars, P, U, n_forest) + 4 * x64_wave_bytes(n_forest, M) <= MLBP_CUTSET_X64_LDS_BYTES ? WALK_X64 : WALK_GENERIC;
}

int64_t lists_bytes_of(int64_t X, int64_t n_vars, int64_t M) {
  const int64_t Xp = (X + 1) / 2 * 2, vl = X * M;
  const int64_t bytes = 8 * (n_vars * Xp + n_vars * vl + vl) + 4 * M * n_vars + 4 * n_vars * vl + 4 * n_vars * M;
  return (bytes + 7) / 8 * 8;
}

// The header's workspace formula over n walked configurations in `chunks` chunks: X^|C| of an exact call, N of a listed one.
// `which` is the library's kernel pick, so the sizes have been checked.
int64_t workspace_of(int which, int64_t B, int64_t X, int64_t n_vars, int64_t P, int64_t U, int64_t n, int64_t chunks, int64_t M) {
  const int64_t lb = lists_bytes_of(X, n_vars, M);
  const bool spill_walk = (which & 15) == WALK_GENERIC && generic_lds_bytes(n_vars, P, U, X) > MLBP_CUTSET_GENERIC_LDS_BYTES;
  const bool spill_lists = which >> 4 == WALK_GENERIC && lists_fixed_bytes(P, U) + lb > MLBP_CUTSET_GENERIC_LDS_BYTES;
  return (B * n * 2 + B * (M + 1) + B * M * M * 2 + (B * M * M * n_vars + 1) / 2 +
          (spill_walk ? B * chunks * vector_doubles(n_vars, X) : 0) + (spill_lists ? B * M * lb / 8 : 0)) * 8;
}

static_assert(MLBP_EXACTMBEST_MAX_CUT == MAX_LISTED_CUT, "the header states the shared walk's bound");

}  // namespace

extern "C" {

const char* mlbp_exactmbest_arch(void) { return "gfx950"; }
const char* mlbp_exactmbest_last_error(void) { return g_last_error.c_str(); }
int mlbp_exactmbest_last_kernel(void) { return g_last_kernel; }

int mlbp_exactmbest_pick_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t M) {
  const int values = pick_walk_kernel(X, n_vars, P, U, n_forest);
  if (values < 0) return values;
  if (int e = check_m(M)) return e;
  if (lists_fixed_bytes(P, U) > MLBP_CUTSET_GENERIC_LDS_BYTES)
    return fail(MLBP_EUNSUPPORTED, "P + U = %lld factors: their exponents do not fit the LDS budget", (long long)P + U);
  return values | pick_lists_kernel(values, n_vars, P, U, n_forest, M) << 4;
}

int mlbp_exactmbest_chunks(int32_t B, int32_t n_configs) {
  if (B <= 0 || n_configs <= 0) return fail(MLBP_EINVAL, "chunks: B = %d, n_configs = %d", B, n_configs);
  return walk_chunks(B, n_configs, MLBP_CUTSET_MIN_WORKGROUPS);
}

int64_t mlbp_exactmbest_lists_bytes(int32_t X, int32_t n_vars, int32_t M) {
  if (X < 2 || n_vars <= 0) return fail(MLBP_EINVAL, "lists_bytes: X = %d, n_vars = %d", X, n_vars);
  if (int e = check_m(M)) return e;
  return lists_bytes_of(X, n_vars, M);
}

int64_t mlbp_exactmbest_workspace_bytes(int32_t B, int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t n_cut,
                                        int32_t M) {
  const int which = mlbp_exactmbest_pick_kernel(X, n_vars, P, U, n_forest, M);
  if (which < 0) return which;
  if (n_cut < 0 || n_cut > n_vars) return fail(MLBP_EINVAL, "workspace: n_cut = %d with %d variables", n_cut, n_vars);
  const int64_t n_configs = count_configs(X, n_cut);
  if (n_configs < 0) return too_many_configs(X, n_cut);
  const int chunks = mlbp_exactmbest_chunks(B, (int32_t)n_configs);
  if (chunks < 0) return chunks;
  return workspace_of(which, B, X, n_vars, P, U, n_configs, chunks, M);
}

int mlbp_exactmbest_check_plan(const int32_t* plan, int32_t n_words, int32_t X) { return check_packed_plan(plan, n_words, X); }

int mlbp_exactmbest_f64(const mlbp_exactmbest_args* a, void* stream) {
  g_last_kernel = MLBP_EXACTMBEST_KERNEL_NONE;
  const bool listed = a && a->N > 0;                           // the header's listed mode: the walk's entries are the list's
  int64_t n_configs = listed ? a->N : 0;
  const int values = check_walk_args(a, [](int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest) {
    return pick_walk_kernel(X, n_vars, P, U, n_forest);
  }, [](const mlbp_exactmbest_args* a) {
    if (int e = check_m(a->M)) return e;
    if (!a->assignments || !a->scores || !a->n_found) return fail(MLBP_EINVAL, "assignments, scores or n_found is NULL");
    if (a->N < 0 || a->N > MLBP_EXACTMBEST_MAX_LISTED)
      return fail(MLBP_EINVAL, "N = %d: a list holds 1 to %d configurations (0: the exact call)", a->N, MLBP_EXACTMBEST_MAX_LISTED);
    if (a->N > 0 && a->n_cut > 0 && !a->configs) return fail(MLBP_EINVAL, "configs is NULL in a listed call with cutset variables");
    return (int)MLBP_OK;
  }, &n_configs, listed);
  if (values < 0) return values;
  const int which = mlbp_exactmbest_pick_kernel(a->X, a->n_vars, a->P, a->U, a->n_forest, a->M);
  if (which < 0) return which;
  int chunks = mlbp_exactmbest_chunks(a->B, (int32_t)n_configs);
  if (chunks < 0) return chunks;
  const int64_t need = listed ? workspace_of(which, a->B, a->X, a->n_vars, a->P, a->U, n_configs, chunks, a->M)
                              : mlbp_exactmbest_workspace_bytes(a->B, a->X, a->n_vars, a->P, a->U, a->n_forest, a->n_cut, a->M);
  if (int e = check_walk_workspace(a, need)) return e;
  if (int e = check_device("libmlbp_exactmbest.so")) return e;
  if (listed && a->n_cut == 0) {                               // the one empty configuration, whatever N: the exact call on a forest
    n_configs = 1;
    chunks = 1;
  }
  const int64_t B = a->B, M = a->M, lb = mlbp_exactmbest_lists_bytes(a->X, a->n_vars, a->M);
  MbestDev d;
  fill_walk_dev(d, a, n_configs, chunks, values);
  d.vc = a->workspace;
  d.sel = d.vc + B * n_configs * 2;
  d.cval = d.sel + B * (M + 1);
  d.cxs = reinterpret_cast<int32_t*>(d.cval + B * M * M * 2);
  double* spill = d.cval + B * M * M * 2 + (B * M * M * a->n_vars + 1) / 2;
  d.assignments = a->assignments; d.scores = a->scores; d.n_found = a->n_found;
  d.M = a->M;
  d.configs = listed && a->n_cut > 0 ? a->configs : nullptr;
  d.entries = a->entries;
  d.lists = nullptr;
  d.lists_bytes = lb;
  d.x64_bytes = d.wave_bytes = 0;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  if (values == WALK_X64) {
    if (int e = grant_x64_lds((const void*)exactmbest_values_x64_kernel, 0, MLBP_CUTSET_X64_LDS_BYTES)) return e;
    // the lists kernel too, whichever form this call takes: a later call of another M may be the captured one
    if (int e = grant_x64_lds((const void*)exactmbest_lists_x64_kernel, 1, MLBP_CUTSET_X64_LDS_BYTES)) return e;
    hipLaunchKernelGGL(exactmbest_values_x64_kernel, dim3(a->B, chunks), dim3(WG), (size_t)x64_lds_bytes(a->n_vars, a->P, a->U, a->n_forest), st, d);
  } else {
    const size_t lds = generic_walk_lds(d, spill);
    if (d.vectors) spill += B * chunks * vector_doubles(a->n_vars, a->X);
    hipLaunchKernelGGL(exactmbest_values_generic_kernel, dim3(a->B, chunks), dim3(WG), lds, st, d);
  }
  if (int e = launched("values")) return e;
  hipLaunchKernelGGL(exactmbest_select_kernel, dim3(a->B), dim3(WG), 0, st, d);
  if (int e = launched("select")) return e;
  if (which >> 4 == WALK_X64) {
    d.x64_bytes = (int32_t)x64_lds_bytes(a->n_vars, a->P, a->U, a->n_forest);
    d.wave_bytes = (int32_t)x64_wave_bytes(a->n_forest, a->M);
    MbestDev dl = d;                                             // the lists pass: its own number of chunks
    dl.chunks = walk_chunks(a->B, (a->M + 3) / 4, MLBP_CUTSET_MIN_WORKGROUPS);
    hipLaunchKernelGGL(exactmbest_lists_x64_kernel, dim3(a->B, dl.chunks), dim3(WG), (size_t)(d.x64_bytes + 4 * d.wave_bytes), st, dl);
  } else {
    size_t lists_lds = (size_t)lists_fixed_bytes(a->P, a->U);
    if ((int64_t)lists_lds + lb > MLBP_CUTSET_GENERIC_LDS_BYTES) d.lists = reinterpret_cast<char*>(spill);
    else lists_lds += (size_t)lb;
    hipLaunchKernelGGL(exactmbest_lists_generic_kernel, dim3(a->B, a->M), dim3(WG), lists_lds, st, d);
  }
  if (int e = launched("lists")) return e;
  hipLaunchKernelGGL(exactmbest_merge_kernel, dim3(a->B), dim3(WG), 0, st, d);
  if (int e = launched("merge")) return e;
  g_last_kernel = which;
  return MLBP_OK;
}

}  // extern "C"
