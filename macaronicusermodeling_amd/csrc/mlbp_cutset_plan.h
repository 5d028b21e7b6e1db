// What the cutset-conditioning libraries share beside the walk itself (libmlbp_cutset.so, libmlbp_exactmap.so,
// libmlbp_exactgrad.so and their later siblings; gfx950 only): the layout of the packed plan of include/mlbp_cutset.h and its validation, the kernel
// arguments every walk reads (WalkDev), the power-of-two arithmetic of the walks -- exponent extraction, the (mantissa,
// exponent) pair, the rescaling of a vector by the exponent of its largest entry -- and the host core: the LDS and vector
// sizing, the kernel pick, the chunks rule, the shape checks of a compute entry and the filling of WalkDev.  The walk over
// the configurations is mlbp_cutset_walk.h.  Helpers only, no kernel: each library keeps its own.  Not part of the ABI.
// Include after include/mlbp_cutset.h (the plan's constants), mlbp_graph_device.h and mlbp_graph_host.h.
#ifndef MLBP_CUTSET_PLAN_H
#define MLBP_CUTSET_PLAN_H

#include <climits>
#include <string>
#include <vector>

namespace mlbp_graph {

constexpr int HEADER = MLBP_CUTSET_PLAN_HEADER;
constexpr int EMPTY = -(1 << 28);           // the exponent of a partial result that holds nothing yet
constexpr int MIN_SHIFT = -4000;            // ldexp by less than this is zero for every finite double
constexpr int ROW = 65;                     // padded row of an X = 64 table in LDS

// The sections of a packed plan behind its header; returns the number of words.  The sizes have been checked.
template <class Ptr>
struct PlanSections { Ptr cutset, order, parent, item_off, items, consts, pav, uvar, fslot; };

template <class Ptr>
__host__ __device__ inline int64_t carve_plan(Ptr plan, int n_vars, int P, int U, int n_cut, int n_free, int n_items, int n_consts,
                                              PlanSections<Ptr>& s) {
  int64_t w = HEADER;
  s.cutset = plan + w; w += n_cut;
  s.order = plan + w; w += n_free;
  s.parent = plan + w; w += 2 * (int64_t)n_vars;
  s.item_off = plan + w; w += (int64_t)n_vars + 1;
  s.items = plan + w; w += 3 * (int64_t)n_items;
  s.consts = plan + w; w += 4 * (int64_t)n_consts;
  s.pav = plan + w; w += 2 * (int64_t)P;
  s.uvar = plan + w; w += U;
  s.fslot = plan + w; w += P;
  return w;
}

inline int64_t plan_words(int64_t n_vars, int64_t P, int64_t U, int64_t n_cut, int64_t n_free, int64_t n_items, int64_t n_consts) {
  return HEADER + n_cut + n_free + 2 * n_vars + n_vars + 1 + 3 * n_items + 4 * n_consts + 2 * P + U + P;
}

// What every kernel of the three libraries is handed: a library's own struct derives from it and adds its inputs and outputs.
struct WalkDev {
  const int32_t* plan;
  const double* pair_tables; const int32_t* pair_tab;
  const double* unary_tables; const int32_t* unary_tab;
  double* partials;                          // [B][parts][the library's partial], parts = chunks (generic) or 4 chunks (X = 64)
  double* vectors;                           // generic kernel, vectors not in LDS: [B][chunks][5 n_vars + 2][round_up(X, 2)]
  int32_t B, X, n_vars, P, U, n_cut, n_free, n_items, n_consts, n_forest, n_pair_tables, n_unary_tables, n_configs, chunks, parts;
};

// X^n_cut, or -1 beyond MLBP_CUTSET_MAX_CONFIGS
inline int64_t count_configs(int32_t X, int32_t n_cut) {
  int64_t n = 1;
  for (int q = 0; q < n_cut; ++q) {
    n *= X;
    if (n > MLBP_CUTSET_MAX_CONFIGS) return -1;
  }
  return n;
}

// ---- powers of two ---------------------------------------------------------------------------------
// The exponent e that brings a positive normal x to x * 2^-e in [1, 2); 0 for zero, a negative number, NaN and +inf.
__device__ __forceinline__ int exp_of(double x) {
  if (!(x > 0.0) || x == __builtin_huge_val()) return 0;
  return ((__double2hiint(x) >> 20) & 0x7ff) - 1023;
}

struct Scaled { double m; int e; };          // m * 2^e

__device__ __forceinline__ void mul(Scaled& z, double v) {
  z.m *= v;
  const int e = exp_of(z.m);
  z.m = ldexp(z.m, -e);
  z.e += e;
}

// The weight of a listed entry, Z_c exp(-log_q), by the formula of include/mlbp_cutsetis.h: exp(-log_q) = r 2^k,
// k = rint(-log_q / ln 2), r = exp(-log_q - k ln 2).  log_q = 0 leaves z as it is.  In two steps, for a kernel that wants the
// exponential taken before its walk, where fewer registers are live: weighted(z, lq) = weighted(z, proposal_factor(lq)).
struct ProposalFactor { double r; int k; };

__device__ __forceinline__ ProposalFactor proposal_factor(double lq) {
  constexpr double ln2 = 0.693147180559945309417232121458;
  const double k = rint(-lq / ln2);
  return {exp(-lq - k * ln2), (int)k};
}

__device__ __forceinline__ Scaled weighted(Scaled z, const ProposalFactor& f) {
  mul(z, f.r);
  z.e += f.k;
  return z;
}

__device__ __forceinline__ Scaled weighted(Scaled z, double lq) { return weighted(z, proposal_factor(lq)); }

// Max over the workgroup of non-negative values, the same bits in every thread (a NaN is passed over); two barriers.
__device__ __forceinline__ double block_max(double v, double* scratch /*[4]*/) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(scratch[0], scratch[1]), fmax(scratch[2], scratch[3]));
}

// The lowest of the workgroup's indices (0xffffffff: none), the same in every thread; two barriers.  Uses scratch[4 .. 6).
__device__ __forceinline__ unsigned block_min_index(unsigned idx, double* scratch) {
  unsigned* s = reinterpret_cast<unsigned*>(scratch + 4);
  const unsigned k = wave_max_u32(~idx);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = k;
  __syncthreads();
  return ~max(max(s[0], s[1]), max(s[2], s[3]));
}

// vec[0 .. X) times 2^-e, e the exponent of its largest entry; returns e.  The entries are visible on entry (a barrier
// behind the writes); ends with a barrier.
__device__ __forceinline__ int rescale(double* vec, int X, double* scratch) {
  const int t = threadIdx.x;
  double m = 0.0;
  for (int j = t; j < X; j += WG) m = fmax(m, vec[j]);
  const int e = exp_of(block_max(m, scratch));
  if (e != 0)
    for (int j = t; j < X; j += WG) vec[j] = ldexp(vec[j], -e);
  __syncthreads();
  return e;
}

// v times 2^-e, e the exponent of the wave's largest entry; e is added to the tally.
__device__ __forceinline__ double wave_rescale(double v, int& tally) {
  const int e = exp_of(wave_max(fmax(v, 0.0)));
  tally += e;
  return e != 0 ? ldexp(v, -e) : v;
}

}  // namespace mlbp_graph

namespace {

int too_many_configs(int32_t X, int32_t n_cut) {
  return fail(MLBP_EUNSUPPORTED, "X^|C| = %d^%d configurations: at most %d are supported", X, n_cut, MLBP_CUTSET_MAX_CONFIGS);
}

// A library that walks a caller's list of configurations (listed) has no bound on X^|C|; its bound is the walk's own: the
// generic walker keeps the states of a configuration in st[16].
constexpr int MAX_LISTED_CUT = 16;
int too_many_cut(int32_t n_cut) {
  return fail(MLBP_EUNSUPPORTED, "|C| = %d cutset variables: a listed walk takes at most %d", n_cut, MAX_LISTED_CUT);
}

// The checks of mlbp_cutset_check_plan (include/mlbp_cutset.h): a host array, for X states.  listed: the configurations come
// from a list, so X^|C| is not bounded and |C| is.
int check_packed_plan(const int32_t* plan, int32_t n_words, int32_t X, bool listed = false) {
  using namespace mlbp_graph;
  if (!plan || n_words < HEADER) return fail(MLBP_EINVAL, "plan: NULL or shorter than its header of %d words", HEADER);
  const int n_vars = plan[0], P = plan[1], U = plan[2], n_cut = plan[3], n_free = plan[4], n_items = plan[5], n_consts = plan[6],
            n_forest = plan[7];
  if (n_vars <= 0 || P < 0 || U < 0 || P + U <= 0 || n_cut < 0 || n_free < 0 || n_items < 0 || n_consts < 0 || n_forest < 0 ||
      (int64_t)n_cut + n_free != n_vars)
    return fail(MLBP_EINVAL, "plan: bad header (n_vars %d, P %d, U %d, n_cut %d, n_free %d, n_items %d, n_consts %d, n_forest %d)", n_vars,
                P, U, n_cut, n_free, n_items, n_consts, n_forest);
  if (plan_words(n_vars, P, U, n_cut, n_free, n_items, n_consts) != n_words)
    return fail(MLBP_EINVAL, "plan: header asks for %lld words, the array has %d", (long long)plan_words(n_vars, P, U, n_cut, n_free, n_items, n_consts),
                n_words);
  if (int e = check_states(X)) return e;
  if (X > MLBP_CUTSET_MAX_X) return fail(MLBP_EUNSUPPORTED, "X = %d: at most %d states are supported", X, MLBP_CUTSET_MAX_X);
  PlanSections<const int32_t*> s;
  carve_plan(plan, n_vars, P, U, n_cut, n_free, n_items, n_consts, s);

  std::vector<int> cutpos(n_vars, -1), pos(n_vars, -1);
  for (int q = 0; q < n_cut; ++q) {
    const int v = s.cutset[q];
    if (v < 0 || v >= n_vars) return fail(MLBP_EINVAL, "plan: cutset entry %d: variable %d out of range [0,%d)", q, v, n_vars);
    if (cutpos[v] >= 0) return fail(MLBP_EINVAL, "plan: cutset entry %d: variable %d is repeated", q, v);
    cutpos[v] = q;
  }
  if (listed ? n_cut > MAX_LISTED_CUT : count_configs(X, n_cut) < 0) return listed ? too_many_cut(n_cut) : too_many_configs(X, n_cut);
  for (int i = 0; i < n_free; ++i) {
    const int v = s.order[i];
    if (v < 0 || v >= n_vars || cutpos[v] >= 0 || pos[v] >= 0)
      return fail(MLBP_EINVAL, "plan: order entry %d: variable %d is out of range, in the cutset or repeated", i, v);
    pos[v] = i;
  }
  for (int p = 0; p < P; ++p) {
    const int a = s.pav[2 * p], b = s.pav[2 * p + 1];
    if (a < 0 || a >= n_vars || b < 0 || b >= n_vars) return fail(MLBP_EINVAL, "plan: pair factor %d: variable out of range [0,%d)", p, n_vars);
    if (a == b) return fail(MLBP_EINVAL, "plan: pair factor %d joins variable %d with itself", p, a);
  }
  for (int u = 0; u < U; ++u)
    if (s.uvar[u] < 0 || s.uvar[u] >= n_vars) return fail(MLBP_EINVAL, "plan: unary factor %d: variable %d out of range [0,%d)", u, s.uvar[u], n_vars);

  // the forest: every parent link joins a variable to a later one through a factor of its own
  std::vector<int> pair_used(P, 0), unary_used(U, 0);
  int slot = 0;
  for (int v = 0; v < n_vars; ++v)
    if (cutpos[v] >= 0 && (s.parent[2 * v] != -1 || s.parent[2 * v + 1] != -1))
      return fail(MLBP_EINVAL, "plan: cutset variable %d has a parent link", v);
  for (int i = 0; i < n_free; ++i) {
    const int v = s.order[i], p = s.parent[2 * v], par = s.parent[2 * v + 1];
    if (p == -1 && par == -1) continue;
    if (p < 0 || p >= P || par < 0 || par >= n_vars || pos[par] <= i ||
        !((s.pav[2 * p] == v && s.pav[2 * p + 1] == par) || (s.pav[2 * p] == par && s.pav[2 * p + 1] == v)))
      return fail(MLBP_EINVAL, "plan: parent link of variable %d (factor %d, parent %d): the factor does not join the two or the parent does not come later", v, p, par);
    if (pair_used[p]++) return fail(MLBP_EINVAL, "plan: pair factor %d is used twice", p);
    if (s.fslot[p] != slot) return fail(MLBP_EINVAL, "plan: forest_slot[%d] = %d, expected %d", p, s.fslot[p], slot);
    ++slot;
  }
  if (slot != n_forest) return fail(MLBP_EINVAL, "plan: n_forest = %d but %d parent links", n_forest, slot);
  for (int p = 0; p < P; ++p) {
    const int a = s.pav[2 * p], b = s.pav[2 * p + 1];
    if (pair_used[p]) continue;
    if (s.fslot[p] != -1) return fail(MLBP_EINVAL, "plan: forest_slot[%d] = %d for a factor that is no parent link", p, s.fslot[p]);
    if (cutpos[a] >= 0 || cutpos[b] >= 0) continue;
    // a factor between two free variables that is no parent link: walk both to their roots
    std::string path_a = std::to_string(a), path_b;
    std::vector<int> seen(n_vars, 0);
    for (int x = a; x >= 0; x = s.parent[2 * x + 1]) seen[x] = 1;
    int meet = b;
    while (meet >= 0 && !seen[meet]) meet = s.parent[2 * meet + 1];
    if (meet < 0) return fail(MLBP_EINVAL, "plan: pair factor %d joins two trees of the remainder: it is left out of the forest", p);
    for (int x = a; x != meet; ) { x = s.parent[2 * x + 1]; path_a += " - " + std::to_string(x); }
    for (int x = b; x != meet; x = s.parent[2 * x + 1]) path_b = " - " + std::to_string(x) + path_b;
    return fail(MLBP_EINVAL, "plan: the remainder has a cycle through factor %d: variables %s%s - %d", p, path_a.c_str(), path_b.c_str(), a);
  }

  // items and consts: every other factor once, where its variables say
  if (s.item_off[0] != 0) return fail(MLBP_EINVAL, "plan: item_off[0] must be 0");
  for (int v = 0; v < n_vars; ++v) {
    const int lo = s.item_off[v], hi = s.item_off[v + 1];
    if (hi < lo || hi > n_items) return fail(MLBP_EINVAL, "plan: item_off not monotone or beyond the %d items at variable %d", n_items, v);
    if (cutpos[v] >= 0 && hi != lo) return fail(MLBP_EINVAL, "plan: cutset variable %d has items", v);
    for (int it = lo; it < hi; ++it) {
      const int kind = s.items[3 * it], f = s.items[3 * it + 1], q = s.items[3 * it + 2];
      if (kind == MLBP_CUTSET_ITEM_UNARY) {
        if (f < 0 || f >= U || s.uvar[f] != v) return fail(MLBP_EINVAL, "plan: item %d: unary factor %d is not on variable %d", it, f, v);
        if (unary_used[f]++) return fail(MLBP_EINVAL, "plan: unary factor %d is used twice", f);
      } else if (kind == MLBP_CUTSET_ITEM_COL || kind == MLBP_CUTSET_ITEM_ROW) {
        const int mine = kind == MLBP_CUTSET_ITEM_COL ? 0 : 1;
        if (f < 0 || f >= P || q < 0 || q >= n_cut || s.pav[2 * f + mine] != v || s.pav[2 * f + 1 - mine] != s.cutset[q])
          return fail(MLBP_EINVAL, "plan: item %d: pair factor %d does not join variable %d (axis %d) and cut position %d", it, f, v, mine, q);
        if (pair_used[f]++) return fail(MLBP_EINVAL, "plan: pair factor %d is used twice", f);
      } else {
        return fail(MLBP_EINVAL, "plan: item %d: unknown kind %d", it, kind);
      }
    }
  }
  if (s.item_off[n_vars] != n_items) return fail(MLBP_EINVAL, "plan: item_off[n_vars] = %d, but %d items", s.item_off[n_vars], n_items);
  for (int i = 0; i < n_consts; ++i) {
    const int kind = s.consts[4 * i], f = s.consts[4 * i + 1], q0 = s.consts[4 * i + 2], q1 = s.consts[4 * i + 3];
    if (q0 < 0 || q0 >= n_cut) return fail(MLBP_EINVAL, "plan: const %d: cut position %d out of range [0,%d)", i, q0, n_cut);
    if (kind == MLBP_CUTSET_CONST_UNARY) {
      if (f < 0 || f >= U || s.uvar[f] != s.cutset[q0]) return fail(MLBP_EINVAL, "plan: const %d: unary factor %d is not on cut position %d", i, f, q0);
      if (unary_used[f]++) return fail(MLBP_EINVAL, "plan: unary factor %d is used twice", f);
    } else if (kind == MLBP_CUTSET_CONST_PAIR) {
      if (q1 < 0 || q1 >= n_cut) return fail(MLBP_EINVAL, "plan: const %d: cut position %d out of range [0,%d)", i, q1, n_cut);
      if (f < 0 || f >= P || s.pav[2 * f] != s.cutset[q0] || s.pav[2 * f + 1] != s.cutset[q1])
        return fail(MLBP_EINVAL, "plan: const %d: pair factor %d does not join cut positions %d and %d", i, f, q0, q1);
      if (pair_used[f]++) return fail(MLBP_EINVAL, "plan: pair factor %d is used twice", f);
    } else {
      return fail(MLBP_EINVAL, "plan: const %d: unknown kind %d", i, kind);
    }
  }
  for (int p = 0; p < P; ++p)
    if (!pair_used[p]) return fail(MLBP_EINVAL, "plan: pair factor %d is left out", p);
  for (int u = 0; u < U; ++u)
    if (!unary_used[u]) return fail(MLBP_EINVAL, "plan: unary factor %d is left out", u);
  return MLBP_OK;
}

// ---- the host core of a walk: sizing, kernel pick, chunks, the checks and the launch of a compute entry -----------------
// The two walk kernels, as every library's header numbers them (MLBP_*_KERNEL_X64 / _GENERIC).
constexpr int WALK_X64 = 1, WALK_GENERIC = 2;

int64_t ints_bytes(int64_t P, int64_t U) { return 4 * ((P + U + 16 + 3) / 4 * 4); }
int64_t vector_doubles(int64_t n_vars, int64_t X) { return (5 * n_vars + 2) * ((X + 1) / 2 * 2); }
int64_t x64_lds_bytes(int64_t n_vars, int64_t P, int64_t U, int64_t n_forest) {
  return n_forest * (64 * mlbp_graph::ROW * 8) + 21 * n_vars * 512 + 64 + ints_bytes(P, U);
}
int64_t generic_lds_bytes(int64_t n_vars, int64_t P, int64_t U, int64_t X) { return vector_doubles(n_vars, X) * 8 + 64 + ints_bytes(P, U); }

// The rule of mlbp_cutset_pick_kernel; max_forest_x64: the most forest factors the library's X = 64 kernel takes.
int pick_walk_kernel(int32_t X, int32_t n_vars, int32_t P, int32_t U, int32_t n_forest, int32_t max_forest_x64 = INT_MAX) {
  if (X < 2 || n_vars <= 0 || P < 0 || U < 0 || n_forest < 0 || n_forest > P)
    return fail(MLBP_EINVAL, "pick_kernel: X = %d, n_vars = %d, P = %d, U = %d, n_forest = %d", X, n_vars, P, U, n_forest);
  if (X > MLBP_CUTSET_MAX_X) return fail(MLBP_EUNSUPPORTED, "X = %d: at most %d states are supported", X, MLBP_CUTSET_MAX_X);
  if (X == 64 && n_forest <= max_forest_x64 && x64_lds_bytes(n_vars, P, U, n_forest) <= MLBP_CUTSET_X64_LDS_BYTES) return WALK_X64;
  if (64 + ints_bytes(P, U) > MLBP_CUTSET_GENERIC_LDS_BYTES)
    return fail(MLBP_EUNSUPPORTED, "P + U = %lld factors: their exponents do not fit the LDS budget", (long long)P + U);
  return WALK_GENERIC;
}

// C of the grid (B, C): every walker (a workgroup, or the four waves of one) gets work until min_workgroups are in flight.
int32_t walk_chunks(int32_t B, int32_t walkers, int32_t min_workgroups) {
  const int32_t spread = (min_workgroups + B - 1) / B;
  return walkers < spread ? walkers : spread;
}

// The doubles of a chunk in the workspace, `per` the library's partial: a partial per wave (X = 64), or the partial and, when
// they do not fit the LDS, the generic kernel's vectors.
int64_t chunk_doubles(int which, int64_t per, int64_t n_vars, int64_t P, int64_t U, int64_t X) {
  if (which == WALK_X64) return 4 * per;
  return per + (generic_lds_bytes(n_vars, P, U, X) > MLBP_CUTSET_GENERIC_LDS_BYTES ? vector_doubles(n_vars, X) : 0);
}

// The checks every compute entry starts with, over the library's args struct (the field names agree): sizes, states, the
// library's kernel pick, the plan's words, the tables, own(a) -- the library's outputs and further inputs --, the number of
// configurations, the extent.  Returns the kernel (WALK_*) or the status; *n_configs is set with the kernel.  listed: the
// configurations come from the caller's list -- |C| is bounded in the place of X^|C|, and *n_configs is left to the library.
template <class Args, class Own>
int check_walk_args(const Args* a, int (*pick)(int32_t, int32_t, int32_t, int32_t, int32_t), Own own, int64_t* n_configs,
                    bool listed = false) {
  using namespace mlbp_graph;
  if (!a) return fail(MLBP_EINVAL, "args is NULL");
  if (a->B <= 0 || a->n_vars <= 0 || a->P < 0 || a->U < 0 || a->P + a->U <= 0 || a->n_cut < 0 || a->n_free < 0 || a->n_items < 0 ||
      a->n_consts < 0 || (int64_t)a->n_cut + a->n_free != a->n_vars)
    return fail(MLBP_EINVAL, "bad sizes: B %d, n_vars %d, P %d, U %d, n_cut %d, n_free %d, n_items %d, n_consts %d", a->B, a->n_vars, a->P,
                a->U, a->n_cut, a->n_free, a->n_items, a->n_consts);
  if (int e = check_states(a->X)) return e;
  const int which = pick(a->X, a->n_vars, a->P, a->U, a->n_forest);
  if (which < 0) return which;
  if (!a->plan || plan_words(a->n_vars, a->P, a->U, a->n_cut, a->n_free, a->n_items, a->n_consts) != a->plan_words)
    return fail(MLBP_EINVAL, "plan is NULL or plan_words = %d disagrees with the sizes", a->plan_words);
  if (int e = check_args_tables(a)) return e;
  if (int e = own(a)) return e;
  if (listed) {
    if (a->n_cut > MAX_LISTED_CUT) return too_many_cut(a->n_cut);
  } else {
    *n_configs = count_configs(a->X, a->n_cut);
    if (*n_configs < 0) return too_many_configs(a->X, a->n_cut);
  }
  if ((int64_t)a->n_vars * a->X > 0x7fffffff / 16) return fail(MLBP_EUNSUPPORTED, "n_vars * X = %lld too large", (long long)a->n_vars * a->X);
  return which;
}

// `need`: the library's workspace_bytes of the call, or its status.
template <class Args>
int check_walk_workspace(const Args* a, int64_t need) {
  if (need < 0) return (int)need;
  if (!a->workspace || a->workspace_bytes < need)
    return fail(MLBP_EINVAL, "workspace is NULL or workspace_bytes = %lld below the %lld the call needs", (long long)a->workspace_bytes, (long long)need);
  return MLBP_OK;
}

// The fields of WalkDev from the args; the partials lead the workspace, the vectors are in LDS until generic_walk_lds says not.
template <class Args>
void fill_walk_dev(mlbp_graph::WalkDev& d, const Args* a, int64_t n_configs, int chunks, int which) {
  d.plan = a->plan;
  d.pair_tables = a->pair_tables; d.pair_tab = a->pair_tab; d.unary_tables = a->unary_tables; d.unary_tab = a->unary_tab;
  d.partials = a->workspace;
  d.vectors = nullptr;
  d.B = a->B; d.X = a->X; d.n_vars = a->n_vars; d.P = a->P; d.U = a->U; d.n_cut = a->n_cut; d.n_free = a->n_free; d.n_items = a->n_items;
  d.n_consts = a->n_consts; d.n_forest = a->n_forest; d.n_pair_tables = a->n_pair_tables; d.n_unary_tables = a->n_unary_tables;
  d.n_configs = (int32_t)n_configs; d.chunks = chunks; d.parts = which == WALK_X64 ? 4 * chunks : chunks;
}

// The dynamic LDS of the generic walk kernel; vectors that do not fit go to `spill`, the library's place for them in the workspace.
size_t generic_walk_lds(mlbp_graph::WalkDev& d, double* spill) {
  const int64_t lds = generic_lds_bytes(d.n_vars, d.P, d.U, d.X);
  if (lds <= MLBP_CUTSET_GENERIC_LDS_BYTES) return (size_t)lds;
  d.vectors = spill;
  return (size_t)(64 + ints_bytes(d.P, d.U));
}

// Behind a launch: `what` names the kernel in the message.
int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MLBP_OK : fail(MLBP_EHIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

}  // namespace

#endif
