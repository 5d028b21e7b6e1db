// The sweep-program compilers of libmlbp.so: one validated op list in, the integer images of the X = 64 kernels out.
//
//   validate_program        range checks on the caller's op list (every later routine indexes freely)
//   drop_unchanged_updates  the op list MLBP_SWEEP_SKIP_UNCHANGED runs
//   build_fused_program     8-word op headers of the exact kernel (sweep_x64_fused_kernel): unary messages hoisted, variable->factor
//                           updates fused into the pairwise update they feed, dead updates dropped, independent updates bundled
//   build_lean_program      micro-ops of the lean kernel (sweep_x64_lean_kernel) and its read-out lists
//   (build_shared_program   the live-tile form of the shared-table kernel: mlbp_compile_shared.cpp)
//   mlbp_program_plan / mlbp_program_image   what the chain makes of an op list, for callers and tests without a device
//
// Pure integer code: no device call, no device header; compiles with a plain C++17 host compiler.  Every word the chain emits is
// pinned by tests/golden/program_images.npz (tests/test_program_images.py).
#include <algorithm>
#include <climits>
#include <cstring>
#include <map>
#include <vector>

#include "mlbp_internal.h"

namespace mlbp {

// Range checks shared by mlbp_program_create, mlbp_program_plan and mlbp_program_image; every later routine indexes freely.
int validate_program(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs, const int32_t* sweeps,
                     int32_t n_sweeps, int32_t n_msgs, int32_t P, int32_t U, int* max_srcs_out) {
  if (!ops || !sweeps || n_ops <= 0 || n_sweeps <= 0 || n_msgs <= 0 || P < 0 || U < 0 || n_srcs < 0 ||
      (n_srcs > 0 && !srcs))
    return fail(MLBP_EINVAL, "program: bad sizes or NULL arrays");
  int max_srcs = 0;
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
        if (b < 0 || b >= n_msgs) return fail(MLBP_EINVAL, "op %d: source slot %d out of range", o, b);
        if (b == c) return fail(MLBP_EINVAL, "op %d: source and destination slot coincide", o);
        break;
      case MLBP_OP_VAR:
        if (a < 0 || b < 0 || (int64_t)a + b > n_srcs) return fail(MLBP_EINVAL, "op %d: srcs range [%d,%d) out of [0,%d)", o, a, a + b, n_srcs);
        for (int q = a; q < a + b; ++q)
          if (srcs[q] < 0 || srcs[q] >= n_msgs) return fail(MLBP_EINVAL, "op %d: source slot %d out of range", o, srcs[q]);
        if (b > max_srcs) max_srcs = b;
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
  if (max_srcs_out) *max_srcs_out = max_srcs;
  return MLBP_OK;
}

// MLBP_SWEEP_SKIP_UNCHANGED: the op list with every update dropped whose inputs -- and therefore whose result, bit for
// bit -- are what they were when the destination slot was last computed.  Value numbering over the whole call: a slot's
// value is named by (kind, table / factor, names of the source values); what the call starts from is opaque.  A root
// sequence re-walks messages that the previous sweep left final (the whole of a tree after its first sweep; the part of a
// loopy graph upstream of the first changed message), LBP.py:223-233 recomputes them, this list does not.  Returns the
// number of updates dropped; sweeps_out are ranges into ops_out (no sharing between equal roots any more).
int drop_unchanged_updates(const int32_t* ops, const int32_t* srcs, const int32_t* sweeps, int n_sweeps, int n_msgs,
                           std::vector<int32_t>& ops_out, std::vector<int32_t>& sweeps_out) {
  std::map<std::vector<int64_t>, int64_t> names;
  std::vector<int64_t> val(n_msgs);
  for (int c = 0; c < n_msgs; ++c) val[c] = -(int64_t)c - 1;
  int dropped = 0;
  std::vector<int64_t> key;
  for (int s = 0; s < n_sweeps; ++s) {
    const int first = sweeps[2 * s], cnt = sweeps[2 * s + 1];
    const int start = (int)ops_out.size() / 4;
    for (int o = first; o < first + cnt; ++o) {
      const int kind = ops[4 * o], a = ops[4 * o + 1], b = ops[4 * o + 2], c = ops[4 * o + 3];
      key.clear();
      key.push_back(kind);
      if (kind == MLBP_OP_VAR) {
        for (int q = a; q < a + b; ++q) key.push_back(val[srcs[q]]);
      } else if (kind == MLBP_OP_UNARY) {
        key.push_back(a);
      } else {
        key.push_back(a);
        key.push_back(val[b]);
      }
      auto it = names.find(key);
      const int64_t name = it != names.end() ? it->second : (int64_t)names.size();
      if (it == names.end()) names.emplace(key, name);
      if (val[c] == name) { ++dropped; continue; }
      val[c] = name;
      ops_out.insert(ops_out.end(), ops + 4 * o, ops + 4 * o + 4);
    }
    sweeps_out.push_back(start);
    sweeps_out.push_back((int)ops_out.size() / 4 - start);
  }
  return dropped;
}

int find_cprod(const std::vector<std::vector<int32_t>>& cprods, const std::vector<int32_t>& consts) {
  for (size_t k = 0; k < cprods.size(); ++k)
    if (cprods[k] == consts) return (int)k;
  return -1;
}

// ------------------------------------------------------------------------------------------------
// Fused program form (see sweep_x64_fused_kernel).  Input: the validated 4-word op list.
// ------------------------------------------------------------------------------------------------
namespace {

bool is_pair_op(int kind) { return kind == MLBP_OP_PAIR_TM || kind == MLBP_OP_PAIR_MT; }
bool is_fused_pair(int kd) { return kd == FOP_VAR_PAIR_TM || kd == FOP_VAR_PAIR_MT; }
bool is_plain_pair(int kd) { return kd == FOP_PAIR_TM || kd == FOP_PAIR_MT; }

// 0. inside each sweep, sink every variable->factor update down to just before the pairwise update that
//    consumes it when nothing in between writes one of its inputs or touches its output.  The up pass of a
//    loopy schedule (LBP.py:227-233) emits "X7->F17, X4->F14, F17->X1, F14->X1": neither pair is adjacent, so
//    without this no fusion happens.  Updates keep their inputs, hence their values; only the order of
//    independent updates changes.
std::vector<int32_t> sink_variable_updates(const int32_t* ops_in, const int32_t* srcs, const int32_t* sweeps, int n_sweeps) {
  int n_total = 0;
  for (int s = 0; s < n_sweeps; ++s) n_total = std::max(n_total, sweeps[2 * s] + sweeps[2 * s + 1]);
  std::vector<int32_t> ops_v(ops_in, ops_in + 4 * (size_t)n_total);
  for (int s = 0; s < n_sweeps; ++s) {
    const int first = sweeps[2 * s], cnt = sweeps[2 * s + 1];
    int32_t* q = ops_v.data() + 4 * (size_t)first;
    for (int i = 0; i < cnt; ++i) {
      if (q[4 * i] != MLBP_OP_VAR) continue;
      const int a = q[4 * i + 1], b = q[4 * i + 2], c = q[4 * i + 3];
      int j = i + 1;
      bool legal = true;
      for (; j < cnt && legal; ++j) {
        if (is_pair_op(q[4 * j]) && q[4 * j + 2] == c) break;                        // the consumer
        const int w = q[4 * j + 3];
        if (w == c) legal = false;
        for (int k = a; k < a + b && legal; ++k) if (srcs[k] == w) legal = false;
        if (q[4 * j] == MLBP_OP_VAR)
          for (int k = q[4 * j + 1]; k < q[4 * j + 1] + q[4 * j + 2] && legal; ++k) if (srcs[k] == c) legal = false;
      }
      if (!legal || j >= cnt || j == i + 1) continue;
      const int32_t v[4] = {q[4 * i], a, b, c};
      for (int k = i; k < j - 1; ++k)
        for (int e = 0; e < 4; ++e) q[4 * k + e] = q[4 * (k + 1) + e];
      for (int e = 0; e < 4; ++e) q[4 * (j - 1) + e] = v[e];
      --i;                                                                           // the op that slid into place i
    }
  }
  return ops_v;
}

// 1. may the unary messages be hoisted?  Every read of a unary factor's message slot must come
//    after a UNARY op has written that slot (then the value read is always the same constant).
//    Returns, per slot, whether it holds a hoisted message (none when the program does not qualify) and fills out.hoist.
std::vector<char> hoist_unary_messages(const int32_t* ops, const int32_t* srcs, const int32_t* sweeps, int n_sweeps, int n_msgs,
                                       FusedProgram& out) {
  std::vector<char> is_unary_dst(n_msgs, 0), written(n_msgs, 0);
  std::vector<int> unary_of(n_msgs, -1);
  bool hoistable = true;
  for (int s = 0; s < n_sweeps; ++s)
    for (int o = sweeps[2 * s]; o < sweeps[2 * s] + sweeps[2 * s + 1]; ++o)
      if (ops[4 * o] == MLBP_OP_UNARY) {
        int c = ops[4 * o + 3];
        if (is_unary_dst[c] && unary_of[c] != ops[4 * o + 1]) hoistable = false;  // two tables, one slot
        is_unary_dst[c] = 1;
        unary_of[c] = ops[4 * o + 1];
      }
  for (int s = 0; s < n_sweeps && hoistable; ++s)
    for (int o = sweeps[2 * s]; o < sweeps[2 * s] + sweeps[2 * s + 1] && hoistable; ++o) {
      const int kind = ops[4 * o], a = ops[4 * o + 1], b = ops[4 * o + 2], c = ops[4 * o + 3];
      if (kind == MLBP_OP_UNARY) {
        written[c] = 1;
      } else if (kind == MLBP_OP_VAR) {
        for (int q = a; q < a + b; ++q)
          if (is_unary_dst[srcs[q]] && !written[srcs[q]]) hoistable = false;
        if (is_unary_dst[c]) hoistable = false;
      } else {
        if ((is_unary_dst[b] && !written[b]) || is_unary_dst[c]) hoistable = false;
      }
    }
  if (!hoistable) return std::vector<char>(n_msgs, 0);
  for (int c = 0; c < n_msgs; ++c)
    if (is_unary_dst[c]) { out.hoist.push_back(unary_of[c]); out.hoist.push_back(c); }
  return is_unary_dst;
}

// source lists start on multiples of 4 words (int4 reads)
void pad4(std::vector<int32_t>& psrcs, int n_msgs) { while (psrcs.size() % 4) psrcs.push_back(n_msgs); }

// 2. per variable update: fast source list = [base slot, varying sources...] where the base is the
//    uniform vector (ext slot 0) or the constant product of the hoisted sources (ext slot 1+k);
//    exact source list = the original one.
// 3. fuse "variable -> factor" into the pairwise update it feeds; drop hoisted unary ops.
void fuse_updates(const int32_t* ops, const int32_t* srcs, const int32_t* sweeps, int n_sweeps, int n_msgs,
                  const std::vector<char>& hoisted, std::vector<std::vector<int32_t>>& cprods, FusedProgram& out) {
  auto var_lists = [&](int a, int b, int& fa, int& fn, int& ea, int& en) {
    std::vector<int32_t> consts, vars;
    for (int q = a; q < a + b; ++q) (hoisted[srcs[q]] ? consts : vars).push_back(srcs[q]);
    int base = n_msgs;                                        // uniform
    if (!consts.empty()) {
      int k = find_cprod(cprods, consts);
      if (k < 0) { k = (int)cprods.size(); cprods.push_back(consts); }
      base = n_msgs + 1 + k;
    }
    pad4(out.psrcs, n_msgs);
    fa = (int)out.psrcs.size();
    out.psrcs.push_back(base);
    for (int v : vars) out.psrcs.push_back(v);
    fn = 1 + (int)vars.size();
    pad4(out.psrcs, n_msgs);
    ea = (int)out.psrcs.size();
    for (int q = a; q < a + b; ++q) out.psrcs.push_back(srcs[q]);
    en = b;
  };
  for (int s = 0; s < n_sweeps; ++s) {
    const int first = sweeps[2 * s], cnt = sweeps[2 * s + 1];
    const int f0 = (int)out.fops.size() / 8;
    for (int o = first; o < first + cnt; ++o) {
      const int kind = ops[4 * o], a = ops[4 * o + 1], b = ops[4 * o + 2], c = ops[4 * o + 3];
      if (kind == MLBP_OP_UNARY) {
        if (!hoisted[c]) out.fops.insert(out.fops.end(), {FOP_UNARY, a, 0, c, 0, 0, 0, 0});
      } else if (kind == MLBP_OP_VAR) {
        int fa, fn, ea, en;
        var_lists(a, b, fa, fn, ea, en);
        const bool next_is_pair = o + 1 < first + cnt && is_pair_op(ops[4 * (o + 1)]) && ops[4 * (o + 1) + 2] == c;
        if (next_is_pair) {
          const int pk = ops[4 * (o + 1)];
          out.fops.insert(out.fops.end(), {pk == MLBP_OP_PAIR_TM ? FOP_VAR_PAIR_TM : FOP_VAR_PAIR_MT, fa, fn, c,
                                           ops[4 * (o + 1) + 1], ops[4 * (o + 1) + 3], ea, en});
          out.pairseq.push_back(ops[4 * (o + 1) + 1]);
          ++o;
        } else {
          out.fops.insert(out.fops.end(), {FOP_VAR, fa, fn, c, 0, 0, ea, en});
        }
      } else {
        out.fops.insert(out.fops.end(), {kind == MLBP_OP_PAIR_TM ? FOP_PAIR_TM : FOP_PAIR_MT, a, b, c, 0, 0, 0, 0});
        out.pairseq.push_back(a);
      }
    }
    out.fsweeps.push_back(f0);
    out.fsweeps.push_back((int)out.fops.size() / 8 - f0);
  }
}

// 3b. drop lone variable->factor updates whose result is overwritten before anything reads it (the last two of a
//     sweep when the next sweep's root differs: the new schedule recomputes those messages first).  Backward
//     liveness over the whole call; every slot is live at the end (the messages are an output).
void drop_dead_variable_updates(int n_slots, FusedProgram& out) {
  const int n = (int)out.fops.size() / 8;
  std::vector<char> live(n_slots, 1), dead(n, 0);
  for (int i = n - 1; i >= 0; --i) {
    const int32_t* w = &out.fops[8 * (size_t)i];
    const int kd = w[0] & 0xFF;
    if (kd == FOP_VAR && !live[w[3]]) { dead[i] = 1; continue; }
    if (kd == FOP_UNARY) { live[w[3]] = 0; continue; }
    if (is_plain_pair(kd)) { live[w[3]] = 0; live[w[2]] = 1; continue; }
    live[w[3]] = 0;
    if (kd != FOP_VAR) live[w[5]] = 0;
    for (int q = 0; q < w[2]; ++q) live[out.psrcs[w[1] + q]] = 1;
    for (int q = 0; q < w[7]; ++q) live[out.psrcs[w[6] + q]] = 1;
  }
  std::vector<int32_t> kept, fs;
  for (size_t sw = 0; sw + 1 < out.fsweeps.size(); sw += 2) {
    const int f0 = (int)kept.size() / 8;
    for (int i = out.fsweeps[sw]; i < out.fsweeps[sw] + out.fsweeps[sw + 1]; ++i)
      if (!dead[i]) kept.insert(kept.end(), out.fops.begin() + 8 * (size_t)i, out.fops.begin() + 8 * (size_t)i + 8);
    fs.push_back(f0); fs.push_back((int)kept.size() / 8 - f0);
  }
  out.fops.swap(kept);
  out.fsweeps.swap(fs);
}

// 3c. bundle adjacent pairwise updates of a sweep that touch disjoint message slots (bundles hold two updates)
void bundle_pairwise_updates(FusedProgram& out) {
  auto is_pair = [&](int i) { const int kd = out.fops[8 * i] & 0xFF; return is_plain_pair(kd) || is_fused_pair(kd); };
  auto sets = [&](int i, std::vector<int>& rd, std::vector<int>& wr) {
    const int32_t* w = &out.fops[8 * i];
    rd.clear(); wr.clear();
    if (is_plain_pair(w[0] & 0xFF)) { rd.push_back(w[2]); wr.push_back(w[3]); }
    else { for (int q = 0; q < w[7]; ++q) rd.push_back(out.psrcs[w[6] + q]); wr.push_back(w[3]); wr.push_back(w[5]); }
  };
  auto meets = [](const std::vector<int>& x, const std::vector<int>& y) {
    for (int u : x) for (int v : y) if (u == v) return true;
    return false;
  };
  std::vector<int> ra, wa, rb, wb;
  for (size_t sw = 0; sw + 1 < out.fsweeps.size(); sw += 2) {
    const int f0 = out.fsweeps[sw], f1 = f0 + out.fsweeps[sw + 1];
    for (int i = f0; i + 1 < f1; ++i) {
      if (!is_pair(i) || !is_pair(i + 1)) continue;
      sets(i, ra, wa); sets(i + 1, rb, wb);
      if (meets(wa, rb) || meets(wb, ra) || meets(wa, wb)) continue;
      out.fops[8 * i] |= FOP_BUNDLED;
      ++i;
    }
  }
}

}  // namespace

void build_fused_program(const int32_t* ops_in, const int32_t* srcs, const int32_t* sweeps, int n_sweeps, int n_msgs,
                         FusedProgram& out) {
  const std::vector<int32_t> ops = sink_variable_updates(ops_in, srcs, sweeps, n_sweeps);
  const std::vector<char> hoisted = hoist_unary_messages(ops.data(), srcs, sweeps, n_sweeps, n_msgs, out);
  std::vector<std::vector<int32_t>> cprods;                      // distinct constant-source lists
  fuse_updates(ops.data(), srcs, sweeps, n_sweeps, n_msgs, hoisted, cprods, out);
  drop_dead_variable_updates(n_msgs + 1 + (int)cprods.size(), out);
  bundle_pairwise_updates(out);
  out.pairseq.push_back(-1);
  std::vector<char> w(n_msgs, 0);
  for (size_t i = 0; i < out.fops.size(); i += 8) {
    const int kind = out.fops[i] & 0xFF;
    if (kind == FOP_UNARY) { out.has_unary_fops = true; continue; }
    w[out.fops[i + 3]] = 1;                                            // VAR dst / standalone PAIR dst
    if (is_fused_pair(kind)) w[out.fops[i + 5]] = 1;
  }
  for (int c = 0; c < n_msgs; ++c)
    if (w[c]) out.written.push_back(c);
  for (int q = 0; q < 8; ++q) out.psrcs.push_back(n_msgs);   // tail padding for the int4 reads
  pad4(out.psrcs, n_msgs);
  out.n_cprod = (int)cprods.size();
  for (auto& l : cprods) {
    out.cpw.push_back((int)l.size());
    for (int v : l) out.cpw.push_back(v);
  }
}

// ------------------------------------------------------------------------------------------------
// Lean form (sweep_x64_lean_kernel)
// ------------------------------------------------------------------------------------------------
// FusedProgram -> micro-ops.  Every operand becomes an LDS byte offset (slot * 512); a variable product with more
// than four sources is split into a chain of variable-only micro-ops ("links") that hand the running product on in a
// register (UOP_CARRY_OUT / UOP_CARRY_IN); only the last link stores.
// Image: bundles [n_bundles][16] | per-wave hoist lists [4][HL][2] | constant-product lists [n_cprod][16] |
// per-wave written-slot lists [4][WL] | one bundle of padding (the loop prefetches one bundle past the end), zeros up to 2 KB.
void build_lean_program(const FusedProgram& fp, int n_msgs, LeanProgram& out) {
  out = LeanProgram();
  if (fp.has_unary_fops) { out.why = "in-loop unary updates (not hoistable)"; return; }
  std::vector<int32_t> U;                            // micro-ops, 8 words each
  // every source list is padded to four entries with the all-ones ext slot: the kernel fetches sources 1-2, and 3-4 when
  // there are more than two, without looking at the count in between
  const int32_t ones = (n_msgs + 1 + fp.n_cprod) * 512;
  std::vector<char> second;                          // micro-op i is the second member of a bundle
  auto emit_var = [&](const int32_t* src, int n, int c) {      // work[c] = prod(src[0..n))
    int done = 0;
    do {
      int32_t w[8] = {0, ones, ones, ones, ones, 0, 0, 0};
      int k = 0;
      const bool first = done == 0;
      while (k < 4 && done < n) w[1 + k++] = src[done++] * 512;
      w[0] = UOP_VAR | (k << UOP_NSRC_SHIFT) | (first ? 0 : UOP_CARRY_IN) | (done < n ? UOP_CARRY_OUT : 0);
      w[5] = c * 512;
      U.insert(U.end(), w, w + 8);
      second.push_back(0);
    } while (done < n);
  };
  const int n_fops = (int)fp.fops.size() / 8;
  for (int i = 0; i < n_fops; ++i) {
    const int32_t* w = &fp.fops[8 * (size_t)i];
    const int kind = w[0] & 0xFF;
    if (kind == FOP_VAR) { emit_var(&fp.psrcs[w[1]], w[2], w[3]); continue; }
    // a bundle: pre-chains of both members first (they touch slots disjoint from the partner's), then the members
    const int members = (w[0] & FOP_BUNDLED) ? 2 : 1;
    for (int m = 0; m < members; ++m) {
      const int32_t* q = &fp.fops[8 * (size_t)(i + m)];
      const int kd = q[0] & 0xFF;
      if ((kd == FOP_VAR_PAIR_TM || kd == FOP_VAR_PAIR_MT) && q[2] > 4) emit_var(&fp.psrcs[q[1]], q[2], q[3]);
    }
    for (int m = 0; m < members; ++m) {
      const int32_t* q = &fp.fops[8 * (size_t)(i + m)];
      const int kd = q[0] & 0xFF;
      int32_t u[8] = {0, ones, ones, ones, ones, -1, 0, 0};
      if (kd == FOP_PAIR_TM || kd == FOP_PAIR_MT) {
        u[0] = (kd == FOP_PAIR_MT ? UOP_MT : 0) | (q[1] << UOP_PSLOT_SHIFT) | (1 << UOP_NSRC_SHIFT);
        u[1] = q[2] * 512;
        u[6] = q[3] * 512;
      } else {
        const bool chained = q[2] > 4;
        const int n = chained ? 1 : q[2];
        u[0] = (kd == FOP_VAR_PAIR_MT ? UOP_MT : 0) | (q[4] << UOP_PSLOT_SHIFT) | (n << UOP_NSRC_SHIFT);
        if (chained) u[1] = q[3] * 512;
        else for (int k = 0; k < n; ++k) u[1 + k] = fp.psrcs[q[1] + k] * 512;
        u[5] = chained ? -1 : q[3] * 512;           // the variable->factor message itself (dropped below when dead)
        u[6] = q[5] * 512;
      }
      U.insert(U.end(), u, u + 8);
      second.push_back(m == 1);
    }
    i += members - 1;
  }
  const int n_uops = (int)U.size() / 8;
  // a fused variable->factor message is stored only when something reads the slot before its next write, or when it
  // is the slot's final value (the messages are an output of the call)
  for (int i = 0; i < n_uops; ++i) {
    int32_t* u = &U[8 * (size_t)i];
    if ((u[0] & UOP_VAR) || u[5] < 0) continue;
    const int c = u[5];
    bool needed = true;
    for (int j = i + 1; j < n_uops; ++j) {
      const int32_t* v = &U[8 * (size_t)j];
      const int n = (v[0] >> UOP_NSRC_SHIFT) & 15;
      bool reads = false;
      for (int k = 0; k < n; ++k) reads |= v[1 + k] == c;
      if (reads) break;
      const bool writes = v[5] == c || (!(v[0] & UOP_VAR) && v[6] == c);
      if (writes) { needed = false; break; }
    }
    if (!needed) u[5] = -1;
  }
  for (int i = 0; i < n_uops; ++i) {
    int32_t* u = &U[8 * (size_t)i];
    if (!(u[0] & UOP_VAR) && u[5] >= 0) u[0] |= UOP_STORE_VF;
    if (u[5] < 0) u[5] = 0;
  }
  std::vector<int32_t>& I = out.image;
  const int32_t nop[8] = {UOP_NOP, 0, 0, 0, 0, -1, 0, 0};
  for (int i = 0; i < n_uops; ++i) {
    I.insert(I.end(), U.begin() + 8 * (size_t)i, U.begin() + 8 * (size_t)i + 8);
    if (i + 1 < n_uops && second[i + 1]) { ++i; I.insert(I.end(), U.begin() + 8 * (size_t)i, U.begin() + 8 * (size_t)i + 8); }
    else I.insert(I.end(), nop, nop + 8);
  }
  out.n_bundles = (int)I.size() / 16;
  // per-wave hoist lists: entry h goes to wave h & 3
  const int n_hoist = (int)fp.hoist.size() / 2;
  out.HL = std::max(8, ((n_hoist + 3) / 4 + 7) / 8 * 8);
  {
    std::vector<int32_t> hl(4 * (size_t)out.HL * 2, -1);
    for (int h = 0; h < n_hoist; ++h) {
      hl[((size_t)(h & 3) * out.HL + (h >> 2)) * 2] = fp.hoist[2 * h];
      hl[((size_t)(h & 3) * out.HL + (h >> 2)) * 2 + 1] = fp.hoist[2 * h + 1];
    }
    I.insert(I.end(), hl.begin(), hl.end());
  }
  // constant-product lists, 16 words each, padded with the all-ones ext slot
  out.n_cprod = fp.n_cprod;
  out.cprods.clear();
  for (size_t at = 0; at < fp.cpw.size();) {
    const int cnt = fp.cpw[at];
    if (cnt > 15) { out.why = "a constant product of more than 15 messages"; out.image.clear(); return; }
    int32_t l[16];
    l[0] = cnt;
    for (int q = 0; q < 15; ++q) l[1 + q] = q < cnt ? fp.cpw[at + 1 + q] : ones / 512;
    I.insert(I.end(), l, l + 16);
    out.cprods.push_back(std::vector<int32_t>(fp.cpw.begin() + at + 1, fp.cpw.begin() + at + 1 + cnt));
    at += 1 + cnt;
  }
  out.hoisted.assign(n_msgs, 0);
  for (int h = 0; h < n_hoist; ++h) out.hoisted[fp.hoist[2 * h + 1]] = 1;
  // per-wave written-slot lists
  const int n_written = (int)fp.written.size();
  out.WL = std::max(4, ((n_written + 3) / 4 + 3) / 4 * 4);
  {
    std::vector<int32_t> wl(4 * (size_t)out.WL, -1);
    for (int i = 0; i < n_written; ++i) wl[(size_t)(i & 3) * out.WL + (i >> 2)] = fp.written[i];
    I.insert(I.end(), wl.begin(), wl.end());
  }
  for (int q = 0; q < 16; ++q) I.push_back(q == 0 || q == 8 ? UOP_NOP : 0);
  if (I.size() < 512) I.resize(512, 0);              // 2 KB at least: where the kernel's loads with nothing to fetch point (a table's 4 x 4 block spans 1.8 KB)
  out.ok = true;
}

// Read-out lists of the lean kernel: per variable 16 words -- count (base included), base slot (the variable's constant
// product, or the uniform vector), then the varying incoming slots.  False when a variable has more than 15 entries.
bool build_lean_readout(const LeanProgram& lp, int n_msgs, int n_vars, const int32_t* in_off, const int32_t* in_slots,
                        std::vector<int32_t>& image) {
  image.assign(16 * (size_t)n_vars, n_msgs);
  for (int v = 0; v < n_vars; ++v) {
    std::vector<int32_t> consts, vars;
    for (int q = in_off[v]; q < in_off[v + 1]; ++q) (lp.hoisted[in_slots[q]] ? consts : vars).push_back(in_slots[q]);
    int base = n_msgs;                               // the uniform vector
    if (!consts.empty()) {
      const int k = find_cprod(lp.cprods, consts);
      if (k >= 0) base = n_msgs + 1 + k;
      else vars.insert(vars.begin(), consts.begin(), consts.end());         // no matching product: multiply them in
    }
    if (vars.size() > 14) return false;
    int32_t* l = &image[16 * (size_t)v];
    l[0] = 1 + (int)vars.size();
    l[1] = base;
    const int ones = n_msgs + 1 + lp.n_cprod;
    for (int q = 0; q < 14; ++q) l[2 + q] = q < (int)vars.size() ? vars[q] : ones;
  }
  return true;
}

}  // namespace mlbp

extern "C" {

/* Host only: what the program rewrites make of an op list (no device needed). */
int mlbp_program_plan(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs, const int32_t* sweeps,
                      int32_t n_sweeps, int32_t n_msgs, int32_t P, int32_t U, int32_t* out8) {
  using namespace mlbp;
  if (!out8) return fail(MLBP_EINVAL, "mlbp_program_plan: out8 is NULL");
  if (int e = validate_program(ops, n_ops, srcs, n_srcs, sweeps, n_sweeps, n_msgs, P, U, nullptr)) return e;
  FusedProgram fp;
  build_fused_program(ops, srcs, sweeps, n_sweeps, n_msgs, fp);
  int lone = 0, fused = 0, bundled = 0;
  for (size_t i = 0; i < fp.fops.size(); i += 8) {
    const int k = fp.fops[i] & 0xFF;
    lone += k == FOP_VAR;
    fused += k == FOP_VAR_PAIR_TM || k == FOP_VAR_PAIR_MT;
    bundled += (fp.fops[i] & FOP_BUNDLED) != 0;
  }
  SharedProgram sp;
  build_shared_program(fp, n_msgs, P, U, sp);
  out8[0] = (int)fp.fops.size() / 8; out8[1] = lone; out8[2] = fused; out8[3] = bundled;
  out8[4] = (sp.ok ? 1 : 0) | (sp.ok && sp.pf_ok ? 2 : 0) | (sp.ok && sp.pf_ok && sp.vf_direct ? 4 : 0) | (sp.ok && sp.p3_ok ? 8 : 0); out8[5] = sp.n_live; out8[6] = sp.n_ops; out8[7] = sp.n_live * (64 * 16 + 64) * 8;
  return MLBP_OK;
}

/* Host only: the images the compilers make of an op list, serialised (include/mlbp.h gives the order of each). */
int mlbp_program_image(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs, const int32_t* sweeps,
                       int32_t n_sweeps, int32_t n_msgs, int32_t P, int32_t U, int32_t n_vars, const int32_t* in_off,
                       const int32_t* in_slots, int32_t which, int32_t* out, int32_t cap) {
  using namespace mlbp;
  if (cap < 0 || (cap > 0 && !out)) return fail(MLBP_EINVAL, "mlbp_program_image: bad output buffer");
  if (which < MLBP_IMAGE_FUSED || which > MLBP_IMAGE_PRUNED) return fail(MLBP_EINVAL, "mlbp_program_image: unknown image %d", which);
  if (int e = validate_program(ops, n_ops, srcs, n_srcs, sweeps, n_sweeps, n_msgs, P, U, nullptr)) return e;
  const bool readout = which == MLBP_IMAGE_LEAN_READOUT || which == MLBP_IMAGE_SHARED_READOUT;
  if (readout) {
    if (n_vars <= 0 || !in_off || !in_slots) return fail(MLBP_EINVAL, "mlbp_program_image: a read-out image needs n_vars, in_off and in_slots");
    if (in_off[0] != 0) return fail(MLBP_EINVAL, "in_off[0] must be 0");
    for (int v = 0; v < n_vars; ++v)
      if (in_off[v + 1] < in_off[v]) return fail(MLBP_EINVAL, "in_off must be non-decreasing");
    for (int q = 0; q < in_off[n_vars]; ++q)
      if (in_slots[q] < 0 || in_slots[q] >= n_msgs) return fail(MLBP_EINVAL, "in_slots[%d] = %d out of [0,%d)", q, in_slots[q], n_msgs);
  }
  std::vector<int32_t> w;
  auto scalar = [&](int64_t v) { w.push_back((int32_t)v); };
  auto vec = [&](const auto& v) { scalar((int64_t)v.size()); for (auto x : v) w.push_back((int32_t)x); };
  FusedProgram fp;
  build_fused_program(ops, srcs, sweeps, n_sweeps, n_msgs, fp);
  if (which == MLBP_IMAGE_FUSED) {
    vec(fp.fops); vec(fp.psrcs); vec(fp.fsweeps); vec(fp.hoist); vec(fp.cpw); vec(fp.pairseq); vec(fp.written);
    scalar(fp.n_cprod); scalar(fp.has_unary_fops);
  } else if (which == MLBP_IMAGE_LEAN || which == MLBP_IMAGE_LEAN_READOUT) {
    LeanProgram lp;
    build_lean_program(fp, n_msgs, lp);
    if (which == MLBP_IMAGE_LEAN) {
      scalar(lp.ok); scalar(lp.n_bundles); scalar(lp.HL); scalar(lp.n_cprod); scalar(lp.WL);
      vec(lp.image); vec(lp.hoisted);
      for (const auto& l : lp.cprods) vec(l);
    } else {
      std::vector<int32_t> img;
      const bool ok = lp.ok && build_lean_readout(lp, n_msgs, n_vars, in_off, in_slots, img);
      if (!ok) img.clear();
      scalar(ok); vec(img);
    }
  } else if (which == MLBP_IMAGE_SHARED || which == MLBP_IMAGE_SHARED_READOUT) {
    SharedProgram sp;
    build_shared_program(fp, n_msgs, P, U, sp);
    if (which == MLBP_IMAGE_SHARED) {
      scalar(sp.ok);
      if (!sp.ok) {
        scalar((int64_t)strlen(sp.why));
      } else {
        for (int v : {sp.n_ops, sp.n_live, sp.n_cpw, sp.n_back, sp.n_fill, sp.n_init, sp.n_bundles, sp.off_ent, sp.off_back, sp.off_fill,
                      sp.off_init, sp.off_ptile, sp.off_written, sp.max_sources, (int)sp.pf_ok, sp.off_pfb, sp.off_stash, sp.off_pinit,
                      sp.n_stash, sp.n_pinit, sp.off_vftile, (int)sp.vf_direct, (int)sp.p3_ok, sp.n_lds, sp.sqrt_mask, sp.off_map3,
                      sp.off_kind3, sp.off_back3})
          scalar(v);
        vec(sp.sweeps); vec(sp.image); vec(sp.live_of_slot); vec(sp.hoisted); vec(sp.written);
        for (const auto& l : sp.cprods) vec(l);
      }
    } else {
      std::vector<int32_t> img;
      const bool ok = sp.ok && build_shared_readout(sp, n_msgs, n_vars, in_off, in_slots, img);
      if (!ok) img.clear();
      scalar(ok); vec(img);
    }
  } else {
    std::vector<int32_t> ops2, sweeps2;
    const int dropped = drop_unchanged_updates(ops, srcs, sweeps, n_sweeps, n_msgs, ops2, sweeps2);
    vec(ops2); vec(sweeps2); scalar(dropped);
  }
  if ((int64_t)w.size() > INT32_MAX) return fail(MLBP_EINVAL, "mlbp_program_image: the image does not fit the return value");
  const size_t n = std::min(w.size(), (size_t)cap);
  if (n) memcpy(out, w.data(), n * sizeof(int32_t));
  return (int)w.size();
}

}  // extern "C"
