// The live-tile form of the fused program: what the shared-table X = 64 kernel (the matrix-core sweep kernel) reads.
//
// build_shared_program is a driver over the stages below, in order: hoisting checks, the two sequence rewrites, liveness and
// tile numbering, member records, uniform-start tiles and bundling, the general image sections, then the analysis and the
// sections of whichever product-fused form applies (PF: variables with at most two pairwise factors; P3: with three).  A stage
// that rules the program out leaves the reason in SharedProgram::why and the driver stops.
//
// Pure integer code, like mlbp_compile.cpp; pinned word for word by tests/golden/program_images.npz.
#include <algorithm>
#include <array>
#include <vector>

#include "mlbp_internal.h"

namespace mlbp {
namespace {

constexpr int NO_TILE = 0xFF;          // the "none" byte of a packed tile field

// Flag bits of a member record; the same bits in word 0 of every packed form (the kernels test them as literals).
enum {
  MF_CONTRACT = 1,       // a contraction (factor update)
  MF_MT = 2,             // m^T . T (else T . m)
  MF_KEEP = 4,           // the variable->factor product is kept as tile `ptile`
  MF_FINAL_VF = 8,       // the product is its slot's last value and goes straight to memory (message slot `pslot`)
  MF_VAR_ONLY = 16,      // variable update only, no contraction
  MF_LAST_WRITE = 32,    // PF / P3 records: the last update of the destination slot (raw result to the stash)
  MF_STORE = 64,         // PF / P3 records: store the product
  MF_SECOND_INPUT = 0x100,   // P3 records: a second input tile
  MF_NSRC_SHIFT = 8,     // general records: bits 8-11 = number of source tiles
  MF_PAIR_SHIFT = 16     // every record: the pair slot
};

// One update of the transformed sequence.  Bundles: two members that touch disjoint tiles share one barrier; the kernel runs
// them on different halves of its eight waves when their (table, orientation) pairs live in different halves (it decides:
// the tables are device data).  A default-constructed member is the empty slot of a bundle.
struct Member {
  int flags = 0;
  int n_src = 0;         // source tiles in use
  int pair = 0;          // pair slot
  int dst = -1;          // destination tile
  int ptile = -1;        // tile of the variable->factor product, or -1
  int pslot = 0;         // message slot of the product
  int src[8] = {-1, -1, -1, -1, -1, -1, -1, -1};   // source tiles (the first one -1: a message nothing has updated yet, i.e. the uniform vector)
  bool plain_pair = false;   // a factor update that reads a STORED variable->factor message
  int dst_written() const { return (flags & MF_CONTRACT) ? dst : -1; }
};

struct SharedBuild {
  std::vector<int32_t> fops;         // transformed op list, 8 words each
  std::vector<char> is_vf;           // [slots, ext included] some variable->factor update writes the slot
  std::vector<Member> mem;           // one per update
  std::vector<int32_t> init_tiles;   // tiles read before anything in the program has written them
  std::vector<int> pairing;          // per bundle: its members' indices (the second -1: alone)
  std::vector<int32_t> bundles;      // the general form's packed records
  std::vector<int32_t> back;         // write-back pairs {tile, slot | 0x40000000 for a variable->factor slot}
};

// Appends a section to the image; returns its offset.
int append(std::vector<int32_t>& image, const std::vector<int32_t>& section) {
  const int off = (int)image.size();
  image.insert(image.end(), section.begin(), section.end());
  return off;
}
int cprod_tile(const SharedProgram& out, int n_msgs, int k) { return out.live_of_slot[n_msgs + 1 + k]; }

// ---- stage 1: every unary message is a hoisted constant that some variable update folds in
bool check_hoisting(const FusedProgram& fp, int n_msgs, int P, int U, SharedProgram& out) {
  const int n_hoist = (int)fp.hoist.size() / 2;
  out.why = "unary messages are not all constant, or no / too many pairwise factors";
  if (fp.has_unary_fops || n_hoist != U || P < 1 || P > 16 || U > 64) return false;
  out.hoisted.assign(n_msgs, -1);
  for (int h = 0; h < n_hoist; ++h) out.hoisted[fp.hoist[2 * h + 1]] = fp.hoist[2 * h];
  out.why = "a unary message is folded into no variable update";
  std::vector<char> in_list(n_msgs, 0);
  size_t at = 0;
  for (int k = 0; k < fp.n_cprod; ++k) {
    const int cnt = fp.cpw[at];
    out.cprods.emplace_back(fp.cpw.begin() + at + 1, fp.cpw.begin() + at + 1 + cnt);
    for (int c : out.cprods.back()) {
      if (c < 0 || c >= n_msgs || out.hoisted[c] < 0) return false;
      in_list[c] = 1;
    }
    at += 1 + cnt;
  }
  for (int c = 0; c < n_msgs; ++c)
    if (out.hoisted[c] >= 0 && !in_list[c]) return false;     // a unary message no variable update folds in
  return true;
}

// ---- stage 2: sweep boundaries mean nothing to this kernel (it runs the updates in order), so the whole call is one
// sequence.  Two rewrites keep the variable->factor messages out of LDS:
//   1. a pairwise update whose input message c was produced by a variable->factor update whose own inputs
//      have not changed since RECOMPUTES c in registers (fused pair) instead of reading a stored tile --
//      the up pass of a loopy schedule (LBP.py:227-233) emits "X7->F17, X4->F14, F17->X1, F14->X1", and the
//      sweep that follows may read X4->F14 once more;
//   2. a lone variable->factor update whose output is rewritten later and not read before that is dropped.
// Both leave every stored value exactly what the original order computes.
std::vector<int32_t> rewrite_sequence(const FusedProgram& fp, SharedProgram& out) {
  std::vector<std::vector<int32_t>> seq;
  for (size_t sw = 0; sw + 1 < fp.fsweeps.size(); sw += 2)
    for (int i = fp.fsweeps[sw]; i < fp.fsweeps[sw] + fp.fsweeps[sw + 1]; ++i) {
      seq.emplace_back(fp.fops.begin() + 8 * (size_t)i, fp.fops.begin() + 8 * (size_t)i + 8);
      seq.back()[0] &= 0xFF;
    }
  auto is_pair = [](const std::vector<int32_t>& w) { return w[0] == FOP_PAIR_TM || w[0] == FOP_PAIR_MT; };
  auto writes = [&](const std::vector<int32_t>& w, int slot) {
    if (is_pair(w) || w[0] == FOP_VAR) return w[3] == slot;
    return w[3] == slot || w[5] == slot;
  };
  for (size_t j = 0; j < seq.size(); ++j) {
    if (!is_pair(seq[j])) continue;
    const int c = seq[j][2];
    int i = (int)j - 1;
    while (i >= 0 && !writes(seq[i], c)) --i;
    if (i < 0 || is_pair(seq[i]) || seq[i][3] != c) continue;               // never written, or not by a variable update
    const std::vector<int32_t> v = seq[i];
    bool legal = true;
    for (size_t k = i + 1; k < j && legal; ++k) {
      for (int q = 0; q < v[2] && legal; ++q) if (writes(seq[k], fp.psrcs[v[1] + q])) legal = false;
      for (int q = 0; q < v[7] && legal; ++q) if (writes(seq[k], fp.psrcs[v[6] + q])) legal = false;
    }
    if (!legal) continue;
    const std::vector<int32_t> pr = seq[j];
    seq[j] = {pr[0] == FOP_PAIR_TM ? FOP_VAR_PAIR_TM : FOP_VAR_PAIR_MT, v[1], v[2], c, pr[1], pr[3], v[6], v[7]};
  }
  for (size_t i = 0; i < seq.size();) {
    if (seq[i][0] != FOP_VAR) { ++i; continue; }
    const int c = seq[i][3];
    bool dead = false;
    for (size_t k = i + 1; k < seq.size(); ++k) {
      if (is_pair(seq[k]) && seq[k][2] == c) break;                          // still read from its tile
      if (writes(seq[k], c)) { dead = true; break; }
    }
    if (dead) seq.erase(seq.begin() + i);
    else ++i;
  }
  out.sweeps.push_back(0);
  out.sweeps.push_back((int)seq.size());
  std::vector<int32_t> fops;
  for (auto& w : seq) append(fops, w);
  return fops;
}

// ---- stage 3: which slots need a tile, and the tile numbering: constant products and factor->variable messages first, stored
// variable->factor messages (each read once, by a later pairwise update) last -- when LDS cannot hold every tile the tail lives
// in global memory (launcher: n_res resident tiles).  A factor update whose input nothing has written yet reads the initial
// uniform message and needs no tile: its source becomes -1.
bool number_tiles(const FusedProgram& fp, int n_msgs, SharedBuild& b, SharedProgram& out) {
  const int n_all = n_msgs + 1 + fp.n_cprod, n_ops = (int)b.fops.size() / 8;
  out.why = "unsupported update kind or slot use";
  std::vector<char> live(n_all, 0), written(n_msgs, 0);
  for (int i = 0; i < n_ops; ++i) {
    const int32_t* w = &b.fops[8 * i];
    const int kind = w[0] & 0xFF;
    if (kind == FOP_PAIR_TM || kind == FOP_PAIR_MT) {
      if (written[w[2]]) live[w[2]] = 1;
      else b.fops[8 * i + 2] = -1;
      live[w[3]] = 1; written[w[3]] = 1;
    } else if (kind == FOP_VAR || kind == FOP_VAR_PAIR_TM || kind == FOP_VAR_PAIR_MT) {
      for (int q = 0; q < w[2]; ++q) live[fp.psrcs[w[1] + q]] = 1;
      written[w[3]] = 1;
      if (kind != FOP_VAR) { live[w[5]] = 1; written[w[5]] = 1; }
    } else {
      return false;
    }
  }
  for (int c = 0; c < n_msgs; ++c)
    if (out.hoisted[c] >= 0 && (live[c] || written[c])) return false;
  out.written = written;
  out.live_of_slot.assign(n_all, -1);
  b.is_vf.assign(n_all, 0);
  for (int i = 0; i < n_ops; ++i)
    if ((b.fops[8 * i] & 0xFF) >= FOP_VAR) b.is_vf[b.fops[8 * i + 3]] = 1;
  for (int pass = 0; pass < 2; ++pass)
    for (int s = 0; s < n_all; ++s)
      if (live[s] && (b.is_vf[s] ? 1 : 0) == pass) out.live_of_slot[s] = out.n_live++;
  out.why = "more than 254 live tiles or 65535 message slots";
  return out.n_live <= 254 && n_msgs <= 65535;
}

// ---- stage 4: one member record per update
bool make_members(const FusedProgram& fp, int n_msgs, SharedBuild& b, SharedProgram& out) {
  const int n_ops = (int)b.fops.size() / 8;
  b.mem.assign(n_ops, Member());
  std::vector<int> last_var_write(n_msgs, -1);
  out.why = "a variable update multiplies more than 8 tiles";
  for (int i = 0; i < n_ops; ++i) {
    const int32_t* w = &b.fops[8 * i];
    Member& m = b.mem[i];
    const int kind = w[0] & 0xFF;
    if (kind == FOP_PAIR_TM || kind == FOP_PAIR_MT) {
      m.flags = MF_CONTRACT | (kind == FOP_PAIR_MT ? MF_MT : 0);
      m.n_src = 1;
      m.plain_pair = true;
      m.pair = w[1]; m.dst = out.live_of_slot[w[3]];
      m.src[0] = w[2] < 0 ? -1 : out.live_of_slot[w[2]];
    } else {
      if (w[2] > 8 || w[2] < 1) return false;
      out.max_sources = std::max(out.max_sources, (int)w[2]);
      m.n_src = w[2];
      for (int q = 0; q < w[2]; ++q) m.src[q] = out.live_of_slot[fp.psrcs[w[1] + q]];
      m.flags = kind == FOP_VAR ? MF_VAR_ONLY : (MF_CONTRACT | (kind == FOP_VAR_PAIR_MT ? MF_MT : 0));
      m.ptile = out.live_of_slot[w[3]]; m.pslot = w[3];
      if (m.ptile >= 0) m.flags |= MF_KEEP;
      else last_var_write[w[3]] = i;
      if (kind != FOP_VAR) { m.pair = w[4]; m.dst = out.live_of_slot[w[5]]; }
    }
  }
  for (int c = 0; c < n_msgs; ++c)
    if (last_var_write[c] >= 0) b.mem[last_var_write[c]].flags |= MF_FINAL_VF;      // write this v->f message out here
  return true;
}

// general device form, 4 words: [0] flags | nsrc << 8 | pair slot << 16   [1] destination tile | product tile << 8 (0xFF = none) |
// message slot of the product << 16   [2] source tiles 0-3, [3] 4-7, one byte each (0xFF = none)
void pack_member(const Member& m, std::vector<int32_t>& bundles) {
  int32_t w[4] = {0, 0, 0, 0};
  w[0] = m.flags | (m.n_src << MF_NSRC_SHIFT) | (m.pair << MF_PAIR_SHIFT);
  w[1] = (m.dst & 0xFF) | ((m.ptile & 0xFF) << 8) | (m.pslot << 16);
  for (int q = 0; q < 8; ++q) w[2 + (q >> 2)] |= (m.src[q] & 0xFF) << (8 * (q & 3));
  bundles.insert(bundles.end(), w, w + 4);
}

// ---- stage 5: tiles read before anything in the program has written them start as the uniform vector (FactorGraph.initialize);
// then adjacent members that touch disjoint tiles are paired into bundles
void bundle_members(const FusedProgram& fp, int n_msgs, SharedBuild& b, SharedProgram& out) {
  const int n_ops = (int)b.mem.size();
  std::vector<char> have(out.n_live, 0);
  for (int k = 0; k < fp.n_cprod; ++k)
    if (cprod_tile(out, n_msgs, k) >= 0) have[cprod_tile(out, n_msgs, k)] = 1;        // written by the prologue (no tile: ruled out in general_sections)
  for (const Member& m : b.mem) {
    for (int q = 0; q < m.n_src; ++q)
      if (m.src[q] >= 0 && !have[m.src[q]]) { have[m.src[q]] = 1; b.init_tiles.push_back(m.src[q]); }
    if (m.dst >= 0) have[m.dst] = 1;
    if (m.ptile >= 0) have[m.ptile] = 1;
  }
  auto disjoint = [&](const Member& x, const Member& y) {
    // y reads nothing x writes, and writes nothing x reads or writes
    auto writes = [](const Member& m, int tile) { return tile >= 0 && (m.dst == tile || m.ptile == tile); };
    for (int q = 0; q < 8; ++q) if (writes(x, y.src[q]) || writes(y, x.src[q])) return false;
    return !(writes(x, y.dst) || writes(x, y.ptile));
  };
  for (int i = 0; i < n_ops;) {
    const bool two = i + 1 < n_ops && disjoint(b.mem[i], b.mem[i + 1]);
    pack_member(b.mem[i], b.bundles);
    pack_member(two ? b.mem[i + 1] : Member(), b.bundles);
    b.pairing.push_back(i); b.pairing.push_back(two ? i + 1 : -1);
    i += two ? 2 : 1;
  }
  out.n_bundles = (int)b.bundles.size() / 8;
  pack_member(Member(), b.bundles); pack_member(Member(), b.bundles);       // the kernel prefetches one bundle past the end
}

// ---- stage 6: the sections every form reads.
// device image: bundles [n_bundles + 1][2][4] | cprod entries | write-back pairs | fill slots | uniform tiles | product tiles | written bits
bool general_sections(const FusedProgram& fp, int n_msgs, SharedBuild& b, SharedProgram& out) {
  // constant products, flattened: {unary factor, message slot, tile, 1 = first | 2 = last of its product}
  std::vector<int32_t> ent, fill;
  out.why = "unsupported update kind or slot use";
  for (int k = 0; k < fp.n_cprod; ++k) {
    const int tile = cprod_tile(out, n_msgs, k);
    if (tile < 0 || out.cprods[k].empty()) return false;
    for (size_t q = 0; q < out.cprods[k].size(); ++q) {
      const int c = out.cprods[k][q];
      ent.insert(ent.end(), {out.hoisted[c], c, tile, (q == 0 ? 1 : 0) | (q + 1 == out.cprods[k].size() ? 2 : 0)});
    }
  }
  for (int c = 0; c < n_msgs; ++c) {
    if (out.hoisted[c] >= 0) continue;
    if (out.written[c] && out.live_of_slot[c] >= 0) { b.back.push_back(out.live_of_slot[c]); b.back.push_back(c | (b.is_vf[c] ? 0x40000000 : 0)); }
    else if (!out.written[c]) fill.push_back(c);
  }
  out.n_ops = (int)b.mem.size(); out.n_cpw = (int)ent.size();
  out.n_back = (int)b.back.size() / 2; out.n_fill = (int)fill.size(); out.n_init = (int)b.init_tiles.size();
  out.image = b.bundles;
  out.off_ent = append(out.image, ent);
  out.off_back = append(out.image, b.back);
  out.off_fill = append(out.image, fill);
  out.off_init = append(out.image, b.init_tiles);
  out.off_ptile = (int)out.image.size();                         // tile of constant product k
  for (int k = 0; k < fp.n_cprod; ++k) out.image.push_back(cprod_tile(out, n_msgs, k));
  out.off_written = (int)out.image.size();                       // bit c: some update of the program writes slot c
  for (int c0 = 0; c0 < n_msgs; c0 += 32) {
    uint32_t w = 0;
    for (int c = c0; c < n_msgs && c < c0 + 32; ++c) w |= (out.written[c] ? 1u : 0u) << (c - c0);
    out.image.push_back((int32_t)w);
  }
  out.image.resize(out.image.size() + 16, 0);
  return true;
}

// ---- stage 7: the product-fused forms.  What PF and P3 share: the constant-tile maps, the tile a member reads when its input is
// still the uniform vector, the prologue's fill list, stash numbering and the flag logic of their records.  Each form keeps its
// own classification rule (which fills cp, last_writer and the members' inputs) and its own packer.
struct FusedAnalysis {
  std::vector<char> is_c;            // [n_live] the tile holds a constant product
  std::vector<int> prod_of_tile;     // [n_live] ... which one, or -1
  std::vector<int> cp;               // [n_live] TILE of the constant product a message tile is read with (< 0: none)
  std::vector<int> last_writer;      // [n_live] the last member whose contraction writes the tile, or -1
  std::vector<int> s1, s2;           // per member: its input tile(s), or NO_TILE
  std::vector<int32_t> uinit;        // tiles the prologue fills with the uniform vector
  FusedAnalysis(const FusedProgram& fp, int n_msgs, int n_ops, const SharedProgram& out, int cp_start)
      : is_c(out.n_live, 0), prod_of_tile(out.n_live, -1), cp(out.n_live, cp_start), last_writer(out.n_live, -1),
        s1(n_ops, NO_TILE), s2(n_ops, NO_TILE) {
    for (int k = 0; k < fp.n_cprod; ++k) { is_c[cprod_tile(out, n_msgs, k)] = 1; prod_of_tile[cprod_tile(out, n_msgs, k)] = k; }
  }
};

// A member whose input is still the uniform vector (s1 == NO_TILE) reads a message tile that nothing touches before a later
// bundle writes it; the prologue fills those tiles (uinit).  touch[i]: the tiles member i reads or writes (-1: unused entry).
// False when some member finds no such tile.
bool pick_uniform_inputs(const SharedBuild& b, const std::vector<std::array<int, 4>>& touch, FusedAnalysis& a) {
  const int n_ops = (int)b.mem.size(), n_live = (int)a.is_c.size();
  std::vector<int> bundle_of(n_ops, 0), first_touch(n_live, n_ops + 1);
  for (size_t p = 0; p < b.pairing.size(); p += 2) {
    bundle_of[b.pairing[p]] = (int)p / 2;
    if (b.pairing[p + 1] >= 0) bundle_of[b.pairing[p + 1]] = (int)p / 2;
  }
  for (int i = n_ops - 1; i >= 0; --i)
    for (int tl : touch[i])
      if (tl >= 0) first_touch[tl] = bundle_of[i];
  for (int q : b.init_tiles) first_touch[q] = -1;              // (holds c (.) uniform from the start)
  for (int i = 0; i < n_ops; ++i) {
    if (a.s1[i] != NO_TILE) continue;
    int pick = -1;
    for (int tl = 0; tl < n_live && pick < 0; ++tl)
      if (!a.is_c[tl] && first_touch[tl] > bundle_of[i]) pick = tl;
    if (pick < 0) return false;
    a.s1[i] = pick;
    if (std::find(a.uinit.begin(), a.uinit.end(), pick) == a.uinit.end()) a.uinit.push_back(pick);
  }
  return true;
}

// stash [n_index]: where the raw result of the last update of a tile goes; pinit: {tile, constant product or -1} the prologue
// fills -- the uniform-input tiles, then the message tiles read before the program writes them (c (.) uniform, i.e. a copy of the
// constant product, or uniform).  index_of: the records' numbering of a live tile.
void number_stash_and_pinit(const SharedBuild& b, const FusedAnalysis& a, const std::vector<int>& index_of, int n_index,
                            SharedProgram& out, std::vector<int32_t>& stash, std::vector<int32_t>& pinit) {
  stash.assign(n_index, -1);
  out.n_stash = 0;
  for (size_t tl = 0; tl < a.is_c.size(); ++tl)
    if (!a.is_c[tl] && a.last_writer[tl] >= 0) stash[index_of[tl]] = out.n_stash++;
  for (int tl : a.uinit) { pinit.push_back(index_of[tl]); pinit.push_back(-1); }
  for (int tl : b.init_tiles) {
    if (a.is_c[tl]) continue;
    pinit.push_back(index_of[tl]); pinit.push_back(a.cp[tl] >= 0 ? a.prod_of_tile[a.cp[tl]] : -1);
  }
  out.n_pinit = (int)pinit.size() / 2;
}

// word 0 of a PF / P3 record: the member's own flags among `keep`, the pair slot, and what the destination needs
int32_t fused_flags(const Member& m, int i, const FusedAnalysis& a, int keep) {
  const int dst = m.dst_written();
  int32_t w = (m.flags & keep) | (m.pair << MF_PAIR_SHIFT);
  if (dst >= 0 && a.last_writer[dst] == i) w |= MF_LAST_WRITE;
  if (dst >= 0) w |= MF_STORE;                              // (a slot nothing reads as an input is kept for the read-out: the raw result, c absent)
  return w;
}

// ---- product-fused form.  When every variable update of the program multiplies at most one constant product and one
// factor->variable message (variables with at most two pairwise factors: K2, K3, chains, rings), the message F->X is only
// ever read as the product  c_X (.) m_{F->X}  (LBP.py:377-389).  The PRODUCER then stores that product -- its 16 rows of the
// D fragment times its 16 rows of c_X: four multiplications -- and every contraction reads ONE tile straight into the matrix
// cores: no products, half the tile reads, and (float64 vector operations share the matrix cores' pipe) some fifty
// operations per update off the dependent chain.  The raw result of the LAST update of each slot goes to a scratch tile
// in memory for the read-out.  Member record, 4 words:
//   [0] flags | pair slot << 16: 1 contraction, 2 m^T.T, 8 the input S, normalised, is this variable->factor slot's last value:
//       to memory, 16 no contraction, 32 last update of the destination slot: raw result to stash [2] >> 8 (when the call writes
//       the messages back), 64 store the product
//   [1] destination tile | S tile << 8 (0xFF: the uniform vector) | message slot of S << 16   [2] constant-product tile the
//       result is multiplied by (0xFF none) | stash index << 8
// Classification: cp = -2 never read, -1 read without a constant product.
bool classify_pf(const SharedBuild& b, const SharedProgram& out, FusedAnalysis& a) {
  if (out.max_sources > 2) return false;
  const int n_ops = (int)b.mem.size();
  std::vector<std::array<int, 4>> touch(n_ops, {-1, -1, -1, -1});
  for (int i = 0; i < n_ops; ++i) {
    const Member& m = b.mem[i];
    if (m.flags & MF_KEEP) return false;                        // a variable->factor message kept as a tile of its own
    int c = -1, mt = -1, nc = 0, nm = 0;
    for (int q = 0; q < m.n_src; ++q) {
      const int tl = m.src[q];
      if (tl < 0) continue;
      if (a.is_c[tl]) { c = tl; ++nc; } else { mt = tl; ++nm; }
    }
    if (nc > 1 || nm > 1) return false;
    if (nm) {
      if (a.cp[mt] == -2) a.cp[mt] = c; else if (a.cp[mt] != c) return false;
      a.s1[i] = mt;
    } else if (nc) {
      a.s1[i] = c;
    }
    if (m.dst_written() >= 0) { if (a.is_c[m.dst]) return false; a.last_writer[m.dst] = i; }
    touch[i] = {m.dst_written(), a.s1[i] != NO_TILE ? a.s1[i] : -1, -1, -1};
  }
  // every stored product needs its constant product (a variable without unary factors: the general form), and a member whose
  // input is still the uniform vector reads a tile nothing touches before a later bundle writes it, filled by the prologue
  for (int tl = 0; tl < out.n_live; ++tl)
    if (!a.is_c[tl] && a.cp[tl] == -1) return false;
  return pick_uniform_inputs(b, touch, a);
}

void pf_sections(int n_msgs, const SharedBuild& b, const FusedAnalysis& a, SharedProgram& out) {
  const int n_ops = (int)b.mem.size();
  std::vector<int> identity(out.n_live);
  for (int tl = 0; tl < out.n_live; ++tl) identity[tl] = tl;
  std::vector<int32_t> stash, pfb, pinit;
  number_stash_and_pinit(b, a, identity, out.n_live, out, stash, pinit);
  auto pack_pf = [&](int i) {
    int32_t w[4] = {0, 0xFFFF, 0xFF, 0};
    if (i >= 0) {
      const Member& m = b.mem[i];
      const int dst = m.dst_written();
      w[0] = fused_flags(m, i, a, MF_CONTRACT | MF_MT | MF_FINAL_VF | MF_VAR_ONLY);
      w[1] = (dst & 0xFF) | ((a.s1[i] & 0xFF) << 8) | (m.pslot << 16);
      w[2] = ((dst >= 0 && a.cp[dst] >= 0 ? a.cp[dst] : NO_TILE) & 0xFF) | ((dst >= 0 ? stash[dst] : 0) << 8);
    }
    pfb.insert(pfb.end(), w, w + 4);
  };
  for (int i : b.pairing) pack_pf(i);
  pack_pf(-1); pack_pf(-1);
  // The gradient epilogue takes a factor's two variable->factor messages straight from LDS when every such slot's last value
  // (the input S of its flag-8 member) is a message tile no later member rewrites: vftile[slot] = that tile, -1 = never updated
  // (uniform), and the form is off (vf_direct false) when some slot has no such tile or its S is a constant-product tile (the
  // read-out stages the marginals there).
  std::vector<int32_t> vftile(n_msgs, -1);
  out.vf_direct = true;
  for (int i = 0; i < n_ops && out.vf_direct; ++i) {
    if (!(b.mem[i].flags & MF_FINAL_VF)) continue;
    const int tl = a.s1[i];
    bool intact = tl != NO_TILE && !a.is_c[tl];
    for (int j = i; j < n_ops && intact; ++j)                   // (member i itself included: its own result must land elsewhere)
      if (b.mem[j].dst_written() == tl) intact = false;
    if (!intact) out.vf_direct = false;
    else vftile[b.mem[i].pslot] = tl;
  }
  for (int c = 0; c < n_msgs && out.vf_direct; ++c)
    if (out.hoisted[c] < 0 && b.is_vf[c] && vftile[c] < 0) out.vf_direct = false;      // (a slot some variable update writes but no flag-8 member hands out)
  out.off_pfb = append(out.image, pfb);
  out.off_stash = append(out.image, stash);
  for (int tl = 0; tl < out.n_live; ++tl) out.image.push_back(a.cp[tl] >= 0 ? 1 : 0);       // [n_live] behind it: the tile holds c (.) message (else the message)
  out.off_pinit = append(out.image, pinit);
  out.off_vftile = append(out.image, vftile);
  out.image.resize(out.image.size() + 16, 0);
}

// ---- product-fused form, variables with THREE pairwise factors (K4 cliques: every variable update multiplies the constant
// product c and two factor->variable messages).  The producer of a message into such a variable stores  sqrt(c) (.) m  (the
// prepare kernel writes sqrt(c) for these products): the input of a contraction is then the PRODUCT OF TWO TILES,
// sqrt(c) m_a (.) sqrt(c) m_b = c (.) m_a (.) m_b -- two tile reads and one multiplication per element instead of three reads
// and two, and 12 message tiles + the stored variable->factor messages instead of 21 tiles: everything stays in LDS (one
// workgroup per CU; the constant products themselves stay in memory: a producer asks for its sixteen rows of them in front of
// its matrix instructions).  A variable with two pairwise factors in the same program keeps the c (.) m form above (the
// exponent is per constant product: sqrt_mask).  Stored variable->factor messages (members with flag 4, read by a later
// plain factor update) are raw tiles.  Record, 4 words:
//   [0] flags | pair slot << 16: as above, and 4 the input product is kept as tile [3] >> 8, 0x100 a second input tile [3] & 0xFF
//   [1] destination | input tile << 8 | message slot of the input product << 16      (tiles: LDS indices, the constant products left out)
//   [2] constant PRODUCT INDEX the result is multiplied by (0xFF none) | stash index << 8      [3] second input | kept tile << 8
// Sections: map3 [n_live] LDS index of a tile (0x100 | product index for a constant product), kind3 [n_lds] 0 raw / 1 c (.) m /
// 2 sqrt(c) (.) m, | 0x100 some update writes it; stash [n_lds]; back3 [n_back][2] the write-back list in LDS indices.
// Classification: kind[tile] = -2 not seen, 0 raw, 1 / 2 read as one of so many messages; ckind the same per constant-product tile.
bool classify_p3(const SharedBuild& b, FusedAnalysis& a, std::vector<int>& kind, std::vector<int>& ckind) {
  const int n_ops = (int)b.mem.size();
  auto raw = [&](int tl) {                                      // the tile holds a raw message (and nothing says otherwise)
    if (tl < 0 || a.is_c[tl] || (kind[tl] != -2 && kind[tl] != 0)) return false;
    kind[tl] = 0;
    return true;
  };
  std::vector<std::array<int, 4>> touch(n_ops, {-1, -1, -1, -1});
  for (int i = 0; i < n_ops; ++i) {
    const Member& m = b.mem[i];
    if (m.plain_pair) {
      if (m.src[0] >= 0) { if (!raw(m.src[0])) return false; a.s1[i] = m.src[0]; }
    } else {
      int c = -1, nc = 0, nm = 0, mt[2] = {-1, -1};
      for (int q = 0; q < m.n_src; ++q) {
        const int tl = m.src[q];
        if (tl < 0) return false;
        if (a.is_c[tl]) { c = tl; ++nc; }
        else if (nm < 2) mt[nm++] = tl;
        else return false;
      }
      if (nc != 1 || nm < 1) return false;
      for (int q = 0; q < nm; ++q) {
        if (kind[mt[q]] == -2) { kind[mt[q]] = nm; a.cp[mt[q]] = c; }
        else if (kind[mt[q]] != nm || a.cp[mt[q]] != c) return false;
      }
      if (ckind[c] == 0) ckind[c] = nm; else if (ckind[c] != nm) return false;
      a.s1[i] = mt[0]; a.s2[i] = nm == 2 ? mt[1] : NO_TILE;
      if ((m.flags & MF_KEEP) && !raw(m.ptile)) return false;
    }
    if (m.dst_written() >= 0) { if (a.is_c[m.dst]) return false; a.last_writer[m.dst] = i; }
    touch[i] = {m.dst_written(), (m.flags & MF_KEEP) ? m.ptile : -1, a.s1[i] != NO_TILE ? a.s1[i] : -1, a.s2[i] != NO_TILE ? a.s2[i] : -1};
  }
  return pick_uniform_inputs(b, touch, a);       // (only a plain factor update whose input nothing has written yet)
}

void p3_sections(const SharedBuild& b, const FusedAnalysis& a, const std::vector<int>& kind, const std::vector<int>& ckind, SharedProgram& out) {
  const int NL = out.n_live;
  std::vector<int> lds_of(NL, -1);
  out.n_lds = 0;
  for (int tl = 0; tl < NL; ++tl) if (!a.is_c[tl]) lds_of[tl] = out.n_lds++;
  out.sqrt_mask = 0;
  for (int tl = 0; tl < NL; ++tl) if (a.is_c[tl] && ckind[tl] == 2) out.sqrt_mask |= 1 << a.prod_of_tile[tl];
  std::vector<int32_t> stash, pfb, pinit, map3(NL, 0), kind3(out.n_lds, 0), back3;
  number_stash_and_pinit(b, a, lds_of, out.n_lds, out, stash, pinit);
  for (int tl = 0; tl < NL; ++tl) {
    map3[tl] = a.is_c[tl] ? (0x100 | a.prod_of_tile[tl]) : lds_of[tl];
    if (!a.is_c[tl]) kind3[lds_of[tl]] = std::max(kind[tl], 0) | (a.last_writer[tl] >= 0 ? 0x100 : 0);
  }
  auto pack3 = [&](int i) {
    int32_t w[4] = {0, 0xFFFF, 0xFF, 0xFFFF};
    if (i >= 0) {
      const Member& m = b.mem[i];
      const int dst = m.dst_written();
      w[0] = fused_flags(m, i, a, MF_CONTRACT | MF_MT | MF_KEEP | MF_FINAL_VF | MF_VAR_ONLY);
      if (a.s2[i] != NO_TILE) w[0] |= MF_SECOND_INPUT;
      w[1] = ((dst >= 0 ? lds_of[dst] : NO_TILE) & 0xFF) | ((lds_of[a.s1[i]] & 0xFF) << 8) | (m.pslot << 16);
      w[2] = ((dst >= 0 && a.cp[dst] >= 0 ? a.prod_of_tile[a.cp[dst]] : NO_TILE) & 0xFF) | ((dst >= 0 ? stash[lds_of[dst]] : 0) << 8);
      w[3] = ((a.s2[i] != NO_TILE ? lds_of[a.s2[i]] : NO_TILE) & 0xFF) | ((((m.flags & MF_KEEP) ? lds_of[m.ptile] : NO_TILE) & 0xFF) << 8);
    }
    pfb.insert(pfb.end(), w, w + 4);
  };
  for (int i : b.pairing) pack3(i);
  pack3(-1); pack3(-1);
  for (size_t q = 0; q + 1 < b.back.size(); q += 2) { back3.push_back(lds_of[b.back[q]]); back3.push_back(b.back[q + 1]); }
  out.vf_direct = false;
  out.off_pfb = append(out.image, pfb);
  out.off_stash = append(out.image, stash);
  out.off_pinit = append(out.image, pinit);
  out.off_map3 = append(out.image, map3);
  out.off_kind3 = append(out.image, kind3);
  out.off_back3 = append(out.image, back3);
  out.image.resize(out.image.size() + 16, 0);
}

}  // namespace

void build_shared_program(const FusedProgram& fp, int n_msgs, int P, int U, SharedProgram& out) {
  out = SharedProgram();
  if (!check_hoisting(fp, n_msgs, P, U, out)) return;
  SharedBuild b;
  b.fops = rewrite_sequence(fp, out);
  if (!number_tiles(fp, n_msgs, b, out)) return;
  if (!make_members(fp, n_msgs, b, out)) return;
  bundle_members(fp, n_msgs, b, out);
  if (!general_sections(fp, n_msgs, b, out)) return;
  const int n_ops = (int)b.mem.size();
  FusedAnalysis pf(fp, n_msgs, n_ops, out, -2);
  out.pf_ok = classify_pf(b, out, pf);
  if (out.pf_ok) {
    pf_sections(n_msgs, b, pf, out);
  } else if (out.max_sources == 3) {
    FusedAnalysis p3(fp, n_msgs, n_ops, out, -1);
    std::vector<int> kind(out.n_live, -2), ckind(out.n_live, 0);
    out.p3_ok = classify_p3(b, p3, kind, ckind);
    if (out.p3_ok) p3_sections(b, p3, kind, ckind, out);
  }
  out.why = "";
  out.ok = true;
}

bool build_shared_readout(const SharedProgram& sp, int n_msgs, int n_vars, const int32_t* in_off, const int32_t* in_slots,
                          std::vector<int32_t>& image) {
  // layout: offset of variable v's list [n_vars], then per variable {base tile or -1, n, tiles...}
  image.assign(n_vars, 0);
  while (image.size() % 4) image.push_back(0);
  for (int v = 0; v < n_vars; ++v) {
    std::vector<int32_t> consts, tiles;
    for (int q = in_off[v]; q < in_off[v + 1]; ++q) {
      const int c = in_slots[q];
      if (sp.hoisted[c] >= 0) consts.push_back(c);
      else if (sp.live_of_slot[c] >= 0) tiles.push_back(sp.live_of_slot[c]);
      else if (sp.written[c]) return false;            // written but not resident: not an incoming message we can read
      // else: never read and never written inside the sweeps -> still uniform, cancels in the normalisation
    }
    int base = -1;
    if (!consts.empty()) {
      const int k = find_cprod(sp.cprods, consts);
      if (k >= 0) base = sp.live_of_slot[n_msgs + 1 + k];
      if (base < 0) return false;
    }
    image[v] = (int)image.size();
    image.push_back(base);
    image.push_back((int)tiles.size());
    image.insert(image.end(), tiles.begin(), tiles.end());
    while (image.size() % 4) image.push_back(0);
  }
  return true;
}

}  // namespace mlbp
