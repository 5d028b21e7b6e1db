"""NumPy float64 interpreters of the integer images the sweep-program compilers emit (csrc/mlbp_compile.cpp), and the seeded
family of random program cases that tests/test_image_semantics_cpu.py and tests/test_gpu_random_programs.py share.

tests/test_program_images.py pins every word of the images; this module says what the words MEAN: each interpreter runs one
image on a graph's tables and returns the messages [n_msgs][X] and the marginals [n_vars][X], to be held against the oracle's
walk of the same graph.  Plain, slow code over the documented layouts only -- include/mlbp.h at MLBP_IMAGE_*, csrc/mlbp_uop.h,
the comments above build_lean_program and the fused passes of mlbp_compile.cpp, and what sweep_x64_fused_kernel and
mlbp_lean_device.h read:

  run_ops      the plain 4-word op list (what compile_program returns, and the pruned list of MLBP_IMAGE_PRUNED)
  run_pruned   MLBP_IMAGE_PRUNED: its op list and sweep table
  run_fused    MLBP_IMAGE_FUSED: fops, psrcs, fsweeps, hoist, cpw, pairseq, written; a variable update through its fast list
               (base slot first) or its exact list; bundled pairs read the state from before either writes
  run_lean     MLBP_IMAGE_LEAN + MLBP_IMAGE_LEAN_READOUT: bundles of two micro-ops, carry links, hoist / constant-product /
               written-slot lists per wave, the ext slots (uniform, constant products, ones), the read-out lists

Operands of the lean image are LDS byte offsets slot * 512 whatever X is: the images are the X = 64 ones, their meaning does
not depend on X, and the CPU tests run them at X = 5.  Every contraction and every hoisted unary message is normalised as the
oracle normalises it; the lean kernel's stored variable products are raw and are normalised by the final pass over the
written-slot lists, and only listed slots (hoisted or written) go back: an unlisted slot keeps its start value (uniform under
init).  The kernels' scale bookkeeping, their bail flags and nan_to_num are device behaviour and not modelled: inputs here are
positive.

NOT interpreted: the shared-table image (MLBP_IMAGE_SHARED / MLBP_IMAGE_SHARED_READOUT, csrc/mlbp_compile_shared.cpp) with its
general, PF and P3 forms.  It still has no CPU semantics; only its words are pinned, and GPU tests check what they compute.
"""
import copy

import numpy as np

OP_UNARY, OP_PAIR_TM, OP_PAIR_MT, OP_VAR = 0, 1, 2, 3                                    # include/mlbp.h MLBP_OP_*
FOP_UNARY, FOP_PAIR_TM, FOP_PAIR_MT, FOP_VAR, FOP_VAR_PAIR_TM, FOP_VAR_PAIR_MT, FOP_BUNDLED = 0, 1, 2, 3, 4, 5, 0x100
UOP_VAR, UOP_MT, UOP_PSLOT_SHIFT, UOP_NOP, UOP_STORE_VF, UOP_NSRC_SHIFT, UOP_CARRY_IN, UOP_CARRY_OUT = 1, 2, 2, 32, 64, 8, 0x1000, 0x2000
SLOT_BYTES = 512


# ---------------------------------------------------------------------------------------------------------------------------
# the serialisations of mlbp_program_image: a scalar is one word, a vector its length and then its words
# ---------------------------------------------------------------------------------------------------------------------------
class _Words:
    def __init__(self, w):
        self.w, self.at = np.asarray(w, dtype=np.int64), 0

    def scalar(self):
        self.at += 1
        return int(self.w[self.at - 1])

    def vec(self):
        n = self.scalar()
        self.at += n
        assert self.at <= len(self.w)
        return self.w[self.at - n:self.at]

    def done(self):
        assert self.at == len(self.w), (self.at, len(self.w))


def parse_fused(words):
    r = _Words(words)
    out = {k: r.vec() for k in ('fops', 'psrcs', 'fsweeps', 'hoist', 'cpw', 'pairseq', 'written')}
    out['n_cprod'], out['has_unary_fops'] = r.scalar(), r.scalar()
    r.done()
    out['fops'] = out['fops'].reshape(-1, 8)
    return out


def parse_lean(words):
    r = _Words(words)
    out = {k: r.scalar() for k in ('ok', 'n_bundles', 'HL', 'n_cprod', 'WL')}
    out['image'], out['hoisted'] = r.vec(), r.vec()
    out['cprods'] = [r.vec() for _ in range(out['n_cprod'])] if out['ok'] else []
    r.done()
    if out['ok']:
        img, nb, HL, nc, WL = out['image'], out['n_bundles'], out['HL'], out['n_cprod'], out['WL']
        at = 16 * nb
        out['bundles'] = img[:at].reshape(nb, 16)
        out['hoist_lists'] = img[at:at + 8 * HL].reshape(4, HL, 2)
        at += 8 * HL
        out['cprod_lists'] = img[at:at + 16 * nc].reshape(nc, 16)
        at += 16 * nc
        out['written_lists'] = img[at:at + 4 * WL].reshape(4, WL)
        at += 4 * WL
        out['pad'] = img[at:]
    return out


def parse_readout(words):
    r = _Words(words)
    ok, img = r.scalar(), r.vec()
    r.done()
    return ok, img.reshape(-1, 16)


def parse_pruned(words):
    r = _Words(words)
    ops, sweeps, dropped = r.vec().reshape(-1, 4), r.vec().reshape(-1, 2), r.scalar()
    r.done()
    return ops, sweeps, dropped


# ---------------------------------------------------------------------------------------------------------------------------
# arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def _norm(v):
    """Message.renormalize: a positive total -> divide by it, else uniform."""
    s = v.sum()
    return v / s if s > 0 else np.full_like(v, 1.0 / v.size)


def _contract(T, m, mt):
    return m.dot(T) if mt else T.dot(m)


def _start(start, init, n_msgs, X):
    if init:
        return np.full((n_msgs, X), 1.0 / X)
    return np.array(start, dtype=np.float64).reshape(n_msgs, X).copy()


def marginals_of(msgs, in_off, in_slots):
    """VariableNode.get_marginal: uniform times the incoming factor->variable messages, normalised."""
    X = msgs.shape[1]
    out = []
    for v in range(len(in_off) - 1):
        acc = np.full(X, 1.0 / X)
        for q in range(in_off[v], in_off[v + 1]):
            acc = acc * msgs[in_slots[q]]
        out.append(_norm(acc))
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------------------------------
# the plain op list and the pruned one
# ---------------------------------------------------------------------------------------------------------------------------
def run_ops(ops, srcs, sweeps, n_msgs, pair, unary, start=None, init=True):
    """The 4-word op list (kind, a, b, destination slot), sweep by sweep (sweeps: first op, count)."""
    X = pair.shape[-1] if len(pair) else unary.shape[-1]
    msgs = _start(start, init, n_msgs, X)
    ops = np.asarray(ops).reshape(-1, 4)
    for first, cnt in np.asarray(sweeps).reshape(-1, 2):
        for kind, a, b, c in ops[first:first + cnt]:
            if kind == OP_UNARY:
                msgs[c] = _norm(unary[a])
            elif kind == OP_VAR:
                acc = np.full(X, 1.0 / X)
                for q in range(a, a + b):
                    acc = acc * msgs[srcs[q]]
                msgs[c] = _norm(acc)
            else:
                assert kind in (OP_PAIR_TM, OP_PAIR_MT)
                msgs[c] = _norm(_contract(pair[a], msgs[b], kind == OP_PAIR_MT))
    return msgs


def run_pruned(words, srcs, n_msgs, pair, unary, start=None, init=True):
    """MLBP_IMAGE_PRUNED: the op list MLBP_SWEEP_SKIP_UNCHANGED runs (its variable updates still index the caller's srcs)."""
    ops, sweeps, _ = parse_pruned(words)
    return run_ops(ops, srcs, sweeps, n_msgs, pair, unary, start, init)


# ---------------------------------------------------------------------------------------------------------------------------
# the fused image (sweep_x64_fused_kernel)
# ---------------------------------------------------------------------------------------------------------------------------
def run_fused(words, n_msgs, pair, unary, start=None, init=True, exact_lists=False):
    """MLBP_IMAGE_FUSED.  Slots [0, n_msgs) are the messages; ext slot n_msgs is the uniform vector, n_msgs + 1 + k constant
    product k (uniform times the hoisted messages of cpw list k).  A header is kind | FOP_BUNDLED, then
      UNARY     unary slot, -, destination
      PAIR_*    pair slot, source slot, destination
      VAR       fast list (offset, count: base slot first), destination, -, -, exact list (offset, count)
      VAR_PAIR  fast list, slot of the variable->factor message, pair slot, destination, exact list
    exact_lists: every variable update through its exact list (uniform times the original sources) instead of the fast one.
    A bundled header and its successor both read the state from before either writes.  Returns the messages; checks pairseq
    (the pair slots in execution order, then -1) and written (the slots the loop writes) on the way."""
    f = parse_fused(words)
    X = pair.shape[-1] if len(pair) else unary.shape[-1]
    msgs = np.vstack([_start(start, init, n_msgs, X), np.zeros((1 + f['n_cprod'], X))])
    msgs[n_msgs] = 1.0 / X
    for u, slot in f['hoist'].reshape(-1, 2):
        msgs[slot] = _norm(unary[u])
    at = 0
    for k in range(f['n_cprod']):
        cnt = int(f['cpw'][at])
        acc = np.full(X, 1.0 / X)
        for s in f['cpw'][at + 1:at + 1 + cnt]:
            assert 0 <= s < n_msgs
            acc = acc * msgs[s]
        msgs[n_msgs + 1 + k] = acc
        at += 1 + cnt
    assert at == len(f['cpw'])
    psrcs, seq, wrote = f['psrcs'], [], set()

    def effects(w, state):
        """[(slot, value)] of one header, reading `state`."""
        kind = int(w[0]) & 0xFF
        if kind == FOP_UNARY:
            return [(int(w[3]), _norm(unary[w[1]]))]
        if kind in (FOP_PAIR_TM, FOP_PAIR_MT):
            seq.append(int(w[1]))
            return [(int(w[3]), _norm(_contract(pair[w[1]], state[w[2]], kind == FOP_PAIR_MT)))]
        assert kind in (FOP_VAR, FOP_VAR_PAIR_TM, FOP_VAR_PAIR_MT), kind
        if exact_lists:
            acc = np.full(X, 1.0 / X)
            lst = psrcs[w[6]:w[6] + w[7]]
            assert all(0 <= s < n_msgs for s in lst)
        else:
            acc = np.ones(X)
            lst = psrcs[w[1]:w[1] + w[2]]
            assert lst[0] >= n_msgs, 'a fast list starts with its base slot'
        for s in lst:
            acc = acc * state[s]
        v = _norm(acc)
        out = [(int(w[3]), v)]
        if kind != FOP_VAR:
            seq.append(int(w[4]))
            out.append((int(w[5]), _norm(_contract(pair[w[4]], v, kind == FOP_VAR_PAIR_MT))))
        return out

    fops = f['fops']
    for first, cnt in f['fsweeps'].reshape(-1, 2):
        i = first
        while i < first + cnt:
            members = 2 if fops[i][0] & FOP_BUNDLED else 1
            assert i + members <= first + cnt, 'a bundle does not straddle a sweep'
            before = msgs.copy() if members == 2 else msgs
            for w in fops[i:i + members]:
                for slot, value in effects(w, before):
                    assert 0 <= slot < n_msgs
                    msgs[slot] = value
                    if (int(w[0]) & 0xFF) != FOP_UNARY:
                        wrote.add(slot)
            i += members
    assert seq + [-1] == [int(p) for p in f['pairseq']], 'pairseq is the pair slots in execution order'
    assert sorted(wrote) == [int(s) for s in f['written']], 'written is what the loop writes'
    assert bool(f['has_unary_fops']) == any((int(w[0]) & 0xFF) == FOP_UNARY for w in fops)
    return msgs[:n_msgs]


# ---------------------------------------------------------------------------------------------------------------------------
# the lean image and its read-out lists (sweep_x64_lean_kernel)
# ---------------------------------------------------------------------------------------------------------------------------
def _slot(off, n_slots):
    assert off >= 0 and off % SLOT_BYTES == 0 and off // SLOT_BYTES < n_slots, off
    return int(off) // SLOT_BYTES


def run_lean(words, readout_words, n_msgs, pair, unary, start=None, init=True):
    """MLBP_IMAGE_LEAN (+ MLBP_IMAGE_LEAN_READOUT, or None) -> (messages, marginals or None).

    Work slots: the messages, then the ext slots -- n_msgs uniform, n_msgs + 1 + k constant product k, the last one all ones.
    A micro-op is 8 words: flags | four source byte offsets | byte offset of the variable->factor message (UOP_STORE_VF) or of
    a UOP_VAR's destination | destination byte offset | unused.  Sources 1-2 are always multiplied, 3-4 when the count
    exceeds two (the lists are padded with the ones slot).  UOP_VAR: the product, started from the carried value under
    UOP_CARRY_IN, handed on under UOP_CARRY_OUT and stored raw otherwise.  A contraction: the product (stored raw under
    UOP_STORE_VF), then T . m or m^T . T of the pair slot's table, normalised; the two members of a bundle read the state from
    before either writes.  Then the read-out from the work slots, the normalisation of the written slots, and the write-back
    of the hoisted and the written slots alone."""
    L = parse_lean(words)
    assert L['ok'] == 1
    X = pair.shape[-1] if len(pair) else unary.shape[-1]
    nc = L['n_cprod']
    n_slots = n_msgs + 2 + nc
    first = _start(start, init, n_msgs, X)
    work = np.vstack([first, np.zeros((2 + nc, X))])
    work[n_msgs] = 1.0 / X
    work[n_slots - 1] = 1.0
    hoisted = []
    for wave in range(4):
        ended = False
        for u, slot in L['hoist_lists'][wave]:
            if u < 0:
                ended = True
                continue
            assert not ended and 0 <= slot < n_msgs
            work[slot] = _norm(unary[u])
            hoisted.append(int(slot))
    assert sorted(hoisted) == [c for c in range(n_msgs) if L['hoisted'][c]], 'the hoisted flags name the hoist lists'' slots'
    for k, lst in enumerate(L['cprod_lists']):
        cnt = int(lst[0])
        assert 1 <= cnt <= 15 and all(int(s) == n_slots - 1 for s in lst[1 + cnt:]), 'padded with the ones slot'
        assert [int(s) for s in lst[1:1 + cnt]] == [int(s) for s in L['cprods'][k]]
        acc = np.full(X, 1.0 / X)
        for s in lst[1:]:
            acc = acc * work[s]
        work[n_msgs + 1 + k] = acc

    def product(u, state):
        n = (int(u[0]) >> UOP_NSRC_SHIFT) & 15
        assert 1 <= n <= 4 and all(int(s) == (n_slots - 1) * SLOT_BYTES for s in u[1 + n:5]), 'sources past the count: ones'
        acc = state[_slot(u[1], n_slots)] * state[_slot(u[2], n_slots)]
        if n > 2:
            acc = acc * state[_slot(u[3], n_slots)] * state[_slot(u[4], n_slots)]
        return acc

    carry, carrying, stored = None, False, set()
    for b in L['bundles']:
        A, B = b[:8], b[8:]
        fa, fb = int(A[0]), int(B[0])
        if fa & UOP_VAR:
            assert fb & UOP_NOP, 'a variable update is alone in its bundle'
            assert bool(fa & UOP_CARRY_IN) == carrying, 'a link follows its predecessor at once'
            acc = product(A, work)
            if fa & UOP_CARRY_IN:
                acc = acc * carry
            carrying = bool(fa & UOP_CARRY_OUT)
            if carrying:
                carry = acc
            else:
                c = _slot(A[5], n_msgs)
                work[c] = acc
                stored.add(c)
            continue
        assert not carrying and not fa & (UOP_NOP | UOP_CARRY_IN | UOP_CARRY_OUT)
        before = work.copy()
        for u in (A,) if fb & UOP_NOP else (A, B):
            f0 = int(u[0])
            assert not f0 & (UOP_VAR | UOP_NOP | UOP_CARRY_IN | UOP_CARRY_OUT)
            m = product(u, before)
            if f0 & UOP_STORE_VF:
                c = _slot(u[5], n_msgs)
                work[c] = m
                stored.add(c)
            p = (f0 >> UOP_PSLOT_SHIFT) & 7
            assert p < len(pair)
            c = _slot(u[6], n_msgs)
            work[c] = _norm(_contract(pair[p], m, bool(f0 & UOP_MT)))
            stored.add(c)
    assert not carrying
    assert int(L['pad'][0]) == UOP_NOP and int(L['pad'][8]) == UOP_NOP, 'the loop fetches one bundle past the end'
    marg = None
    if readout_words is not None:
        ok, lists = parse_readout(readout_words)
        assert ok == 1
        marg = []
        for lst in lists:
            cnt = int(lst[0])
            assert 1 <= cnt <= 15 and lst[1] >= n_msgs and all(int(s) == n_slots - 1 for s in lst[1 + cnt:])
            acc = np.ones(X)
            for s in lst[1:]:
                acc = acc * work[s]
            marg.append(_norm(acc))
        marg = np.stack(marg)
    written = []
    for wave in range(4):
        ended = False
        for s in L['written_lists'][wave]:
            if s < 0:
                ended = True
                continue
            assert not ended and 0 <= s < n_msgs
            written.append(int(s))
    assert len(set(written)) == len(written) and not set(written) & set(hoisted)
    out = first.copy()
    for s in hoisted:
        out[s] = work[s]
    for s in written:
        out[s] = _norm(work[s])
    return out, marg


# ---------------------------------------------------------------------------------------------------------------------------
# what a lean image holds, in the manner of test_gpu_lean_static._forms
# ---------------------------------------------------------------------------------------------------------------------------
def lean_forms(bundles):
    """The set of loop forms of bundle words [n_bundles][16], with the lengths of their carry chains ('CARRY x2', 'CARRY x3')."""
    out, links = set(), 0
    for r in bundles:
        fa, fb = int(r[0]), int(r[8])
        if fa & UOP_VAR:
            out.add('VAR')
            links += 1
            if not fa & UOP_CARRY_OUT:
                if links > 1:
                    out.add('CARRY x%d' % links)
                links = 0
            continue
        d = lambda f: 'MT' if f & UOP_MT else 'TM'      # noqa: E731
        out.add('%s|%s' % (d(fa), 'NOP' if fb & UOP_NOP else d(fb)))
        for f in (fa,) if fb & UOP_NOP else (fa, fb):
            if ((f >> UOP_NSRC_SHIFT) & 15) > 2 and f & UOP_STORE_VF:
                out.add('3SRC+VF')
    out.add('ends in VAR' if int(bundles[-1][0]) & UOP_VAR else 'ends in a contraction')
    out.add('odd n_bundles' if len(bundles) % 2 else 'even n_bundles')
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the family of random program cases
# ---------------------------------------------------------------------------------------------------------------------------
def explicit(spec, X):
    """The spec's topology -- ids, creation order, axes -- as an explicit-style spec at X states with one table per factor."""
    return dict(name='%s_x%d' % (spec['name'], X), style='explicit', X=X, var_ids=list(spec['var_ids']), labels=[0] * len(spec['var_ids']),
                factors=[dict(id=f['id'], vars=list(f['vars']), dims=list(f['dims']), table=k) for k, f in enumerate(spec['factors'])])


def random_case(seed, X=5):
    """(spec, roots) number `seed` of the family: a random tree over 2-9 variables with shuffled, non-contiguous ids -- under
    the hub bias (three cases in ten) most edges go to one variable, which then carries 5-8 pairwise factors --, up to three
    extra pairwise factors (loops, parallel factors), a unary factor on a variable with probability 0.7 and then further ones
    with probability 0.3 each, factor ids in random creation order, table axes either way round; 1-6 roots with repeats, the
    last one doubled in four cases in ten."""
    rs = np.random.RandomState(77000 + seed)
    n = int(rs.randint(2, 10))
    vids = sorted(rs.choice(40, size=n, replace=False).tolist())
    rs.shuffle(vids)
    hub = rs.rand() < 0.3
    edges = [(vids[i], vids[0 if hub and rs.rand() < 0.85 else int(rs.randint(0, i))]) for i in range(1, n)]
    for _ in range(int(rs.randint(0, 4))):
        a, b = rs.choice(n, size=2, replace=False)
        edges.append((vids[a], vids[b]))
    facs = []
    for v in vids:
        p = 0.7
        while rs.rand() < p:
            facs.append([v])
            p = 0.3
    facs += [[a, b] if rs.rand() < 0.5 else [b, a] for a, b in edges]
    order = rs.permutation(len(facs))
    ids = sorted(rs.choice(200, size=len(facs), replace=False).tolist())
    factors = []
    for k, j in enumerate(order):
        vs = facs[j]
        dims = [0] if len(vs) == 1 else ([0, 1] if rs.rand() < 0.5 else [1, 0])
        factors.append(dict(id=int(ids[k]), vars=[int(v) for v in vs], dims=dims, table=k))
    rs.shuffle(factors)                                  # creation order != id order
    seen = []
    for f in factors:
        for v in f['vars']:
            if v not in seen:
                seen.append(v)
    roots = [int(vids[int(rs.randint(n))]) for _ in range(int(rs.randint(1, 7)))]
    if rs.rand() < 0.4 and len(roots) < 6:
        roots.append(roots[-1])
    spec = dict(name='family_%d' % seed, style='explicit', X=X, var_ids=seen, labels=[0] * len(seen), factors=factors)
    return spec, roots


def with_X(spec, X):
    s = copy.deepcopy(spec)
    s['X'] = X
    s['name'] = '%s_x%d' % (spec['name'], X)
    return s
