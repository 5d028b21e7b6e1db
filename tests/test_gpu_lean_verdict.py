"""The verdict of the lean X = 64 kernel's main loop and the stored product of a bundle (csrc/mlbp_lean.hip, the three-table
instances): "negative or non-finite" is decided ONCE behind the loop, from a per-lane running maximum of the results' keys
(rescale_kmax), "no normal entry" per update on the scalar side; a member's variable->factor product is stored under a scalar
branch on its flag bit; and the loop's LDS accesses go by integer byte address.  None of it may change a bit of a result or the
set of graphs handed to the exact kernel, so every call below

- compares messages and marginals with the per-graph exact kernel (mlbp_set_sweep_variant(3)) at 1e-11 and with the float64
  oracle (oracle/lbp_oracle.py) at 1e-10 (the tolerances of tests/test_gpu_lean_bundle.py),
- asserts that the lean kernel ran (mlbp_last_sweep_kernel() == 7), status() == 0 and the expected exact_count.

The verdict is sticky.  A pairwise table that is negative throughout turns every result contracted with it negative while the
input is positive -- and positive again once a negative message comes round to it.  The reference divides by the (negative) sum
and sees nothing odd: its messages and marginals of such a graph are positive and finite.  `_signs` follows the signs through the
decoded micro-op image on the CPU, which tells where the negative results fall: in the first contraction bundle, in the last
one, in member A alone, in member B alone -- and, for two of the batches, that every slot the program wrote is positive again
when the loop ends, so that nothing but a verdict remembered from mid-loop can flag the graph.

Shapes: |X| = 64 (one batch 48), three topologies (user_k3, chain4, star3), 5 to 13 graphs.
"""
import functools

import numpy as np
import pytest

import cases as C
from macaronicusermodeling_amd import _ffi
from macaronicusermodeling_amd.topology import GraphTopology

RTOL = 1e-10            # tests/test_gpu_lean_bundle.py: against the oracle
RTOL_EXACT = 1e-11      # ... and against the per-graph kernels
LEAN = 7

UOP_VAR, UOP_MT, UOP_NOP, UOP_STORE_VF, UOP_NSRC_SHIFT, UOP_CARRY_IN, UOP_CARRY_OUT = 1, 2, 32, 64, 8, 0x1000, 0x2000    # csrc/mlbp_internal.h
UOP_PSLOT_SHIFT = 2


def _user_spec(X=64):
    return C.user_spec(10, [1, 4, 7], X, 40, seed=1)


# name -> (spec, roots, graphs, seed, {graph: what is wrong with it}).  What can be wrong:
#   ('neg', tables)   those pairwise tables negative throughout            -> flagged by the main loop (negative results)
#   ('inf',)          one +inf entry in a pairwise table                   -> flagged by the main loop (non-finite results)
#   ('zero_table',)   one pairwise table zero throughout                   -> flagged by the main loop (no normal entry)
#   ('zero_row',)     one unary row zero throughout                        -> flagged by the prologue
BATCHES = {
    'user_k3': (lambda: _user_spec(), [1, 4, 7], 13, 301, {2: ('neg', (0, 2)), 5: ('inf',), 8: ('zero_row',), 11: ('zero_table',)}),
    'user_k3_x48': (lambda: _user_spec(48), [1, 4, 7], 9, 303, {1: ('neg', (0, 2)), 4: ('inf',), 7: ('zero_row',)}),
    'user_k3_r114': (lambda: _user_spec(), [1, 1, 4], 7, 305, {3: ('neg', (1,))}),
    'user_k3_r11': (lambda: _user_spec(), [1, 1], 5, 307, {4: ('neg', (2,))}),
    'chain4': (lambda: C.chain_spec(4, 64), [0, 3, 1], 7, 309, {0: ('neg', (1,)), 6: ('neg', (0, 2))}),
    'star3': (lambda: C.star_spec(3, 64), [0, 2, 1], 7, 311, {5: ('neg', (0, 1, 2))}),
}


def _bundles(spec, roots):
    """The bundles of the lean program of (spec, roots) as an [n_bundles, 16] array (MLBP_IMAGE_LEAN: ok, n_bundles, HL, n_cprod,
    WL, then the image as a vector -- its first n_bundles x 16 words the bundles)."""
    w = GraphTopology.from_spec(spec).images(roots)['lean']
    assert w[0] == 1, 'no lean program for this shape'
    n = int(w[1])
    return w[6:6 + 16 * n].reshape(n, 16)


def _signs(bundles, negative):
    """Signs through the main loop for a graph whose pairwise tables `negative` (pair slots) are negative throughout and whose
    other inputs are positive -> (the (bundle, member) pairs whose result is negative, every written slot positive at the end?,
    the contraction bundles).  A bundle's two members read before either writes (they are independent by construction)."""
    sign, carry, bad, contractions = {}, 1, [], []
    at = lambda off: sign.get(int(off) // 512, 1)       # noqa: E731  (operands are byte offsets of 512-byte slots)
    for k, r in enumerate(bundles):
        fa = int(r[0])
        if fa & UOP_VAR:
            s = at(r[1]) * at(r[2]) * (carry if fa & UOP_CARRY_IN else 1)
            if ((fa >> UOP_NSRC_SHIFT) & 15) > 2:
                s *= at(r[3]) * at(r[4])
            if fa & UOP_CARRY_OUT:
                carry = s
            else:
                sign[int(r[5]) // 512] = s
            continue
        contractions.append(k)
        out = []
        for m, u in enumerate((r[0:8], r[8:16])):
            f = int(u[0])
            if f & UOP_NOP:
                continue
            s = at(u[1]) * at(u[2])
            if ((f >> UOP_NSRC_SHIFT) & 15) > 2:
                s *= at(u[3]) * at(u[4])
            if f & UOP_STORE_VF:
                out.append((int(u[5]) // 512, s))
            res = -s if ((f >> UOP_PSLOT_SHIFT) & 7) in negative else s
            if res < 0:
                bad.append((k, 'AB'[m]))
            out.append((int(u[6]) // 512, res))
        sign.update(out)
    return bad, all(s > 0 for s in sign.values()), contractions


def _stores(bundles):
    """Which members of the contraction bundles store their variable->factor product: a set of 'none', 'A', 'B', 'both'."""
    out = set()
    for r in bundles:
        fa, fb = int(r[0]), int(r[8])
        if fa & UOP_VAR:
            continue
        a, b = bool(fa & UOP_STORE_VF), bool(fb & UOP_STORE_VF) and not fb & UOP_NOP
        out.add('both' if a and b else 'A' if a else 'B' if b else 'none')
    return out


def test_where_the_negative_results_fall():
    """The positions the module's docstring promises, on the decoded images."""
    got = {}
    for name, (make, roots, B, seed, wrong) in sorted(BATCHES.items()):
        bundles = _bundles(make(), roots)
        for b, what in sorted(wrong.items()):
            if what[0] == 'neg':
                got[name, b] = _signs(bundles, set(what[1]))
                print(name, b, what, got[name, b])
    members = lambda bad, k: {m for kk, m in bad if kk == k}       # noqa: E731
    # two negative tables of the K3 program: a result turns negative in the first contraction bundle and in the last one, and a
    # slot that was negative is positive again later (the sign of what a bundle writes changes between sweeps)
    for key in (('user_k3', 2), ('user_k3_x48', 1)):
        bad, positive_at_the_end, contractions = got[key]
        assert members(bad, contractions[0]) and members(bad, contractions[-1])
        assert any(not members(bad, k) for k in contractions)
    # one negative table, roots [1, 1, 4]: member A alone, member B alone, and every written slot positive at the end
    bad, positive_at_the_end, contractions = got['user_k3_r114', 3]
    assert positive_at_the_end
    assert any(members(bad, k) == {'A'} for k in contractions) and any(members(bad, k) == {'B'} for k in contractions)
    assert not members(bad, contractions[-1])
    # ... roots [1, 1]: the first contraction bundle, both members; positive at the end
    bad, positive_at_the_end, contractions = got['user_k3_r11', 4]
    assert positive_at_the_end and members(bad, contractions[0]) == {'A', 'B'} and not members(bad, contractions[-1])
    # beside an empty member (chain4), and the last contraction bundle being the last bundle of the program (chain4, star3)
    for key in (('chain4', 0), ('chain4', 6), ('star3', 5)):
        bad, positive_at_the_end, contractions = got[key]
        assert bad
    bundles = _bundles(BATCHES['chain4'][0](), BATCHES['chain4'][1])
    assert any(int(bundles[k][8]) & UOP_NOP for k, m in got['chain4', 0][0])
    assert members(got['star3', 5][0], len(_bundles(BATCHES['star3'][0](), BATCHES['star3'][1])) - 1)


def test_the_programs_hold_every_store_form_and_both_parities():
    stores, count, last_is_var = {}, {}, {}
    for name, (make, roots, B, seed, wrong) in BATCHES.items():
        bundles = _bundles(make(), roots)
        stores[name], count[name], last_is_var[name] = _stores(bundles), len(bundles), bool(int(bundles[-1][0]) & UOP_VAR)
        print(name, sorted(stores[name]), count[name], last_is_var[name])
    assert stores['user_k3'] == {'none', 'A', 'B', 'both'} and stores['user_k3_x48'] == stores['user_k3']
    assert {'none', 'A', 'both'} <= stores['chain4']            # ('A' beside an empty member)
    assert count['user_k3'] % 2 == 1 and last_is_var['user_k3']       # odd, the last bundle a lone variable update
    assert count['chain4'] % 2 == 0 and not last_is_var['chain4']     # even, the last bundle a contraction
    assert count['star3'] % 2 == 1 and not last_is_var['star3']
    assert count['user_k3_r11'] % 2 == 0 and last_is_var['user_k3_r11']
    for name, (make, roots, B, seed, wrong) in BATCHES.items():
        assert GraphTopology.from_spec(make()).P == 3, name     # the instance all of this is built into


# ---------------------------------------------------------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch(name):
    import test_gpu_lean_memory as TM          # its _Batch: per-graph random tables on the device and the oracle's view of each graph
    make, roots, B, seed, wrong = BATCHES[name]
    spec = make()
    bt = TM._Batch(spec if spec.get('style') == 'explicit' else TM._explicit(spec), roots, B, seed)
    assert bt.topo.P == 3
    for b, what in wrong.items():
        if what[0] == 'neg':
            for p in what[1]:
                bt.pair[b, p] *= -1.0
        elif what[0] == 'inf':
            bt.pair[b, 1, 17, 40 % bt.X] = np.inf
        elif what[0] == 'zero_table':
            bt.pair[b, 2] = 0.0
        else:
            bt.unary[b, 5] = 0.0
    bt.upload()
    return bt


def _call(bt, init, start, **kw):
    import test_gpu_lean_bundle as TB
    return TB._call(bt, init, start, **kw)


@functools.lru_cache(maxsize=None)
def _first(name):
    """The messages an initialising call of the default path leaves: where the continuing calls start."""
    return _call(_batch(name), True, None)[1]


@functools.lru_cache(maxsize=None)
def _reference(name, init):
    """(start, oracle messages, oracle marginals, exact-kernel messages, exact-kernel marginals) of one batch, computed once.
    init=False: the second call, on the first call's messages."""
    bt = _batch(name)
    start = None if init else _first(name)
    want = [bt.oracle(b, start) for b in range(bt.B)]
    prog, msgs3, marg3, _ = _call(bt, init, start, variant=3)
    assert prog.status() == 0
    wmsgs, wmarg = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    # the reference sees nothing odd about a graph whose tables are negative throughout
    for b, what in BATCHES[name][4].items():
        if what[0] == 'neg':
            assert np.isfinite(wmsgs[b]).all() and np.isfinite(wmarg[b]).all()
            assert (wmsgs[b] > 0).all() and (wmarg[b] > 0).all(), (name, b)
    return start, wmsgs, wmarg, msgs3, marg3


def _compare(name, what, msgs, marg, ref, keep=True, start=None, flagged=()):
    bt = _batch(name)
    _, want, wmarg, msgs3, marg3 = ref
    rel = lambda a, b: float(np.nanmax(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))       # noqa: E731
    with np.errstate(all='ignore'):
        print('%s %s: marginals: largest relative difference to the exact kernel %.3g, to the oracle %.3g'
              % (name, what, rel(marg, marg3), rel(marg, wmarg)))
    np.testing.assert_allclose(marg, marg3, rtol=RTOL_EXACT, atol=1e-300)
    np.testing.assert_allclose(marg, wmarg, rtol=RTOL, atol=1e-300)
    if keep:
        with np.errstate(all='ignore'):
            print('   messages: largest relative difference to the exact kernel %.3g, to the oracle %.3g' % (rel(msgs, msgs3), rel(msgs, want)))
        np.testing.assert_allclose(msgs, msgs3, rtol=RTOL_EXACT, atol=1e-300)
        np.testing.assert_allclose(msgs, want, rtol=RTOL, atol=1e-300)
    elif bt.X == 64:            # (a padded state space reads out in a launch of its own, over the messages in memory)
        good = [b for b in range(bt.B) if b not in flagged]
        assert np.array_equal(msgs[good], start[good]) if start is not None else np.isnan(msgs[good]).all()


@pytest.mark.gpu
@pytest.mark.parametrize('keep', [True, False], ids=['keep', 'waived'])
@pytest.mark.parametrize('init', [True, False], ids=['init', 'continue'])
@pytest.mark.parametrize('name', sorted(BATCHES))
def test_the_flagged_graphs_are_exactly_the_expected_ones(name, init, keep):
    bt = _batch(name)
    ref = _reference(name, init)
    flagged = sorted(BATCHES[name][4])
    prog, msgs, marg, kernel = _call(bt, init, ref[0], keep=keep)
    count = prog.exact_count(bt.B)
    print('%s init=%s keep=%s: kernel %d, exact_count %d (expected %d)' % (name, init, keep, kernel, count, len(flagged)))
    assert kernel == LEAN and prog.status() == 0
    _compare(name, 'init=%s keep=%s' % (init, keep), msgs, marg, ref, keep, ref[0], flagged)
    assert count == len(flagged)        # those and only those (their results were compared with the exact kernel's above)


@pytest.mark.gpu
def test_every_kind_of_flagged_graph_counts_once():
    """The K3 batch with one kind of bad graph at a time: exact_count is 1 for each -- a graph negative in mid-loop only, the
    +inf entry, the all-zero table (no normal entry in an update's result: the per-update half of the verdict) and the all-zero
    unary row (the prologue's)."""
    import test_gpu_lean_memory as TM
    make, roots, B, seed, wrong = BATCHES['user_k3']
    full = _batch('user_k3')
    for b, what in sorted(wrong.items()):
        bt = TM._Batch(TM._explicit(make()), roots, B, seed)
        bt.pair[b], bt.unary[b] = full.pair[b], full.unary[b]
        bt.upload()
        prog, msgs, marg, kernel = _call(bt, True, None)
        count = prog.exact_count(bt.B)
        print(what, 'exact_count', count)
        assert kernel == LEAN and prog.status() == 0 and count == 1, what
        good = [g for g in range(B) if g not in wrong]
        ref = _reference('user_k3', True)
        assert np.array_equal(msgs[good], _first('user_k3')[good])      # the unflagged graphs: the same tables, the same bits
        np.testing.assert_allclose(marg[b], ref[4][b], rtol=RTOL_EXACT, atol=1e-300)


@pytest.mark.gpu
def test_grouped_call_flags_the_same_graphs():
    """Two groups in one launch (the MULTI instance): each group's flagged graphs are its own, and every result equals the single
    launch's bit for bit."""
    import torch
    from macaronicusermodeling_amd import batch as batch_mod
    names = ['user_k3', 'chain4']
    bts = [_batch(n) for n in names]
    single = [_call(bt, True, None)[1:3] for bt in bts]
    margs = []
    for bt in bts:
        bt.fb.msgs.fill_(float('nan'))
        margs.append(torch.full((bt.B, bt.topo.n_vars, bt.X), float('nan'), dtype=torch.float64, device=bt.fb.device))
    progs = batch_mod.sweep_groups([bt.fb for bt in bts], [bt.roots for bt in bts], init=True, marginals=margs)
    torch.cuda.synchronize()
    assert _ffi.lib.mlbp_last_sweep_kernel() == LEAN and all(p.status() == 0 for p in progs)
    for name, bt, prog, (msgs, marg), gm in zip(names, bts, progs, single, margs):
        flagged = sorted(BATCHES[name][4])
        count = prog.exact_count(bt.B)
        print(name, 'exact_count', count, 'expected', len(flagged))
        assert count == len(flagged)
        got_msgs, got_marg = bt.fb.msgs.cpu().numpy(), gm.cpu().numpy()
        assert np.array_equal(got_msgs, msgs, equal_nan=True) and np.array_equal(got_marg, marg, equal_nan=True)
        _compare(name, 'grouped', got_msgs, got_marg, _reference(name, True))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['user_k3', 'star3'])
def test_skip_unchanged_flags_the_same_graphs(name):
    """(the unflagged graphs equal the full schedule bit for bit; the flagged ones are the exact kernel's, which agrees with its
    own full schedule to rounding)"""
    bt = _batch(name)
    flagged = sorted(BATCHES[name][4])
    good = [b for b in range(bt.B) if b not in flagged]
    msgs = _first(name)
    prog, msgs_s, marg_s, kernel = _call(bt, True, None, skip_unchanged=True)
    assert kernel == LEAN and prog.status() == 0 and prog.exact_count(bt.B) == len(flagged)
    assert prog.skippable_updates() > 0
    assert np.array_equal(msgs[good], msgs_s[good])
    _compare(name, 'skip_unchanged', msgs_s, marg_s, _reference(name, True))
