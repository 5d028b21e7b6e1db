"""The packed wave reductions of the lean X = 64 kernel (csrc/mlbp_lean.hip, the three-table instances; LAB_NOTES R20):
PACKED_HOIST forms the hoisted unary messages two rows per wave instruction (a lane holds two consecutive entries of its
half-wave's row), PACKED_NORM the deferred normalisations of the tail four slots per pass (a lane holds four consecutive entries
of its lane group's slot).  Both add in wave_sum's order -- the balanced pairwise tree, tests/test_lean_packed_cpu.py -- so no
bit of a result and no flagged graph may change.  Every call below asserts

- that the lean kernel ran (mlbp_last_sweep_kernel() == 7), status() == 0 and the expected exact_count,
- messages and marginals against the per-graph exact kernel (mlbp_set_sweep_variant(3)) at 1e-11 and against the float64 oracle
  (oracle/lbp_oracle.py) at 1e-10, the project's standing tolerances for this kernel,
- and, where the messages go back to memory, that every hoisted unary-message slot of every graph the lean kernel did not flag
  equals row / tree_sum(row) bit for bit, every entry (tree_sum: the NumPy pairwise tree of the CPU test).

Each batch runs from uniform messages and continuing from its own first call's messages, with and without the write-back.
Shapes: 5 to 13 graphs; what each is there for is said in BATCHES and asserted on the decoded images by the first test.
"""
import functools

import numpy as np
import pytest

import cases as C
import test_lean_packed_cpu as TP
from macaronicusermodeling_amd import _ffi
from macaronicusermodeling_amd.topology import GraphTopology

RTOL = 1e-10            # against the oracle
RTOL_EXACT = 1e-11      # against the per-graph kernels
LEAN = 7
HB = 8                  # unary rows per wave the prologue holds in registers (csrc/mlbp_lean.hip)


def _user(sent_len, predicted, X=64):
    return C.user_spec(sent_len, predicted, X, 40, seed=1)


def _chain4_many_unary():
    """chain4 with nine unary factors at every variable: 36 rows, nine per wave."""
    factors = [dict(id=i, vars=[i // 9], dims=[0], table=i) for i in range(36)]
    for v in range(3):
        factors.append(dict(id=36 + v, vars=[v, v + 1], dims=[0, 1] if v % 2 else [1, 0], table=36 + v))
    return dict(name='chain4_u36', style='explicit', X=64, var_ids=list(range(4)), labels=[0] * 4, factors=factors)


def _chain3_plus_chain2():
    """chain5 without its (2, 3) factor: three tables, and sweeps rooted in {0, 1, 2} write the messages of two of them only."""
    s = C.chain_spec(5, 64, 'chain3_plus_chain2_x64')
    s['factors'] = [f for f in s['factors'] if f['vars'] != [2, 3]]
    return s


def _chain4_pairwise_only():
    s = C.chain_spec(4, 64, 'chain4_pairwise_only_x64')
    s['factors'] = [f for f in s['factors'] if len(f['vars']) == 2]
    return s


# name -> (spec, roots, graphs, seed, {graph: what is wrong with it}).  What can be wrong:
#   ('zero_row',)       one unary row zero throughout                   -> flagged by the prologue (zero total -> uniform)
#   ('neg_unary',)      one negative entry in a unary row               -> flagged by the prologue
#   ('neg_pair',)       one pairwise table entry of -1000               -> flagged by the main loop (a negative result)
BATCHES = {
    # 6 real + 2 empty hoist entries per wave (three full passes, one skipped), WL = 4 with one padding slot
    'user_k3': (lambda: _user(10, [1, 4, 7]), [1, 4, 7], 13, 401, {2: ('zero_row',), 6: ('neg_unary',), 11: ('neg_pair',)}),
    # 21 unary factors over four waves: 6, 5, 5, 5 rows -- the upper half of a wave's last pass is empty
    'user_k3_s9': (lambda: _user(9, [1, 4, 7]), [4, 1, 7], 7, 403, {}),
    # the issue's odd-row shape, two predicted words: 18 unary factors, 5, 5, 4, 4 rows; one table (<1,...>: the parent's code)
    'user_k2': (lambda: _user(10, [2, 6]), [2, 6], 7, 405, {}),
    # 36 unary factors: nine rows per wave, four packed passes and one round of the loop behind them
    'chain4_u36': (_chain4_many_unary, [0, 3, 1, 2], 5, 407, {}),
    # one row per wave (every upper half empty), other WL / real-slot counts
    'chain4': (lambda: C.chain_spec(4, 64), [0, 3, 1], 7, 409, {3: ('zero_row',)}),
    'star3': (lambda: C.star_spec(3, 64), [0, 2, 1], 7, 411, {}),
    # eight written slots: two real and two padding lane groups in every wave's pass
    'chain3_chain2': (_chain3_plus_chain2, [0, 2, 1], 5, 421, {}),
    # no unary factor at all: every pass skipped, the tail alone
    'chain4_u0': (_chain4_pairwise_only, [0, 3, 1], 5, 413, {}),
    # instances that keep the parent's code: unchanged results only
    'user_k4': (lambda: _user(10, [1, 3, 5, 8]), [1, 5, 8, 3], 5, 415, {}),
    'ring7': (lambda: C.ring_spec(7, 64), [0, 3, 5], 5, 417, {}),
    'user_k3_x48': (lambda: _user(10, [1, 4, 7], 48), [1, 4, 7], 9, 419, {4: ('zero_row',)}),
}
PACKED = ['user_k3', 'user_k3_s9', 'chain4_u36', 'chain4', 'star3', 'chain3_chain2', 'chain4_u0']       # P = 3, X = 64


@functools.lru_cache(maxsize=None)
def _image(name):
    """The lean program of a batch, decoded (MLBP_IMAGE_LEAN: ok, n_bundles, HL, n_cprod, WL, then the image as a vector: bundles
    [n_bundles][16] | hoist [4][HL][2] (unary factor, message slot; -1 padded) | constant products [n_cprod][16] | written [4][WL])."""
    make, roots = BATCHES[name][:2]
    w = GraphTopology.from_spec(make()).images(roots)['lean']
    assert w[0] == 1, 'no lean program for this shape'
    n, HL, n_cprod, WL = (int(x) for x in w[1:5])
    img = w[6:]
    hoist = img[16 * n:16 * n + 8 * HL].reshape(4, HL, 2)
    at = 16 * n + 8 * HL + 16 * n_cprod
    written = img[at:at + 4 * WL].reshape(4, WL)
    return dict(HL=HL, WL=WL, hoist=hoist, written=written)


def test_the_programs_hold_the_shapes_the_packed_passes_can_go_wrong_at():
    rows, slots = {}, {}
    for name in BATCHES:
        im = _image(name)
        rows[name] = [int((im['hoist'][w, :, 0] >= 0).sum()) for w in range(4)]
        slots[name] = [int((im['written'][w] >= 0).sum()) for w in range(4)]
        print(name, 'HL', im['HL'], 'rows per wave', rows[name], 'WL', im['WL'], 'written slots per wave', slots[name])
        for w in range(4):          # real entries first, then padding: a pass's lower half is never the empty one alone
            assert (im['hoist'][w, :rows[name][w], 0] >= 0).all() and (im['hoist'][w, :rows[name][w], 1] >= 0).all()
            assert (im['written'][w, :slots[name][w]] >= 0).all()
        assert im['WL'] % 4 == 0
    for name in PACKED:
        assert GraphTopology.from_spec(BATCHES[name][0]()).P == 3, name
    assert rows['user_k3'] == [6, 6, 6, 6] and _image('user_k3')['HL'] == 8
    assert _image('user_k3')['WL'] == 4 and slots['user_k3'] == [3, 3, 3, 3]                # one padding slot per wave
    assert any(r % 2 == 1 for r in rows['user_k3_s9']) and any(r % 2 == 0 for r in rows['user_k3_s9'])
    assert any(r % 2 == 1 for r in rows['user_k2'])
    assert _image('chain4_u36')['HL'] > HB and rows['chain4_u36'] == [9, 9, 9, 9]
    assert rows['chain4'] == [1, 1, 1, 1] and rows['star3'] == [1, 1, 1, 0] and rows['chain4_u0'] == [0, 0, 0, 0]
    assert any(s % 4 for s in slots['chain4']) and any(s % 4 for s in slots['star3'])      # real slots: no multiple of 4
    # (a three-table program that touches every factor writes 12 slots, three per wave, whatever its topology)
    assert slots['chain3_chain2'] == [2, 2, 2, 2]                                          # another filling of a pass than K3's


# ---------------------------------------------------------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------------------------------------------------------
def _spoil(bt, wrong):
    for b, what in wrong.items():
        if what[0] == 'zero_row':
            bt.unary[b, min(5, bt.topo.U - 1)] = 0.0
        elif what[0] == 'neg_unary':
            bt.unary[b, 7, 9] = -0.25
        else:
            bt.pair[b, 1, 17, 40] = -1000.0
    bt.upload()


@functools.lru_cache(maxsize=None)
def _batch(name):
    import test_gpu_lean_memory as TM          # its _Batch: per-graph random tables on the device and the oracle's view of each graph
    make, roots, B, seed, wrong = BATCHES[name]
    spec = make()
    bt = TM._Batch(spec if spec.get('style') == 'explicit' else TM._explicit(spec), roots, B, seed)
    _spoil(bt, wrong)
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
    """(start, oracle messages, oracle marginals, exact-kernel messages, exact-kernel marginals) of one batch, computed once."""
    bt = _batch(name)
    start = None if init else _first(name)
    want = [bt.oracle(b, start) for b in range(bt.B)]
    prog, msgs3, marg3, _ = _call(bt, init, start, variant=3)
    assert prog.status() == 0
    return start, np.stack([w[0] for w in want]), np.stack([w[1] for w in want]), msgs3, marg3


def _compare(name, what, msgs, marg, ref, keep=True, flagged=()):
    bt = _batch(name)
    start, want, wmarg, msgs3, marg3 = ref
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


def _hoisted_slots_are_row_over_tree_sum(name, msgs, flagged=()):
    """Every hoisted slot of every unflagged graph: row / tree_sum(row), the same bits in every entry."""
    bt = _batch(name)
    pairs = _image(name)['hoist'].reshape(-1, 2)
    pairs = pairs[pairs[:, 0] >= 0]
    assert len(pairs) == (3 if name == 'chain3_chain2' else bt.topo.U)      # (the unary factors of the component the sweeps touch)
    good = [b for b in range(bt.B) if b not in flagged]
    checked = 0
    for u, slot in pairs:
        rows = bt.unary[good, int(u)]                                   # [graphs][X]
        padded = np.zeros((len(good), 64))
        padded[:, :bt.X] = rows
        want = rows / TP.tree_sum(padded)[:, None]
        got = msgs[good, int(slot)]
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, int(u), int(slot))
        checked += got.size
    print('   %s: %d hoisted entries equal row / tree_sum(row) bit for bit' % (name, checked))


@pytest.mark.gpu
@pytest.mark.parametrize('keep', [True, False], ids=['keep', 'waived'])
@pytest.mark.parametrize('init', [True, False], ids=['init', 'continue'])
@pytest.mark.parametrize('name', sorted(BATCHES))
def test_results_and_flags_are_what_they_were(name, init, keep):
    bt = _batch(name)
    ref = _reference(name, init)
    flagged = sorted(BATCHES[name][4])
    prog, msgs, marg, kernel = _call(bt, init, ref[0], keep=keep)
    count = prog.exact_count(bt.B)
    print('%s init=%s keep=%s: kernel %d, exact_count %d (expected %d)' % (name, init, keep, kernel, count, len(flagged)))
    assert kernel == LEAN and prog.status() == 0
    _compare(name, 'init=%s keep=%s' % (init, keep), msgs, marg, ref, keep, flagged)
    assert count == len(flagged)
    if keep:
        _hoisted_slots_are_row_over_tree_sum(name, msgs, flagged)


@pytest.mark.gpu
def test_the_flagged_graphs_are_exactly_the_spoiled_ones():
    """The K3 batch clean (no graph flagged), with one spoiled graph at a time (one each) and with all three (three): graphs are
    independent, so the three the full batch flags are those three -- and the other graphs' messages are the clean batch's bits."""
    import test_gpu_lean_memory as TM
    make, roots, B, seed, wrong = BATCHES['user_k3']
    clean = TM._Batch(TM._explicit(make()), roots, B, seed)
    prog, msgs0, marg0, kernel = _call(clean, True, None)
    assert kernel == LEAN and prog.status() == 0 and prog.exact_count(B) == 0
    for b, what in sorted(wrong.items()):
        bt = TM._Batch(TM._explicit(make()), roots, B, seed)
        _spoil(bt, {b: what})
        prog, msgs, marg, kernel = _call(bt, True, None)
        count = prog.exact_count(B)
        print(what, 'exact_count', count)
        assert kernel == LEAN and prog.status() == 0 and count == 1, what
        others = [g for g in range(B) if g != b]
        assert np.array_equal(msgs[others], msgs0[others]) and np.array_equal(marg[others], marg0[others])
        np.testing.assert_allclose(marg[b], _reference('user_k3', True)[4][b], rtol=RTOL_EXACT, atol=1e-300)
    full = _first('user_k3')
    good = [g for g in range(B) if g not in wrong]
    assert np.array_equal(full[good], msgs0[good])


@pytest.mark.gpu
def test_grouped_call_is_bit_equal_to_the_single_launches():
    """Two user_k3 groups in one launch (the MULTI instance: the packed tail, the parent's prologue): each group's flagged graphs
    are its own, and every result equals the single launch's bit for bit."""
    import torch
    from macaronicusermodeling_amd import batch as batch_mod
    names = ['user_k3', 'user_k3_s9']
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
        _hoisted_slots_are_row_over_tree_sum(name, got_msgs, flagged)


@pytest.mark.gpu
def test_skip_unchanged_is_bit_equal_on_the_unflagged_graphs():
    name = 'user_k3'
    bt = _batch(name)
    flagged = sorted(BATCHES[name][4])
    good = [b for b in range(bt.B) if b not in flagged]
    msgs = _first(name)
    prog, msgs_s, marg_s, kernel = _call(bt, True, None, skip_unchanged=True)
    assert kernel == LEAN and prog.status() == 0 and prog.exact_count(bt.B) == len(flagged)
    assert prog.skippable_updates() > 0
    assert np.array_equal(msgs[good], msgs_s[good])
    _compare(name, 'skip_unchanged', msgs_s, marg_s, _reference(name, True))
    _hoisted_slots_are_row_over_tree_sum(name, msgs_s, flagged)
