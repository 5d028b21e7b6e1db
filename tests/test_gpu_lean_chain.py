"""The serial chain of one workgroup of the lean X = 64 kernel (csrc/mlbp_lean.hip): the prologue that runs while the tables
are still arriving (every load behind the unary rows issued unconditionally, the dense-layout index word parked in a register
and compared after the sweeps) and the gather of an update's source messages (lists padded with the all-ones slot, sources
1-2 fetched together, 3-4 together).  None of it may change a bit of a result, so

- every case compares messages and marginals with the float64 oracle (oracle/lbp_oracle.py) at the tolerance of
  tests/test_gpu_lean_memory.py (1e-10), and
- two paths of this build that must agree -- dense and indexed table layouts, the full schedule and skip_unchanged, a
  grouped launch and its single launches -- are compared with torch.equal.

Shapes: |X| = 64 (one case 48), 5 to 13 graphs; every call asserts that the lean kernel ran (mlbp_last_sweep_kernel() == 7).
"""
import numpy as np
import pytest

import cases as C
import test_gpu_lean_memory as TM          # its _Batch: per-graph random tables on the device and the oracle's view of each graph

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

RTOL = TM.RTOL
LEAN = TM.LEAN


def _user(K, B, seed, X=64, roots=None):
    predicted = [1, 4, 7, 8][:K]
    return TM._Batch(TM._explicit(C.user_spec(10, predicted, X, 40, seed=1)), roots or (predicted + predicted[:1]), B, seed)


def _run(bt, init=True, start=None, dense=True, skip_unchanged=False):
    """One call of the default path; returns (program, messages, marginals) as device tensors (clones)."""
    from macaronicusermodeling_amd import _ffi
    fb = bt.fb
    if start is None:
        fb.msgs.fill_(float('nan'))
    else:
        fb.msgs.copy_(torch.from_numpy(start))
    fb._pair_dense = fb._unary_dense = dense
    marg = torch.full((bt.B, bt.topo.n_vars, bt.X), float('nan'), dtype=torch.float64, device=fb.device)
    prog = fb.sweep(bt.roots, init=init, marginals=marg, skip_unchanged=skip_unchanged)
    torch.cuda.synchronize()
    assert _ffi.lib.mlbp_last_sweep_kernel() == LEAN
    return prog, fb.msgs.clone(), marg


def _against_oracle(bt, msgs, marg, start=None, graphs=None):
    msgs, marg = msgs.cpu().numpy(), marg.cpu().numpy()
    worst = 0.0
    for b in (range(bt.B) if graphs is None else graphs):
        want, wmarg = bt.oracle(b, start)
        worst = max(worst, float(np.max(np.abs(msgs[b] - want) / np.maximum(np.abs(want), 1e-300))))
        np.testing.assert_allclose(msgs[b], want, rtol=RTOL, atol=1e-300, err_msg='messages of graph %d' % b)
        np.testing.assert_allclose(marg[b], wmarg, rtol=RTOL, atol=1e-300, err_msg='marginals of graph %d' % b)
    print('%s: largest relative message error against the oracle %.3g' % (bt.spec['name'], worst))


def test_user_k3_dense_and_indexed_calls_agree_bit_for_bit():
    bt = _user(3, 13, 101, roots=[4, 1, 7])
    assert bt.topo.P == 3 and bt.topo.U == 24
    prog, msgs, marg = _run(bt, dense=True)
    assert prog.status() == 0 and prog.exact_count(bt.B) == 0
    _against_oracle(bt, msgs, marg)
    prog, msgs_i, marg_i = _run(bt, dense=False)
    assert prog.status() == 0 and prog.exact_count(bt.B) == 0
    assert torch.equal(msgs, msgs_i) and torch.equal(marg, marg_i)


def test_a_false_dense_flag_is_found_after_the_sweeps():
    """The dense flag is a statement about the index arrays.  Here it is false for four of thirteen graphs: graphs 2 and 5 have
    exchanged their pair-table rows, graphs 7 and 9 their unary rows.  The kernel computes them from the dense layout, finds the
    index words wrong when the sweeps are over, writes nothing of them and hands them to the exact kernel, which reads the
    arrays: the call returns what the indexed call returns, and exact_count counts exactly those four."""
    bt = _user(3, 13, 103, roots=[4, 1, 7])
    fb = bt.fb
    pt, ut = fb.pair_tab.clone(), fb.unary_tab.clone()
    pt[[2, 5]] = pt[[5, 2]]
    ut[[7, 9]] = ut[[9, 7]]
    fb.pair_tab.copy_(pt)
    fb.unary_tab.copy_(ut)
    bt.pair[[2, 5]] = bt.pair[[5, 2]]               # the oracle's view: what the index arrays say
    bt.unary[[7, 9]] = bt.unary[[9, 7]]
    wrong = [2, 5, 7, 9]
    right = [b for b in range(bt.B) if b not in wrong]
    prog, msgs_i, marg_i = _run(bt, dense=False)
    assert prog.status() == 0 and prog.exact_count(bt.B) == 0
    _against_oracle(bt, msgs_i, marg_i)
    prog, msgs, marg = _run(bt, dense=True)
    assert prog.status() == 0
    count = prog.exact_count(bt.B)
    print('exact_count %d (expected %d)' % (count, len(wrong)))
    _against_oracle(bt, msgs, marg)
    assert torch.equal(msgs[right], msgs_i[right]) and torch.equal(marg[right], marg_i[right])
    # (the four graphs come from the exact kernel here and from the lean kernel in the indexed call: two kernels, the tolerance
    # of tests/test_gpu_lean_memory.py between them)
    np.testing.assert_allclose(msgs[wrong].cpu().numpy(), msgs_i[wrong].cpu().numpy(), rtol=TM.RTOL_EXACT, atol=1e-300)
    np.testing.assert_allclose(marg[wrong].cpu().numpy(), marg_i[wrong].cpu().numpy(), rtol=TM.RTOL_EXACT, atol=1e-300)
    assert count == len(wrong)


def _pairwise_only(X):
    """chain3 without its unary factors: U = 0, so a call brings no unary tables and no unary_tab at all."""
    s = C.chain_spec(3, X, 'chain3_pairwise_only_x%d' % X)
    s['factors'] = [f for f in s['factors'] if len(f['vars']) == 2]
    return s


def test_a_graph_without_unary_factors_indexed_and_dense():
    """Every hoist entry is empty and the indexed call has no unary index array to read (a null pointer): the prologue's row
    loads must all go nowhere without asking for an index word."""
    bt = TM._Batch(_pairwise_only(64), [0, 2, 1], 7, 105)
    assert bt.topo.U == 0 and bt.topo.P == 2
    prog, msgs_i, marg_i = _run(bt, dense=False)
    assert prog.status() == 0 and prog.exact_count(bt.B) == 0
    _against_oracle(bt, msgs_i, marg_i)
    prog, msgs, marg = _run(bt, dense=True)
    assert prog.status() == 0 and prog.exact_count(bt.B) == 0
    assert torch.equal(msgs, msgs_i) and torch.equal(marg, marg_i)
    start = bt.start(106)
    prog, msgs, marg = _run(bt, init=False, start=start, dense=False)
    assert prog.status() == 0 and prog.exact_count(bt.B) == 0
    _against_oracle(bt, msgs, marg, start)


def _star6(B, seed):
    return TM._Batch(C.star_spec(6, 64), [0, 3, 0, 5], B, seed)


# shape -> (batch, pairwise factors, largest number of pairwise factors at one variable).  A variable with d pairwise
# factors sends each of them the product of the other d - 1 incoming messages and its constant product (unary messages):
# d = 1: one source; d = 3: three sources, the second fetch group; d = 6: five varying messages, more than a micro-op's four
# sources, so the product is a chain of carry links.  (The compiled micro-ops are not visible through the library's interface;
# the degrees that force them are asserted instead.)
SHAPES = {
    'user_k2': (lambda: _user(2, 9, 111), 1, 1),
    'user_k4': (lambda: _user(4, 7, 113), 6, 3),
    'star6': (lambda: _star6(5, 115), 6, 6),
}


def _largest_pairwise_degree(spec):
    return max(sum(1 for f in spec['factors'] if len(f['vars']) == 2 and v in f['vars']) for v in spec['var_ids'])


@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_source_counts_one_to_four_and_carry_links(shape):
    make, P, degree = SHAPES[shape]
    bt = make()
    assert bt.topo.P == P and _largest_pairwise_degree(bt.spec) == degree
    prog, msgs, marg = _run(bt)
    assert prog.status() == 0 and prog.exact_count(bt.B) == 0
    _against_oracle(bt, msgs, marg)
    prog, msgs_s, marg_s = _run(bt, skip_unchanged=True)
    assert prog.status() == 0 and prog.exact_count(bt.B) == 0
    assert torch.equal(msgs, msgs_s) and torch.equal(marg, marg_s)


def test_user_k3_skip_unchanged_agrees_bit_for_bit():
    bt = _user(3, 9, 117)
    prog, msgs, marg = _run(bt)
    assert prog.skippable_updates() > 0
    prog, msgs_s, marg_s = _run(bt, skip_unchanged=True)
    assert prog.status() == 0 and prog.exact_count(bt.B) == 0
    assert torch.equal(msgs, msgs_s) and torch.equal(marg, marg_s)


def test_continuing_from_stored_messages():
    """init=False: the messages come from memory (behind the table loads); dense and indexed calls agree bit for bit; and a
    second call continues where an initialising one stopped."""
    bt = _user(3, 11, 121)
    start = bt.start(122)
    prog, msgs, marg = _run(bt, init=False, start=start)
    assert prog.status() == 0 and prog.exact_count(bt.B) == 0
    _against_oracle(bt, msgs, marg, start)
    prog, msgs_i, marg_i = _run(bt, init=False, start=start, dense=False)
    assert torch.equal(msgs, msgs_i) and torch.equal(marg, marg_i)
    prog, first, _ = _run(bt, init=True)
    prog, msgs2, marg2 = _run(bt, init=False, start=first.cpu().numpy())
    assert prog.status() == 0 and prog.exact_count(bt.B) == 0
    _against_oracle(bt, msgs2, marg2, first.cpu().numpy())


def test_padded_state_space_x48():
    bt = _user(3, 9, 131, X=48)
    assert bt.topo.P == 3
    bt.check(True)
    bt.check(False, bt.start(132))
    prog, msgs, marg = _run(bt)
    prog, msgs_i, marg_i = _run(bt, dense=False)
    assert torch.equal(msgs, msgs_i) and torch.equal(marg, marg_i)


def test_seven_table_chain():
    """chain8: six tables in registers, the seventh in LDS by LDS-DMA (NL = 1)."""
    bt = TM._Batch(C.chain_spec(8, 64), [0, 7, 3], 5, 141)
    assert bt.topo.P == 7
    prog, msgs, marg = _run(bt)
    assert prog.status() == 0 and prog.exact_count(bt.B) == 0
    _against_oracle(bt, msgs, marg)
    prog, msgs_i, marg_i = _run(bt, dense=False)
    assert torch.equal(msgs, msgs_i) and torch.equal(marg, marg_i)
    start = bt.start(142)
    prog, msgs, marg = _run(bt, init=False, start=start)
    _against_oracle(bt, msgs, marg, start)


def test_grouped_call_agrees_with_its_single_launches():
    """Two shapes in one launch: a K3 user graph (three tables) beside a star whose tables fill the instance (six): the K3
    group's three absent tables are the loads with nothing to fetch."""
    from macaronicusermodeling_amd import _ffi
    from macaronicusermodeling_amd import batch as batch_mod
    bts = [_user(3, 7, 151), _star6(5, 152)]
    single = [_run(bt)[1:] for bt in bts]
    for bt, (msgs, marg) in zip(bts, single):
        _against_oracle(bt, msgs, marg)
    margs = []
    for bt in bts:
        bt.fb.msgs.fill_(float('nan'))
        margs.append(torch.full((bt.B, bt.topo.n_vars, bt.X), float('nan'), dtype=torch.float64, device=bt.fb.device))
    progs = batch_mod.sweep_groups([bt.fb for bt in bts], [bt.roots for bt in bts], init=True, marginals=margs)
    torch.cuda.synchronize()
    assert _ffi.lib.mlbp_last_sweep_kernel() == LEAN and all(p.status() == 0 for p in progs)
    for bt, (msgs, marg), gm in zip(bts, single, margs):
        assert torch.equal(bt.fb.msgs, msgs) and torch.equal(gm, marg)


@pytest.mark.parametrize('init', [True, False])
@pytest.mark.parametrize('what', ['unary', 'pair'])
def test_an_out_of_range_index_still_skips_its_graph_only(what, init):
    """(the loads of a graph with a bad index go nowhere instead of not being issued; the graph is skipped as before)"""
    bt = TM._Batch(TM._explicit(C.user_spec(10, [1, 4, 7], 64, 40, seed=1)), [4, 1, 7], 11, 161, unary_pool=96)
    b = 3
    if what == 'unary':
        bt.fb.unary_tab[b, 0] = 10 ** 6
    else:
        bt.fb.pair_tab[b, 0] = 10 ** 6
        bt.fb._pair_dense = False
    start = bt.start(162)
    msgs = bt.check(init, None if init else start, status=1, skipped=(b,))
    assert np.array_equal(msgs[b], np.full_like(msgs[b], 1.0 / 64) if init else start[b])


@pytest.mark.parametrize('init', [True, False])
def test_an_all_zero_unary_row_still_flags_its_graph(init):
    bt = _user(3, 13, 171)
    bt.unary[8, 0] = 0.0
    bt.unary[8, 23] = 0.0
    bt.upload()
    bt.check(init, None if init else bt.start(172), exact=1)
