"""Sweeps to convergence on the GPU (libmlbp_converge.so) against the float64 NumPy walk of tests/test_converge_cpu.py.

Tolerances: messages and marginals rtol 1e-10 (atol 1e-300) -- the project's tolerance for sums taken in a different order;
residual and history 1e-9 absolute (a difference of two entries in [0, 1], each within 1e-10); `rounds` exactly, which
tests/test_converge_cpu.py justifies: every case uses tol = 1e-6 and no residual of any round of the walk lies within
1e-3 * tol of tol -- asserted there on the CPU, and again here before the device is looked at, for every graph and round.
The walks are computed once per case (CV.gpu_case is cached) and never changed.

Mutations these cases are built to catch: the residual taken against the wrong `old` or over wave 0's first update only
(history at 1e-9 in every round); a stop decision that is not per graph (the mixed batch: 3 to 12 rounds side by side, and each
graph alone gives the batch's bits); `<` for `<=` at tol = 0 (the trees: residual exactly 0.0 must stop); history's tail or a
refused graph's outputs left unwritten; init=False ignored (warm start); messages not written back (log_partition,
marginals() after the call); a UNARY op skipped after round one although another row is written to its slot
(test_a_unary_slot_with_two_rows_is_never_skipped)."""
import numpy as np
import pytest

import cases as C
import test_converge_cpu as CV
from helpers import batch_tables, tidir_oracle_graph
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

X64_RESIDENT = ('converge_x64_kernel', (True,))          # P <= 3: tables in registers
X64_STREAMED = ('converge_x64_kernel', (False,))
GENERIC = ('converge_generic_kernel', ())
# kernel instance -> the tests that launch it (tests/test_converge_cpu.py holds this against the library's symbol table)
CASES = {
    X64_RESIDENT: ['test_mixed_batch', 'test_one_round_equals_sweep', 'test_warm_start', 'test_converged_messages_feed_log_partition',
                   'test_trees_stop_at_an_exact_fixed_point', 'test_each_graph_alone_gives_the_bits_of_the_batch',
                   'test_power_of_two_scaling_gives_the_same_bits', 'test_non_finite_and_empty_tables', 'test_table_index_out_of_range',
                   'test_one_round_one_graph', 'test_a_unary_slot_with_two_rows_is_never_skipped', 'test_capture_and_replay',
                   'test_tidir_convergence_report'],
    X64_STREAMED: ['test_mixed_batch', 'test_one_round_equals_sweep', 'test_both_sides_of_the_lds_budget', 'test_tidir_convergence_report'],
    GENERIC: ['test_mixed_batch', 'test_one_round_equals_sweep', 'test_trees_stop_at_an_exact_fixed_point',
              'test_each_graph_alone_gives_the_bits_of_the_batch', 'test_both_sides_of_the_lds_budget', 'test_non_finite_and_empty_tables',
              'test_table_index_out_of_range', 'test_one_round_one_graph', 'test_a_unary_slot_with_two_rows_is_never_skipped'],
}
KERNEL_OF = {X64_RESIDENT: 1, X64_STREAMED: 1, GENERIC: 2}     # mlbp_converge.h MLBP_CONVERGE_KERNEL_*
INSTANCE_OF = {'k3_x64': X64_RESIDENT, 'k4_x64': X64_STREAMED, 'ring4_x4': GENERIC, 'k3_x65': GENERIC, 'k3_x301': GENERIC}
TOL = CV.TOL
OUT_KEYS = ('rounds', 'residual', 'history', 'msgs', 'marg')


def _V():
    from macaronicusermodeling_amd import converge
    return converge


def _batch(spec, inputs_list, tables=None):
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(spec)
    fb = FactorGraphBatch(topo, spec['X'], len(inputs_list))
    pair, unary = batch_tables(spec, topo, inputs_list) if tables is None else tables
    if topo.P:
        fb.set_pair_tables(pair)
    if topo.U:
        fb.set_unary_tables(unary)
    return fb


def _run(fb, roots=None, tol=TOL, max_rounds=12, init=True):
    marg = torch.full((fb.B, fb.topo.n_vars, fb.X), float('nan'), dtype=torch.float64, device=fb.device)
    if init:
        fb.msgs.fill_(float('nan'))                      # init=True must not read them
    rounds, residual, history = fb.converge(roots, tol=tol, max_rounds=max_rounds, init=init, marginals=marg, history=True)
    kernel = _V().last_kernel()
    torch.cuda.synchronize()
    assert rounds.dtype == torch.int32 and tuple(rounds.shape) == (fb.B,)
    assert residual.dtype == torch.float64 and tuple(residual.shape) == (fb.B,) and tuple(history.shape) == (fb.B, max_rounds)
    return dict(rounds=rounds.cpu().numpy(), residual=residual.cpu().numpy(), history=history.cpu().numpy(),
                msgs=fb.msgs.cpu().numpy().copy(), marg=marg.cpu().numpy(), kernel=kernel)


def _same_bits(a, b, rows=slice(None), rows_b=None):
    rows_b = rows if rows_b is None else rows_b
    for k in OUT_KEYS:
        assert np.array_equal(a[k][rows], b[k][rows_b], equal_nan=True), k


def _check_margin(name, walks):
    near = CV.nearest_to_tol(walks)
    print('%s: rounds of the walk %r, nearest residual to tol %.3e' % (name, [w['rounds'] for w in walks], near))
    assert near > CV.MARGIN, (name, near)


def _compare(name, topo, got, walks, max_rounds, graphs=None):
    for i, b in enumerate(range(len(walks)) if graphs is None else graphs):
        w = walks[i]
        tag = '%s graph %d' % (name, b)
        assert got['rounds'][b] == w['rounds'], (tag, got['rounds'][b], w['history'], got['history'][b])
        np.testing.assert_allclose(got['residual'][b], w['residual'], rtol=0, atol=1e-9, err_msg=tag)
        np.testing.assert_allclose(got['history'][b, :w['rounds']], w['history'], rtol=0, atol=1e-9, err_msg=tag)
        assert (got['history'][b, w['rounds']:] == -1.0).all(), tag
        assert got['history'][b, w['rounds'] - 1] == got['residual'][b], tag
        want = np.stack([w['msgs'][k] for k in topo.slot_keys()])
        np.testing.assert_allclose(got['msgs'][b], want, rtol=1e-10, atol=1e-300, err_msg=tag, equal_nan=True)
        want = np.stack([w['marginals'][v] for v in topo.var_ids])
        np.testing.assert_allclose(got['marg'][b], want, rtol=1e-10, atol=1e-300, err_msg=tag)


def _gpu_case(name):
    spec, inputs, walks, max_rounds = CV.gpu_case(name)
    _check_margin(name, walks)                           # before the device is looked at
    fb = _batch(spec, inputs)
    V = _V()
    assert V.pick_kernel(spec['X'], fb.topo.n_msgs, fb.topo.n_vars) == KERNEL_OF[INSTANCE_OF[name]]
    assert (fb.topo.P <= 3) == (INSTANCE_OF[name] != X64_STREAMED) or INSTANCE_OF[name] == GENERIC
    return spec, inputs, walks, max_rounds, fb


# ---- the mixed batch: every graph stops on its own ---------------------------------------------------
@pytest.mark.parametrize('name', list(CV.GPU_CASES))
def test_mixed_batch(name):
    spec, inputs, walks, max_rounds, fb = _gpu_case(name)
    got = _run(fb, max_rounds=max_rounds)
    assert got['kernel'] == KERNEL_OF[INSTANCE_OF[name]], name
    print('%s: rounds %r residual %s' % (name, got['rounds'].tolist(), ['%.2e' % r for r in got['residual']]))
    _compare(name, fb.topo, got, walks, max_rounds)
    assert np.isfinite(got['msgs']).all() and np.isfinite(got['marg']).all()
    # the messages are left in fb.msgs: marginals() reads the converged ones
    np.testing.assert_allclose(fb.marginals().cpu().numpy(), got['marg'], rtol=1e-10, atol=1e-300)


@pytest.mark.parametrize('name', ['k3_x64', 'k4_x64', 'ring4_x4', 'k3_x65'])
def test_one_round_equals_sweep(name):
    """Against the shipped sum-product kernels, not the walk: one round at tol = 0 is sweep(roots, init=True)."""
    spec, inputs, _, _, fb = _gpu_case(name)
    for roots in (list(fb.topo.var_ids), [fb.topo.var_ids[-1], fb.topo.var_ids[0]]):
        marg = torch.empty(fb.B, fb.topo.n_vars, fb.X, dtype=torch.float64, device=fb.device)
        fb.sweep(roots, init=True, marginals=marg)
        torch.cuda.synchronize()
        want_msgs, want_marg = fb.msgs.cpu().numpy().copy(), marg.cpu().numpy()
        got = _run(fb, roots=roots, tol=0.0, max_rounds=1)
        assert got['kernel'] == KERNEL_OF[INSTANCE_OF[name]]
        assert (got['rounds'] == 1).all() and (got['residual'] > 0).all() and np.array_equal(got['history'][:, 0], got['residual'])
        np.testing.assert_allclose(got['msgs'], want_msgs, rtol=1e-10, atol=1e-300)
        np.testing.assert_allclose(got['marg'], want_marg, rtol=1e-10, atol=1e-300)


def test_warm_start():
    """sweep(every variable once, init=True) is round 1; converge(init=False) then runs the walk's remaining rounds: rounds - 1
    for a graph that converges inside max_rounds, and max_rounds more for one that does not (the walk continued says so)."""
    name = 'k3_x64'
    spec, inputs, walks, max_rounds, fb = _gpu_case(name)
    roots = list(fb.topo.var_ids)
    warm = []
    for inp in inputs:
        first = CV.walk(spec, inp, max_rounds=1)
        warm.append(CV.walk(spec, inp, max_rounds=max_rounds, msgs=first['msgs']))
    _check_margin(name + ' warm', warm)
    for w, c in zip(warm, walks):
        assert w['rounds'] == (c['rounds'] - 1 if c['residual'] <= TOL else max_rounds)
    cold = _run(fb, max_rounds=max_rounds)
    fb.sweep(roots, init=True)
    got = _run(fb, max_rounds=max_rounds, init=False)
    assert got['kernel'] == 1
    _compare(name + ' warm', fb.topo, got, warm, max_rounds)
    done = np.array([c['residual'] <= TOL for c in walks])
    assert done.sum() >= 4
    np.testing.assert_allclose(got['msgs'][done], cold['msgs'][done], rtol=1e-10, atol=1e-300)
    assert np.array_equal(got['rounds'][done], cold['rounds'][done] - 1)


def test_converged_messages_feed_log_partition():
    """After a converged call log_partition(roots=None) reads the converged messages: the value of log_partition after the same
    number of sweeps by sweep()."""
    spec, inputs, walks, max_rounds, _ = _gpu_case('k3_x64')
    for b in (0, 2):
        fb = _batch(spec, [inputs[b]])
        got = _run(fb, max_rounds=max_rounds)
        assert got['rounds'][0] == walks[b]['rounds'] and got['residual'][0] <= TOL
        have = fb.log_partition(roots=None).cpu().numpy()
        want = fb.log_partition(roots=list(fb.topo.var_ids) * int(got['rounds'][0]), init=True).cpu().numpy()
        np.testing.assert_allclose(have, want, rtol=1e-10)


# ---- exact cases that need no reference ----------------------------------------------------------------
@pytest.mark.parametrize('X,instance', [(64, X64_RESIDENT), (5, GENERIC)])
def test_trees_stop_at_an_exact_fixed_point(X, instance):
    spec = C.chain_spec(4, X)
    inputs = [C.make_inputs(spec, s, kind) for s, kind in ((1, 'uniform'), (2, 'lognormal'), (3, 'lognormal'))]
    fb = _batch(spec, inputs)
    got = _run(fb, tol=0.0, max_rounds=7)
    assert got['kernel'] == KERNEL_OF[instance]
    assert (got['rounds'] == 2).all() and (got['residual'] == 0.0).all(), (got['rounds'], got['residual'])
    assert (got['history'][:, 0] > 0).all() and (got['history'][:, 1] == 0.0).all() and (got['history'][:, 2:] == -1.0).all()
    walks = [CV.walk(spec, inp, tol=0.0, max_rounds=7) for inp in inputs]
    _compare('chain4_x%d' % X, fb.topo, got, walks, 7)


@pytest.mark.parametrize('name', ['k3_x64', 'ring4_x4'])
def test_each_graph_alone_gives_the_bits_of_the_batch(name):
    spec, inputs, walks, max_rounds, fb = _gpu_case(name)
    got = _run(fb, max_rounds=max_rounds)
    for b in range(len(inputs)):
        one = _run(_batch(spec, [inputs[b]]), max_rounds=max_rounds)
        assert one['kernel'] == got['kernel']
        _same_bits(one, got, rows=slice(0, 1), rows_b=slice(b, b + 1))


def test_power_of_two_scaling_gives_the_same_bits():
    """Every table of graph b times 2^p_b: renorm divides the power out exactly, so rounds, residual, history, messages and
    marginals keep their bits."""
    spec, inputs, walks, max_rounds, fb = _gpu_case('k3_x64')
    got = _run(fb, max_rounds=max_rounds)
    powers = [200, -200, 64, -1, 137, -90]
    scaled = [dict(tables=[t * 2.0 ** p for t in inp['tables']]) for inp, p in zip(inputs, powers)]
    again = _run(_batch(spec, scaled), max_rounds=max_rounds)
    assert again['kernel'] == 1
    _same_bits(again, got)


# ---- edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('leaves,instance', [(30, X64_STREAMED), (31, GENERIC)])
def test_both_sides_of_the_lds_budget(leaves, instance):
    """A star at X = 64 has 5 message slots per leaf: 30 leaves are the 150 slots that still fit the X = 64 kernel's LDS budget,
    31 leaves go to the generic kernel.  A tree: two rounds at tol = 0, and the walk's messages and marginals."""
    spec = C.star_spec(leaves, 64)
    inputs = [C.make_inputs(spec, s, 'lognormal') for s in (1, 2)]
    fb = _batch(spec, inputs)
    assert fb.topo.n_msgs == 5 * leaves
    got = _run(fb, tol=0.0, max_rounds=4)
    assert got['kernel'] == KERNEL_OF[instance] == _V().pick_kernel(64, fb.topo.n_msgs, fb.topo.n_vars)
    assert (got['rounds'] == 2).all() and (got['residual'] == 0.0).all()
    walks = [CV.walk(spec, inputs[0], tol=0.0, max_rounds=4)]
    _compare('star%d' % leaves, fb.topo, got, walks, 4, graphs=[0])


@pytest.mark.parametrize('name', ['k3_x64', 'k3_x65'])
def test_non_finite_and_empty_tables(name):
    """NaN, all-zero or +inf in one pairwise table of graph 1: the graph follows the walk (CV.test_non_finite_and_empty_tables
    states what that is: finite messages for NaN and zero; for +inf NaN message entries exactly where the reference's own
    arithmetic leaves them, a first residual of +inf, a NaN that stays NaN counted as unmoved, and finite marginals), the other
    graphs keep the bits of a run without the edit."""
    spec, inputs, walks, max_rounds, fb = _gpu_case(name)
    clean = _run(fb, max_rounds=max_rounds)
    pair = [f['table'] for f in spec['factors'] if len(f['vars']) == 2][1]
    for what in ('nan', 'zero', 'inf'):
        edited = dict(tables=[t.copy() for t in inputs[1]['tables']])
        if what == 'zero':
            edited['tables'][pair][:] = 0.0
        else:
            edited['tables'][pair][3, 9] = dict(nan=np.nan, inf=np.inf)[what]
        w = CV.walk(spec, edited, max_rounds=max_rounds)
        _check_margin('%s %s' % (name, what), [w])
        got = _run(_batch(spec, [inputs[0], edited, inputs[2]]), max_rounds=max_rounds)
        assert got['kernel'] == clean['kernel']
        _same_bits(got, clean, rows=[0, 2])
        assert np.isfinite(got['marg']).all()
        _compare('%s %s' % (name, what), fb.topo, got, [w], max_rounds, graphs=[1])
        if what == 'inf':
            want = np.stack([w['msgs'][k] for k in fb.topo.slot_keys()])
            assert np.array_equal(np.isnan(got['msgs'][1]), np.isnan(want)) and np.isnan(want).sum() >= 1
            assert np.isposinf(got['history'][1, 0]) and np.isposinf(w['history'][0]) and np.isfinite(got['residual'][1])
        else:
            assert np.isfinite(got['msgs']).all()


@pytest.mark.parametrize('name', ['k3_x64', 'k3_x65'])
def test_table_index_out_of_range(name):
    """A graph that names a table outside its array is not computed: rounds -1, residual NaN, its history row NaN, its messages and
    marginals untouched; its neighbours keep their bits."""
    spec, inputs, walks, max_rounds, fb = _gpu_case(name)
    clean = _run(fb, max_rounds=max_rounds)
    fb.pair_tab[1, 2] = fb.pair_tables.shape[0]
    fb.unary_tab[2, 0] = -1
    fb.msgs.fill_(7.0)
    marg = torch.full((fb.B, fb.topo.n_vars, fb.X), 5.0, dtype=torch.float64, device=fb.device)
    rounds, residual, history = fb.converge(tol=TOL, max_rounds=max_rounds, init=True, marginals=marg, history=True)
    torch.cuda.synchronize()
    got = dict(rounds=rounds.cpu().numpy(), residual=residual.cpu().numpy(), history=history.cpu().numpy(), msgs=fb.msgs.cpu().numpy(),
               marg=marg.cpu().numpy())
    for b in (1, 2):
        assert got['rounds'][b] == -1 and np.isnan(got['residual'][b]) and np.isnan(got['history'][b]).all()
        assert (got['msgs'][b] == 7.0).all() and (got['marg'][b] == 5.0).all()
    _same_bits(got, clean, rows=[0])


@pytest.mark.parametrize('name', ['k3_x64', 'ring4_x4'])
def test_one_round_one_graph(name):
    """max_rounds = 1 and B = 1: one round, its residual reported, above tol."""
    spec, inputs, walks, _, _ = _gpu_case(name)
    fb = _batch(spec, [inputs[2]])
    got = _run(fb, max_rounds=1)
    assert got['kernel'] == KERNEL_OF[INSTANCE_OF[name]]
    w = CV.walk(spec, inputs[2], max_rounds=1)
    assert w['history'] == walks[2]['history'][:1] and w['residual'] > TOL
    _compare(name + ' one round', fb.topo, got, [w], 1)


def _run_ops(fb, ops, srcs, sweeps, tol, max_rounds):
    """mlbp_converge_f64 with a hand-made op list (FactorGraphBatch.converge only runs compiled root sequences)."""
    import ctypes
    V = _V()
    topo, dev = fb.topo, fb.device
    prog = V.program(topo, topo.var_ids, dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))).to(dev)      # noqa: E731
    d_ops, d_srcs, d_sweeps = up(ops), up(srcs), up(sweeps)
    assert V.check_program(ops, srcs, sweeps, topo.n_msgs, topo.P, topo.U) == 0
    a = V.ConvergeArgs()
    a.B, a.X, a.n_msgs, a.P, a.U, a.n_vars = fb.B, fb.X, topo.n_msgs, topo.P, topo.U, topo.n_vars
    a.n_ops, a.n_srcs, a.n_sweeps = d_ops.numel() // 4, d_srcs.numel(), d_sweeps.numel() // 2
    a.ops, a.srcs, a.sweeps = d_ops.data_ptr(), d_srcs.data_ptr(), d_sweeps.data_ptr()
    a.n_pair_tables, a.n_unary_tables = fb.pair_tables.shape[0], fb.unary_tables.shape[0]
    a.pair_tables, a.pair_tab = fb.pair_tables.data_ptr(), fb.pair_tab.data_ptr()
    a.unary_tables, a.unary_tab = fb.unary_tables.data_ptr(), fb.unary_tab.data_ptr()
    a.normalize_messages, a.init_messages, a.max_rounds, a.tol = 1, 1, max_rounds, tol
    a.in_off, a.in_slots = prog.in_off.data_ptr(), prog.in_slots.data_ptr()
    rounds = torch.empty(fb.B, dtype=torch.int32, device=dev)
    residual = torch.empty(fb.B, dtype=torch.float64, device=dev)
    history = torch.empty(fb.B, max_rounds, dtype=torch.float64, device=dev)
    a.msgs, a.rounds, a.residual, a.history = fb.msgs.data_ptr(), rounds.data_ptr(), residual.data_ptr(), history.data_ptr()
    V.check(V.lib.mlbp_converge_f64(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    kernel = V.last_kernel()
    torch.cuda.synchronize()
    return rounds.cpu().numpy(), history.cpu().numpy(), fb.msgs.cpu().numpy().copy(), kernel


@pytest.mark.parametrize('name', ['k3_x64', 'k3_x65'])
def test_a_unary_slot_with_two_rows_is_never_skipped(name):
    """After the first round the kernels skip a UNARY op only where every writer of its slot is the same unary row.  The compiled
    program (every unary op skippable after round one) and a hand-made one in which one slot receives two different rows in
    every round (none of its writers may be skipped) both follow CV.run_ops, which runs every op of every round."""
    spec, inputs, walks, max_rounds, fb = _gpu_case(name)
    topo = fb.topo
    ops, srcs, sweeps = topo.compile_program(list(topo.var_ids))
    bad, slot = CV.two_rows_one_slot(ops)
    pair, unary = batch_tables(spec, topo, inputs)
    for program, cap in ((ops, max_rounds), (bad, 6)):
        rounds, history, msgs, kernel = _run_ops(fb, program, srcs, sweeps, TOL, cap)
        assert kernel == KERNEL_OF[INSTANCE_OF[name]]
        for b in range(fb.B):
            want_msgs, want = CV.run_ops(program, srcs, sweeps, pair[b * topo.P:(b + 1) * topo.P], unary[b * topo.U:(b + 1) * topo.U],
                                         topo.n_msgs, spec['X'], max_rounds=cap)
            assert min(abs(r - TOL) for r in want) > CV.MARGIN
            assert rounds[b] == len(want), (name, b, want, history[b])
            np.testing.assert_allclose(history[b, :len(want)], want, rtol=0, atol=1e-9)
            np.testing.assert_allclose(msgs[b], want_msgs, rtol=1e-10, atol=1e-300)
            if program is bad:
                assert rounds[b] == cap and history[b].min() > 1e-3


def test_python_layer_refusals():
    spec, inputs, _, _, fb = _gpu_case('k3_x64')
    V = _V()
    for kwargs in (dict(tol=-1.0), dict(tol=float('nan')), dict(max_rounds=0), dict(max_rounds=65536)):
        with pytest.raises((V.ConvergeError, ValueError)):
            fb.converge(**kwargs)
    with pytest.raises(ValueError):
        fb.converge(roots=[99])
    with pytest.raises(ValueError):
        fb.converge(marginals=torch.empty(1, 1, 1, dtype=torch.float64, device=fb.device))
    fb.normalize_messages = False
    with pytest.raises(ValueError):
        fb.converge()
    fb.normalize_messages = True
    fb.use_approx_inference = True
    with pytest.raises(NotImplementedError):
        fb.converge()
    spec32 = C.user_spec(10, [1, 4, 7], 256, 64, seed=1)
    fb32 = _batch(spec32, [C.make_inputs(spec32, 1)])
    fb32.set_pair_tables(fb32.pair_tables, dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        fb32.converge()
    # two values are returned without history
    fb.use_approx_inference = False
    assert len(fb.converge(max_rounds=2)) == 2


def test_capture_and_replay():
    """After one eager call the call is captured (one stream, no parallel branch) and replayed twice: the bits of the eager call."""
    spec, inputs, walks, max_rounds, fb = _gpu_case('k3_x64')
    eager = _run(fb, max_rounds=max_rounds)
    marg = torch.empty(fb.B, fb.topo.n_vars, fb.X, dtype=torch.float64, device=fb.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rounds, residual, history = fb.converge(tol=TOL, max_rounds=max_rounds, init=True, marginals=marg, history=True)
    for _ in range(2):
        for t in (residual, history, marg, fb.msgs):
            t.fill_(float('nan'))
        rounds.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        replayed = dict(rounds=rounds.cpu().numpy(), residual=residual.cpu().numpy(), history=history.cpu().numpy(),
                        msgs=fb.msgs.cpu().numpy(), marg=marg.cpu().numpy())
        _same_bits(replayed, eager)


# ---- trainer --------------------------------------------------------------------------------------------
def test_tidir_convergence_report(tmp_path):
    """TiDirTrainer.convergence_report() on a synthetic file: every instance against the walk on its own graph as
    tidir_oracle_graph builds it -- rounds exactly (under the margin condition, asserted first), residual and gap to 1e-9 -- and
    the totals are the sums."""
    from macaronicusermodeling_amd import tidir
    from macaronicusermodeling_amd.train import TiDirTrainer
    V = _V()
    paths = tidir.synthesize(str(tmp_path), n_instances=24, X=64, Vde=64, sent_len=(4, 7), n_predicted=(1, 4), seed=9)
    tt = TiDirTrainer(paths['ti'], paths['end'], paths['ded'], paths['phi_pmi'], paths['phi_pmi_w1'], paths['phi_ed'], paths['phi_ped'], sweeps=3)
    phi_ee, phi_w1, phi_ed = tidir.load_features(paths['phi_pmi'], paths['phi_pmi_w1'], paths['phi_ed'], paths['phi_ped'])
    rs = np.random.RandomState(1)
    th_ee, th_ed = rs.randn(1, 3) * 0.6, rs.randn(1, 6) * 0.6
    tt.theta_en_en.copy_(torch.from_numpy(th_ee.reshape(-1)))
    tt.theta_en_de.copy_(torch.from_numpy(th_ed.reshape(-1)))
    max_rounds = 20
    want, walks = {}, []
    for key, b in tt.buckets.items():
        topo = tt.trainers[key].topo
        for r, row in enumerate(b['rows']):
            g, inputs, roots, _ = tidir_oracle_graph(key, b, r, phi_ee, phi_w1, phi_ed, th_ee, th_ed)
            n = 3 if O.has_loops(g, roots[0]) else 1
            assert n == tt.trainers[key].n_sweeps_run
            _, stopped, _ = O.run(g.spec, inputs, roots[:n], n, force_loopy=True)
            w = CV.walk(g.spec, inputs, roots=list(topo.var_ids), tol=TOL, max_rounds=max_rounds)
            gap = max(float(np.abs(O.marginal(g, stopped, v) - w['marginals'][v]).max()) for v in topo.var_ids)
            want[row['index']] = (tuple(key[1]), w['rounds'], w['residual'], gap)
            walks.append(w)
    _check_margin('synthetic file', walks)
    per_instance, totals = tt.convergence_report(tol=TOL, max_rounds=max_rounds)
    ran = set()
    for key, tr in tt.trainers.items():
        ran.add((V.pick_kernel(64, tr.topo.n_msgs, tr.topo.n_vars), tr.topo.P <= 3))
    assert (1, True) in ran and (1, False) in ran
    assert len(per_instance) == 24 and len(want) == sum(1 for p in per_instance if p[0])
    for i, p in enumerate(per_instance):
        if i not in want:
            assert p == ((), 0, 0.0, 0.0)
            continue
        positions, rounds, residual, gap = want[i]
        assert p[0] == positions and p[1] == rounds, (i, p, want[i])
        assert abs(p[2] - residual) <= 1e-9 and abs(p[3] - gap) <= 1e-9, (i, p, want[i])
    assert totals[0] == len(want) and totals[1] == sum(1 for w in want.values() if not w[2] <= TOL)
    assert totals[2] == sum(w[1] for w in want.values())
    assert abs(totals[3] - sum(w[3] for w in want.values())) <= 1e-9 * len(want)
    assert totals[3] == sum(p[3] for p in per_instance) or abs(totals[3] - sum(p[3] for p in per_instance)) <= 1e-12
    assert max(w[3] for w in want.values()) > TOL          # stopping at three sweeps is visible at these thetas
    # one bucket on its own: host arrays
    tr = next(iter(tt.trainers.values()))
    rounds, residual, gap = tr.convergence(tol=TOL, max_rounds=max_rounds)
    assert rounds.dtype == np.int32 and residual.dtype == np.float64 and gap.shape == (tr.batch.B,)
