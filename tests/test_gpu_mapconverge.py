"""Max-product sweeps to convergence on the GPU (the max-product mode of libmlbp_converge.so, FactorGraphBatch.map_converge)
against the float64 NumPy walk of tests/test_mapconverge_cpu.py.

Tolerances, the converge library's own: `rounds` exactly, residual and history 1e-9 absolute, messages and max-marginals rtol
1e-10 (atol 1e-300), assignments equal, scores 1e-12.  tests/test_mapconverge_cpu.py says why rounds and assignments may be
compared exactly and which cases' messages may be compared at all (MC.check_walks: asserted there without a device and here
again before the device is looked at, for every graph, none left out).  The walks are computed once per case and never changed.

The shipped max-product kernels are the second reference: one round from uniform messages is map_sweep(roots) in every bit.
The sum mode is held to the bits it had before the mode existed (tests/golden/converge_sum_bits.json, recorded through the
parent's library by tests/golden/make_converge_bits.py)."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import cases as C
import test_converge_cpu as CV
import test_map_cpu as W
import test_mapconverge_cpu as MC
from helpers import batch_tables, tidir_oracle_graph
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

TOL = MC.TOL
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'converge_sum_bits.json')
# case -> (MLBP_CONVERGE_KERNEL_*, tables resident)
KERNEL_OF = {'k3_x64': (1, True), 'k4_x64': (1, False), 'k4_x64_short': (1, False), 'star31_x64': (2, False), 'k3_x5': (2, True),
             'k3_x65': (2, True), 'ring8_x4': (2, False), 'k3_x64_one': (1, True)}
OUT_KEYS = ('x', 'score', 'rounds', 'residual', 'history', 'msgs', 'mm')


def _V():
    from macaronicusermodeling_amd import converge
    return converge


def _batch(spec, inputs_list):
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(spec)
    fb = FactorGraphBatch(topo, spec['X'], len(inputs_list))
    pair, unary = batch_tables(spec, topo, inputs_list)
    if topo.P:
        fb.set_pair_tables(pair)
    if topo.U:
        fb.set_unary_tables(unary)
    return fb


def _run(fb, roots=None, tol=TOL, max_rounds=20, init=True):
    mm = torch.full((fb.B, fb.topo.n_vars, fb.X), float('nan'), dtype=torch.float64, device=fb.device)
    if init:
        fb.msgs.fill_(float('nan'))                      # init=True must not read them
    x, score, rounds, residual, history = fb.map_converge(roots, tol=tol, max_rounds=max_rounds, init=init, max_marginals=mm, history=True)
    kernel = _V().last_kernel()
    torch.cuda.synchronize()
    assert x.dtype == torch.int32 and tuple(x.shape) == (fb.B, fb.topo.n_vars) and score.dtype == torch.float64
    assert rounds.dtype == torch.int32 and tuple(rounds.shape) == tuple(score.shape) == tuple(residual.shape) == (fb.B,)
    assert tuple(history.shape) == (fb.B, max_rounds)
    return dict(x=x.cpu().numpy(), score=score.cpu().numpy(), rounds=rounds.cpu().numpy(), residual=residual.cpu().numpy(),
                history=history.cpu().numpy(), msgs=fb.msgs.cpu().numpy().copy(), mm=mm.cpu().numpy(), kernel=kernel)


def _same_bits(a, b, rows=slice(None), rows_b=None, keys=OUT_KEYS):
    rows_b = rows if rows_b is None else rows_b
    for k in keys:
        assert np.array_equal(a[k][rows], b[k][rows_b], equal_nan=True), k


def _compare(name, topo, got, walks, graphs=None):
    for i, b in enumerate(range(len(walks)) if graphs is None else graphs):
        w = walks[i]
        tag = '%s graph %d' % (name, b)
        assert got['rounds'][b] == w['rounds'], (tag, got['rounds'][b], w['history'], got['history'][b])
        np.testing.assert_allclose(got['residual'][b], w['residual'], rtol=0, atol=1e-9, err_msg=tag)
        np.testing.assert_allclose(got['history'][b, :w['rounds']], w['history'], rtol=0, atol=1e-9, err_msg=tag)
        assert (got['history'][b, w['rounds']:] == -1.0).all(), tag
        assert got['history'][b, w['rounds'] - 1] == got['residual'][b], tag
        want = np.stack([w['msgs'][k] for k in topo.slot_keys()])
        np.testing.assert_allclose(got['msgs'][b], want, rtol=1e-10, atol=1e-300, err_msg=tag)
        want = np.stack([w['mm'][v] for v in topo.var_ids])
        np.testing.assert_allclose(got['mm'][b], want, rtol=1e-10, atol=1e-300, err_msg=tag)
        assert got['x'][b].tolist() == [w['x'][v] for v in topo.var_ids], tag
        np.testing.assert_allclose(got['score'][b], w['score'], rtol=1e-12, atol=1e-12, err_msg=tag)


def _gpu_case(name):
    spec, inputs, walks, max_rounds, roots = MC.gpu_case(name)
    MC.check_walks(name, walks, max_rounds, name in MC.SETTLES)          # before the device is looked at
    fb = _batch(spec, inputs)
    assert (_V().pick_kernel(spec['X'], fb.topo.n_msgs, fb.topo.n_vars), fb.topo.P <= 3) == KERNEL_OF[name]
    return spec, inputs, walks, max_rounds, roots, fb


# ---- against the walk ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(MC.GPU_CASES))
def test_the_walk(name):
    spec, inputs, walks, max_rounds, roots, fb = _gpu_case(name)
    got = _run(fb, roots=roots, max_rounds=max_rounds)
    assert got['kernel'] == KERNEL_OF[name][0]
    print('%s: rounds %r residual %s' % (name, got['rounds'].tolist(), ['%.2e' % r for r in got['residual']]))
    _compare(name, fb.topo, got, walks)
    if name == 'star31_x64':
        assert fb.topo.n_msgs > 150


# ---- against the shipped max-product kernels ----------------------------------------------------------------
@pytest.mark.parametrize('name', ['k3_x64', 'k4_x64', 'star31_x64', 'k3_x5', 'k3_x65', 'ring8_x4'])
def test_one_round_equals_map_sweep(name):
    """One round from uniform messages IS map_sweep(roots): messages, max-marginals, assignment and score, bit for bit."""
    spec, inputs, _, _, _, fb = _gpu_case(name)
    for roots in (list(fb.topo.var_ids), [fb.topo.var_ids[-1], fb.topo.var_ids[0]]):
        mm = torch.empty(fb.B, fb.topo.n_vars, fb.X, dtype=torch.float64, device=fb.device)
        x, score = fb.map_sweep(roots, init=True, max_marginals=mm)
        torch.cuda.synchronize()
        want = dict(x=x.cpu().numpy(), score=score.cpu().numpy(), msgs=fb.msgs.cpu().numpy().copy(), mm=mm.cpu().numpy())
        got = _run(fb, roots=roots, tol=0.0, max_rounds=1)
        assert got['kernel'] == KERNEL_OF[name][0] and (got['rounds'] == 1).all() and (got['residual'] > 0).all()
        _same_bits(got, want, keys=('x', 'score', 'msgs', 'mm'))


@pytest.mark.parametrize('X', [64, 5])
def test_trees_decode_the_exact_map(X):
    """A chain: two rounds at tol = 0, residual exactly 0.0, and exact_map()'s assignment and score."""
    spec = C.chain_spec(4, X)
    inputs = [C.make_inputs(spec, s, kind) for s, kind in ((1, 'uniform'), (2, 'lognormal'), (3, 'lognormal'))]
    fb = _batch(spec, inputs)
    got = _run(fb, tol=0.0, max_rounds=6)
    assert (got['rounds'] == 2).all() and (got['residual'] == 0.0).all(), (got['rounds'], got['residual'])
    x, score = fb.exact_map()
    torch.cuda.synchronize()
    assert np.array_equal(got['x'], x.cpu().numpy())
    np.testing.assert_allclose(got['score'], score.cpu().numpy(), rtol=1e-12, atol=1e-12)
    walks = [MC.walk(spec, inp, tol=0.0, max_rounds=6) for inp in inputs]
    MC.check_walks('chain4_x%d' % X, walks, 6, True)
    _compare('chain4_x%d' % X, fb.topo, got, walks)


def test_warm_start():
    """map_sweep(every variable once) is round 1; map_converge(init=False) then runs the walk's remaining rounds."""
    name = 'k3_x64'
    spec, inputs, walks, max_rounds, roots, fb = _gpu_case(name)
    warm = []
    for inp in inputs:
        first = MC.walk(spec, inp, max_rounds=1)
        warm.append(MC.walk(spec, inp, max_rounds=max_rounds, msgs=first['msgs']))
    MC.check_walks(name + ' warm', warm, max_rounds, True)
    assert [w['rounds'] for w in warm] == [w['rounds'] - 1 for w in walks]
    fb.map_sweep(list(fb.topo.var_ids), init=True)
    got = _run(fb, max_rounds=max_rounds, init=False)
    _compare(name + ' warm', fb.topo, got, warm)


def test_power_of_two_scaling_gives_the_same_bits():
    """Every table of graph b times 2^p_b: every normalised output keeps its bits (the score moves by the logs of the powers)."""
    spec, inputs, _, max_rounds, _, fb = _gpu_case('k3_x64')
    got = _run(fb, max_rounds=max_rounds)
    powers = [200, -200, 64, -1, 137, -90, 3]
    scaled = [dict(tables=[t * 2.0 ** p for t in inp['tables']]) for inp, p in zip(inputs, powers)]
    again = _run(_batch(spec, scaled), max_rounds=max_rounds)
    _same_bits(again, got, keys=('x', 'rounds', 'residual', 'history', 'msgs', 'mm'))
    n_factors = len(spec['factors'])
    np.testing.assert_allclose(again['score'], got['score'] + n_factors * np.log(2.0) * np.array(powers), rtol=1e-12)


@pytest.mark.parametrize('name,one', [('k3_x64', 'k3_x64_one'), ('k3_x5', None)])
def test_a_graph_alone_gives_the_bits_it_has_in_the_batch(name, one):
    spec, inputs, _, max_rounds, _, fb = _gpu_case(name)
    got = _run(fb, max_rounds=max_rounds)
    if one is not None:                                  # the B = 1 case is graph 3 of the B = 7 case
        assert MC.GPU_CASES[one][1] == [MC.GPU_CASES[name][1][3]]
    for b in ([3] if one else range(len(inputs))):
        alone = _run(_batch(spec, [inputs[b]]), max_rounds=max_rounds)
        assert alone['kernel'] == got['kernel']
        _same_bits(alone, got, rows=slice(0, 1), rows_b=slice(b, b + 1))


@pytest.mark.parametrize('name', ['k3_x64', 'k4_x64', 'k3_x65'])
def test_a_refused_graph_leaves_its_neighbours_alone(name):
    """A table index out of range: assignment -1, score NaN, rounds -1, residual NaN, history NaN, messages and max-marginals
    untouched; the other graphs keep their bits.  A variable index out of range in the decode's arrays refuses every graph."""
    spec, inputs, _, max_rounds, _, fb = _gpu_case(name)
    clean = _run(fb, max_rounds=max_rounds)
    fb.pair_tab[1, 2] = fb.pair_tables.shape[0]
    fb.unary_tab[2, 0] = -1
    fb.msgs.fill_(7.0)
    mm = torch.full((fb.B, fb.topo.n_vars, fb.X), 5.0, dtype=torch.float64, device=fb.device)
    out = fb.map_converge(tol=TOL, max_rounds=max_rounds, init=True, max_marginals=mm, history=True)
    torch.cuda.synchronize()
    got = dict(zip(('x', 'score', 'rounds', 'residual', 'history'), (t.cpu().numpy() for t in out)), msgs=fb.msgs.cpu().numpy(), mm=mm.cpu().numpy())
    for b in (1, 2):
        assert (got['x'][b] == -1).all() and np.isnan(got['score'][b])
        assert got['rounds'][b] == -1 and np.isnan(got['residual'][b]) and np.isnan(got['history'][b]).all()
        assert (got['msgs'][b] == 7.0).all() and (got['mm'][b] == 5.0).all()
    _same_bits(got, clean, rows=[0])
    # the decode's own indices
    V = _V()
    fb = _batch(spec, inputs)
    prog = V.program(fb.topo, fb.topo.var_ids, fb.device)
    for arr, at in ((prog.pair_axis_var, 1), (prog.unary_var, 0)):
        kept = arr.clone()
        try:
            arr.view(-1)[at] = fb.topo.n_vars
            fb.msgs.fill_(7.0)
            x, score, rounds, residual = fb.map_converge(tol=TOL, max_rounds=max_rounds)
            torch.cuda.synchronize()
            assert (x.cpu().numpy() == -1).all() and np.isnan(score.cpu().numpy()).all()
            assert (rounds.cpu().numpy() == -1).all() and (fb.msgs.cpu().numpy() == 7.0).all()
        finally:
            arr.copy_(kept)
    _same_bits(_run(fb, max_rounds=max_rounds), clean)


def test_capture_and_replay():
    """After one eager call the call is captured (one stream, no parallel branch) and replayed twice: the bits of the eager call."""
    spec, inputs, _, max_rounds, _, fb = _gpu_case('k3_x64')
    eager = _run(fb, max_rounds=max_rounds)
    mm = torch.empty(fb.B, fb.topo.n_vars, fb.X, dtype=torch.float64, device=fb.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x, score, rounds, residual, history = fb.map_converge(tol=TOL, max_rounds=max_rounds, init=True, max_marginals=mm, history=True)
    for _ in range(2):
        for t in (score, residual, history, mm, fb.msgs):
            t.fill_(float('nan'))
        rounds.fill_(-7)
        x.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        replayed = dict(x=x.cpu().numpy(), score=score.cpu().numpy(), rounds=rounds.cpu().numpy(), residual=residual.cpu().numpy(),
                        history=history.cpu().numpy(), msgs=fb.msgs.cpu().numpy(), mm=mm.cpu().numpy())
        _same_bits(replayed, eager)


# ---- the sum mode is what it was ---------------------------------------------------------------------------
def golden_batches():
    """name -> (batch, max_rounds): the sum-product cases of tests/test_converge_cpu.py, one per kernel instance."""
    out = {}
    for name in ('k3_x64', 'k4_x64', 'k3_x65'):
        spec, inputs, _, max_rounds = CV.gpu_case(name)
        out[name] = (_batch(spec, inputs), max_rounds)
    return out


def golden_record(fb, max_rounds):
    """Every output of converge() on `fb`: rounds as integers, residual and history as hex floats, the messages and the
    marginals as the SHA-256 of their bytes."""
    marg = torch.empty(fb.B, fb.topo.n_vars, fb.X, dtype=torch.float64, device=fb.device)
    rounds, residual, history = fb.converge(tol=CV.TOL, max_rounds=max_rounds, init=True, marginals=marg, history=True)
    torch.cuda.synchronize()
    sha = lambda t: hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()          # noqa: E731
    return dict(rounds=rounds.cpu().numpy().tolist(), residual=[float(v).hex() for v in residual.cpu().numpy()],
                history=[float(v).hex() for v in history.cpu().numpy().reshape(-1)], msgs=sha(fb.msgs), marginals=sha(marg))


@pytest.mark.parametrize('name', ['k3_x64', 'k4_x64', 'k3_x65'])
def test_the_sum_mode_computes_the_bits_it_computed_before(name):
    """max_product = 0 with the new fields in the struct: converge() on the sum-product cases equals, in every bit, what the
    library returned before it had a max-product mode."""
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    fb, max_rounds = golden_batches()[name]
    assert golden_record(fb, max_rounds) == want
    V = _V()
    assert [f[0] for f in V.ConvergeArgs._fields_[-5:]] == ['max_product', 'assignment', 'score', 'pair_axis_var', 'unary_var']


def test_host_refusals_on_a_device():
    """The refusal the header puts behind the device check, and the Python layer's."""
    spec, inputs, _, _, _, fb = _gpu_case('k3_x64')
    V = _V()
    from macaronicusermodeling_amd import _ffi
    a = CV._valid_args(V)                                # every pointer set, max_product 0: refused before anything is enqueued
    assert V.lib.mlbp_converge_f64(ctypes.byref(a), None) == _ffi.MLBP_EINVAL and 'without max_product' in V.last_error()
    assert V.last_kernel() == V.KERNEL_NONE
    for kwargs in (dict(tol=-1.0), dict(max_rounds=0), dict(max_rounds=65536)):
        with pytest.raises((V.ConvergeError, ValueError)):
            fb.map_converge(**kwargs)
    with pytest.raises(ValueError):
        fb.map_converge(max_marginals=torch.empty(1, 1, 1, dtype=torch.float64, device=fb.device))
    fb.normalize_messages = False
    with pytest.raises(ValueError):
        fb.map_converge()
    fb.normalize_messages = True
    fb.use_approx_inference = True
    with pytest.raises(NotImplementedError):
        fb.map_converge()
    fb.use_approx_inference = False
    assert len(fb.map_converge(max_rounds=2)) == 4


# ---- search decoding from the settled entry ---------------------------------------------------------------
def test_search_map_from_the_settled_entry():
    """entry0='settled': the score never lies below the settled score (the settled assignment is among those the list admits), and
    map_sweep's score comes back beside it.  The default call is the sequence of calls it was, bit for bit."""
    spec = CV.clique_spec(5, 64)
    inputs = [CV.scaled_inputs(spec, s, seed) for s, seed in ((0.5, 0), (1, 1), (2, 2))]
    fb = _batch(spec, inputs)
    fb.initialize()
    roots, N = list(fb.topo.var_ids), 16
    x, score, score_settled, score_bp = (t.cpu().numpy() for t in fb.search_map(roots, n_samples=N, seed=5, entry0='settled', max_rounds=20))
    x_s, s_s = (t.cpu().numpy() for t in fb.map_converge(roots, max_rounds=20)[:2])
    x_bp, s_bp = (t.cpu().numpy() for t in fb.map_sweep(roots, init=True))
    assert np.array_equal(score_settled, s_s) and np.array_equal(score_bp, s_bp)
    assert (score >= score_settled - 1e-9 * np.maximum(1.0, np.abs(score))).all(), score - score_settled
    one = fb.search_map(roots, n_samples=1, entry0='settled', max_rounds=20)
    assert (one[1].cpu().numpy() >= s_s - 1e-9 * np.maximum(1.0, np.abs(s_s))).all()
    ranked = fb.search_mbest(roots, 2, n_samples=N, seed=5, entry0='settled', max_rounds=20)
    assert len(ranked) == 5 and np.array_equal(ranked[3].cpu().numpy(), s_s) and np.array_equal(ranked[1][:, 0].cpu().numpy(), score)
    with pytest.raises(ValueError):
        fb.search_map(roots, n_samples=N, entry0='other')
    # the default: map_sweep, sweep, cutset_draw, cutset_map, as the call was written before it took entry0
    got = [t.cpu().numpy() for t in fb.search_map(roots, n_samples=N, seed=5)]
    assert len(got) == 3
    from macaronicusermodeling_amd import cutset as K0, cutsetis as KP
    pl, _ = fb._cutset_args(KP, KP.CutsetisArgs, None, '')
    cut = [int(v) for v in pl.words[K0.PLAN_HEADER:K0.PLAN_HEADER + pl.n_cut]]
    assert len(cut) >= 2
    x0, s0 = fb.map_sweep(roots, init=True)
    fb.sweep(roots, init=True)
    configs = torch.empty(fb.B, N, len(cut), dtype=torch.int32, device=fb.device)
    configs[:, 0] = x0.index_select(1, torch.tensor(cut, dtype=torch.int64, device=fb.device))
    configs[:, 1:] = fb.cutset_draw(N - 1, seed=5)[0]
    want = [t.cpu().numpy() for t in fb.cutset_map(configs)] + [s0.cpu().numpy()]
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ---- trainers ----------------------------------------------------------------------------------------------
def test_settled_decode_of_both_trainers(tmp_path):
    """TiDirTrainer.settled_decode() on a synthetic file: every instance against the walk on its own graph over the predict()
    schedule (max_rounds = 5, so every instance may be compared, settled or not); the totals are recomputed from the rows;
    UserGraphTrainer.settled_decode gives the same numbers as host arrays."""
    from macaronicusermodeling_amd import tidir
    from macaronicusermodeling_amd.train import SEARCH_ROSE, TiDirTrainer
    paths = tidir.synthesize(str(tmp_path), n_instances=24, X=64, Vde=64, sent_len=(4, 7), n_predicted=(1, 4), seed=9)
    tt = TiDirTrainer(paths['ti'], paths['end'], paths['ded'], paths['phi_pmi'], paths['phi_pmi_w1'], paths['phi_ed'], paths['phi_ped'], sweeps=3)
    phi_ee, phi_w1, phi_ed = tidir.load_features(paths['phi_pmi'], paths['phi_pmi_w1'], paths['phi_ed'], paths['phi_ped'])
    rs = np.random.RandomState(1)
    th_ee, th_ed = rs.randn(1, 3) * 0.6, rs.randn(1, 6) * 0.6
    tt.theta_en_en.copy_(torch.from_numpy(th_ee.reshape(-1)))
    tt.theta_en_de.copy_(torch.from_numpy(th_ed.reshape(-1)))
    max_rounds = 5
    want, walks = {}, []
    for key, b in tt.buckets.items():
        for r, row in enumerate(b['rows']):
            g, inputs, roots, _ = tidir_oracle_graph(key, b, r, phi_ee, phi_w1, phi_ed, th_ee, th_ed)
            n = 3 if O.has_loops(g, roots[0]) else 1
            assert n == tt.trainers[key].n_sweeps_run
            w = MC.walk(g.spec, inputs, roots=roots[:n], tol=TOL, max_rounds=max_rounds)
            plain = W.walk(g.spec, inputs, roots[:n])
            want[row['index']] = (tuple(key[1]), w, plain)
            walks.append(w)
    MC.check_walks('synthetic file', walks, max_rounds, False)
    guesses, totals, reached = tt.settled_decode(tol=TOL, max_rounds=max_rounds)
    assert len(guesses) == 24
    tally = np.zeros(5, dtype=np.int64)
    for i, p in enumerate(guesses):
        if i not in want:
            assert p == ((), [], 0.0, 0, 0.0, 0.0)
            continue
        positions, w, plain = want[i]
        assert p[0] == positions and p[1] == [tt.en[w['x'][v]] for v in positions], (i, p)
        np.testing.assert_allclose(p[2], w['score'], rtol=1e-12, atol=1e-12)
        assert p[3] == w['rounds'] and abs(p[4] - w['residual']) <= 1e-9, (i, p, w['history'])
        np.testing.assert_allclose(p[5], w['score'] - plain['score'], rtol=0, atol=1e-10)
        gain, bar = w['score'] - plain['score'], SEARCH_ROSE * max(1.0, abs(w['score']))
        assert abs(abs(gain) - bar) > 1e-10                  # no gain sits on the bar the totals count against
        tally += [1, w['residual'] <= TOL, gain > bar, gain < -bar, w['x'] != plain['x']]
    assert totals == tuple(int(v) for v in tally), (totals, tally)
    assert reached[0] == totals[0] and 0 <= reached[1] <= reached[0] and reached[3] >= 0.0          # K1 to K4: exact_map() answers all
    # one shape on its own: host arrays
    key, tr = next(iter(tt.trainers.items()))
    x, score, rounds, residual, gain = tr.settled_decode(tol=TOL, max_rounds=max_rounds)
    assert x.dtype == np.int64 and rounds.dtype == np.int32 and score.dtype == residual.dtype == gain.dtype == np.float64
    for b, row in enumerate(tt.buckets[key]['rows']):
        _, w, plain = want[row['index']]
        assert x[b].tolist() == [w['x'][v] for v in key[1]] and rounds[b] == w['rounds']
        np.testing.assert_allclose(score[b], w['score'], rtol=1e-12, atol=1e-12)
