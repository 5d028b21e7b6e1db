"""Exact posterior sampling by cutset conditioning on the GPU (libmlbp_exactsample.so) against the NumPy statement of
include/mlbp_exactsample.h in tests/test_exactsample_cpu.py, and against exact_inference through the identity
logp = score(x) - log Z, which needs no statistics.

Bars.  Samples are compared exactly with the statement's: every input whose samples are compared is listed in
test_exactsample_cpu.INPUTS, where the statement's smallest margin is asserted to be at least MARGIN = 1e-8 before any device
is involved (cap on left-out (graph, sample) pairs: 0); the trainer fixture's margin is asserted here, before the device's
answer is looked at.  logp, log_z and score: rtol 1e-10, the project's tolerance for sums taken in another order.  The identity
is held to the bar tests/test_gpu_cutset.py holds joint_logp to: 1e-10 relative to max(1, |value|).  Bit-for-bit claims hold
across batch sizes, batch positions and sample counts: the header makes a sample's bits a function of the graph, the cutset and
the sample's uniforms alone."""
import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_exactsample_cpu as E
import test_map_cpu as W
from helpers import batch_tables, tidir_gold, tidir_oracle_graph, write_tidir
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

WEIGHTS_X64, DRAW_X64 = ('exactsample_weights_x64_kernel', ()), ('exactsample_draw_x64_kernel', ())
WEIGHTS_GENERIC, DRAW_GENERIC = ('exactsample_weights_generic_kernel', ()), ('exactsample_draw_generic_kernel', ())
SCAN = ('exactsample_scan_kernel', ())
X64, GENERIC = 1, 2
# kernel -> the tests that launch it (tests/test_exactsample_cpu.py holds this against the library's symbol table); every call
# runs a weights kernel, the scan and a draw kernel of the same form
_X64_TESTS = ['test_x64_kernel_equals_the_statement', 'test_both_sides_of_the_x64_lds_budget', 'test_trees_with_the_empty_and_a_redundant_cutset',
              'test_batch_position_and_sample_count_give_the_same_bits', 'test_shared_tables_give_the_same_bits', 'test_power_of_two_scaling',
              'test_zero_nan_inf_tables_and_bad_index', 'test_draw_rule_on_dyadic_weights', 'test_capture_and_replay_with_changed_tables_and_uniforms',
              'test_tidir_exact_sample']
_GENERIC_TESTS = ['test_generic_kernel_equals_the_statement', 'test_both_sides_of_the_x64_lds_budget', 'test_k3_x1024_vectors_in_the_workspace',
                  'test_trees_with_the_empty_and_a_redundant_cutset', 'test_batch_position_and_sample_count_give_the_same_bits',
                  'test_shared_tables_give_the_same_bits', 'test_power_of_two_scaling', 'test_zero_nan_inf_tables_and_bad_index',
                  'test_draw_rule_on_dyadic_weights']
CASES = {WEIGHTS_X64: _X64_TESTS, DRAW_X64: _X64_TESTS, WEIGHTS_GENERIC: _GENERIC_TESTS, DRAW_GENERIC: _GENERIC_TESTS,
         SCAN: ['test_x64_kernel_equals_the_statement', 'test_generic_kernel_equals_the_statement']}


def _M():
    from macaronicusermodeling_amd import exactsample
    return exactsample


def _batch(spec, inputs_list, tables=None, pair_tab=None, unary_tab=None, B=None):
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(spec)
    assert topo.var_ids == O.Graph(spec).var_order
    fb = FactorGraphBatch(topo, spec['X'], len(inputs_list) if B is None else B)
    pair, unary = batch_tables(spec, topo, inputs_list) if tables is None else tables
    if topo.P:
        fb.set_pair_tables(pair, pair_tab)
    if topo.U:
        fb.set_unary_tables(unary, unary_tab)
    return fb


def _run(fb, uniforms, cutset=None, kernel=None):
    """uniforms: numpy [S][B][n_vars] -> dict(x, logp, log_z, score)."""
    S = uniforms.shape[0]
    u = torch.from_numpy(np.ascontiguousarray(uniforms)).to(fb.device)
    msgs_before = fb.msgs.clone()
    x, logp, log_z, score = fb.exact_sample(n_samples=S, uniforms=u, cutset=cutset, log_z=True, score=True)
    ran = _M().last_kernel()
    torch.cuda.synchronize()
    assert x.dtype == torch.int32 and tuple(x.shape) == (S, fb.B, fb.topo.n_vars)
    assert logp.dtype == torch.float64 and tuple(logp.shape) == tuple(score.shape) == (S, fb.B) and tuple(log_z.shape) == (fb.B,)
    assert torch.equal(fb.msgs.view(torch.int64), msgs_before.view(torch.int64))          # self.msgs is left untouched (bits)
    if kernel is not None:
        assert ran == kernel, ran
    return dict(x=x.cpu().numpy(), logp=logp.cpu().numpy(), log_z=log_z.cpu().numpy(), score=score.cpu().numpy(), labels=x)


def _identity(name, fb, got, cutset=None):
    """logp of every draw is the joint_logp exact_inference gives the draw, and log_z its log_z."""
    worst = 0.0
    for s in range(got['x'].shape[0]):
        log_z, _, joint = fb.exact_inference(labels=got['labels'][s], cutset=cutset)
        log_z, joint = log_z.cpu().numpy(), joint.cpu().numpy()
        worst = max(worst, float((np.abs(got['logp'][s] - joint) / np.maximum(1.0, np.abs(joint))).max()),
                    float((np.abs(got['log_z'] - log_z) / np.maximum(1.0, np.abs(log_z))).max()))
        np.testing.assert_allclose(got['score'][s] - got['log_z'], joint, rtol=1e-10, atol=1e-10)
    print('%s: logp and log_z within %.1e of exact_inference(labels=samples)' % (name, worst))
    assert worst <= 1e-10, name


def _compare(name, spec, inputs, got, walks, stmts):
    g = O.Graph(spec)
    wrong = []
    for (s, b), w in sorted(walks.items()):
        x_dev = [int(v) for v in got['x'][s, b]]
        if x_dev != [w['x'][v] for v in g.var_order]:
            wrong.append((s, b, x_dev, w['x']))
            continue
        np.testing.assert_allclose(got['logp'][s, b], w['logp'], rtol=1e-10, err_msg='%s sample %d graph %d' % (name, s, b))
        np.testing.assert_allclose(got['score'][s, b], W.score_of(g, inputs[b], w['x']), rtol=1e-10)
    assert not wrong, (name, wrong[:6])
    np.testing.assert_allclose(got['log_z'], [st.log_z for st in stmts], rtol=1e-10)


def _case(name, kernel):
    """Family `name` of test_exactsample_cpu.INPUTS on `kernel`: the statement's samples, logp, log_z, score; the identity."""
    spec, inputs, cut, uniforms, walks, stmts = E.family(name)
    E.check_margin(name, walks)                                 # the CPU module asserts it too: before the device is looked at
    fb = _batch(spec, inputs)
    M = _M()
    pl = M.plan(fb.topo, None if cut is None else [fb.topo.var_index[v] for v in cut], fb.X, fb.device)
    assert M.pick_kernel(fb.X, fb.topo.n_vars, fb.topo.P, fb.topo.U, pl.n_forest) == kernel
    got = _run(fb, uniforms, cutset=cut, kernel=kernel)
    _compare(name, spec, inputs, got, walks, stmts)
    _identity(name, fb, got, cutset=cut)
    return fb, got


# ---- against the statement ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['k3_x64', 'k3_x64_lognormal', 'k4_x64', 'chain3_x64'])
def test_x64_kernel_equals_the_statement(name):
    """K3 with B = 5, S = 4 (one cutset variable, 64 configurations); K4 with B = 2, S = 3 (4096 configurations, the pairwise
    constant inside the cutset); a chain of three (the empty cutset: no uniform for the configuration, two tables on chip)."""
    if name == 'k4_x64':
        assert _M().chunks(2, 4096) == 256
    _case(name, X64)


@pytest.mark.parametrize('name', ['ring3_x2', 'ring3_x5', 'ring3_x65', 'k3_x128', 'chain260_x2', 'ring5_x7', 'forest_x9', 'double_pair_x6',
                                  'shuffled_x5', 'star4_x8'])
def test_generic_kernel_equals_the_statement(name):
    """Ring 3 at X = 2, 5 and 65 (one past a wave), K3 at X = 128, 259 forest edges at X = 2, and the small loopy families."""
    _case(name, GENERIC)


def test_both_sides_of_the_x64_lds_budget():
    """A chain of three at X = 64 keeps its two tables on chip; a chain of four (three tables) streams them."""
    M = _M()
    assert M.pick_kernel(64, 3, 2, 3, 2) == M.KERNEL_X64 and M.pick_kernel(64, 4, 3, 4, 3) == M.KERNEL_GENERIC
    _case('chain3_x64', X64)
    _case('chain4_x64', GENERIC)


def test_k3_x1024_vectors_in_the_workspace():
    M = _M()
    assert M.workspace_bytes(1, 1, 1024, 3, 3, 3, 1, 1) == (1024 * 3 + M.HEAD + 512 * 17 * 1024) * 8
    _case('k3_x1024', GENERIC)


def test_trees_with_the_empty_and_a_redundant_cutset():
    """On a tree the empty cutset is forward filtering, backward sampling; a redundant cutset spends the first uniform on the
    configuration, so the same uniforms need not give the same draws -- each draw's logp is still its joint_logp."""
    for plain, cut, kernel in (('chain3_x64', 'chain3_x64_cut1', X64), ('chain5_x8', 'chain5_x8_cut2', GENERIC)):
        _, a = _case(plain, kernel)
        _, b = _case(cut, kernel)
        np.testing.assert_allclose(a['log_z'], b['log_z'], rtol=1e-10)
    fb, _ = _case('chain5_x8', GENERIC)
    with pytest.raises(ValueError):
        fb.exact_sample(n_samples=1, seed=0, cutset=[9])
    with pytest.raises(_M().ExactSampleError, match='cycle'):
        _batch(*E.family('ring5_x7')[:2]).exact_sample(n_samples=1, seed=0, cutset=[])


# ---- bits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel', [('k3_x64', X64), ('ring5_x7', GENERIC)], ids=['x64', 'generic'])
def test_batch_position_and_sample_count_give_the_same_bits(name, kernel):
    """A graph alone (B = 1: its configurations and samples spread over many chunks) and at position 599 of B = 600 (one
    chunk); S = 2 against S = 64 (other chunk counts in the draw pass): the same samples and the same bits of logp."""
    M = _M()
    spec, inputs, _, _, _, _ = E.family(name)
    n = len(spec['var_ids'])
    rs = np.random.RandomState(77)
    u600, u64 = rs.rand(2, 600, n), rs.rand(64, 1, n)
    alone = _run(_batch(spec, inputs[1:2]), np.ascontiguousarray(u600[:, 599:600]), kernel=kernel)
    topo = _batch(spec, inputs[:1]).topo
    pair, unary = batch_tables(spec, topo, inputs)
    index = np.arange(600) % len(inputs)
    index[599] = 1
    ptab = np.arange(len(inputs) * topo.P).reshape(-1, topo.P)[index]
    utab = np.arange(len(inputs) * topo.U).reshape(-1, topo.U)[index]
    big = _run(_batch(spec, inputs, (pair, unary), ptab, utab, B=600), u600, kernel=kernel)
    assert M.chunks(1, spec['X']) != M.chunks(600, spec['X'])
    for key in ('x', 'logp', 'score'):
        assert np.array_equal(big[key][:, 599], alone[key][:, 0]), key
    assert big['log_z'][599] == alone['log_z'][0]
    assert (big['x'] >= 0).all() and np.isfinite(big['logp']).all()
    few = _run(_batch(spec, inputs[1:2]), u64[:2], kernel=kernel)
    many = _run(_batch(spec, inputs[1:2]), u64, kernel=kernel)
    for key in ('x', 'logp', 'score'):
        assert np.array_equal(many[key][:2], few[key]), key
    assert np.array_equal(many['log_z'], few['log_z'])


@pytest.mark.parametrize('name,kernel', [('k3_x64', X64), ('ring5_x7', GENERIC)], ids=['x64', 'generic'])
def test_shared_tables_give_the_same_bits(name, kernel):
    spec, inputs, _, uniforms, _, _ = E.family(name)
    inputs, uniforms = inputs[:4], np.ascontiguousarray(uniforms[:, :4])
    fb = _batch(spec, inputs)
    full = _run(fb, uniforms, kernel=kernel)
    pair, unary = batch_tables(spec, fb.topo, inputs)
    P, U = fb.topo.P, fb.topo.U
    ptab = np.arange(4 * P).reshape(4, P)
    utab = np.arange(4 * U).reshape(4, U)
    ptab[0], utab[0] = ptab[2], utab[2]                          # graphs 0 and 2 both read the tables of graph 2
    u2 = uniforms.copy()
    u2[:, 0] = uniforms[:, 2]
    shared = _run(_batch(spec, inputs, (pair, unary), ptab, utab), u2, kernel=kernel)
    for key in ('x', 'logp', 'score'):
        assert np.array_equal(shared[key][:, 0], full[key][:, 2]) and np.array_equal(shared[key][:, 1:], full[key][:, 1:]), key
    assert shared['log_z'][0] == full['log_z'][2] and np.array_equal(shared['log_z'][1:], full['log_z'][1:])


def test_power_of_two_scaling():
    """Tables times 2^+-400, unary rows times 2^+-500: the same samples and the same bits of logp; log_z and score move by k ln 2."""
    for name, kernel, moves in (('k3_x64_lognormal', X64, [({0: 400}, {}), ({2: -400}, {}), ({}, {0: 500}), ({}, {1: -500}),
                                                            ({0: 37, 1: -5, 2: 400}, {0: -300, 1: 3, 2: 500})]),
                                ('ring5_x7', GENERIC, [({0: 400}, {}), ({4: -400}, {}), ({}, {0: 500}), ({1: -400, 3: 400}, {2: -500})])):
        spec, inputs, _, uniforms, _, _ = E.family(name)
        inputs, uniforms = inputs[:2], np.ascontiguousarray(uniforms[:, :2])
        fb = _batch(spec, inputs)
        base = _run(fb, uniforms, kernel=kernel)
        pair, unary = batch_tables(spec, fb.topo, inputs)
        P, U = fb.topo.P, fb.topo.U
        for pk, uk in moves:
            p2, u2 = pair.copy(), unary.copy()
            for b in range(2):
                for p, k in pk.items():
                    p2[b * P + p] = np.ldexp(p2[b * P + p], k)
                for u, k in uk.items():
                    u2[b * U + u] = np.ldexp(u2[b * U + u], k)
            got = _run(_batch(spec, inputs, (p2, u2)), uniforms, kernel=kernel)
            shift = (sum(pk.values()) + sum(uk.values())) * np.log(2.0)
            assert np.array_equal(got['x'], base['x']) and np.array_equal(got['logp'], base['logp']), (name, pk, uk)
            np.testing.assert_allclose(got['log_z'], base['log_z'] + shift, rtol=1e-12)
            np.testing.assert_allclose(got['score'], base['score'] + shift, rtol=1e-12)


# ---- edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel', [('k3_x64', X64), ('ring5_x7', GENERIC)], ids=['x64', 'generic'])
def test_zero_nan_inf_tables_and_bad_index(name, kernel):
    """An all-zero table, a NaN, a +inf and a table index outside the array: -1 / NaN for that graph, log_z as
    include/mlbp_cutset.h gives it, and the bits of the base run for every neighbour."""
    spec, inputs, _, uniforms, _, _ = E.family(name)
    X = spec['X']
    inputs = [inputs[i % len(inputs)] for i in range(6)]
    uniforms = np.ascontiguousarray(uniforms[:, [i % uniforms.shape[1] for i in range(6)]])
    fb = _batch(spec, inputs)
    base = _run(fb, uniforms, kernel=kernel)
    pair, unary = batch_tables(spec, fb.topo, inputs)
    P = fb.topo.P
    p2 = pair.copy()
    p2[0 * P + 1][:] = 0.0                                       # graph 0: an all-zero table
    p2[1 * P + 0][3 % X, 1] = np.nan                             # graph 1: a NaN entry
    p2[2 * P + 2][0, 2 % X] = np.inf                             # graph 2: +inf
    fb2 = _batch(spec, inputs, (p2, unary))
    fb2.pair_tab[3, 1] = fb2.pair_tables.shape[0]                # graph 3: a table index outside the array
    got = _run(fb2, uniforms, kernel=kernel)
    for b in (0, 1, 2, 3):
        assert (got['x'][:, b] == -1).all() and np.isnan(got['logp'][:, b]).all() and np.isnan(got['score'][:, b]).all(), b
    assert got['log_z'][0] == -np.inf and not np.isfinite(got['log_z'][1]) and not np.isfinite(got['log_z'][2]) and np.isnan(got['log_z'][3])
    for b in (4, 5):
        for key in ('x', 'logp', 'score'):
            assert np.array_equal(got[key][:, b], base[key][:, b]), (key, b)
        assert got['log_z'][b] == base['log_z'][b]
    want = fb2.exact_inference()[0].cpu().numpy()                # what include/mlbp_cutset.h gives
    assert want[0] == -np.inf and not np.isfinite(want[1]) and not np.isfinite(want[2]) and np.isnan(want[3])


@pytest.mark.parametrize('X,kernel', [(64, X64), (5, GENERIC)], ids=['x64', 'generic'])
def test_draw_rule_on_dyadic_weights(X, kernel):
    """Weights whose sums are exact in any order (test_exactsample_cpu.dyadic_inputs): a uniform exactly on a boundary takes
    the next index, a zero-weight configuration or state is never drawn, and u = 1 (none crosses) takes the highest index of
    positive weight.  logp is compared exactly up to the rounding of three logarithms."""
    spec, inputs, uniforms, want = E.dyadic_inputs(X)
    st = E.statement(spec, inputs)
    fb = _batch(spec, [inputs])
    got = _run(fb, np.ascontiguousarray(uniforms[:, None, :]), kernel=kernel)
    assert got['x'][:, 0].tolist() == want == [[st.walk(u)['x'][v] for v in st.order] for u in uniforms]
    logp = np.array([st.walk(u)['logp'] for u in uniforms])
    np.testing.assert_allclose(got['logp'][:, 0], logp, rtol=1e-14)
    np.testing.assert_allclose(got['log_z'], [np.log(64.0)], rtol=1e-14)                  # Z = 4 * 4 * 4
    np.testing.assert_allclose(got['score'][:, 0], logp + np.log(64.0), rtol=1e-12, atol=1e-14)


# ---- errors ---------------------------------------------------------------------------------------------
def test_float32_tables_seed_and_uniforms_and_k5_are_refused():
    M = _M()
    spec = C.user_spec(10, [1, 4, 7], 256, 64, seed=1)
    fb = _batch(spec, [C.make_inputs(spec, 1)])
    fb.set_pair_tables(fb.pair_tables, dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        fb.exact_sample(n_samples=1, seed=0)
    spec, inputs, _, uniforms, _, _ = E.family('k3_x64')
    fb = _batch(spec, inputs)
    u = torch.from_numpy(uniforms).to(fb.device)
    with pytest.raises(ValueError, match='exactly one'):
        fb.exact_sample(n_samples=4, seed=0, uniforms=u)
    with pytest.raises(ValueError, match='exactly one'):
        fb.exact_sample(n_samples=4)
    with pytest.raises(ValueError):
        fb.exact_sample(n_samples=3, uniforms=u)                 # the shape is [4][B][n_vars]
    with pytest.raises(ValueError):
        fb.exact_sample(n_samples=0, seed=0)
    x, logp = fb.exact_sample(n_samples=4, seed=11)              # seed: the documented torch.rand call
    gen = torch.Generator(fb.device).manual_seed(11)
    x2, logp2 = fb.exact_sample(n_samples=4, uniforms=torch.rand((4, fb.B, fb.topo.n_vars), dtype=torch.float64, device=fb.device, generator=gen))
    assert torch.equal(x, x2) and torch.equal(logp.view(torch.int64), logp2.view(torch.int64))
    k5 = R.kn_spec(5, 64)
    with pytest.raises(M.ExactSampleError, match='configurations') as err:
        _batch(k5, [C.make_inputs(k5, 1)]).exact_sample(n_samples=1, seed=0)
    from macaronicusermodeling_amd import _ffi
    assert err.value.code == _ffi.MLBP_EUNSUPPORTED


# ---- capture --------------------------------------------------------------------------------------------
def test_capture_and_replay_with_changed_tables_and_uniforms():
    """After one eager call the call is captured; a replay gives the bits of the eager call, and after the tables and the
    uniforms are overwritten in place the bits of an eager call on the new ones."""
    spec, inputs, _, uniforms, _, _ = E.family('k3_x64')
    fb = _batch(spec, inputs[:2])
    u_first, u_other = np.ascontiguousarray(uniforms[:, :2]), np.ascontiguousarray(uniforms[:, 2:4])
    first = _run(fb, u_first, kernel=X64)
    other = _run(_batch(spec, inputs[2:4]), u_other, kernel=X64)
    assert not np.array_equal(first['x'], other['x'])
    u = torch.from_numpy(u_first).to(fb.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x, logp, log_z, score = fb.exact_sample(n_samples=u.shape[0], uniforms=u, log_z=True, score=True)
    pair, unary = batch_tables(spec, fb.topo, inputs[2:4])
    for want in (first, other):
        x.fill_(-5)
        for t in (logp, log_z, score):
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(x.cpu().numpy(), want['x']) and np.array_equal(logp.cpu().numpy(), want['logp'])
        assert np.array_equal(log_z.cpu().numpy(), want['log_z']) and np.array_equal(score.cpu().numpy(), want['score'])
        fb.pair_tables.copy_(torch.from_numpy(pair))
        fb.unary_tables.copy_(torch.from_numpy(unary))
        u.copy_(torch.from_numpy(u_other))


# ---- trainer --------------------------------------------------------------------------------------------
def test_tidir_exact_sample(tmp_path):
    """TiDirTrainer.exact_sample() on the clique fixture (K1 to K12 at X = 64, its own thetas): K1 to K4 against the statement
    on every instance's own graph, with the uniforms of the documented generator call; K5 and up listed as skipped."""
    from macaronicusermodeling_amd import tidir
    from test_gpu_cliques import _trainer
    gold = tidir_gold('tidir_cliques_reference')
    paths = write_tidir(gold, str(tmp_path))
    tt = _trainer(paths, gold)
    phi_ee, phi_w1, phi_ed = tidir.load_features(paths['phi.pmi'], paths['phi.pmi_w1'], paths['phi.ed'], paths['phi.ped'])
    th_ee, th_ed = np.array(gold['theta_en_en']).reshape(1, -1), np.array(gold['theta_en_de']).reshape(1, -1)
    n_samples, seed = 3, 40
    want, walks, too_large = {}, {}, {}
    for i, (key, tr) in enumerate(tt.trainers.items()):
        b = tt.buckets[key]
        if len(key[1]) >= 5:
            too_large[tuple(key[1])] = len(b['rows'])
            continue
        u = torch.rand((n_samples, tr.batch.B, tr.topo.n_vars), dtype=torch.float64, device=tr.device,
                       generator=torch.Generator(tr.device).manual_seed(seed + i)).cpu().numpy()
        for r, row in enumerate(b['rows']):
            g, inputs, _, _ = tidir_oracle_graph(key, b, r, phi_ee, phi_w1, phi_ed, th_ee, th_ed)
            assert tuple(g.var_order) == tuple(key[1])
            st = E.Statement(g, inputs, R.chosen_ids(g.spec))
            for s in range(n_samples):
                walks[row['index'], s] = st.walk(u[s, r])
            want[row['index']] = (tuple(key[1]), [[tt.en[walks[row['index'], s]['x'][v]] for v in key[1]] for s in range(n_samples)],
                                  [walks[row['index'], s]['logp'] for s in range(n_samples)])
    E.check_margin('clique fixture K1 to K4', walks)            # before the device's answer is looked at
    per_instance, skipped = tt.exact_sample(n_samples=n_samples, seed=seed)
    assert len(per_instance) == 11 and len(want) >= 4 and too_large
    seen = 0
    for key, b in tt.buckets.items():
        for row in b['rows']:
            got = per_instance[row['index']]
            if tuple(key[1]) in too_large:
                assert got == (tuple(key[1]), None, None)
                continue
            positions, words, logp = got
            assert positions == want[row['index']][0] and words == want[row['index']][1], (key, words)
            np.testing.assert_allclose(logp, want[row['index']][2], rtol=1e-10)
            seen += 1
    assert seen == len(want)
    assert sorted(s[0] for s in skipped) == sorted(too_large) and all('configurations' in s[2] for s in skipped)
    assert sum(s[1] for s in skipped) == sum(too_large.values())
    key = next(k for k in tt.trainers if len(k[1]) == 3)
    x, lp = tt.trainers[key].exact_sample(n_samples=2, seed=5)
    assert x.dtype == np.int64 and lp.dtype == np.float64 and x.shape == (2, tt.trainers[key].batch.B, 3) and lp.shape == x.shape[:2]
    assert _M().last_kernel() == X64
