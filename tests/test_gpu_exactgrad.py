"""Exact pair marginals, expected features and the true gradient on the GPU (libmlbp_exactgrad.so) against the float64
references of tests/test_exactgrad_cpu.py and tests/test_cutset_cpu.py: exhaustive enumeration in the log domain where X^n
allows it, NumPy elimination (einsum) beyond -- each pinned on enumeration there.

Bars.  pair_marginals and marginals within 1e-10 absolute, log_z within 1e-10 * max(1, |log_z|): library six's.  expect_* and
grad_* against the NumPy contraction of the tensors THE SAME CALL returned, phi in [-1, 1], within (P + U) * max(1e-12, X^2 *
2^-51): a sum of X^2 terms whose absolute values sum to at most 1, reordered, moves by at most X^2 * 2^-53 per factor; the bar
is four times that.  With the pair-marginal bar this pins the gradient on enumeration.  Rows and columns of every M_p sum to the
marginals of the same call at X * 2^-50.  Bit-for-bit claims compare graphs at an equal number of chunks."""
import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_exactgrad_cpu as G
from helpers import batch_tables, tidir_oracle_graph
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

X64_1 = ('exactgrad_x64_kernel', (1,))
X64_2 = ('exactgrad_x64_kernel', (2,))
GENERIC = ('exactgrad_generic_kernel', ())
COMBINE = ('exactgrad_combine_kernel', ())
# kernel -> the tests that launch it (tests/test_exactgrad_cpu.py holds this against the library's symbol table)
CASES = {
    X64_1: ['test_k3_x64_against_enumeration', 'test_k4_x64_against_elimination', 'test_double_pair_x64', 'test_cutset_override_and_redundant_cutset',
            'test_shared_tables_and_batch_position_give_the_same_bits', 'test_power_of_two_scaling', 'test_edge_rules', 'test_capture_and_replay',
            'test_tidir_gradient_report_and_exact_step'],
    X64_2: ['test_chain3_x64_two_forest_factors', 'test_both_sides_of_the_x64_budget', 'test_trees_equal_the_shipped_pair_beliefs'],
    GENERIC: ['test_small_graphs_on_the_generic_kernel', 'test_generic_sizes_on_ring3', 'test_both_sides_of_the_x64_budget',
              'test_trees_equal_the_shipped_pair_beliefs', 'test_shared_tables_and_batch_position_give_the_same_bits', 'test_edge_rules',
              'test_exact_step_ascends_the_true_likelihood'],
    COMBINE: ['test_k3_x64_against_enumeration', 'test_k4_x64_against_elimination', 'test_small_graphs_on_the_generic_kernel'],
}
KERNEL_OF = {X64_1: 1, X64_2: 1, GENERIC: 2}


def _M():
    from macaronicusermodeling_amd import exactgrad
    return exactgrad


def _batch(spec, inputs_list, tables=None, pair_tab=None, unary_tab=None, labels=None, obs=None, seed=0):
    """The batch with its tables, features (phi in [-1, 1], unary factors of all three kinds in turn, Vde = X + 3), labels and
    observed columns; what NumPy needs to restate the call rides along as fb.ref."""
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(spec)
    g = O.Graph(spec)
    assert topo.var_ids == g.var_order
    B, X = len(inputs_list), spec['X']
    fb = FactorGraphBatch(topo, X, B)
    pair, unary = batch_tables(spec, topo, inputs_list) if tables is None else tables
    if topo.P:
        fb.set_pair_tables(pair, pair_tab)
    if topo.U:
        fb.set_unary_tables(unary, unary_tab)
    feat = G.make_features(g, 77, kinds=[0, 1, 2])
    pair_ids = [topo.factor_ids[j] for j in topo.pair_factors]
    unary_ids = [topo.factor_ids[j] for j in topo.unary_factors]
    kinds = [feat['sel'][f] for f in unary_ids]
    fb.set_features(feat['phi_en_en'], feat['phi_en_en_w1'], feat['phi_en_de'], [feat['sel'][f] for f in pair_ids], kinds)
    rs = np.random.RandomState(seed)
    Vde = feat['phi_en_de'].shape[1]
    assert Vde != X
    if labels is None:
        labels = rs.randint(0, X, size=(B, topo.n_vars)).astype(np.int32)
    if obs is None:
        obs = np.array([[rs.randint(0, Vde if k == 2 else X) for k in kinds] for _ in range(B)], dtype=np.int32).reshape(B, topo.U)
    fb.set_observations(labels, obs)
    fb.ref = dict(g=g, feat=feat, labels=labels, obs=obs, pair_ids=pair_ids, unary_ids=unary_ids)
    return fb


def _run(fb, cutset=None, kernel=None, labels=None):
    """One full call (every output), then the lean calls, which must repeat its bits."""
    M = _M()
    topo, nan = fb.topo, float('nan')
    pm = torch.full((fb.B, topo.P, fb.X, fb.X), nan, dtype=torch.float64, device=fb.device)
    mg = torch.full((fb.B, topo.n_vars, fb.X), nan, dtype=torch.float64, device=fb.device)
    g_ee, g_ed, log_z = fb.exact_gradient(labels=labels, pair_marginals=pm, marginals=mg, cutset=cutset)
    ran = M.last_kernel()
    e_ee, e_ed, log_z2 = fb.exact_gradient(expect_only=True, cutset=cutset)
    l_ee, l_ed, _ = fb.exact_gradient(labels=labels, cutset=cutset)
    pm2 = fb.exact_pair_marginals(cutset=cutset)
    torch.cuda.synchronize()
    if kernel is not None:
        assert ran == KERNEL_OF[kernel], ran
    got = dict(log_z=log_z.cpu().numpy(), marg=mg.cpu().numpy(), pm=pm.cpu().numpy(), grad_ee=g_ee.cpu().numpy(), grad_ed=g_ed.cpu().numpy(),
               exp_ee=e_ee.cpu().numpy(), exp_ed=e_ed.cpu().numpy(), kernel=ran)
    assert np.array_equal(got['log_z'], log_z2.cpu().numpy(), equal_nan=True) and np.array_equal(got['pm'], pm2.cpu().numpy(), equal_nan=True)
    assert np.array_equal(got['grad_ee'], l_ee.cpu().numpy(), equal_nan=True) and np.array_equal(got['grad_ed'], l_ed.cpu().numpy(), equal_nan=True)
    return got


def _feat_of(fb, b):
    ref = fb.ref
    return dict(ref['feat'], obs={fid: int(ref['obs'][b, u]) for u, fid in enumerate(ref['unary_ids'])})


def _check_features(name, fb, got, graphs=None):
    """expect_* and grad_* against the NumPy contraction of the pair marginals and marginals the same call returned."""
    ref, topo, X = fb.ref, fb.topo, fb.X
    g = ref['g']
    bar = (topo.P + topo.U) * max(1e-12, X * X * 2.0 ** -51)
    worst = 0.0
    for b in range(fb.B) if graphs is None else graphs:
        feat = _feat_of(fb, b)
        ex = G.features_of(g, feat, got['marg'][b], {fid: got['pm'][b, p] for p, fid in enumerate(ref['pair_ids'])})
        ob = G.observed_of(g, feat, dict(zip(g.var_order, (int(x) for x in ref['labels'][b]))))
        for key, want in (('exp_ee', ex[0]), ('exp_ed', ex[1]), ('grad_ee', ob[0] - ex[0]), ('grad_ed', ob[1] - ex[1])):
            worst = max(worst, float(np.abs(got[key][b] - want).max()))
    print('%s: expect_* and grad_* within %.1e of the contraction of the returned tensors (bar %.1e)' % (name, worst, bar))
    assert worst <= bar, name
    assert np.abs(got['exp_ee']).max() > 0 and (np.abs(got['exp_ed']).max() > 0) == (2 in [int(k) for k in fb._unary_kind_host])


def _check_consistency(name, fb, got, graphs=None):
    from macaronicusermodeling_amd import cutset as S
    X = fb.X
    worst = 0.0
    for b in range(fb.B) if graphs is None else graphs:
        for p, (a, c) in enumerate(S.pair_edges(fb.topo)):
            worst = max(worst, float(np.abs(got['pm'][b, p].sum(axis=1) - got['marg'][b, a]).max()),
                        float(np.abs(got['pm'][b, p].sum(axis=0) - got['marg'][b, c]).max()))
            assert abs(got['pm'][b, p].sum() - 1) <= X * 2.0 ** -50
    print('%s: rows and columns of every M_p sum to the marginals within %.1e (bar %.1e)' % (name, worst, X * 2.0 ** -50))
    assert worst <= X * 2.0 ** -50, name


def _compare(name, fb, got, refs):
    """refs: [(log_z, marginals, {factor id: M})] per graph."""
    wz = wm = wp = 0.0
    for b, (z, m, pairs) in enumerate(refs):
        wz = max(wz, abs(got['log_z'][b] - z) / max(1.0, abs(z)))
        wm = max(wm, float(np.abs(got['marg'][b] - m).max()))
        for p, fid in enumerate(fb.ref['pair_ids']):
            wp = max(wp, float(np.abs(got['pm'][b, p] - pairs[fid]).max()))
    print('%s: log_z within %.1e, marginals within %.1e, pair marginals within %.1e of the reference' % (name, wz, wm, wp))
    assert wz <= 1e-10 and wm <= 1e-10 and wp <= 1e-10, name
    _check_consistency(name, fb, got)
    _check_features(name, fb, got)


def by_enumeration(g, inputs):
    return G.pair_marginals_enum(g, inputs)


def by_elimination(g, inputs):
    z, m = R.eliminate(g, inputs)
    return z, m, G.eliminate_pairs(g, inputs)


def _case(name, spec, seeds, how, kernel, kind='uniform', cutset=None):
    g = O.Graph(spec)
    inputs = [C.make_inputs(spec, s, kind) for s in seeds]
    fb = _batch(spec, inputs, seed=seeds[0])
    got = _run(fb, cutset=cutset, kernel=kernel)
    _compare(name, fb, got, [how(g, i) for i in inputs])
    return fb, inputs, got


# ---- against enumeration / elimination ------------------------------------------------------------------
def test_k3_x64_against_enumeration():
    """The X = 64 kernel with one cutset variable: one forest factor in registers, two cutset-incident factors (a ROW and a COL
    item), unary factors of all three kinds."""
    M = _M()
    fb, _, _ = _case('k3_x64', R.kn_spec(3, 64), (1, 2, 3), by_enumeration, X64_1)
    assert M.chunks(3, 64, M.KERNEL_X64) == 16
    assert sorted(int(k) for k in fb._unary_kind_host) == [0, 1, 2]


def test_k4_x64_against_elimination():
    """4096 configurations over 128 chunks of four waves, a factor inside the cutset, four cutset-incident factors."""
    M = _M()
    assert M.chunks(2, 4096, M.KERNEL_X64) == 128
    _case('k4_x64', R.kn_spec(4, 64), (1, 2), by_elimination, X64_1, kind='lognormal')


def test_chain3_x64_two_forest_factors():
    """The empty cutset: one configuration, both factors in the wave's registers."""
    M = _M()
    assert M.pick_kernel(64, 3, 2, 3, 2) == M.KERNEL_X64
    _case('chain3_x64', C.chain_spec(3, 64), (1, 2), by_enumeration, X64_2)


def test_double_pair_x64():
    """Two factors over one pair: both are cutset-incident, on opposite axes."""
    _case('double_pair_x64', R.double_pair_spec(64), (3, 4), by_enumeration, X64_1)


SMALL = [('ring5_x7', lambda: C.ring_spec(5, 7)),                  # odd X, a remainder of four edges
         ('forest_x9', lambda: R.forest_spec(9)),                  # two trees and a variable with unary factors only: no cutset
         ('k5_x4', lambda: R.kn_spec(5, 4))]                       # three cutset variables, three factors inside the cutset


@pytest.mark.parametrize('name,make', SMALL, ids=[s[0] for s in SMALL])
def test_small_graphs_on_the_generic_kernel(name, make):
    spec = make()
    for kind in ('uniform', 'lognormal'):
        _case(name + '/' + kind, spec, (3, 4, 5), by_enumeration, GENERIC, kind=kind)


@pytest.mark.parametrize('X', [2, 257, 512])
def test_generic_sizes_on_ring3(X):
    """X = 2, an odd size past a workgroup's 256 threads (masked tails), and the smallest power of two whose vectors leave LDS for
    the workspace (17 vectors of X doubles against 64 KB)."""
    M = _M()
    stride, chunks = 2 + 3 * X + 3 * X * X, M.chunks(2, X, M.KERNEL_GENERIC)
    assert M.workspace_bytes(2, X, 3, 3, 3, 1, 1) == 2 * chunks * (stride + (17 * X if X == 512 else 0)) * 8
    _case('ring3_x%d' % X, C.ring_spec(3, X), (7, 8), by_enumeration if X == 2 else by_elimination, GENERIC)


def test_both_sides_of_the_x64_budget():
    """A chain of three at X = 64 keeps its two accumulators in registers; a chain of four (three forest factors) goes to the
    generic kernel."""
    M = _M()
    assert M.X64_MAX_FOREST == 2
    assert M.pick_kernel(64, 3, 2, 3, 2) == M.KERNEL_X64 and M.pick_kernel(64, 4, 3, 4, 3) == M.KERNEL_GENERIC
    _case('chain3_x64', C.chain_spec(3, 64), (3,), by_enumeration, X64_2)
    _case('chain4_x64', C.chain_spec(4, 64), (1,), by_elimination, GENERIC)


def test_trees_equal_the_shipped_pair_beliefs():
    """On a tree the sweeps are exact: pair_marginals equals pair_beliefs() after sweeps from every root, within 1e-10."""
    for spec, kernel in ((R.forest_spec(9), GENERIC), (C.chain_spec(3, 64), X64_2), (C.chain_spec(5, 8), GENERIC)):
        fb = _batch(spec, [C.make_inputs(spec, s) for s in (1, 2, 3)])
        got = _run(fb, kernel=kernel)
        fb.initialize()
        fb.sweep(list(fb.topo.var_ids))
        beliefs = fb.pair_beliefs().cpu().numpy()
        assert np.abs(got['pm'] - beliefs).max() <= 1e-10, spec['name']


# ---- the cutset is a choice, not a result -----------------------------------------------------------------
def test_cutset_override_and_redundant_cutset():
    M = _M()
    spec = R.kn_spec(3, 64)
    fb = _batch(spec, [C.make_inputs(spec, s) for s in (1, 2)])
    base = _run(fb, kernel=X64_1)
    other = _run(fb, cutset=[1], kernel=X64_1)
    for key in ('marg', 'pm', 'grad_ee', 'grad_ed', 'exp_ee', 'exp_ed'):
        assert np.abs(base[key] - other[key]).max() <= 1e-10, key
    assert np.abs(base['log_z'] - other['log_z']).max() <= 1e-10 * max(1.0, np.abs(base['log_z']).max())
    with pytest.raises(ValueError):
        fb.exact_pair_marginals(cutset=[9])
    with pytest.raises(M.ExactGradError, match='cycle'):
        fb.exact_gradient(cutset=[])
    spec = C.chain_spec(5, 8)
    fb = _batch(spec, [C.make_inputs(spec, s) for s in (1, 2)])
    base, redundant = _run(fb, kernel=GENERIC), _run(fb, cutset=[2, 0], kernel=GENERIC)
    for key in ('marg', 'pm', 'grad_ee', 'grad_ed'):
        assert np.abs(base[key] - redundant[key]).max() <= 1e-10, key


KEYS = ('log_z', 'marg', 'pm', 'grad_ee', 'grad_ed', 'exp_ee', 'exp_ed')


def test_shared_tables_and_batch_position_give_the_same_bits():
    M = _M()
    for spec, kernel, code in ((R.kn_spec(3, 64), X64_1, 1), (C.ring_spec(5, 7), GENERIC, 2)):
        n_configs = spec['X']
        inputs = [C.make_inputs(spec, s) for s in (1, 2, 3, 4)]
        fb = _batch(spec, inputs)
        full = _run(fb, kernel=kernel)
        pair, unary = batch_tables(spec, fb.topo, inputs)
        P, U = fb.topo.P, fb.topo.U
        # two graphs naming one table: graphs 0 and 2 of the shared batch both read the tables, labels and columns of graph 2
        ptab = np.arange(4 * P).reshape(4, P)
        utab = np.arange(4 * U).reshape(4, U)
        ptab[0], utab[0] = ptab[2], utab[2]
        order = [2, 1, 2, 3]
        shared = _run(_batch(spec, inputs, (pair, unary), ptab, utab, labels=fb.ref['labels'][order], obs=fb.ref['obs'][order]))
        for key in KEYS:
            assert np.array_equal(shared[key][0], full[key][2]) and np.array_equal(shared[key][1:], full[key][1:]), key
        # B = 1 equals the graph inside the batch, at an equal number of chunks
        assert M.chunks(1, n_configs, code) == M.chunks(4, n_configs, code)
        alone = _run(_batch(spec, inputs[1:2], labels=fb.ref['labels'][1:2], obs=fb.ref['obs'][1:2]), kernel=kernel)
        for key in KEYS:
            assert np.array_equal(alone[key][0], full[key][1]), key


# ---- range ----------------------------------------------------------------------------------------------
def test_power_of_two_scaling():
    """Any table times 2^k, k = +-400: no bit of a normalised output moves, log_z moves by k ln 2."""
    for spec, kernel, seeds in ((R.kn_spec(3, 64), X64_1, (1, 2)), (C.ring_spec(5, 7), GENERIC, (3,)), (C.chain_spec(3, 64), X64_2, (4,))):
        inputs = [C.make_inputs(spec, s, 'lognormal') for s in seeds]
        fb = _batch(spec, inputs)
        base = _run(fb, kernel=kernel)
        pair, unary = batch_tables(spec, fb.topo, inputs)
        P, U, B = fb.topo.P, fb.topo.U, len(inputs)
        moves = [({p: k}, {}) for p in range(P) for k in (400, -400)] + [({}, {0: 400}), ({}, {U - 1: -400}), ({0: 37, 1: -400, P - 1: 400}, {0: -300, 1: 3})]
        for pk, uk in moves:
            p2, u2 = pair.copy(), unary.copy()
            for b in range(B):
                for p, k in pk.items():
                    p2[b * P + p] = np.ldexp(p2[b * P + p], k)
                for u, k in uk.items():
                    u2[b * U + u] = np.ldexp(u2[b * U + u], k)
            got = _run(_batch(spec, inputs, (p2, u2)), kernel=kernel)
            for key in KEYS[1:]:
                assert np.array_equal(got[key], base[key]), (spec['name'], key, pk, uk)
            want = base['log_z'] + (sum(pk.values()) + sum(uk.values())) * np.log(2.0)
            assert (np.abs(got['log_z'] - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), (pk, uk, got['log_z'], want)


# ---- edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,make,kernel', [('k3_x64', lambda: R.kn_spec(3, 64), X64_1), ('ring5_x7', lambda: C.ring_spec(5, 7), GENERIC)],
                         ids=['x64', 'generic'])
def test_edge_rules(name, make, kernel):
    """An all-zero table, a NaN and a +inf entry, a table index, a label and an observed column out of range, each in a graph of
    its own; the seventh graph and every normalised output of the label and column graphs keep the bits of the clean batch."""
    spec = make()
    X = spec['X']
    inputs = [C.make_inputs(spec, s) for s in range(1, 8)]
    fb = _batch(spec, inputs)
    base = _run(fb, kernel=kernel)
    pair, unary = batch_tables(spec, fb.topo, inputs)
    P = fb.topo.P
    p2 = pair.copy()
    p2[0 * P + 1][:] = 0.0                                       # graph 0: an all-zero table
    p2[1 * P + 0][3 % X, 1] = np.nan                             # graph 1: a NaN entry
    p2[2 * P + 2][0, 2 % X] = np.inf                             # graph 2: +inf
    lab = fb.ref['labels'].copy()
    lab[4, 1] = X                                                # graph 4: a label outside [0, X)
    fb2 = _batch(spec, inputs, (p2, unary), labels=fb.ref['labels'], obs=fb.ref['obs'])
    fb2.pair_tab[3, 1] = fb2.pair_tables.shape[0]                # graph 3: a table index outside the array: the kernels' own range check
    fb2._unary_obs[5, 0] = X + fb2.phi_en_de.shape[1]            # graph 5: an observed column outside every feature tensor
    pm = torch.full((fb2.B, P, X, X), -7.0, dtype=torch.float64, device=fb2.device)
    mg = torch.full((fb2.B, fb2.topo.n_vars, X), -7.0, dtype=torch.float64, device=fb2.device)
    g_ee, g_ed, log_z = fb2.exact_gradient(labels=lab, pair_marginals=pm, marginals=mg)
    e_ee, e_ed, _ = fb2.exact_gradient(expect_only=True)
    torch.cuda.synchronize()
    assert _M().last_kernel() == KERNEL_OF[kernel]
    got = dict(log_z=log_z.cpu().numpy(), marg=mg.cpu().numpy(), pm=pm.cpu().numpy(), grad_ee=g_ee.cpu().numpy(), grad_ed=g_ed.cpu().numpy(),
               exp_ee=e_ee.cpu().numpy(), exp_ed=e_ed.cpu().numpy())
    assert got['log_z'][0] == -np.inf and np.array_equal(got['marg'][0], np.full_like(got['marg'][0], 1.0 / X))
    assert np.array_equal(got['pm'][0], np.full_like(got['pm'][0], (1.0 / X) * (1.0 / X)))
    assert np.isfinite(got['exp_ee'][0]).all() and np.isfinite(got['grad_ed'][0]).all()
    assert not np.isfinite(got['log_z'][1]) and not np.isfinite(got['log_z'][2])
    assert np.isnan(got['log_z'][3]) and (got['marg'][3] == -7.0).all() and (got['pm'][3] == -7.0).all()
    for key in KEYS[3:]:
        assert np.isnan(got[key][3]).all(), key
    for b in (4, 5):                                             # no gradient; everything that needs neither the label nor the column
        assert np.isnan(got['grad_ee'][b]).all() and np.isnan(got['grad_ed'][b]).all()
        for key in ('log_z', 'marg', 'pm'):
            assert np.array_equal(got[key][b], base[key][b]), (key, b)
    assert np.array_equal(got['exp_ee'][4], base['exp_ee'][4]) and np.array_equal(got['exp_ed'][4], base['exp_ed'][4])
    assert np.isfinite(got['exp_ee'][5]).all() and np.isfinite(got['exp_ed'][5]).all()
    for key in KEYS:
        assert np.array_equal(got[key][6], base[key][6]), key


def test_float32_tables_are_refused():
    spec = C.user_spec(10, [1, 4, 7], 256, 64, seed=1)
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(spec)
    fb = FactorGraphBatch(topo, 256, 1)
    pair, unary = batch_tables(spec, topo, [C.make_inputs(spec, 1)])
    fb.set_pair_tables(pair, dtype=torch.float32)
    fb.set_unary_tables(unary)
    with pytest.raises(NotImplementedError):
        fb.exact_pair_marginals()
    with pytest.raises(NotImplementedError):
        fb.exact_gradient()


def test_capture_and_replay():
    """After one eager call exact_gradient is captured and replayed twice: the bits of the eager call."""
    spec = R.kn_spec(3, 64)
    fb = _batch(spec, [C.make_inputs(spec, s) for s in (1, 2, 3)])
    eager = _run(fb, kernel=X64_1)
    pm = torch.empty(fb.B, fb.topo.P, fb.X, fb.X, dtype=torch.float64, device=fb.device)
    mg = torch.empty(fb.B, fb.topo.n_vars, fb.X, dtype=torch.float64, device=fb.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_ee, g_ed, log_z = fb.exact_gradient(pair_marginals=pm, marginals=mg)
    for _ in range(2):
        for t in (g_ee, g_ed, log_z, pm, mg):
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for key, t in (('grad_ee', g_ee), ('grad_ed', g_ed), ('log_z', log_z), ('pm', pm), ('marg', mg)):
            assert np.array_equal(t.cpu().numpy(), eager[key]), key


# ---- trainer --------------------------------------------------------------------------------------------
def _trainer(tmp_path, **kw):
    from macaronicusermodeling_amd import tidir
    from macaronicusermodeling_amd.train import TiDirTrainer
    opts = dict(n_instances=24, X=64, Vde=64, sent_len=(4, 7), n_predicted=(1, 5), seed=9)
    extra = {k: kw.pop(k) for k in list(kw) if k not in opts}
    opts.update(kw)
    paths = tidir.synthesize(str(tmp_path), **opts)
    tt = TiDirTrainer(paths['ti'], paths['end'], paths['ded'], paths['phi_pmi'], paths['phi_pmi_w1'], paths['phi_ed'], paths['phi_ped'], sweeps=3, **extra)
    rs = np.random.RandomState(1)
    th_ee, th_ed = rs.randn(1, 3) * 0.6, rs.randn(1, 6) * 0.6
    tt.theta_en_en.copy_(torch.from_numpy(th_ee.reshape(-1)))
    tt.theta_en_de.copy_(torch.from_numpy(th_ed.reshape(-1)))
    return tt, paths, th_ee, th_ed


def test_tidir_gradient_report_and_exact_step(tmp_path):
    """On the synthetic file of the exactness report's test (up to five predicted words; K5 at X = 64 is above the limit):
    gradient_report() totals are the sums of UserGraphTrainer.exact_gradient(), the BP half is what the trainer's own statistics
    launch sums, exact_step() moves the thetas by apply_update of the exact statistics, and refuses what it must."""
    from macaronicusermodeling_amd import exactgrad as K
    from macaronicusermodeling_amd.train import apply_update
    tt, _, _, _ = _trainer(tmp_path)
    exact, bp, all_bp, fall = np.zeros(9), np.zeros(9), np.zeros(9), np.zeros(9)
    loglik, seen, n_skipped, lp_skipped = 0.0, 0, 0, 0.0
    for key, tr in tt.trainers.items():
        tr.build_potentials()
        b_ee, b_ed, lp = tr._bp_gradient()
        all_bp += np.concatenate([b_ee.sum(axis=0), b_ed.sum(axis=0)])
        try:
            g_ee, g_ed, joint, bp_ee, bp_ed = tr.exact_gradient()
        except K.ExactGradError:
            assert tr.topo.n_vars >= 5
            n_skipped += b_ee.shape[0]
            lp_skipped += float(lp.sum())
            fall += np.concatenate([b_ee.sum(axis=0), b_ed.sum(axis=0)])
            continue
        assert np.array_equal(bp_ee, b_ee) and np.array_equal(bp_ed, b_ed)
        assert np.isfinite(g_ee).all() and np.isfinite(g_ed).all() and (joint < 0).all()
        seen += g_ee.shape[0]
        loglik += float(joint.sum())
        exact += np.concatenate([g_ee.sum(axis=0), g_ed.sum(axis=0)])
        bp += np.concatenate([bp_ee.sum(axis=0), bp_ed.sum(axis=0)])
    assert seen and n_skipped
    # the BP half is the gradient the trainer follows: its own statistics launch over every bucket
    stats = tt._local_statistics_eager().cpu().numpy()
    assert np.abs(stats[:9] - all_bp).max() <= 1e-9 * max(1.0, np.abs(all_bp).max()), (stats[:9], all_bp)
    totals, skipped = tt.gradient_report()
    assert np.abs(totals[0] - exact).max() <= 1e-12 * np.abs(exact).max() and np.abs(totals[1] - bp).max() <= 1e-12 * np.abs(bp).max()
    cosine = exact.dot(bp) / np.linalg.norm(exact) / np.linalg.norm(bp)
    rel = np.linalg.norm(bp - exact) / np.linalg.norm(exact)
    print('gradient gap on %d instances: cosine %.6f, |bp - exact| / |exact| = %.3e, true log-likelihood %.6f' % (seen, cosine, rel, loglik))
    assert abs(totals[2] - cosine) <= 1e-12 and abs(totals[3] - rel) <= 1e-12 * max(1.0, rel) and abs(totals[4] - loglik) <= 1e-9 * abs(loglik)
    assert totals[5] == seen and totals[6] == n_skipped and sum(s[1] for s in skipped) == n_skipped
    assert all('configurations' in s[2] for s in skipped)
    assert rel > 1e-6                                           # the BP gradient is visibly not the true one
    with pytest.raises(K.ExactGradError, match='configurations'):
        tt.exact_step(0.01, 0.1)
    with pytest.raises(ValueError):
        tt.exact_step(0.01, 0.1, fallback='eager')
    before_ee, before_ed = tt.theta_en_en.clone(), tt.theta_en_de.clone()
    mean_ll, n_fallback = tt.exact_step(0.01, 0.1, fallback='bp')
    want = torch.from_numpy(np.concatenate([exact + fall, [loglik + lp_skipped, float(seen + n_skipped)]])).to(tt.device)
    apply_update(before_ee, before_ed, want, 3, 6, 0.01, 0.1)
    assert n_fallback == n_skipped and abs(mean_ll - (loglik + lp_skipped) / (seen + n_skipped)) <= 1e-12 * abs(mean_ll)
    assert (tt.theta_en_en - before_ee).abs().max().item() <= 1e-13 and (tt.theta_en_de - before_ed).abs().max().item() <= 1e-13


def test_exact_step_refuses_per_domain_thetas(tmp_path):
    tt, _, _, _ = _trainer(tmp_path, n_instances=6, n_predicted=(1, 2), adapt='user')
    assert tt.domains
    with pytest.raises(NotImplementedError):
        tt.exact_step(0.01, 0.1)


def _cpu_loglik(tt, phi, th_ee, th_ed):
    """The true total log-likelihood of the stored labels by enumeration, instance by instance."""
    total = 0.0
    for key, b in tt.buckets.items():
        for r in range(len(b['rows'])):
            g, inputs, _, _ = tidir_oracle_graph(key, b, r, phi[0], phi[1], phi[2], th_ee, th_ed)
            score = 0.0
            for vs, T in R._factor_arrays(g, inputs):
                score += float(np.log(T[tuple(g.label[v] for v in vs)]))
            total += score - R.enumerate_exact(g, inputs)[0]
    return total


def test_exact_step_ascends_the_true_likelihood(tmp_path):
    """On K3 and K4 buckets (X = 16, so that the CPU reference can enumerate them) one exact_step without regulariser does not
    lower the true total log-likelihood.  The rate is found by halving from the trainer's default 0.1 until the CPU reference --
    enumeration at theta + rate * gradient -- ascends: 0.1 / 2^k with the k printed below.  Recorded on an MI355X: k = 2, rate
    0.025, true total log-likelihood -156.667846 -> -128.853375."""
    from macaronicusermodeling_amd import tidir
    tt, paths, th_ee, th_ed = _trainer(tmp_path, n_instances=12, X=16, Vde=16, sent_len=(5, 7), n_predicted=(3, 4), seed=5)
    assert sorted({tr.topo.n_vars for tr in tt.trainers.values()}) == [3, 4]
    phi = tidir.load_features(paths['phi_pmi'], paths['phi_pmi_w1'], paths['phi_ed'], paths['phi_ped'])
    totals, skipped = tt.gradient_report()
    assert not skipped and totals[5] == 12
    before_cpu = _cpu_loglik(tt, phi, th_ee, th_ed)
    assert abs(totals[4] - before_cpu) <= 1e-9 * abs(before_cpu), (totals[4], before_cpu)
    rate, k = 0.1, 0
    while _cpu_loglik(tt, phi, th_ee + rate * totals[0][None, :3], th_ed + rate * totals[0][None, 3:]) < before_cpu:
        rate, k = rate / 2, k + 1
        assert k < 30
    print('exact_step ascends at rate 0.1 / 2^%d = %g: CPU log-likelihood %.6f before' % (k, rate, before_cpu))
    mean_ll, n_fallback = tt.exact_step(rate, 0.0)
    assert n_fallback == 0 and abs(mean_ll - before_cpu / 12) <= 1e-9 * abs(before_cpu)
    after = tt.gradient_report()[0][4]
    print('true total log-likelihood %.6f -> %.6f' % (totals[4], after))
    assert after >= totals[4]
    per_instance, _, _ = tt.exactness_report()
    assert len(per_instance) == 12
