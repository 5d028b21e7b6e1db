"""Posterior sampling on the GPU (libmlbp_sample.so) against the float64 NumPy walk of tests/test_sample_cpu.py.

Tolerances: conditional marginals and log q rtol 1e-10 (atol 1e-300) -- the project's tolerance for sums taken in a different
order.  Samples are compared exactly.  A draw lands where the prefix sum of the marginal crosses t = u * total; a (graph,
sample) pair would be left out if any of its draws in the WALK had a margin min_i |c_i - t| below 1e-8 (two decades above the
marginals' tolerance; one differing draw changes every later step) -- but the cap on left-out pairs is 0 in every case: the
walk's smallest margin is asserted before the device is looked at, and the seeds were chosen so that it holds.  Drawn states
and margins are always the walk's, never the device's.  Uniforms come from np.random.RandomState and are uploaded.

Mutations these cases are built to catch: a sum turned back into a maximum in either contraction (every parity case compares
conditional marginals at 1e-10); the clamp dropped or applied to the wrong variable (every conditional after step 0, and
test_all_but_one_given_equals_sweep_on_zeroed_tables against the shipped sum-product kernels); `>` turned into `>=` in the draw
or a zero-probability state drawn (test_draw_rule_on_dyadic_marginals); the cached step-0 marginal reused across graphs or
stale (test_chunk_rule_gives_the_samples_of_single_graph_batches: C < S loops over samples); uniforms indexed by variable
instead of step (test_non_default_order)."""
import numpy as np
import pytest

import cases as C
import test_map_cpu as W
import test_sample_cpu as SC
from helpers import batch_tables, tidir_gold, tidir_oracle_graph, write_tidir
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

X64_RESIDENT = ('sample_x64_kernel', (True,))          # P <= 3: tables in registers
X64_STREAMED = ('sample_x64_kernel', (False,))
GENERIC = ('sample_generic_kernel', ())
# kernel instance -> the tests that launch it (tests/test_sample_cpu.py holds this against the library's symbol table)
CASES = {
    X64_RESIDENT: ['test_k3_resident', 'test_k1', 'test_non_default_order', 'test_unnormalised_messages',
                   'test_chunk_rule_gives_the_samples_of_single_graph_batches', 'test_first_step_equals_sweep_marginals',
                   'test_all_but_one_given_equals_sweep_on_zeroed_tables', 'test_given', 'test_draw_rule_on_dyadic_marginals',
                   'test_shared_tables_give_the_bits_of_unique_copies', 'test_capture_and_replay',
                   'test_tidir_sample_at_zero_thetas', 'test_tidir_sample_equals_the_walk_on_one_bucket'],
    X64_STREAMED: ['test_k4_streamed', 'test_chain_equals_joint_logp', 'test_tidir_sample_at_zero_thetas'],
    GENERIC: ['test_ring5_x8', 'test_k3_x128', 'test_x3_trees_equal_the_brute_force_grid', 'test_draw_rule_on_dyadic_marginals',
              'test_chunk_rule_gives_the_samples_of_single_graph_batches', 'test_first_step_equals_sweep_marginals',
              'test_all_but_one_given_equals_sweep_on_zeroed_tables', 'test_given', 'test_tidir_sample_at_zero_thetas'],
}
KERNEL_OF = {X64_RESIDENT: 1, X64_STREAMED: 1, GENERIC: 2}     # mlbp_sample.h MLBP_SAMPLE_KERNEL_*
MARGIN = 1e-8
MAY_OMIT = 0


def _S():
    from macaronicusermodeling_amd import sample
    return sample


def _batch(spec, inputs_list, normalize=True, tables=None, pair_tab=None):
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(spec)
    fb = FactorGraphBatch(topo, spec['X'], len(inputs_list), normalize_messages=normalize)
    pair, unary = batch_tables(spec, topo, inputs_list) if tables is None else tables
    if topo.P:
        fb.set_pair_tables(pair, pair_tab)
    if topo.U:
        fb.set_unary_tables(unary)
    return fb


def _run(fb, roots, uniforms, order=None, given=None):
    """uniforms: numpy [S][B][n_vars]; given: numpy [B][n_vars] or None."""
    n_samples = uniforms.shape[0]
    u = torch.from_numpy(np.ascontiguousarray(uniforms)).to(fb.device)
    cm = torch.full((n_samples, fb.B, fb.topo.n_vars, fb.X), float('nan'), dtype=torch.float64, device=fb.device)
    msgs_before = fb.msgs.clone()
    x, logq = fb.sample(roots, n_samples=n_samples, uniforms=u, order=order, given=given, cond_marginals=cm)
    kernel = _S().last_kernel()
    torch.cuda.synchronize()
    assert x.dtype == torch.int32 and tuple(x.shape) == (n_samples, fb.B, fb.topo.n_vars)
    assert logq.dtype == torch.float64 and tuple(logq.shape) == (n_samples, fb.B)
    assert torch.equal(fb.msgs.view(torch.int64), msgs_before.view(torch.int64))          # self.msgs is left untouched (bits)
    return dict(x=x.cpu().numpy(), logq=logq.cpu().numpy(), cm=cm.cpu().numpy(), kernel=kernel)


def _walks(spec, inputs_list, roots, uniforms, order=None, given=None, normalize=True, graphs=None):
    """{(s, b): walk} and the smallest margin of any draw."""
    var_ids = list(O.Graph(spec).var_order)
    out, smallest = {}, np.inf
    for b in (range(len(inputs_list)) if graphs is None else graphs):
        giv = None if given is None else {v: int(given[b][i]) for i, v in enumerate(var_ids)}
        for s in range(uniforms.shape[0]):
            w = out[s, b] = SC.walk(spec, inputs_list[b], roots, uniforms[s, b], order=order, given=giv, normalize=normalize)
            smallest = min([smallest] + list(w['margin'].values()))
    return out, smallest


def _check_margin(name, walks, smallest):
    omitted = sum(1 for w in walks.values() if min(w['margin'].values()) < MARGIN)
    draws = sum(1 for w in walks.values() for m in w['margin'].values() if np.isfinite(m))
    print('%s: %d (graph, sample) pairs, %d draws, smallest margin of the walk %.2e, %d pairs left out (cap %d)'
          % (name, len(walks), draws, smallest, omitted, MAY_OMIT))
    assert omitted <= MAY_OMIT and smallest >= MARGIN, (name, smallest)


def _compare(name, topo, got, walks):
    wrong = []
    for (s, b), w in sorted(walks.items()):
        np.testing.assert_allclose(got['cm'][s, b], np.stack([w['cm'][v] for v in topo.var_ids]), rtol=1e-10, atol=1e-300,
                                   err_msg='%s sample %d graph %d' % (name, s, b))
        np.testing.assert_allclose(got['logq'][s, b], w['logq'], rtol=1e-10, err_msg='%s sample %d graph %d' % (name, s, b))
        x_dev = [int(v) for v in got['x'][s, b]]
        if x_dev != [w['x'][v] for v in topo.var_ids]:
            wrong.append((s, b, x_dev, w['x']))
    assert not wrong, (name, wrong[:6])


def _case(name, spec, seeds, roots, instance, n_samples=2, u_seed=0, order=None, given=None, normalize=True, kind='uniform'):
    inputs = [C.make_inputs(spec, s, kind) for s in seeds]
    n_vars = len(spec['var_ids'])
    uniforms = np.random.RandomState(u_seed).rand(n_samples, len(inputs), n_vars)
    walks, smallest = _walks(spec, inputs, roots, uniforms, order=order, given=given, normalize=normalize)
    _check_margin(name, walks, smallest)                       # before the device is looked at
    fb = _batch(spec, inputs, normalize=normalize)
    got = _run(fb, roots, uniforms, order=order, given=given)
    assert got['kernel'] == KERNEL_OF[instance] == _S().pick_kernel(spec['X'], fb.topo.n_msgs, fb.topo.n_vars), name
    assert (fb.topo.P <= 3) == (instance != X64_STREAMED) or instance == GENERIC
    _compare(name, fb.topo, got, walks)
    assert (got['x'] >= 0).all() and (got['x'] < spec['X']).all()
    return fb, inputs, uniforms, got, walks


K3 = dict(spec=lambda: C.user_spec(10, [1, 4, 7], 64, 64, seed=1), seeds=range(500, 532), roots=[1, 4, 7])


def test_k3_resident():
    _case('K3', K3['spec'](), K3['seeds'], K3['roots'], X64_RESIDENT, n_samples=2, u_seed=1)


def test_k1():
    fb, _, _, _, _ = _case('K1', C.user_spec(10, [4], 64, 64, seed=3), range(16), [4], X64_RESIDENT, u_seed=2)
    assert fb.topo.P == 0


def test_k4_streamed():
    fb, _, _, _, _ = _case('K4', C.user_spec(10, [0, 2, 5, 8], 64, 64, seed=4), range(700, 716), [0, 2, 5], X64_STREAMED, u_seed=3)
    assert fb.topo.P == 6


def test_chain_equals_joint_logp():
    """A chain is a tree: one sweep per step is exact, so log q of every drawn sample is its log-probability under the model --
    FactorGraphBatch.log_partition's joint_logp at the drawn samples, from the shipped third library."""
    spec = C.chain_spec(8, 64)
    fb, inputs, uniforms, got, _ = _case('chain8', spec, range(1, 9), [0], X64_STREAMED, u_seed=4)
    for s in range(uniforms.shape[0]):
        _, joint = fb.log_partition([0], init=True, labels=got['x'][s])
        np.testing.assert_allclose(got['logq'][s], joint.cpu().numpy(), rtol=1e-10)


def test_ring5_x8():
    _case('ring5_x8', C.ring_spec(5, 8), range(1, 9), [0, 2, 4], GENERIC, u_seed=5)


def test_k3_x128():
    _case('K3 X=128', C.user_spec(10, [1, 4, 7], 128, 128, seed=1), range(500, 508), [1, 4, 7], GENERIC, u_seed=6)


def test_non_default_order():
    """Step k handles order[k] and reads uniforms[..., k]."""
    spec = K3['spec']()
    _, _, uniforms, got, _ = _case('K3 order 7,1,4', spec, range(500, 508), K3['roots'], X64_RESIDENT, u_seed=7, order=[7, 1, 4])
    inputs = [C.make_inputs(spec, s) for s in range(500, 508)]
    default = _run(_batch(spec, inputs), K3['roots'], uniforms)
    assert not np.array_equal(default['x'], got['x'])
    _case('ring5_x8 order', C.ring_spec(5, 8), range(1, 5), [0, 2, 4], GENERIC, u_seed=8, order=[3, 0, 4, 1, 2])


def test_unnormalised_messages():
    _case('K3 unnormalised', K3['spec'](), range(500, 508), K3['roots'], X64_RESIDENT, u_seed=9, normalize=False)


def test_x3_trees_equal_the_brute_force_grid():
    """X = 3 trees with `given` set to every one of the X^n assignments, one graph per assignment: log q is the grid entry minus
    the grid's logsumexp, directly."""
    for name, spec, order in (('chain4_x3', C.chain_spec(4, 3), None), ('star4_x3', C.star_spec(4, 3), [2, 0, 4, 1, 3])):
        g = O.Graph(spec)
        inp = C.make_inputs(spec, 3)
        _, _, grid = W.brute_force(g, inp)
        lse = SC.logsumexp(grid)
        given = np.array(list(np.ndindex(*grid.shape)), dtype=np.int32)
        fb = _batch(spec, [inp] * len(given))
        got = _run(fb, [g.var_order[0] if order is None else order[0]], np.zeros((1, len(given), fb.topo.n_vars)), order=order, given=given)
        assert got['kernel'] == KERNEL_OF[GENERIC] and np.array_equal(got['x'][0], given)
        np.testing.assert_allclose(got['logq'][0], grid.reshape(-1) - lse, rtol=1e-10, err_msg=name)
        np.testing.assert_allclose(np.exp(got['logq'][0]).sum(), 1.0, rtol=1e-12)


def test_draw_rule_on_dyadic_marginals():
    """m = [1/4, 0, 1/4, 1/2, 0, ...] exactly: the comparison is strict and a state of probability zero is never drawn, on the
    generic kernel (X = 8) and on the X = 64 kernel (P = 0)."""
    for X, instance in ((8, GENERIC), (64, X64_RESIDENT)):
        spec, inputs, row = SC.dyadic_case(X)
        us = np.array([u for u, _ in SC.DYADIC_DRAWS])
        fb = _batch(spec, [inputs] * len(us))
        got = _run(fb, [0], us.reshape(1, -1, 1))
        assert got['kernel'] == KERNEL_OF[instance]
        assert [int(v) for v in got['x'][0, :, 0]] == [state for _, state in SC.DYADIC_DRAWS]
        assert np.array_equal(got['cm'][0, :, 0], np.tile(row, (len(us), 1)))
        np.testing.assert_allclose(got['logq'][0], np.log(row[got['x'][0, :, 0]]), rtol=1e-14)


CHUNK_SHAPES = [(1, 5), (3, 1), (257, 3), (600, 2)]


@pytest.mark.parametrize('B,n_samples', CHUNK_SHAPES, ids=['B%d_S%d' % bs for bs in CHUNK_SHAPES])
def test_chunk_rule_gives_the_samples_of_single_graph_batches(B, n_samples):
    """The grid is (B, C), C = min(S, ceil(512 / B)): (1, 5) C = 5; (3, 1) C = 1; (257, 3) C = 2 < S -- a workgroup loops over
    its samples and reuses its step-0 marginal; (600, 2) C = 1.  Every checked graph's samples, log q and conditional marginals
    are the bits of the same graph in a batch of one (C = S there: one workgroup per sample), which are compared with the
    walk."""
    S = _S()
    assert S.chunks(B, n_samples) == {(1, 5): 5, (3, 1): 1, (257, 3): 2, (600, 2): 1}[B, n_samples]
    for name, spec, seeds, roots, instance in (('K3', K3['spec'](), range(500, 504), K3['roots'], X64_RESIDENT),
                                               ('ring5_x8', C.ring_spec(5, 8), range(1, 5), [0, 2, 4], GENERIC)):
        distinct = [C.make_inputs(spec, s) for s in seeds]
        inputs = [distinct[b % len(distinct)] for b in range(B)]
        uniforms = np.random.RandomState(100 + B).rand(n_samples, B, len(spec['var_ids']))
        graphs = sorted(set(range(B)) if B <= 3 else {0, 1, B // 2, B - 2, B - 1})
        walks, smallest = _walks(spec, inputs, roots, uniforms, graphs=graphs)
        _check_margin('%s B=%d S=%d' % (name, B, n_samples), walks, smallest)
        fb = _batch(spec, inputs)
        got = _run(fb, roots, uniforms)
        assert got['kernel'] == KERNEL_OF[instance]
        assert (got['x'] >= 0).all() and np.isfinite(got['logq']).all() and np.isfinite(got['cm']).all()       # every pair was written
        for b in graphs:
            one = _run(_batch(spec, [inputs[b]]), roots, uniforms[:, b:b + 1])
            for k in ('x', 'logq', 'cm'):
                assert np.array_equal(one[k][:, 0], got[k][:, b]), (name, b, k)
            _compare('%s B=1 graph %d' % (name, b), fb.topo, one, {(s, 0): walks[s, b] for s in range(n_samples)})


# ---- against the shipped sum-product kernels, not the walk ------------------------------------------
SWEEP_CASES = [('K3', K3['spec'], range(500, 508), K3['roots'], 1), ('ring5_x8', lambda: C.ring_spec(5, 8), range(1, 9), [0, 2, 4], 2)]


@pytest.mark.parametrize('name,make,seeds,roots,kernel', SWEEP_CASES, ids=[c[0] for c in SWEEP_CASES])
def test_first_step_equals_sweep_marginals(name, make, seeds, roots, kernel):
    """Nothing given: the conditional marginal of order[0] is that variable's row of fb.sweep(roots, init=True, marginals=...)."""
    spec = make()
    inputs = [C.make_inputs(spec, s) for s in seeds]
    fb = _batch(spec, inputs)
    marg = torch.empty(fb.B, fb.topo.n_vars, fb.X, dtype=torch.float64, device=fb.device)
    fb.sweep(roots, init=True, marginals=marg)
    marg = marg.cpu().numpy()
    uniforms = np.random.RandomState(11).rand(2, fb.B, fb.topo.n_vars)
    for order in (None, list(fb.topo.var_ids[::-1])):
        got = _run(fb, roots, uniforms, order=order)
        assert got['kernel'] == kernel
        first = 0 if order is None else fb.topo.var_index[order[0]]
        for s in range(2):
            np.testing.assert_allclose(got['cm'][s, :, first], marg[:, first], rtol=1e-10, atol=1e-300)


@pytest.mark.parametrize('name,make,seeds,roots,kernel', SWEEP_CASES, ids=[c[0] for c in SWEEP_CASES])
def test_all_but_one_given_equals_sweep_on_zeroed_tables(name, make, seeds, roots, kernel):
    """All but one variable given (and handled first): the free variable's conditional marginal is sweep()'s marginal on a copy of
    the batch whose tables keep, of every given variable, only the row / column / unary entry of its given state."""
    from macaronicusermodeling_amd import mapdecode
    spec = make()
    inputs = [C.make_inputs(spec, s) for s in seeds]
    fb = _batch(spec, inputs)
    topo, X, B = fb.topo, fb.X, fb.B
    pav, uv = mapdecode.readout_arrays(topo)
    rs = np.random.RandomState(12)
    for free in (0, topo.n_vars - 1):
        given = rs.randint(0, X, size=(B, topo.n_vars)).astype(np.int32)
        given[:, free] = -1
        order = [v for i, v in enumerate(topo.var_ids) if i != free] + [topo.var_ids[free]]
        got = _run(fb, roots, rs.rand(1, B, topo.n_vars), order=order, given=given)
        assert got['kernel'] == kernel
        pair, unary = fb.pair_tables.cpu().numpy().copy(), fb.unary_tables.cpu().numpy().copy()
        for b in range(B):
            for p in range(topo.P):
                for axis in range(2):
                    x = given[b, pav[p, axis]]
                    if x >= 0:
                        keep = np.zeros(X)
                        keep[x] = 1.0
                        pair[b * topo.P + p] *= keep[:, None] if axis == 0 else keep[None, :]
            for u in range(topo.U):
                x = given[b, uv[u]]
                if x >= 0:
                    unary[b * topo.U + u, np.arange(X) != x] = 0.0
        zeroed = _batch(spec, inputs, tables=(pair, unary))
        marg = torch.empty(B, topo.n_vars, X, dtype=torch.float64, device=fb.device)
        zeroed.sweep(roots, init=True, marginals=marg)
        np.testing.assert_allclose(got['cm'][0, :, free], marg.cpu().numpy()[:, free], rtol=1e-10, atol=1e-300)
        mask = np.arange(topo.n_vars) != free
        assert np.array_equal(got['x'][0][:, mask], given[:, mask])


# ---- given, shared tables, capture ------------------------------------------------------------------
@pytest.mark.parametrize('name,make,seeds,roots,kernel', SWEEP_CASES, ids=[c[0] for c in SWEEP_CASES])
def test_given(name, make, seeds, roots, kernel):
    """A fixed variable comes back as given in every sample (and the others follow the walk); an out-of-range value gives -1 and
    NaN for that graph only; a given state of probability zero gives log q = -inf."""
    spec = make()
    inputs = [C.make_inputs(spec, s) for s in seeds]
    X, B, n_vars = spec['X'], len(inputs), len(spec['var_ids'])
    rs = np.random.RandomState(13)
    given = np.full((B, n_vars), -1, dtype=np.int32)
    given[:, 1] = rs.randint(0, X, size=B)
    given[::2, 0] = rs.randint(0, X, size=len(given[::2]))
    uniforms = rs.rand(3, B, n_vars)
    walks, smallest = _walks(spec, inputs, roots, uniforms, given=given)
    _check_margin(name + ' given', walks, smallest)
    fb = _batch(spec, inputs)
    topo = fb.topo
    clean = _run(fb, roots, uniforms, given=given)
    assert clean['kernel'] == kernel
    _compare(name + ' given', topo, clean, walks)
    for s in range(3):
        assert np.array_equal(clean['x'][s][given >= 0], given[given >= 0])
    # as a device tensor, used as it is
    again = _run(fb, roots, uniforms, given=torch.from_numpy(given).to(fb.device))
    assert all(np.array_equal(again[k], clean[k]) for k in ('x', 'logq', 'cm'))
    # out of range: graphs 2 (too large) and 5 (below -1) are not computed, the others keep their bits
    bad = given.copy()
    bad[2, topo.n_vars - 1], bad[5, 0] = X, -2
    got = _run(fb, roots, uniforms, given=bad)
    for b in range(B):
        if b in (2, 5):
            assert (got['x'][:, b] == -1).all() and np.isnan(got['logq'][:, b]).all() and np.isnan(got['cm'][:, b]).all()
        else:
            assert all(np.array_equal(got[k][:, b], clean[k][:, b]) for k in ('x', 'logq', 'cm')), b
    # probability zero: graph 1's variable 1 cannot take its given state
    x0 = int(given[1, 1])
    unary = fb.unary_tables.cpu().numpy().copy()
    from macaronicusermodeling_amd import mapdecode
    _, uv = mapdecode.readout_arrays(topo)
    for u in range(topo.U):
        if uv[u] == 1:
            unary[1 * topo.U + u, x0] = 0.0
    fz = _batch(spec, inputs, tables=(fb.pair_tables.cpu().numpy(), unary))
    got = _run(fz, roots, uniforms, given=given)
    assert np.isneginf(got['logq'][:, 1]).all() and (got['x'][:, 1, 1] == x0).all() and (got['cm'][:, 1, 1, x0] == 0.0).all()
    assert np.isfinite(got['cm']).all() and (got['x'] >= 0).all()
    others = np.arange(B) != 1
    assert all(np.array_equal(got[k][:, others], clean[k][:, others]) for k in ('x', 'logq', 'cm'))


def test_shared_tables_give_the_bits_of_unique_copies():
    """The K3 case with two tables behind every graph through pair_tab == the same tables passed as unique copies, bit for bit."""
    spec = K3['spec']()
    inputs = [C.make_inputs(spec, s) for s in range(500, 516)]
    B = len(inputs)
    fb_u = _batch(spec, inputs)
    two = fb_u.pair_tables[:2].clone()
    tab = np.tile(np.array([[0, 1, 0]]), (B, 1))
    tab[1::2] = [1, 1, 0]
    unary = fb_u.unary_tables
    fb_s = _batch(spec, inputs, tables=(two, unary), pair_tab=tab)
    fb_c = _batch(spec, inputs, tables=(two[torch.from_numpy(tab.reshape(-1)).to(two.device)], unary))
    uniforms = np.random.RandomState(14).rand(2, B, 3)
    a, b = _run(fb_s, K3['roots'], uniforms), _run(fb_c, K3['roots'], uniforms)
    assert a['kernel'] == b['kernel'] == 1
    for k in ('x', 'logq', 'cm'):
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a['cm'], _run(fb_u, K3['roots'], uniforms)['cm'])          # (other tables, other answers)


def test_capture_and_replay():
    """One call recorded in a HIP graph after one eager call; the uniforms tensor overwritten in place; the replayed samples are
    those of an eager call with the new uniforms.  (The kernel holds no generator: a call is a function of its arguments.)"""
    spec = K3['spec']()
    inputs = [C.make_inputs(spec, s) for s in range(500, 508)]
    fb = _batch(spec, inputs)
    rs = np.random.RandomState(15)
    first, second = rs.rand(2, fb.B, 3), rs.rand(2, fb.B, 3)
    u = torch.from_numpy(first).to(fb.device)
    cm = torch.empty(2, fb.B, 3, 64, dtype=torch.float64, device=fb.device)
    fb.sample(K3['roots'], n_samples=2, uniforms=u, cond_marginals=cm)                    # eager warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x, logq = fb.sample(K3['roots'], n_samples=2, uniforms=u, cond_marginals=cm)
    for uniforms in (first, second, first):
        u.copy_(torch.from_numpy(uniforms))
        x.fill_(-7); logq.fill_(float('nan')); cm.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        replayed = dict(x=x.cpu().numpy(), logq=logq.cpu().numpy(), cm=cm.cpu().numpy())
        eager = _run(fb, K3['roots'], uniforms)
        for k in ('x', 'logq', 'cm'):
            assert np.array_equal(replayed[k], eager[k]), k
    assert not np.array_equal(_run(fb, K3['roots'], first)['x'], _run(fb, K3['roots'], second)['x'])


def test_python_layer_refusals():
    spec = K3['spec']()
    fb = _batch(spec, [C.make_inputs(spec, 500)])
    u = torch.zeros(1, 1, 3, dtype=torch.float64, device=fb.device)
    with pytest.raises(ValueError):
        fb.sample(K3['roots'])                                   # neither seed nor uniforms
    with pytest.raises(ValueError):
        fb.sample(K3['roots'], seed=1, uniforms=u)               # both
    with pytest.raises(ValueError):
        fb.sample(K3['roots'], n_samples=2, uniforms=u)          # wrong shape
    with pytest.raises(ValueError):
        fb.sample(K3['roots'], seed=1, order=[1, 4])             # not every variable
    with pytest.raises(_S().SampleError):
        fb.sample(K3['roots'], seed=1, order=[1, 4, 4])          # not a permutation
    # seed: the documented generator call
    x, logq = fb.sample(K3['roots'], n_samples=4, seed=9)
    want = torch.rand((4, 1, 3), dtype=torch.float64, device=fb.device, generator=torch.Generator(fb.device).manual_seed(9))
    x2, logq2 = fb.sample(K3['roots'], n_samples=4, uniforms=want)
    assert torch.equal(x, x2) and torch.equal(logq, logq2)
    spec32 = C.user_spec(10, [1, 4, 7], 256, 64, seed=1)
    fb32 = _batch(spec32, [C.make_inputs(spec32, 1)])
    fb32.set_pair_tables(fb32.pair_tables, dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        fb32.sample([1], seed=1)
    fb.use_approx_inference = True
    with pytest.raises(NotImplementedError):
        fb.sample([1], seed=1)


# ---- trainers -------------------------------------------------------------------------------------
def _clique_trainer(tmp_path, thetas=None):
    from macaronicusermodeling_amd import tidir
    from macaronicusermodeling_amd.train import TiDirTrainer
    gold = tidir_gold('tidir_cliques_reference')
    paths = write_tidir(gold, str(tmp_path))
    tt = TiDirTrainer(paths['ti'], paths['vocab.en'], paths['vocab.de'], paths['phi.pmi'], paths['phi.pmi_w1'], paths['phi.ed'],
                      paths['phi.ped'], sweeps=3, use_correct_feat=True, history=True, session_history=True)
    if thetas is not None:
        tt.theta_en_en.copy_(torch.from_numpy(thetas[0].reshape(-1)))
        tt.theta_en_de.copy_(torch.from_numpy(thetas[1].reshape(-1)))
    phi = tidir.load_features(paths['phi.pmi'], paths['phi.pmi_w1'], paths['phi.ed'], paths['phi.ped'])
    return tt, phi


def test_tidir_sample_at_zero_thetas(tmp_path):
    """Zero thetas: every potential is 1 and every conditional marginal exactly uniform, so each drawn word index is
    floor(u * X) for the uniforms the documented generator call reproduces, and log q = -n_vars log X.  K1 to K12: all three
    kernel instances at trainer level."""
    S = _S()
    tt, _ = _clique_trainer(tmp_path)
    n_samples, seed = 3, 40
    per_instance = tt.sample(n_samples=n_samples, seed=seed)
    assert len(per_instance) == 11
    X, seen, ran = len(tt.en), 0, set()
    for i, (key, tr) in enumerate(tt.trainers.items()):
        B, n = tr.batch.B, tr.topo.n_vars
        u = torch.rand((n_samples, B, n), dtype=torch.float64, device=tr.device, generator=torch.Generator(tr.device).manual_seed(seed + i))
        want = np.floor(u.cpu().numpy() * X).astype(np.int64)
        ran.add((S.pick_kernel(X, tr.topo.n_msgs, n), tr.topo.P <= 3))
        for b, row in enumerate(tt.buckets[key]['rows']):
            positions, words, logq = per_instance[row['index']]
            assert positions == tuple(key[1]) and len(words) == len(logq) == n_samples
            for s in range(n_samples):
                assert words[s] == [tt.en[w] for w in want[s, b]], (key, b, s)
            np.testing.assert_allclose(logq, [-n * np.log(X)] * n_samples, rtol=1e-12)
            seen += 1
        x, lq = tr.sample(n_samples=2, seed=seed + i)
        assert x.dtype == np.int64 and lq.dtype == np.float64 and x.shape == (2, B, n) and lq.shape == (2, B)
        assert np.array_equal(x, want[:2])
        assert S.last_kernel() == S.pick_kernel(X, tr.topo.n_msgs, n)
    assert seen == 11 and ran == {(1, True), (1, False), (2, False)}


def test_tidir_sample_equals_the_walk_on_one_bucket(tmp_path):
    """Random thetas: the K3 bucket's samples and log q equal the walk on every instance's own graph as tidir_oracle_graph
    builds it, with the uniforms of the documented generator call; known words stay as given."""
    rs = np.random.RandomState(1)
    th_ee, th_ed = rs.randn(1, 3) * 0.3, rs.randn(1, 6) * 0.3
    tt, (phi_ee, phi_w1, phi_ed) = _clique_trainer(tmp_path, (th_ee, th_ed))
    i, key = [(i, k) for i, k in enumerate(tt.trainers) if len(k[1]) == 3][0]
    tr, b = tt.trainers[key], tt.buckets[key]
    n_samples, seed = 4, 70
    u = torch.rand((n_samples, tr.batch.B, 3), dtype=torch.float64, device=tr.device,
                   generator=torch.Generator(tr.device).manual_seed(seed + i)).cpu().numpy()
    walks, smallest = {}, np.inf
    for r in range(len(b['rows'])):
        g, inputs, roots, _ = tidir_oracle_graph(key, b, r, phi_ee, phi_w1, phi_ed, th_ee, th_ed)
        n = 3 if O.has_loops(g, roots[0]) else 1
        for s in range(n_samples):
            w = walks[s, r] = SC.walk(g.spec, inputs, roots[:n], u[s, r])
            smallest = min([smallest] + list(w['margin'].values()))
    _check_margin('clique fixture K3 bucket', walks, smallest)
    per_instance = tt.sample(n_samples=n_samples, seed=seed)
    x, logq = tr.sample(n_samples=n_samples, seed=seed + i)
    for (s, r), w in walks.items():
        assert [int(v) for v in x[s, r]] == [w['x'][v] for v in key[1]], (s, r)
        np.testing.assert_allclose(logq[s, r], w['logq'], rtol=1e-10)
        positions, words, lq = per_instance[b['rows'][r]['index']]
        assert positions == tuple(key[1]) and words[s] == [tt.en[w['x'][v]] for v in key[1]] and lq[s] == logq[s, r]
    # the remaining words given that one guess is known
    given = np.full((tr.batch.B, 3), -1, dtype=np.int32)
    given[:, 1] = b['var_labels'][:, 1]
    xg, _ = tr.sample(n_samples=2, seed=5, given=given)
    assert (xg[:, :, 1] == given[:, 1]).all()
