"""Cutset importance sampling on the GPU (libmlbp_cutsetis.so) against the NumPy statement of tests/test_cutsetis_cpu.py -- the
same `configs` and `log_q` on both sides -- and against the shipped exact library where it accepts the graph.

Bars, the sixth library's: log_z_hat, log_w and joint_logp within 1e-10 * max(1, |value|), marginals within 1e-10 absolute, ess
within 1e-10 relative.  The statement's own distance from enumeration is below 1e-12 (asserted in the CPU module).  Lists are
drawn by NumPy from a fixed seed (test_cutsetis_cpu.make_list), so log_q is exact on the host.  No test asserts a statistical
accuracy: every assertion is a deterministic function of its inputs.  Bit-for-bit claims compare graphs at an equal number of
chunks: the header makes a graph's bits a function of the graph, the cutset, its list and C = mlbp_cutsetis_chunks(B, N)."""
import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_cutsetis_cpu as S
import test_logz_cpu as LZ
import test_map_cpu as W
from helpers import batch_tables, tidir_gold, tidir_oracle_graph, write_tidir
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

X64 = ('cutsetis_x64_kernel', ())
GENERIC = ('cutsetis_generic_kernel', ())
COMBINE = ('cutsetis_combine_kernel', ())
# kernel -> the tests that launch it (tests/test_cutsetis_cpu.py holds this against the library's symbol table)
CASES = {
    X64: ['test_x64_shapes', 'test_list_edges', 'test_a_list_that_repeats_one_configuration', 'test_dead_entries',
          'test_the_full_list_is_exact_inference_and_the_zero_variance_list', 'test_shared_tables_and_batch_position_give_the_same_bits',
          'test_power_of_two_scaling', 'test_wide_range_tables', 'test_bad_entries_change_their_graph_alone', 'test_capture_and_replay',
          'test_the_default_proposal', 'test_tidir_estimate_report'],
    GENERIC: ['test_generic_shapes', 'test_list_edges', 'test_dead_entries', 'test_the_full_list_is_exact_inference_and_the_zero_variance_list',
              'test_shared_tables_and_batch_position_give_the_same_bits', 'test_power_of_two_scaling', 'test_wide_range_tables',
              'test_bad_entries_change_their_graph_alone', 'test_the_default_proposal'],
    COMBINE: ['test_x64_shapes', 'test_generic_shapes', 'test_list_edges'],
}
KERNEL_OF = {X64: 1, GENERIC: 2}
# every input family held against the statement here (tests/test_cutsetis_cpu.py asserts each is finite where claimed)
INPUTS_USED = {
    'k5_x64': 'test_x64_shapes', 'k8_x64': 'test_x64_shapes', 'k9_x64': 'test_x64_shapes', 'chain3_x64': 'test_x64_shapes',
    'k10_x64': 'test_generic_shapes', 'k5_x7': 'test_generic_shapes', 'ring5_x7': 'test_generic_shapes', 'ring3_x2': 'test_generic_shapes',
    'ring3_x65': 'test_generic_shapes', 'ring3_x257': 'test_generic_shapes', 'k3_x1024': 'test_generic_shapes',
    'star4_x9_cut': 'test_generic_shapes', 'star4_x9': 'test_generic_shapes',
    'k3_x64': 'test_list_edges', 'k3_x64_n1': 'test_list_edges', 'k3_x64_n5': 'test_list_edges', 'k3_x64_b1': 'test_list_edges',
    'ring5_x7_n1': 'test_list_edges',
    'k3_x64_dead': 'test_dead_entries', 'ring5_x7_dead': 'test_dead_entries',
    'k3_x64_wide': 'test_wide_range_tables', 'ring5_x7_wide': 'test_wide_range_tables',
}


def _M():
    from macaronicusermodeling_amd import cutsetis
    return cutsetis


def _batch(spec, inputs_list, tables=None, pair_tab=None, unary_tab=None):
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(spec)
    assert topo.var_ids == O.Graph(spec).var_order
    fb = FactorGraphBatch(topo, spec['X'], len(inputs_list))
    pair, unary = batch_tables(spec, topo, inputs_list) if tables is None else tables
    if topo.P:
        fb.set_pair_tables(pair, pair_tab)
    if topo.U:
        fb.set_unary_tables(unary, unary_tab)
    return fb


def _labels(fb, seed=0):
    return np.random.RandomState(seed).randint(0, fb.X, size=(fb.B, fb.topo.n_vars)).astype(np.int32)


def _dev(fb, configs, log_q):
    return (torch.from_numpy(np.ascontiguousarray(configs, dtype=np.int32)).to(fb.device),
            torch.from_numpy(np.ascontiguousarray(log_q, dtype=np.float64)).to(fb.device))


def _run(fb, configs, log_q, labels=None, cutset=None, kernel=None, fill=float('nan')):
    """One cutset_estimate(configs, log_q, log_w=True) call; last_kernel is held against pick_kernel in every case."""
    M = _M()
    marg = torch.full((fb.B, fb.topo.n_vars, fb.X), fill, dtype=torch.float64, device=fb.device)
    c, lq = _dev(fb, configs, log_q)
    out = fb.cutset_estimate(configs=c, log_q=lq, labels=labels, marginals=marg, cutset=cutset, log_w=True)
    ran = M.last_kernel()
    torch.cuda.synchronize()
    pl = M.plan(fb.topo, None if cutset is None else [fb.topo.var_index[v] for v in cutset], fb.X, fb.device)
    assert ran == M.pick_kernel(fb.X, fb.topo.n_vars, fb.topo.P, fb.topo.U, pl.n_forest), ran
    if kernel is not None:
        assert ran == KERNEL_OF[kernel], ran
    assert out[1] is marg and tuple(out[0].shape) == (fb.B,) and tuple(out[-1].shape) == tuple(lq.shape)
    got = dict(log_z_hat=out[0].cpu().numpy(), marg=marg.cpu().numpy(), ess=out[2].cpu().numpy(), log_w=out[-1].cpu().numpy())
    if labels is not None:
        got['joint'] = out[3].cpu().numpy()
    return got


def _close(a, b):
    """|a - b| / max(1, |b|), with equal infinities at distance 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        d = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    return float(np.where(a == b, 0.0, d).max()) if a.size else 0.0


def _compare(name, got, stated, labels=None, specs=None):
    worst = dict(z=0.0, m=0.0, e=0.0, w=0.0, j=0.0)
    for b, want in enumerate(stated):
        worst['z'] = max(worst['z'], _close(got['log_z_hat'][b], want['log_z_hat']))
        worst['m'] = max(worst['m'], float(np.abs(got['marg'][b] - want['marg']).max()))
        worst['e'] = max(worst['e'], abs(got['ess'][b] - want['ess']) / max(want['ess'], 1e-300) if want['ess'] else abs(got['ess'][b]))
        worst['w'] = max(worst['w'], _close(got['log_w'][b], want['log_w']))
        if labels is not None:
            g, inputs = specs
            score = W.score_of(g, inputs[b], dict(zip(g.var_order, (int(x) for x in labels[b]))))
            worst['j'] = max(worst['j'], _close(got['joint'][b], score - want['log_z_hat']))
    print('%s: log_z_hat within %.1e, marginals %.1e, ess %.1e (relative), log_w %.1e, joint_logp %.1e' % (
        name, worst['z'], worst['m'], worst['e'], worst['w'], worst['j']))
    assert max(worst.values()) <= 1e-10, (name, worst)


def _family(name, kernel, labels=True):
    spec, inputs, cut, configs, log_q, stated = S.family(name)
    fb = _batch(spec, inputs)
    lab = _labels(fb, 1) if labels else None
    got = _run(fb, configs, log_q, labels=lab, cutset=cut if INPUTS_CUTSET.get(name) else None, kernel=kernel)
    _compare(name, got, stated, lab, (O.Graph(spec), inputs))
    return fb, got


INPUTS_CUTSET = {'star4_x9_cut': True}                           # families that name their cutset


# ---- shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['k5_x64', 'k8_x64', 'k9_x64', 'chain3_x64'])
def test_x64_shapes(name):
    """K5: the first shape the exact family refuses.  K8: six cut positions, 36 bits of configuration.  K9: the last on the
    X = 64 kernel.  The chain of three: the empty cutset, every entry the one configuration -- log_z_hat is log Z."""
    fb, got = _family(name, X64)
    if name == 'chain3_x64':
        spec, inputs = S.family(name)[:2]
        assert tuple(S.family(name)[3].shape[1:]) == (6, 0)
        for b, i in enumerate(inputs):
            z, m, _ = R.enumerate_exact(O.Graph(spec), i)
            assert _close(got['log_z_hat'][b], z) <= 1e-10 and np.abs(got['marg'][b] - m).max() <= 1e-10 and abs(got['ess'][b] - 6) <= 1e-9
    else:
        from macaronicusermodeling_amd import cutset
        with pytest.raises(cutset.CutsetError, match='configurations'):
            fb.exact_inference()


@pytest.mark.parametrize('name', ['k10_x64', 'k5_x7', 'ring5_x7', 'ring3_x2', 'ring3_x65', 'ring3_x257', 'k3_x1024', 'star4_x9_cut', 'star4_x9'])
def test_generic_shapes(name):
    """K10 at X = 64 falls to the generic kernel by the LDS rule; odd sizes around a wave and past a workgroup's 256 threads; K3
    at X = 1024 with its vectors in the workspace; a branching forest under one cut leaf; a tree with the empty cutset."""
    M = _M()
    fb, got = _family(name, GENERIC)
    if name == 'k3_x1024':
        assert M.workspace_bytes(1, 1024, 3, 3, 3, 1, 2) == 2 * (3 * 1024 + 3 + 17 * 1024) * 8
    if name == 'star4_x9':
        spec, inputs = S.family(name)[:2]
        for b, i in enumerate(inputs):
            z, m, _ = R.enumerate_exact(O.Graph(spec), i)
            assert _close(got['log_z_hat'][b], z) <= 1e-10 and np.abs(got['marg'][b] - m).max() <= 1e-10


# ---- list edges -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel', [('k3_x64_n1', X64), ('k3_x64_n5', X64), ('k3_x64', X64), ('k3_x64_b1', X64), ('ring5_x7_n1', GENERIC)])
def test_list_edges(name, kernel):
    """N = 1; N = 5, where waves have no entry and their partials are empty; N = 64 at B = 4, below the 4 C = 256 walkers; the
    longest list, 65536 entries on K3 at B = 1."""
    M = _M()
    N = S.family(name)[4].shape[1]
    B = len(S.family(name)[1])
    if name == 'k3_x64':
        assert N < 4 * M.chunks(B, N)
    if name == 'k3_x64_n5':
        assert M.chunks(B, N) == 5                              # 20 walkers for 5 entries
    if name == 'k3_x64_b1':
        assert (B, N) == (1, M.MAX_LISTED) and M.chunks(B, N) == 512
    _family(name, kernel)


def test_a_list_that_repeats_one_configuration():
    """Every weight is the same number: ess = (N w)^2 / (N w^2) = N, log_z_hat = log_w, the marginals are m_c."""
    spec, inputs, cut = S.family('k5_x64')[:3]
    g = O.Graph(spec)
    N = 12
    configs = np.tile(np.array([[3, 60, 17]], dtype=np.int32), (len(inputs), N, 1))
    log_q = np.tile(np.array([[-2.5], [-7.0], [-11.25]]), (1, N))
    got = _run(_batch(spec, inputs), configs, log_q, kernel=X64)
    stated = [S.Statement(g, i, cut).run(configs[b], log_q[b]) for b, i in enumerate(inputs)]
    _compare('k5_x64 repeated', got, stated)
    for b in range(len(inputs)):
        assert np.ptp(got['log_w'][b]) == 0.0
        assert abs(got['ess'][b] - N) <= 1e-12 * N and abs(got['log_z_hat'][b] - got['log_w'][b][0]) <= 1e-12 * abs(got['log_w'][b][0])


@pytest.mark.parametrize('name,kernel', [('k3_x64_dead', X64), ('ring5_x7_dead', GENERIC)])
def test_dead_entries(name, kernel):
    """Graph 0: dead entries (Z_c = 0) among live ones -- log_w -inf, nothing added.  Graph 1: an all-dead list -- log_z_hat -inf,
    uniform marginals, ess 0."""
    fb, got = _family(name, kernel, labels=False)
    stated = S.family(name)[5]
    dead = np.isneginf(stated[0]['log_w'])
    assert dead.any() and not dead.all() and np.array_equal(np.isneginf(got['log_w'][0]), dead)
    assert got['log_z_hat'][1] == -np.inf and got['ess'][1] == 0.0 and np.isneginf(got['log_w'][1]).all()
    assert np.array_equal(got['marg'][1], np.full_like(got['marg'][1], 1.0 / fb.X))


# ---- against the shipped exact library --------------------------------------------------------------------
@pytest.mark.parametrize('name,make,seeds,kernel', [('k3_x64', lambda: R.kn_spec(3, 64), (1, 2, 3), X64), ('k4_x64', lambda: R.kn_spec(4, 64), (1, 2), X64),
                                                    ('ring5_x7', lambda: C.ring_spec(5, 7), (1, 2, 3), GENERIC)], ids=['k3_x64', 'k4_x64', 'ring5_x7'])
def test_the_full_list_is_exact_inference_and_the_zero_variance_list(name, make, seeds, kernel):
    """Every configuration once with log_q = -ln N: log_z_hat and the marginals are exact_inference's at 1e-10.  Then log_q =
    log_w - log_z from that call, the proposal Z_c / Z: ess = N at 1e-9 relative and log_z_hat = log_z at 1e-10."""
    spec = make()
    inputs = [C.make_inputs(spec, s, 'lognormal') for s in seeds]
    fb = _batch(spec, inputs)
    n_cut = len(R.chosen_ids(spec))
    full = S.full_list(spec['X'], n_cut)
    N, B = len(full), len(inputs)
    configs, log_q = np.tile(full[None], (B, 1, 1)), np.full((B, N), -np.log(N))
    log_z, marg = fb.exact_inference()
    log_z, marg = log_z.cpu().numpy(), marg.cpu().numpy()
    got = _run(fb, configs, log_q, kernel=kernel)
    print('%s: N = %d, log_z_hat within %.1e of exact_inference, marginals %.1e' % (name, N, _close(got['log_z_hat'], log_z), np.abs(got['marg'] - marg).max()))
    assert _close(got['log_z_hat'], log_z) <= 1e-10 and np.abs(got['marg'] - marg).max() <= 1e-10
    zero = _run(fb, configs, got['log_w'] + log_q - log_z[:, None], kernel=kernel)
    assert (np.abs(zero['ess'] - N) <= 1e-9 * N).all(), zero['ess']
    assert _close(zero['log_z_hat'], log_z) <= 1e-10 and _close(zero['log_w'], np.tile(log_z[:, None], (1, N))) <= 1e-10


# ---- properties -----------------------------------------------------------------------------------------
def test_shared_tables_and_batch_position_give_the_same_bits():
    M = _M()
    for name, kernel in (('k3_x64', X64), ('ring5_x7', GENERIC)):
        spec, inputs, cut, configs, log_q, _ = S.family(name)
        N = log_q.shape[1]
        fb = _batch(spec, inputs)
        labels = _labels(fb)
        full = _run(fb, configs, log_q, labels=labels, kernel=kernel)
        pair, unary = batch_tables(spec, fb.topo, inputs)
        P, U = fb.topo.P, fb.topo.U
        ptab, utab = np.arange(4 * P).reshape(4, P), np.arange(4 * U).reshape(4, U)
        ptab[0], utab[0] = ptab[2], utab[2]                     # graphs 0 and 2 both read the tables of graph 2
        c2, q2, l2 = configs.copy(), log_q.copy(), labels.copy()
        c2[0], q2[0], l2[0] = configs[2], log_q[2], labels[2]
        shared = _run(_batch(spec, inputs, (pair, unary), ptab, utab), c2, q2, labels=l2)
        for key in ('log_z_hat', 'marg', 'ess', 'log_w', 'joint'):
            assert np.array_equal(shared[key][0], full[key][2]) and np.array_equal(shared[key][1:], full[key][1:]), key
        assert M.chunks(1, N) == M.chunks(4, N) == N            # B = 1 equals the graph inside the batch, at an equal number of chunks
        alone = _run(_batch(spec, inputs[1:2]), configs[1:2], log_q[1:2], labels=labels[1:2], kernel=kernel)
        for key in ('log_z_hat', 'marg', 'ess', 'log_w', 'joint'):
            assert np.array_equal(alone[key][0], full[key][1]), key


def test_power_of_two_scaling():
    """Any table times 2^k: no bit of the marginals or of ess moves, log_z_hat and log_w move by k ln 2."""
    for name, kernel, moves in (('k5_x64', X64, [({0: 400}, {}), ({3: -400, 9: 37}, {1: -300}), ({}, {0: 400, 4: -11})]),
                                ('ring5_x7', GENERIC, [({0: 400}, {}), ({4: -400}, {2: 5}), ({1: 3}, {0: -400})])):
        spec, inputs, cut, configs, log_q, _ = S.family(name)
        fb = _batch(spec, inputs)
        base = _run(fb, configs, log_q, kernel=kernel)
        pair, unary = batch_tables(spec, fb.topo, inputs)
        P, U = fb.topo.P, fb.topo.U
        for pk, uk in moves:
            p2, u2 = pair.copy(), unary.copy()
            for b in range(fb.B):
                for p, k in pk.items():
                    p2[b * P + p] = np.ldexp(p2[b * P + p], k)
                for u, k in uk.items():
                    u2[b * U + u] = np.ldexp(u2[b * U + u], k)
            got = _run(_batch(spec, inputs, (p2, u2)), configs, log_q, kernel=kernel)
            shift = (sum(pk.values()) + sum(uk.values())) * np.log(2.0)
            assert np.array_equal(got['marg'], base['marg']) and np.array_equal(got['ess'], base['ess']), (name, pk, uk)
            assert _close(got['log_z_hat'], base['log_z_hat'] + shift) <= 1e-12 and _close(got['log_w'], base['log_w'] + shift) <= 1e-12, (name, pk, uk)


@pytest.mark.parametrize('name,kernel', [('k3_x64_wide', X64), ('ring5_x7_wide', GENERIC)])
def test_wide_range_tables(name, kernel):
    """exp(20 N(0, 1)) tables, 170 decades each, as the siblings' *_wide families."""
    _family(name, kernel)


@pytest.mark.parametrize('name,kernel', [('k5_x64', X64), ('ring5_x7', GENERIC)])
def test_bad_entries_change_their_graph_alone(name, kernel):
    """A state outside [0, X), a NaN log_q, a table index outside its array: log_z_hat, ess and joint_logp NaN, the marginals left
    as they were.  A NaN table entry that the listed entries read: log_z_hat not finite.  Every neighbour keeps its bits."""
    spec, inputs, cut, configs, log_q, _ = S.family(name)
    X, N = spec['X'], log_q.shape[1]
    inputs = list(inputs) + [C.make_inputs(spec, s, 'lognormal') for s in (11, 12, 13)]
    g = O.Graph(spec)
    more = [S.make_list(g, i, cut, N, 40 + b) for b, i in enumerate(inputs[len(configs):])]
    configs = np.concatenate([configs] + [c[None] for c, _ in more])
    log_q = np.concatenate([log_q] + [q[None] for _, q in more])
    B = len(inputs)
    assert B >= 6
    fb = _batch(spec, inputs)
    labels = _labels(fb)
    base = _run(fb, configs, log_q, labels=labels, kernel=kernel)
    pair, unary = batch_tables(spec, fb.topo, inputs)
    u2 = unary.copy()
    u2[3 * fb.topo.U + fb.topo.U - 1][1] = np.nan               # graph 3: a NaN table entry, on a free variable: every entry reads it
    c2, q2 = configs.copy(), log_q.copy()
    c2[0, N // 2, len(cut) - 1] = X                             # graph 0: a state one past the last
    c2[1, 0, 0] = -1                                            # graph 1: a negative state
    q2[2, N - 1] = np.nan                                       # graph 2: a NaN log_q
    fb2 = _batch(spec, inputs, (pair, u2))
    fb2.unary_tab[4, 0] = fb2.unary_tables.shape[0]             # graph 4: a table index outside the array
    got = _run(fb2, c2, q2, labels=labels, kernel=kernel, fill=-7.0)
    for b in (0, 1, 2, 4):
        assert np.isnan(got['log_z_hat'][b]) and np.isnan(got['ess'][b]) and np.isnan(got['joint'][b]) and (got['marg'][b] == -7.0).all(), b
    assert not np.isfinite(got['log_z_hat'][3])
    for b in range(5, B):
        for key in ('log_z_hat', 'marg', 'ess', 'log_w', 'joint'):
            assert np.array_equal(got[key][b], base[key][b]), (b, key)
    q3 = log_q.copy()
    q3[0, 1], q3[1, 2] = np.inf, -2e6                           # +inf, and a magnitude past MLBP_CUTSETIS_MAX_ABS_LOG_Q
    got = _run(fb, configs, q3, labels=labels, kernel=kernel, fill=-7.0)
    assert np.isnan(got['log_z_hat'][:2]).all() and (got['marg'][:2] == -7.0).all()
    for key in ('log_z_hat', 'marg', 'ess', 'log_w', 'joint'):
        assert np.array_equal(got[key][2:], base[key][2:]), key


def test_capture_and_replay():
    """After one eager call the call is captured; replayed with changed tables and a changed list it gives the eager bits of those."""
    spec, inputs, cut, configs, log_q, _ = S.family('k5_x64')
    fb = _batch(spec, inputs)
    labels = torch.from_numpy(_labels(fb)).to(fb.device)
    _run(fb, configs, log_q, labels=labels, kernel=X64)
    c, lq = _dev(fb, configs, log_q)
    marg = torch.empty(fb.B, fb.topo.n_vars, fb.X, dtype=torch.float64, device=fb.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fb.cutset_estimate(configs=c, log_q=lq, labels=labels, marginals=marg, log_w=True)
    g = O.Graph(spec)
    for round_ in range(2):
        if round_:
            fb.pair_tables.mul_(1.5)
            fb.unary_tables[0].mul_(0.25)
            other = [S.make_list(g, i, cut, log_q.shape[1], 90 + b) for b, i in enumerate(inputs)]
            c.copy_(torch.from_numpy(np.stack([x for x, _ in other])).to(fb.device))
            lq.copy_(torch.from_numpy(np.stack([x for _, x in other])).to(fb.device))
        eager = _run(fb, c.cpu().numpy(), lq.cpu().numpy(), labels=labels, kernel=X64)
        for t in out:
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for key, t in zip(('log_z_hat', 'marg', 'ess', 'joint', 'log_w'), out):
            assert np.array_equal(t.cpu().numpy(), eager[key]), (round_, key)


# ---- the proposal ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,make', [('k5_x64', lambda: R.kn_spec(5, 64)), ('ring5_x7', lambda: C.ring_spec(5, 7))], ids=['k5_x64', 'ring5_x7'])
def test_the_default_proposal(name, make, monkeypatch):
    from macaronicusermodeling_amd import batch as BT
    spec = make()
    inputs = [C.make_inputs(spec, s, 'lognormal') for s in (1, 2, 3)]
    fb = _batch(spec, inputs)
    topo = fb.topo
    roots = list(topo.var_ids)
    N = 16
    configs, log_q = fb.cutset_proposal(roots, N, seed=3)
    assert configs.dtype == torch.int32 and tuple(configs.shape) == (fb.B, N, len(R.chosen_ids(spec))) and tuple(log_q.shape) == (fb.B, N)
    # cutset_estimate(roots, n_samples, seed) is cutset_estimate(configs, log_q) of that list, bit for bit
    a = fb.cutset_estimate(roots, n_samples=N, seed=3, log_w=True)
    b = fb.cutset_estimate(configs=configs, log_q=log_q, log_w=True)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    assert np.isfinite(a[0].cpu().numpy()).all() and (a[2].cpu().numpy() >= 1 - 1e-9).all()
    # the list is what one sample(order=..., cond_marginals=...) call gives
    cut = [topo.var_index[v] for v in R.chosen_ids(spec)]
    order = R.chosen_ids(spec) + [v for v in topo.var_ids if v not in R.chosen_ids(spec)]
    gen = torch.Generator(fb.device).manual_seed(3)
    uniforms = torch.rand((N, fb.B, topo.n_vars), dtype=torch.float64, device=fb.device, generator=gen)
    cond = torch.empty(N, fb.B, topo.n_vars, fb.X, dtype=torch.float64, device=fb.device)
    samples, _ = fb.sample(roots, N, uniforms=uniforms, order=order, cond_marginals=cond)
    samples, cond = samples.cpu().numpy(), cond.cpu().numpy()
    want_c = np.transpose(samples[:, :, cut], (1, 0, 2))
    want_q = np.zeros((fb.B, N))
    for s in range(N):
        for g_ in range(fb.B):
            lq = 0.0
            for q, v in enumerate(cut):
                term = np.log(cond[s, g_, v, samples[s, g_, v]])
                lq = term if q == 0 else lq + term
            want_q[g_, s] = lq
    assert np.array_equal(configs.cpu().numpy(), want_c)
    assert np.abs(log_q.cpu().numpy() - want_q).max() <= 1e-12 * np.abs(want_q).max()
    same = fb.cutset_proposal(roots, N, uniforms=uniforms)
    assert np.array_equal(same[0].cpu().numpy(), want_c) and np.array_equal(same[1].cpu().numpy(), log_q.cpu().numpy())
    # the byte bound only slices the draws: one draw per sample() call, then five
    per_draw = fb.B * topo.n_vars * fb.X * 8
    for bound in (1, 5 * per_draw):
        monkeypatch.setattr(BT, 'CUTSET_PROPOSAL_BYTES', bound)
        c2, q2 = fb.cutset_proposal(roots, N, seed=3)
        assert np.array_equal(c2.cpu().numpy(), want_c) and np.array_equal(q2.cpu().numpy(), log_q.cpu().numpy()), bound
    with pytest.raises(ValueError):
        fb.cutset_estimate(configs=configs)
    with pytest.raises(ValueError):
        fb.cutset_estimate(roots, n_samples=N)


def test_the_proposal_on_a_tree():
    spec = C.star_spec(4, 9)
    fb = _batch(spec, [C.make_inputs(spec, s) for s in (1, 2)])
    configs, log_q = fb.cutset_proposal(list(fb.topo.var_ids), 4, seed=1)
    assert tuple(configs.shape) == (2, 4, 0) and (log_q.cpu().numpy() == 0.0).all()
    log_z_hat, marg, ess = fb.cutset_estimate(list(fb.topo.var_ids), n_samples=4, seed=1)
    for b in range(2):
        z, m, _ = R.enumerate_exact(O.Graph(spec), C.make_inputs(spec, b + 1))
        assert _close(log_z_hat[b].item(), z) <= 1e-10 and np.abs(marg[b].cpu().numpy() - m).max() <= 1e-10


def test_float32_tables_are_refused():
    spec = C.user_spec(10, [1, 4, 7], 256, 64, seed=1)
    fb = _batch(spec, [C.make_inputs(spec, 1)])
    fb.set_pair_tables(fb.pair_tables, dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        fb.cutset_estimate(list(fb.topo.var_ids), n_samples=4, seed=0)


# ---- trainer --------------------------------------------------------------------------------------------
def test_tidir_estimate_report(tmp_path):
    """TiDirTrainer.estimate_report(16, seed=5) on the clique fixture's sentences of 3, 4 and 6 predicted words, under its own
    thetas: every instance against the statement on its own graph (tidir_oracle_graph) and the list the trainer's proposal drew
    for it; K3 and K4 carry exact_inference's log_z, the six-word sentences None -- and exactness_report() still skips them."""
    from macaronicusermodeling_amd import tidir
    from test_gpu_cliques import _trainer
    gold = dict(tidir_gold('tidir_cliques_reference'))
    keep, count = [], {3: 0, 4: 0, 6: 0}
    for line in gold['instances']:
        for key in tidir.bucket_instances([tidir.parse_instance(line)], gold['vocab_en'], gold['vocab_de']):
            if len(key[1]) in count and count[len(key[1])] < 2:
                count[len(key[1])] += 1
                keep.append(line)
    assert all(count.values())
    gold['instances'] = keep
    paths = write_tidir(gold, str(tmp_path))
    tt = _trainer(paths, gold)
    phi_ee, phi_w1, phi_ed = tidir.load_features(paths['phi.pmi'], paths['phi.pmi_w1'], paths['phi.ed'], paths['phi.ped'])
    th_ee, th_ed = np.array(gold['theta_en_en']).reshape(1, -1), np.array(gold['theta_en_de']).reshape(1, -1)
    n, seed = 16, 5
    per_instance, totals, skipped = tt.estimate_report(n_samples=n, seed=seed)
    assert skipped == [] and len(per_instance) == len(keep)
    seen = both = 0
    sum_err = worst = share = 0.0
    for i, (key, tr) in enumerate(tt.trainers.items()):
        b = tt.buckets[key]
        tr.build_potentials()
        roots = tr.roots[:tr.n_sweeps_run]
        configs, log_q = tr.batch.cutset_proposal(roots, n, seed=seed + i)
        configs, log_q = configs.cpu().numpy(), log_q.cpu().numpy()
        exact = tr.exact_inference()[0] if len(key[1]) <= 4 else None
        for r, row in enumerate(b['rows']):
            g, inputs, oroots, _ = tidir_oracle_graph(key, b, r, phi_ee, phi_w1, phi_ed, th_ee, th_ed)
            assert list(g.var_order) == list(tr.topo.var_ids)
            want = S.Statement(g, inputs, list(g.var_order)[:len(key[1]) - 2]).run(configs[r], log_q[r])
            _, msgs, _ = O.run(g.spec, inputs, oroots[:tr.n_sweeps_run], tr.n_sweeps_run, force_loopy=True)
            bethe = LZ.log_partition(g, inputs, msgs)
            positions, z_hat, rse, gap, z = per_instance[row['index']]
            assert positions == tuple(key[1])
            assert _close(z_hat, want['log_z_hat']) <= 1e-10, (key, r, z_hat, want['log_z_hat'])
            assert abs(rse - np.sqrt(max(1.0 / want['ess'] - 1.0 / n, 0.0))) <= 1e-8
            assert abs(gap - (bethe - want['log_z_hat'])) <= 2e-10 * max(1.0, abs(want['log_z_hat']))
            seen += 1
            share += want['ess'] / n
            if exact is None:
                assert z is None
            else:
                assert z == float(exact[r])
                both += 1
                sum_err += abs(z_hat - z)
                worst = max(worst, abs(z_hat - z))
    assert totals[0] == seen == len(keep) and totals[1] == both == count[3] + count[4]
    assert abs(totals[2] - sum_err) <= 1e-9 and abs(totals[3] - worst) <= 1e-12 and abs(totals[4] - share) <= 1e-8
    report = tt.exactness_report()
    assert [s[0] for s in report[2]] == [tuple(k[1]) for k in tt.trainers if len(k[1]) == 6] and all('configurations' in s[2] for s in report[2])
