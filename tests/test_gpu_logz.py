"""log Z and the joint log-likelihood on the GPU (libmlbp_logz.so) against the float64 NumPy statement of
tests/test_logz_cpu.py.

Two comparisons per case, for log_z, score and joint_logp of every graph.
  Kernel alone: sweep() on the device, copy the messages back, evaluate the NumPy statement on those DEVICE messages.
    atol = 2 (F + V) (X^2 + 16) 2^-53, plus rtol 1e-12: a positive sum of n terms carries (n - 1) u relative error, each of
    the F + V logarithms takes one such sum of at most X^2 terms (16 more for the products under it), and the factor 2 covers
    the two summation orders.  2.7e-11 for the K3 user graph (F = 27, V = 3).
  End to end: the oracle's sweeps, then the statement.  The same atol plus 1e-10 per message factor that enters a Z term (the
    project's 1e-10 bar on messages, propagated linearly; the count is computed from the topology and printed).
Every case records last_kernel() and asserts the instance it was written for.

Mutations these cases are built to catch:
  * the uniform 1/X left in the products (the sweeps' own product has it): off by n_vars log X -- every case, and exactly
    so in test_trainer_at_zero_thetas;
  * d_v in place of d_v - 1: off by sum_v log Z_v -- every case; test_k1_equals_the_log_marginal has d_v = 10 and no pairwise
    factor to hide behind;
  * the two table axes swapped in Z_f or in the score: every case with a pairwise factor compares against the statement's
    by-axis contraction and score; test_small_x_trees_equal_brute_force holds star graphs with the hub on either axis;
  * stale variable->factor slots used instead of leave-one-out products of factor->variable messages: identical on trees, but
    after 3 sweeps on a loopy graph the stored variable->factor messages are older than the incoming ones; test_ring,
    test_k3_unique_tables, test_k4 and test_k7 compare against the statement, which reads factor->variable messages only."""
import numpy as np
import pytest

import cases as C
import test_logz_cpu as S
import test_map_cpu as W
from helpers import batch_tables, tidir_gold, tidir_oracle_graph, write_tidir
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

X64 = ('logz_x64_kernel', ())
X64_SHARED = ('logz_x64_shared_kernel', ())
GENERIC = ('logz_generic_kernel', ())
SUM = ('logz_sum_kernel', ())
# kernel -> the tests that launch it (tests/test_logz_cpu.py holds this against the library's symbol table)
CASES = {
    X64: ['test_k3_unique_tables', 'test_k1_equals_the_log_marginal', 'test_k4', 'test_k7', 'test_chain_equals_the_forward_algorithm',
          'test_ring', 'test_unnormalised_messages', 'test_degenerate_inputs', 'test_capture_and_replay'],
    X64_SHARED: ['test_shared_tables_equal_unique_copies', 'test_shared_group_with_an_odd_graph', 'test_shared_batch_sizes',
                 'test_degenerate_inputs', 'test_tidir_on_synthetic_sentences', 'test_tidir_on_the_clique_fixture'],
    GENERIC: ['test_x128', 'test_x512', 'test_small_x_trees_equal_brute_force', 'test_unnormalised_messages', 'test_degenerate_inputs'],
    SUM: ['test_k3_unique_tables', 'test_x128', 'test_shared_batch_sizes', 'test_capture_and_replay'],
}
KERNEL_OF = {X64: 1, X64_SHARED: 2, GENERIC: 3}     # mlbp_logz.h MLBP_LOGZ_KERNEL_*


def _L():
    from macaronicusermodeling_amd import logz
    return logz


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


def _labels(fb, seed=0):
    return np.random.RandomState(seed).randint(0, fb.X, size=(fb.B, fb.topo.n_vars)).astype(np.int32)


def _run(fb, roots, labels, init=True):
    """log_partition with every output; roots=None reads fb.msgs as they are."""
    nan = float('nan')
    lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(fb.device)
    score = torch.full((fb.B,), nan, dtype=torch.float64, device=fb.device)
    sums = torch.full((2,), nan, dtype=torch.float64, device=fb.device)
    log_z, joint = fb.log_partition(roots, init=init, labels=lab, score=score, sum_out=sums)
    kernel = _L().last_kernel()
    torch.cuda.synchronize()
    return dict(log_z=log_z.cpu().numpy(), score=score.cpu().numpy(), joint=joint.cpu().numpy(), sums=sums.cpu().numpy(),
                msgs=fb.msgs.cpu().numpy(), kernel=kernel)


def kernel_atol(topo, X):
    return 2.0 * (topo.n_factors + topo.n_vars) * (X * X + 16) * 2.0 ** -53


def message_factors(topo):
    """How many message factors enter the Z terms of one graph: d_v in Z_v, d_v - 1 in the Z_f of each of v's factors."""
    d = [int(topo.in_off[v + 1] - topo.in_off[v]) for v in range(topo.n_vars)]
    return sum(dv + dv * (dv - 1) for dv in d)


def _close(got, want, atol, what):
    if np.isnan(want):
        assert np.isnan(got), (what, got, want)
        return 0.0
    if np.isinf(want):
        assert got == want, (what, got, want)
        return 0.0
    err = abs(got - want)
    assert err <= atol + 1e-12 * abs(want), (what, got, want, err, atol)
    return err


def _compare(name, spec, topo, inputs_list, roots, labels, got, normalize=True, graphs=None, walk=True, ref=None):
    """Device results against the statement on the device's own messages (kernel alone) and on the oracle's sweeps (end to
    end), graph by graph.  Prints the figures before it asserts the batch sums.
    ref: {graph: messages of S.sweeps} computed beforehand on the same inputs, roots and `normalize` (read, never written)."""
    keys = C.msg_keys(spec)
    a_kernel = kernel_atol(topo, spec['X'])
    n_mf = message_factors(topo)
    a_walk = a_kernel + 1e-10 * n_mf
    worst = dict(kernel=0.0, walk=0.0)
    todo = list(range(len(inputs_list)) if graphs is None else graphs)
    for b in todo:
        g = O.Graph(spec)
        x = {v: int(labels[b, i]) for i, v in enumerate(topo.var_ids)}
        dev = dict(zip(keys, got['msgs'][b]))
        want = S.joint_logp(g, inputs_list[b], dev, x)
        for k, w in zip(('log_z', 'score', 'joint'), want):
            worst['kernel'] = max(worst['kernel'], _close(got[k][b], w, a_kernel, '%s graph %d %s (kernel alone)' % (name, b, k)))
        if walk:
            msgs = S.sweeps(spec, inputs_list[b], roots, normalize=normalize)[1] if ref is None else ref[b]
            want = S.joint_logp(g, inputs_list[b], msgs, x)
            for k, w in zip(('log_z', 'score', 'joint'), want):
                worst['walk'] = max(worst['walk'], _close(got[k][b], w, a_walk, '%s graph %d %s (end to end)' % (name, b, k)))
    print('%s: %d graphs, kernel alone worst |diff| %.2e (atol %.2e), end to end worst %.2e (atol %.2e, %d message factors)'
          % (name, len(todo), worst['kernel'], a_kernel, worst['walk'], a_walk, n_mf))
    if np.isfinite(got['joint']).all():
        B = len(got['log_z'])
        _close(got['sums'][0], float(np.sum(got['log_z'])), B * a_kernel, name + ' sum of log_z')
        _close(got['sums'][1], float(np.sum(got['joint'])), B * a_kernel, name + ' sum of joint_logp')


def _case(name, spec, seeds, roots, instance, kind='uniform', normalize=True):
    inputs = [C.make_inputs(spec, s, kind) for s in seeds]
    fb = _batch(spec, inputs, normalize=normalize)
    labels = _labels(fb, seed=len(inputs))
    got = _run(fb, roots, labels)
    flags = _L().SHARED_PAIR_TABLES if getattr(fb, 'pair_tables_shared', False) else 0
    assert got['kernel'] == KERNEL_OF[instance] == _L().pick_kernel(spec['X'], int(fb.topo.in_off[-1]), fb.topo.n_vars, flags), name
    _compare(name, spec, fb.topo, inputs, roots, labels, got, normalize=normalize)
    return fb, inputs, labels, got


K3 = dict(spec=lambda: C.user_spec(10, [1, 4, 7], 64, 64, seed=1), seeds=range(500, 564), roots=[1, 4, 7])


def test_k3_unique_tables():
    fb, _, _, _ = _case('K3', K3['spec'](), K3['seeds'], K3['roots'], X64)
    assert (fb.topo.n_factors, fb.topo.n_vars) == (27, 3) and abs(kernel_atol(fb.topo, 64) - 2.7e-11) < 1e-12


def test_k1_equals_the_log_marginal():
    """P = 0: the graph is one variable under its unary factors, and the joint log-likelihood of its label is the log of its
    marginal at the label."""
    fb, _, labels, got = _case('K1', C.user_spec(10, [4], 64, 64, seed=3), range(16), [4], X64)
    assert fb.topo.P == 0 and fb.topo.n_vars == 1
    marg = fb.marginals().cpu().numpy()
    for b in range(fb.B):
        _close(got['joint'][b], float(np.log(marg[b, 0, labels[b, 0]])), kernel_atol(fb.topo, 64), 'K1 graph %d' % b)


def test_k4():
    fb, _, _, _ = _case('K4', C.user_spec(10, [0, 2, 5, 8], 64, 64, seed=4), range(700, 732), [0, 2, 5], X64)
    assert fb.topo.P == 6


def test_k7():
    """84 in-slots = 42 KiB of messages: inside the X = 64 kernel's LDS budget of mlbp_logz.h."""
    L = _L()
    spec = C.user_spec(12, [0, 1, 3, 5, 7, 9, 11], 64, 64, seed=5)
    fb, _, _, _ = _case('K7', spec, range(800, 816), [0, 1, 3], X64)
    assert (int(fb.topo.in_off[-1]), fb.topo.P) == (84, 21) and 84 * 512 + 4096 + 64 <= L.X64_LDS_BYTES


def _forward_log_z(spec, inputs):
    """Exact log Z of a chain by the forward algorithm over the tables, rescaled at every step."""
    g = O.Graph(spec)
    n = len(spec['var_ids'])
    unary = [O.factor_table(g, inputs, g.by_id[i]).reshape(-1) for i in range(n)]
    pair = [O.factor_table(g, inputs, g.by_id[n + i]) for i in range(n - 1)]
    alpha, total = unary[0], 0.0
    for i in range(n - 1):
        s = alpha.sum()
        total += np.log(s)
        alpha = (alpha / s).dot(pair[i]) * unary[i + 1]
    return float(total + np.log(alpha.sum()))


def test_chain_equals_the_forward_algorithm():
    spec = C.chain_spec(8, 64)
    fb, inputs, _, got = _case('chain8', spec, range(1, 33), [0], X64)
    for b, inp in enumerate(inputs):
        _close(got['log_z'][b], _forward_log_z(spec, inp), kernel_atol(fb.topo, 64) + 1e-10 * message_factors(fb.topo), 'chain8 graph %d' % b)


@pytest.mark.parametrize('roots', [[0, 3, 5], [0, 3, 5, 0, 3, 5, 0, 3, 5, 0]], ids=['3_sweeps', '10_sweeps'])
def test_ring(roots):
    _case('ring8/%d sweeps' % len(roots), C.ring_spec(8, 64), range(1, 33), roots, X64)


def test_x128():
    _case('X128', C.user_spec(10, [1, 4, 7], 128, 128, seed=1), range(500, 516), [1, 4, 7], GENERIC)


def test_x512():
    _case('X512', C.ring_spec(8, 512), range(1, 5), [0, 3, 5], GENERIC)


def test_small_x_trees_equal_brute_force():
    """The CPU module's tree cases on the device (X = 8 and X = 4, the generic kernel with its masked tails): log_z is the
    logsumexp of the whole grid and joint_logp the grid entry at the labels minus it."""
    todo = [(name, make(), [C.make_inputs(make(), s, kind) for s in range(40)], roots) for name, make, roots, kind in W.TREE_CASES]
    todo += [(s['name'], s, [C.make_inputs(s, i), C.make_inputs(s, 100 + i)], [s['var_ids'][0]]) for i, s in enumerate(W.random_trees())]
    for name, spec, inputs, roots in todo:
        fb = _batch(spec, inputs)
        labels = _labels(fb, seed=3)
        got = _run(fb, roots, labels)
        assert got['kernel'] == KERNEL_OF[GENERIC]
        _compare(name, spec, fb.topo, inputs, roots, labels, got)
        bound = kernel_atol(fb.topo, spec['X']) + 1e-10 * message_factors(fb.topo)
        for b, inp in enumerate(inputs):
            _, _, grid = W.brute_force(O.Graph(spec), inp)
            lse = S.logsumexp(grid)
            _close(got['log_z'][b], lse, bound, '%s graph %d log_z' % (name, b))
            _close(got['joint'][b], float(grid[tuple(int(v) for v in labels[b])]) - lse, bound, '%s graph %d joint' % (name, b))


def test_unnormalised_messages():
    """normalize_messages=False: other messages, the same log Z (the statement on the unnormalised walk)."""
    for sp, seeds, roots, inst in ((K3['spec'](), range(500, 508), [1, 4, 7], X64),
                                   (C.user_spec(10, [1, 4, 7], 128, 128, seed=1), (500, 501), [1, 4, 7], GENERIC)):
        fb, inputs, labels, got = _case('unnormalised X=%d' % sp['X'], sp, seeds, roots, inst, normalize=False)
        fb_n = _batch(sp, inputs)
        ref = _run(fb_n, roots, labels)
        assert not np.allclose(ref['msgs'], got['msgs'], rtol=1e-3)
        bound = kernel_atol(fb.topo, sp['X']) + 1e-10 * message_factors(fb.topo)
        for b in range(fb.B):
            _close(got['log_z'][b], ref['log_z'][b], 2 * bound, 'graph %d' % b)


# ---- shared tables ----------------------------------------------------------------------------------
def _shared_pair(B, odd=()):
    """K3 with two pairwise tables behind every graph ([0, 1, 0]; the graphs in `odd` name [1, 1, 0]) as (shared batch, batch of
    unique copies, inputs of the unique tables' source)."""
    spec = K3['spec']()
    distinct = [C.make_inputs(spec, s) for s in K3['seeds']]
    inputs = [distinct[b % len(distinct)] for b in range(B)]
    fb_u = _batch(spec, inputs)
    two = fb_u.pair_tables[:2].clone()
    tab = np.tile(np.array([[0, 1, 0]]), (B, 1))
    for b in odd:
        tab[b] = [1, 1, 0]
    unary = fb_u.unary_tables
    fb_s = _batch(spec, inputs, tables=(two, unary), pair_tab=tab)
    fb_c = _batch(spec, inputs, tables=(two[torch.from_numpy(tab.reshape(-1)).to(two.device)], unary))
    return spec, fb_s, fb_c


def _same(name, a, b, atol, B):
    worst = 0.0
    for k in ('log_z', 'score', 'joint'):
        for g in range(B):
            worst = max(worst, _close(a[k][g], b[k][g], atol, '%s graph %d %s' % (name, g, k)))
    print('%s: %d graphs, shared form against unique copies: worst |diff| %.2e (atol %.2e)' % (name, B, worst, atol))


def test_shared_tables_equal_unique_copies():
    spec, fb_s, fb_c = _shared_pair(64)
    assert fb_s.pair_tables_shared and not fb_c.pair_tables_shared
    labels = _labels(fb_s, seed=9)
    a, b = _run(fb_s, K3['roots'], labels), _run(fb_c, K3['roots'], labels)
    assert (a['kernel'], b['kernel']) == (KERNEL_OF[X64_SHARED], KERNEL_OF[X64])
    _same('K3 shared', a, b, kernel_atol(fb_s.topo, 64) + 1e-10 * message_factors(fb_s.topo), 64)
    # the messages of the shared batch, through both kernels: the kernels alone
    fb_c.msgs.copy_(fb_s.msgs)
    _same('K3 shared, one set of messages', a, _run(fb_c, None, labels), kernel_atol(fb_s.topo, 64), 64)


def test_shared_group_with_an_odd_graph():
    """One graph of the second 16-group, and the last graph of the ragged last group, name another table for factor 0: the
    claim fails for those two groups and that factor alone, which is then walked graph by graph -- same answers."""
    B, odd = 40, (21, 39)
    spec, fb_s, fb_c = _shared_pair(B, odd=odd)
    assert not fb_s.pair_tables_shared
    labels = _labels(fb_s, seed=10)
    fb_s.sweep(K3['roots'], init=True)
    fb_c.sweep(K3['roots'], init=True)
    fb_s.pair_tables_shared = True                    # the caller's claim; the kernel checks it per workgroup
    a, b = _run(fb_s, None, labels), _run(fb_c, None, labels)
    assert (a['kernel'], b['kernel']) == (KERNEL_OF[X64_SHARED], KERNEL_OF[X64])
    _same('K3 odd graph', a, b, kernel_atol(fb_s.topo, 64) + 1e-10 * message_factors(fb_s.topo), B)
    assert abs(a['log_z'][21] - a['log_z'][20]) > 1e-6


@pytest.mark.parametrize('B', [1, 15, 17, 100])
def test_shared_batch_sizes(B):
    """A ragged last workgroup in the 16-graph form: every graph is computed, nothing beyond the batch is touched."""
    spec, fb_s, fb_c = _shared_pair(B)
    labels = _labels(fb_s, seed=B)
    a = _run(fb_s, K3['roots'], labels)
    fb_c.pair_tables_shared = False                   # (B = 1: one row is trivially shared)
    b = _run(fb_c, K3['roots'], labels)
    assert (a['kernel'], b['kernel']) == (KERNEL_OF[X64_SHARED], KERNEL_OF[X64])
    _same('K3 shared B=%d' % B, a, b, kernel_atol(fb_s.topo, 64) + 1e-10 * message_factors(fb_s.topo), B)
    assert np.isfinite(a['joint']).all()
    _close(a['sums'][0], float(a['log_z'].sum()), B * kernel_atol(fb_s.topo, 64), 'sum of log_z')
    _close(a['sums'][1], float(a['joint'].sum()), B * kernel_atol(fb_s.topo, 64), 'sum of joint_logp')


# ---- degenerate inputs --------------------------------------------------------------------------------
def test_degenerate_inputs():
    """A zero table entry at the labels: score and joint_logp are -inf, log_z stays finite.  A table index outside the table
    array (written behind Python's check, after the sweeps): NaN for that graph only.  A label outside [0, X): NaN for that
    graph's score and joint_logp only.  On all three kernels."""
    L = _L()
    for sp, seeds, inst in ((K3['spec'](), range(500, 520), X64), (K3['spec'](), range(500, 520), X64_SHARED),
                            (C.user_spec(10, [1, 4, 7], 128, 128, seed=1), range(500, 506), GENERIC)):
        inputs = [C.make_inputs(sp, s) for s in seeds]
        fb = _batch(sp, inputs)
        topo, B = fb.topo, fb.B
        labels = _labels(fb, seed=2)
        pav = L.readout_arrays(topo)[0]
        i, j = int(labels[1, pav[0, 0]]), int(labels[1, pav[0, 1]])
        fb.pair_tables[1 * topo.P + 0, i, j] = 0.0                  # graph 1, pairwise factor 0, at its labels
        fb.sweep([1, 4, 7], init=True)
        fb.pair_tables_shared = inst == X64_SHARED                  # (unique tables: every group falls back factor by factor)
        clean = _run(fb, None, labels)
        assert clean['kernel'] == KERNEL_OF[inst]
        assert np.isneginf(clean['score'][1]) and np.isneginf(clean['joint'][1]) and np.isfinite(clean['log_z']).all()
        others = [b for b in range(B) if b != 1]
        assert np.isfinite(clean['score'][others]).all() and np.isfinite(clean['joint'][others]).all()
        _compare('zero entry %s' % inst[0], sp, topo, inputs, None, labels,
                 dict(clean, score=np.where(np.arange(B) == 1, np.nan, clean['score']), joint=np.where(np.arange(B) == 1, np.nan, clean['joint'])),
                 graphs=others, walk=False)
        bad_labels = labels.copy()
        bad_labels[2, 1] = sp['X']
        bad_labels[3, 0] = -1
        fb.pair_tab[B - 1, 1] = fb.pair_tables.shape[0]                # the last graph names a table beyond the array
        fb.unary_tab[4, 0] = -1
        got = _run(fb, None, bad_labels)
        for b in range(B):
            if b in (4, B - 1):
                assert np.isnan(got['log_z'][b]) and np.isnan(got['score'][b]) and np.isnan(got['joint'][b]), b
            elif b in (2, 3):
                assert got['log_z'][b] == clean['log_z'][b] and np.isnan(got['score'][b]) and np.isnan(got['joint'][b]), b
            else:
                assert all(np.array_equal(got[k][b], clean[k][b]) for k in ('log_z', 'score', 'joint')), b


def test_refusals():
    spec = C.user_spec(10, [1, 4, 7], 256, 64, seed=1)
    fb32 = _batch(spec, [C.make_inputs(spec, 1)])
    fb32.set_pair_tables(fb32.pair_tables, dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        fb32.log_partition([1])
    fb = _batch(K3['spec'](), [C.make_inputs(K3['spec'](), 500)])
    with pytest.raises(ValueError):
        fb.log_partition([1], labels=np.zeros((1, 2), dtype=np.int32))
    with pytest.raises(ValueError):
        fb.log_partition([1], score=torch.zeros(1, dtype=torch.float64, device=fb.device))
    spec = C.user_spec(10, [1, 4, 7], 128, 128, seed=1)
    fba = _batch(spec, [C.make_inputs(spec, s) for s in (500, 501)])
    fba.use_approx_inference = True                   # allowed: the call reads whatever messages the sweeps left
    lz = fba.log_partition([1, 4, 7])
    assert lz.shape == (2,) and bool(torch.isfinite(lz).all())


# ---- capture ----------------------------------------------------------------------------------------------
def test_capture_and_replay():
    """sweep + log_partition recorded in a HIP graph on one stream after an eager call, replayed with the tables overwritten
    in place between the replays: the outputs follow the tables."""
    spec = K3['spec']()
    first = [C.make_inputs(spec, s) for s in range(500, 508)]
    second = [C.make_inputs(spec, s) for s in range(540, 548)]
    fb, other = _batch(spec, first), _batch(spec, second)
    labels = _labels(fb, seed=4)
    lab = torch.from_numpy(labels).to(fb.device)
    score = torch.empty(fb.B, dtype=torch.float64, device=fb.device)
    sums = torch.empty(2, dtype=torch.float64, device=fb.device)
    fb.log_partition(K3['roots'], labels=lab, score=score, sum_out=sums)                   # eager call
    assert _L().last_kernel() == KERNEL_OF[X64]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        log_z, joint = fb.log_partition(K3['roots'], labels=lab, score=score, sum_out=sums)
    for inputs, src in ((first, fb), (second, other), (first, None)):
        if src is other:
            fb.pair_tables.copy_(other.pair_tables)
            fb.unary_tables.copy_(other.unary_tables)
        elif src is None:
            pair, unary = batch_tables(spec, fb.topo, first)
            fb.pair_tables.copy_(torch.from_numpy(pair))
            fb.unary_tables.copy_(torch.from_numpy(unary))
        for t in (log_z, joint, score, sums, fb.msgs):
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        got = dict(log_z=log_z.cpu().numpy(), score=score.cpu().numpy(), joint=joint.cpu().numpy(), sums=sums.cpu().numpy(),
                   msgs=fb.msgs.cpu().numpy())
        _compare('K3 replay', spec, fb.topo, inputs, K3['roots'], labels, got)


# ---- trainers -------------------------------------------------------------------------------------------
def _check_trainer(name, tt, phi, th_ee, th_ed, per_instance, totals):
    """TiDirTrainer.joint_log_likelihood() against the statement on every instance's own graph (three sweeps when it is
    loopy, one when it is a tree, as the trainer runs them), in file order; each bucket's UserGraphTrainer gives the same
    numbers; totals are the sums."""
    from macaronicusermodeling_amd.topology import GraphTopology
    phi_ee, phi_w1, phi_ed = phi
    seen, total, worst, kernels = 0, 0.0, 0.0, set()
    for key, b in sorted(tt.buckets.items()):
        tr = tt.trainers[key]
        joint, log_z = tr.joint_log_likelihood()
        kernels.add(_L().last_kernel())
        assert joint.dtype == log_z.dtype == np.float64 and joint.shape == log_z.shape == (len(b['rows']),)
        for i, row in enumerate(b['rows']):
            g, inputs, roots, _ = tidir_oracle_graph(key, b, i, phi_ee, phi_w1, phi_ed, th_ee, th_ed)
            n = 3 if O.has_loops(g, roots[0]) else 1
            _, msgs = S.sweeps(g.spec, inputs, roots[:n])
            x = {v: int(b['var_labels'][i][k]) for k, v in enumerate(key[1])}
            lz, _, jl = S.joint_logp(g, inputs, msgs, x)
            topo = GraphTopology.from_spec(g.spec)
            bound = kernel_atol(topo, g.X) + 1e-10 * message_factors(topo)
            positions, got_jl, got_lz = per_instance[row['index']]
            assert positions == tuple(key[1]) == tuple(g.var_order)
            worst = max(worst, _close(got_lz, lz, bound, '%s instance %d log_z' % (name, row['index'])),
                        _close(got_jl, jl, bound, '%s instance %d joint' % (name, row['index'])))
            assert got_jl == joint[i] and got_lz == log_z[i]
            total += got_jl
            seen += 1
    print('%s: %d sentences, worst |diff| to the statement %.2e, total joint log-likelihood %.6f, kernels %s'
          % (name, seen, worst, total, sorted(kernels)))
    assert totals[1] == seen
    np.testing.assert_allclose(totals[0], total, rtol=1e-12)
    return seen, kernels


def test_tidir_on_synthetic_sentences(tmp_path):
    from test_gpu_map import _synthetic
    tt, phi = _synthetic(tmp_path)
    rs = np.random.RandomState(1)
    th_ee, th_ed = rs.randn(1, 3) * 0.3, rs.randn(1, 6) * 0.3
    tt.theta_en_en.copy_(torch.from_numpy(th_ee.reshape(-1)))
    tt.theta_en_de.copy_(torch.from_numpy(th_ed.reshape(-1)))
    per_instance, totals = tt.joint_log_likelihood()
    seen, kernels = _check_trainer('synthetic', tt, phi, th_ee, th_ed, per_instance, totals)
    assert seen == len(per_instance) == 60 and kernels == {KERNEL_OF[X64], KERNEL_OF[X64_SHARED]}       # K1 has no pairwise table to share
    # one predicted word: the graph is a tree of one variable, and the joint log-likelihood is predict()'s log-posterior
    singles = 0
    for key, tr in tt.trainers.items():
        if len(key[1]) != 1:
            continue
        lp = tr.predict()[0]
        joint, _ = tr.joint_log_likelihood()
        for b in range(len(lp)):
            if lp[b] > -99.99:
                _close(joint[b], lp[b], kernel_atol(tr.topo, 64) + 1e-10 * message_factors(tr.topo), 'single word %s %d' % (key, b))
                singles += 1
    assert singles >= 5


def test_trainer_at_zero_thetas(tmp_path):
    """Zero thetas: every table is constant 1, so Z = X^n_vars exactly: log_z = n_vars log X and every assignment has
    joint_logp = -n_vars log X, up to the kernel bound."""
    from test_gpu_map import _synthetic
    tt, _ = _synthetic(tmp_path)
    per_instance, totals = tt.joint_log_likelihood()
    total = 0.0
    for key, b in tt.buckets.items():
        n = len(key[1])
        bound = kernel_atol(tt.trainers[key].topo, 64)
        for row in b['rows']:
            positions, jl, lz = per_instance[row['index']]
            _close(lz, n * np.log(64.0), bound, 'log_z %s' % (key,))
            _close(jl, -n * np.log(64.0), bound, 'joint %s' % (key,))
            total += jl
    assert totals[1] == 60
    np.testing.assert_allclose(totals[0], total, rtol=1e-12)
    np.testing.assert_allclose(totals[0], -162 * np.log(64.0), rtol=1e-12)


def test_tidir_on_the_clique_fixture(tmp_path):
    """K1 to K12 at X = 64 at the fixture's own thetas: the shared-table kernel takes every bucket with a pairwise factor,
    whatever its size."""
    from macaronicusermodeling_amd import tidir
    from test_gpu_cliques import _trainer
    gold = tidir_gold('tidir_cliques_reference')
    paths = write_tidir(gold, str(tmp_path))
    tt = _trainer(paths, gold)
    per_instance, totals = tt.joint_log_likelihood()
    phi = tidir.load_features(paths['phi.pmi'], paths['phi.pmi_w1'], paths['phi.ed'], paths['phi.ped'])
    seen, kernels = _check_trainer('clique fixture', tt, phi, np.array(gold['theta_en_en']).reshape(1, -1),
                                   np.array(gold['theta_en_de']).reshape(1, -1), per_instance, totals)
    assert seen == 11 and KERNEL_OF[X64_SHARED] in kernels
