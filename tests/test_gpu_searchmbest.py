"""M-best decoding beyond the exact limit on the GPU: the listed mode of libmlbp_exactmbest.so -- FactorGraphBatch.cutset_mbest,
search_mbest and the trainers' search_nbest -- against exact_mbest() where the list is full and against the NumPy statement of
tests/test_searchmbest_cpu.py (listed_mbest) beyond it.

Bars.  Every input whose rows are compared is listed in test_searchmbest_cpu.INPUTS, where ranks 0 .. m among the admitted
assignments of every graph are asserted to lie 1e-6 nats apart by enumeration restricted to the listed states (none is left
out); given that, rows and entries are compared exactly and scores at 1e-12 relative (the score is a sum of logarithms of table
entries at the row).  Ties are tested on power-of-two tables, where every product of the walk is exact.  Bit-for-bit claims hold
across batch sizes, chunk counts and m: the header makes a graph's bits a function of the graph, the cutset, the list and m's
prefix alone.  The exact call (N == 0) is held to the bits recorded through the library as it was before the listed mode
(tests/golden/exactmbest_exact_bits.json, tests/golden/make_exactmbest_bits.py).  No test asserts a statistical accuracy."""
import json
import os

import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_exactmap_cpu as E
import test_searchmbest_cpu as S
import test_map_cpu as W
from helpers import batch_tables, tidir_gold, tidir_oracle_graph, write_tidir
from oracle import lbp_oracle as O
from test_gpu_exactmbest import _batch

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

VALUES_X64, VALUES_GENERIC = ('exactmbest_values_x64_kernel', ()), ('exactmbest_values_generic_kernel', ())
LISTS_X64, LISTS_GENERIC = ('exactmbest_lists_x64_kernel', ()), ('exactmbest_lists_generic_kernel', ())
SELECT, MERGE = ('exactmbest_select_kernel', ()), ('exactmbest_merge_kernel', ())
_X64 = ['test_full_list_equals_the_exact_call', 'test_order_and_duplicates', 'test_beyond_the_exact_limit', 'test_row_0_is_cutset_map',
        'test_prefix', 'test_bits_across_runs', 'test_ties', 'test_bad_inputs', 'test_search_mbest', 'test_tidir_search_nbest',
        'test_capture_and_replay_with_changed_tables']
_GENERIC = [t for t in _X64 if t != 'test_capture_and_replay_with_changed_tables']
# the six kernels -> the tests that launch them in the listed mode
CASES = {VALUES_X64: _X64, VALUES_GENERIC: _GENERIC, SELECT: _X64, MERGE: _X64,
         LISTS_X64: ['test_full_list_equals_the_exact_call', 'test_order_and_duplicates', 'test_beyond_the_exact_limit', 'test_prefix',
                     'test_bits_across_runs', 'test_ties', 'test_bad_inputs', 'test_capture_and_replay_with_changed_tables'],
         LISTS_GENERIC: _GENERIC}
X64, GENERIC = 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'exactmbest_exact_bits.json')
# the families of test_searchmbest_cpu.INPUTS this module ranks (held against INPUTS there)
INPUTS_USED = ['k3_x64_full', 'k4_x4_full', 'k3_x64_shuffled', 'k4_x4_shuffled', 'k5_x64_n1', 'k5_x64_n7', 'k5_x64_n64', 'k5_x64_n7_m4',
               'k9_x64', 'k10_x64', 'k5_x7', 'k5_x7_m4', 'k3_x257', 'chain3_x64']
KEYS = ('x', 'score', 'n', 'entries')


def _M():
    from macaronicusermodeling_amd import exactmbest
    return exactmbest


def _configs(fb, lists):
    return torch.from_numpy(np.ascontiguousarray(np.stack(lists), dtype=np.int32)).to(fb.device)


def _run(fb, lists, m, kernels=None, cutset=None):
    """cutset_mbest over per-graph lists -> dict(x [B][m][n_vars], score [B][m], n [B], entries [B][m]); kernels: the (values,
    lists) kernels the call must have taken."""
    M = _M()
    x, score, n, entries = fb.cutset_mbest(_configs(fb, lists), m, cutset=cutset, entries=True)
    ran = M.last_kernel()
    torch.cuda.synchronize()
    assert x.dtype == torch.int32 and tuple(x.shape) == (fb.B, m, fb.topo.n_vars)
    assert score.dtype == torch.float64 and tuple(score.shape) == (fb.B, m) and n.dtype == torch.int32 and tuple(n.shape) == (fb.B,)
    assert entries.dtype == torch.int32 and tuple(entries.shape) == (fb.B, m)
    if kernels is not None:
        assert M.kernels(ran) == kernels, (ran, kernels)
    return dict(x=x.cpu().numpy(), score=score.cpu().numpy(), n=n.cpu().numpy(), entries=entries.cpu().numpy())


def _same_bits(a, b, rows=None):
    for key in KEYS:
        u, v = (a[key], b[key]) if rows is None else (a[key][rows[0]], b[key][rows[1]])
        assert np.array_equal(u, v, equal_nan=(key == 'score')), key


def _compare(name, got, refs, m, index=None):
    worst = 0.0
    for b in range(got['x'].shape[0]):
        r = refs[b if index is None else index[b]]
        n = min(m, r['n_found'])
        assert got['n'][b] == n, (name, b, got['n'][b])
        assert got['x'][b, :n].tolist() == r['rows'][:n], (name, b)
        assert got['entries'][b, :n].tolist() == r['entries'][:n], (name, b)
        np.testing.assert_allclose(got['score'][b, :n], r['scores'][:n], rtol=1e-12, err_msg='%s graph %d' % (name, b))
        assert (got['x'][b, n:] == -1).all() and (got['score'][b, n:] == -np.inf).all() and (got['entries'][b, n:] == -1).all(), (name, b)
        worst = max([worst] + [abs(u - v) / max(1.0, abs(v)) for u, v in zip(got['score'][b, :n], r['scores'][:n])])
    print('%s: %d lists of %d rows and entries equal, scores within %.1e relative' % (name, got['x'].shape[0], m, worst))


def _case(name, kernels, m=None):
    spec, inputs, cut, lists, fm, refs = S.family(name)
    m = fm if m is None else m
    fb = _batch(spec, inputs)
    got = _run(fb, lists, m, kernels=kernels)
    _compare(name, got, refs, m)
    return fb, got


# ---- 1, 2: the full list is the exact call; its order and duplicates do not matter ---------------------------------
@pytest.mark.parametrize('m', [1, 4, 16])
@pytest.mark.parametrize('name,kernels', [('k3_x64', (X64, X64)), ('k4_x4', (GENERIC, GENERIC))], ids=['x64', 'generic'])
def test_full_list_equals_the_exact_call(name, kernels, m):
    """Every configuration in index order: exact_mbest()'s bits in rows, scores and n_found, and the configuration numbers as
    entries."""
    fb, got = _case(name + '_full', kernels, m=m)
    x, score, n = fb.exact_mbest(m)
    torch.cuda.synchronize()
    assert np.array_equal(got['x'], x.cpu().numpy()) and np.array_equal(got['score'], score.cpu().numpy()) and np.array_equal(got['n'], n.cpu().numpy())
    X, cut_pos = fb.X, [fb.topo.var_index[v] for v in S.family(name + '_full')[2]]
    assert np.array_equal(got['entries'], sum(got['x'][:, :, v].astype(np.int64) * X ** q for q, v in enumerate(cut_pos)))


@pytest.mark.parametrize('name,kernels', [('k3_x64', (X64, X64)), ('k4_x4', (GENERIC, GENERIC))], ids=['x64', 'generic'])
def test_order_and_duplicates(name, kernels):
    """The full list permuted, with repeats behind: the same rows, the scores within 1e-12, every entry the lowest index of its
    row's state, and the bits of the call on the list with the later repeats removed."""
    _, full = _case(name + '_full', kernels)
    fb, got = _case(name + '_shuffled', kernels)
    lists = S.family(name + '_shuffled')[3]
    assert np.array_equal(got['x'], full['x']) and np.array_equal(got['n'], full['n'])
    np.testing.assert_allclose(got['score'], full['score'], rtol=1e-12)
    clean = []
    for b, c in enumerate(lists):
        rows = [tuple(r) for r in c.tolist()]
        for e in got['entries'][b]:
            assert e == rows.index(rows[e]), (b, e)
        clean.append(np.array([r for k, r in enumerate(c.tolist()) if rows.index(tuple(r)) == k], dtype=np.int32))
    assert len({len(c) for c in clean}) == 1 and len(clean[0]) < len(lists[0])
    _same_bits(_run(fb, clean, 16, kernels=kernels), got)


# ---- 3: beyond the exact limit -------------------------------------------------------------------------------
BEYOND = [('k5_x64_n1', (X64, GENERIC)), ('k5_x64_n7', (X64, GENERIC)), ('k5_x64_n64', (X64, GENERIC)), ('k5_x64_n7_m4', (X64, X64)),
          ('k9_x64', (X64, GENERIC)), ('k10_x64', (GENERIC, GENERIC)), ('k5_x7', (GENERIC, GENERIC)), ('k5_x7_m4', (GENERIC, GENERIC)),
          ('k3_x257', (GENERIC, GENERIC)), ('chain3_x64', (X64, GENERIC))]


@pytest.mark.parametrize('name,kernels', BEYOND, ids=[n for n, _ in BEYOND])
def test_beyond_the_exact_limit(name, kernels):
    """N = 1, 7 (ragged against four waves) and 64 at K5; K9 and K10 on both sides of the X = 64 LDS rule; odd X; X past a
    workgroup's threads; a chain of three (nothing to cut: the one empty configuration, listed twice); m = 4 and 16."""
    M = _M()
    fb, _ = _case(name, kernels)
    if fb.X == 64 and fb.topo.n_vars >= 5:
        with pytest.raises(M.ExactMbestError, match='configurations'):
            fb.exact_mbest(4)


# ---- 4: row 0 is cutset_map ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernels', [('k5_x64_n7', (X64, GENERIC)), ('k5_x64_n7_m4', (X64, X64)), ('k5_x7', (GENERIC, GENERIC))],
                         ids=['x64_generic', 'x64', 'generic'])
def test_row_0_is_cutset_map(name, kernels):
    spec, inputs, cut, lists, m, _ = S.family(name)
    fb = _batch(spec, inputs)
    got = _run(fb, lists, m, kernels=kernels)
    x, score, entry = fb.cutset_map(_configs(fb, lists), entry=True)
    torch.cuda.synchronize()
    assert np.array_equal(got['x'][:, 0], x.cpu().numpy()) and np.array_equal(got['score'][:, 0], score.cpu().numpy())
    assert np.array_equal(got['entries'][:, 0], entry.cpu().numpy())


# ---- 5: prefix -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernels', [('k5_x64_n64', (X64, GENERIC)), ('k5_x7', (GENERIC, GENERIC))], ids=['x64', 'generic'])
def test_prefix(name, kernels):
    """Rows 0 .. m' - 1 of the call with m = 16 are the call with m' = 1, 5 (at K5, X = 64 the shorter calls take the X = 64
    lists kernel, the longest the generic one)."""
    spec, inputs, cut, lists, m, _ = S.family(name)
    assert m == 16
    fb = _batch(spec, inputs)
    long = _run(fb, lists, 16, kernels=kernels)
    for short in (1, 5):
        got = _run(fb, lists, short, kernels=(kernels[0], X64 if kernels[0] == X64 else GENERIC))
        assert np.array_equal(got['x'], long['x'][:, :short]) and np.array_equal(got['score'], long['score'][:, :short])
        assert np.array_equal(got['entries'], long['entries'][:, :short]) and np.array_equal(got['n'], np.minimum(long['n'], short))


# ---- 6: the bits are a function of the graph, the cutset, the list and m's prefix --------------------------------------
@pytest.mark.parametrize('name,kernels', [('k5_x64_n7_m4', (X64, X64)), ('k5_x7_m4', (GENERIC, GENERIC))], ids=['x64', 'generic'])
def test_bits_across_runs(name, kernels):
    """B = 1 and B = 600 (other chunk counts), another position, shared tables: the same bits.  Tables times 2^k: the same
    rows and entries, the scores moved by k ln 2."""
    M = _M()
    spec, inputs, cut, lists, m, refs = S.family(name)
    N = len(lists[0])
    assert M.chunks(1, N) == N and M.chunks(600, N) == 1 and M.chunks(3, N) == N
    base = _run(_batch(spec, inputs), lists, m, kernels=kernels)
    topo = _batch(spec, inputs[:1]).topo
    pair, unary = batch_tables(spec, topo, inputs)
    index = np.arange(600) % len(inputs)
    ptab = np.arange(len(inputs) * topo.P).reshape(-1, topo.P)[index]
    utab = np.arange(len(inputs) * topo.U).reshape(-1, topo.U)[index]
    big = _run(_batch(spec, inputs, (pair, unary), ptab, utab, B=600), [lists[i] for i in index], m, kernels=kernels)
    _compare(name + ' B = 600', big, refs, m, index=index)
    alone = _run(_batch(spec, inputs[1:2]), lists[1:2], m, kernels=kernels)
    ptab3, utab3 = ptab[:3].copy(), utab[:3].copy()
    ptab3[0], utab3[0] = ptab3[2], utab3[2]                      # graphs 0 and 2 both read the tables of graph 2
    shared = _run(_batch(spec, inputs, (pair, unary), ptab3, utab3), [lists[2], lists[1], lists[2]], m, kernels=kernels)
    for lo in (0, 3, 597):
        _same_bits(big, base, rows=(slice(lo, lo + 3), slice(0, 3)))
    _same_bits(alone, base, rows=(0, 1))
    _same_bits(shared, base, rows=(0, 2))
    _same_bits(shared, base, rows=(slice(1, 3), slice(1, 3)))
    P, U = topo.P, topo.U
    for pk, uk in (({0: 400}, {}), ({P - 1: -400}, {}), ({}, {0: 400}), ({1: 400, 4: -400, 7: 37}, {2: -400, 3: 5})):
        p2, u2 = pair.copy(), unary.copy()
        for b in range(len(inputs)):
            for p, k in pk.items():
                p2[b * P + p] = np.ldexp(p2[b * P + p], k)
            for u, k in uk.items():
                u2[b * U + u] = np.ldexp(u2[b * U + u], k)
        got = _run(_batch(spec, inputs, (p2, u2)), lists, m, kernels=kernels)
        shift = (sum(pk.values()) + sum(uk.values())) * np.log(2.0)
        assert np.array_equal(got['x'], base['x']) and np.array_equal(got['entries'], base['entries']) and np.array_equal(got['n'], base['n'])
        assert E.close(got['score'], base['score'] + shift, 1e-12), (name, pk, uk)


# ---- 7: ties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('X,kernels', [(64, (X64, X64)), (5, (GENERIC, GENERIC))], ids=['x64', 'generic'])
def test_ties(X, kernels):
    """Powers of two: every product is exact, so ties are ties.  The rows are pairwise distinct and their scores the restricted
    enumeration's m best as a multiset; among rows of equal score the lower entry index comes first, and within one entry
    the rows keep the order of the call on that entry alone -- the lower rank inside the entry."""
    m = 16
    spec = R.kn_spec(3, X)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    assert cut == [0]
    inputs = [E.ones_inputs(spec), E.ones_inputs(spec)] + [E.power_of_two_inputs(spec, s, -1, 1) for s in range(4)]
    rs = np.random.RandomState(X)
    lists = [np.array([[3], [1], [3], [4], [0], [1], [2]], dtype=np.int32), np.array([[X - 1]] * 7, dtype=np.int32)]
    lists += [rs.randint(0, X, size=(7, 1)).astype(np.int32) for _ in range(4)]
    fb = _batch(spec, inputs)
    got = _run(fb, lists, m, kernels=kernels)
    assert (got['n'] == m).all() and (got['score'][:2] == 0.0).all()
    assert (got['entries'][0] == 0).all() and (got['x'][0][:, 0] == 3).all()      # all ones: the first entry's own sixteen
    assert (got['entries'][1] == 0).all() and (got['x'][1][:, 0] == X - 1).all()
    tied = 0
    for b, (i, c) in enumerate(zip(inputs, lists)):
        want = S.restricted_top(g, i, cut, c, m)
        assert len({tuple(r) for r in got['x'][b].tolist()}) == m, b
        np.testing.assert_allclose(sorted(got['score'][b]), sorted(s for s, _, _ in want), rtol=1e-12, atol=1e-12)
        assert (np.diff(got['score'][b]) <= 1e-12).all()
        for r in range(m):
            host = W.score_of(g, i, dict(zip(g.var_order, (int(v) for v in got['x'][b, r]))))
            np.testing.assert_allclose(got['score'][b, r], host, rtol=1e-12, atol=1e-12)
            assert int(c[got['entries'][b, r]][0]) == got['x'][b, r, 0] and got['entries'][b, r] == c[:, 0].tolist().index(got['x'][b, r, 0])
        for r in range(m - 1):
            if abs(got['score'][b, r] - got['score'][b, r + 1]) <= 1e-12:
                tied += 1
                assert got['entries'][b, r] <= got['entries'][b, r + 1], (b, r)
    assert tied >= 8
    for b in (2, 3):                                            # within an entry: the order of the call on that entry alone
        for e in sorted(set(got['entries'][b].tolist())):
            alone = _run(_batch(spec, inputs[b:b + 1]), [lists[b][e:e + 1]], m, kernels=kernels)
            mine = [r for r in got['x'][b].tolist() if r[0] == int(lists[b][e][0])]
            assert alone['x'][0, :len(mine)].tolist() == mine, (b, e)


# ---- 8: bad inputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernels', [('k5_x64_n7_m4', (X64, X64)), ('k5_x7_m4', (GENERIC, GENERIC))], ids=['x64', 'generic'])
def test_bad_inputs(name, kernels):
    """A state of X or -1 in a graph's list refuses that graph alone, and so does a table index outside its array; the
    neighbours keep their bits."""
    spec, inputs, cut, lists, m, _ = S.family(name)
    X = spec['X']
    five = [inputs[i % 3] for i in range(5)]
    good = [lists[i % 3] for i in range(5)]
    base = _run(_batch(spec, five), good, m, kernels=kernels)
    bad = [c.copy() for c in good]
    bad[1][5, 2] = X                                             # graph 1: a state of X in entry 5 ...
    bad[1][2, 0] = -1                                            # ... and -1 in entry 2
    bad[3][0, 0] = -1                                            # graph 3: -1 in entry 0
    bad[4][6, 1] = X + 1000000                                   # graph 4: far outside, in the last entry
    got = _run(_batch(spec, five), bad, m, kernels=kernels)
    for b in (1, 3, 4):
        assert got['n'][b] == -1 and (got['x'][b] == -1).all() and np.isnan(got['score'][b]).all() and (got['entries'][b] == -1).all(), b
    for b in (0, 2):
        _same_bits(got, base, rows=(b, b))
    fb2 = _batch(spec, five)
    fb2.pair_tab[3, 1] = fb2.pair_tables.shape[0]                # graph 3: a table index outside the array
    got = _run(fb2, good, m, kernels=kernels)
    assert got['n'][3] == -1 and (got['x'][3] == -1).all() and np.isnan(got['score'][3]).all() and (got['entries'][3] == -1).all()
    for b in (0, 1, 2, 4):
        _same_bits(got, base, rows=(b, b))
    fb = _batch(spec, five)
    with pytest.raises(ValueError):
        fb.cutset_mbest(_configs(fb, good)[:, :, :2].contiguous(), m)
    with pytest.raises(ValueError):
        fb.cutset_mbest(_configs(fb, good).long(), m)
    for wrong in (0, 17):
        with pytest.raises(ValueError):
            fb.cutset_mbest(_configs(fb, good), wrong)


# ---- 9: the exact call is what it was ------------------------------------------------------------------------------
def golden_batches():
    """The K3, X = 64 and K4, X = 4 batches of the two full-list families."""
    return {name: _batch(S.family(name + '_full')[0], S.family(name + '_full')[1]) for name in ('k3_x64', 'k4_x4')}


def golden_record(fb, m=16):
    """Every output of exact_mbest(m) on `fb`: the rows and n_found as integers, the scores as hex floats."""
    x, score, n = fb.exact_mbest(m)
    torch.cuda.synchronize()
    return dict(assignments=x.cpu().numpy().reshape(-1).tolist(), n_found=n.cpu().numpy().tolist(),
                scores=[float(v).hex() for v in score.cpu().numpy().reshape(-1)])


@pytest.mark.parametrize('name', ['k3_x64', 'k4_x4'])
def test_the_exact_call_computes_the_bits_it_computed_before(name):
    """N == 0: exact_mbest(16) on the K3 and K4 inputs equals, in every bit, what the library returned before it had a listed
    mode."""
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    assert golden_record(golden_batches()[name]) == want


# ---- 10: search_mbest ------------------------------------------------------------------------------------------------
def _slack(score):
    return 1e-9 * np.maximum(1.0, np.abs(score))


@pytest.mark.parametrize('n,X,B', [(3, 64, 6), (4, 64, 3), (5, 64, 4), (3, 4, 6)], ids=['k3', 'k4', 'k5', 'k3_x4'])
def test_search_mbest(n, X, B):
    """scores[:, 0] >= map_sweep's score on every graph; at K3 / K4 no row scores above exact_mbest()'s row of the same rank,
    and a graph whose list holds every cutset state gets exact_mbest()'s rows; every score is its row's own."""
    m = 4
    spec = R.kn_spec(n, X)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    inputs = [C.make_inputs(spec, 40 + s, 'lognormal' if s % 2 else 'uniform') for s in range(B)]
    fb = _batch(spec, inputs)
    fb.initialize()
    roots = list(g.var_order)
    s_bp = fb.map_sweep(roots, init=True)[1].cpu().numpy()
    N = 64 if X == 4 else 16
    x, score, found, score_bp = (t.cpu().numpy() for t in fb.search_mbest(roots, m, n_samples=N, seed=5))
    assert np.array_equal(score_bp, s_bp) and (found == m).all()
    assert (score[:, 0] >= score_bp - _slack(score[:, 0])).all(), score[:, 0] - score_bp
    assert (np.diff(score, axis=1) <= _slack(score[:, 1:])).all()
    for b in range(B):
        assert len({tuple(r) for r in x[b].tolist()}) == m
        for r in range(m):
            np.testing.assert_allclose(score[b, r], W.score_of(g, inputs[b], dict(zip(g.var_order, (int(v) for v in x[b, r])))), rtol=1e-12)
    if n <= 4:
        ex, es, _ = (t.cpu().numpy() for t in fb.exact_mbest(m))
        assert (score <= es + _slack(es)).all()
        configs = fb._search_list(roots, N, 5, None, None)[0].cpu().numpy()
        full = [b for b in range(B) if len({tuple(r) for r in configs[b].tolist()}) == X ** len(cut)]
        for b in full:
            assert np.array_equal(x[b], ex[b]) and np.array_equal(score[b], es[b]), b
        assert full or X == 64
        print('K%d X = %d: %d of %d lists hold every cutset state' % (n, X, len(full), B))
    else:
        with pytest.raises(_M().ExactMbestError, match='configurations'):
            fb.exact_mbest(m)
    with pytest.raises(ValueError):
        fb.search_mbest(roots, m, n_samples=0)


# ---- 11: trainer -----------------------------------------------------------------------------------------------------
def test_tidir_search_nbest(tmp_path):
    """TiDirTrainer.search_nbest(4) on the clique fixture (K1 to K12 at X = 64, its own thetas): every instance with 2 to 6
    predicted words against the statement on the list its shape's trainer walked -- K5 and K6 among them, nothing skipped --,
    the totals recomputed on the host; exact_nbest() skips what it skipped."""
    from macaronicusermodeling_amd import cutset
    from test_gpu_cliques import _trainer
    from macaronicusermodeling_amd import tidir
    gold = tidir_gold('tidir_cliques_reference')
    paths = write_tidir(gold, str(tmp_path))
    tt = _trainer(paths, gold)
    phi_ee, phi_w1, phi_ed = tidir.load_features(paths['phi.pmi'], paths['phi.pmi_w1'], paths['phi.ed'], paths['phi.ped'])
    th_ee, th_ed = np.array(gold['theta_en_en']).reshape(1, -1), np.array(gold['theta_en_de']).reshape(1, -1)
    m, N, seed = 4, 8, 3
    per_sentence, totals = tt.search_nbest(m, n_samples=N, seed=seed)
    sizes, seen, n_bp, want_recall = set(), 0, 0, np.zeros(m, dtype=np.int64)
    for k, (key, tr) in enumerate(tt.trainers.items()):
        b = tt.buckets[key]
        x, score, found, label_rank, bp_rank, configs = tr.search_nbest(m, n_samples=N, seed=seed + k, with_list=True)
        assert x.dtype == np.int64 and x.shape == (len(b['rows']), m, len(key[1])) and label_rank.dtype == np.int64
        cut = [tr.topo.var_ids[q] for q in cutset.choose(tr.topo)]
        bp_x = tr.decode()[0]
        for i, row in enumerate(b['rows']):
            positions, words, sc = per_sentence[row['index']]
            have = int(found[i])
            assert positions == tuple(key[1]) and len(words) == len(sc) == have
            rows = x[i, :have].tolist()
            assert words == [[tt.en[w] for w in r] for r in rows]
            label = [int(v) for v in b['var_labels'][i]]
            assert label_rank[i] == (rows.index(label) if label in rows else -1), (key, i)
            assert bp_rank[i] == (rows.index(bp_x[i].tolist()) if bp_x[i].tolist() in rows else -1), (key, i)
            if label in rows:
                want_recall[rows.index(label):] += 1
            n_bp += bp_rank[i] >= 0
            seen += 1
            if 2 <= len(key[1]) <= 6:
                g, inputs, _, _ = tidir_oracle_graph(key, b, i, phi_ee, phi_w1, phi_ed, th_ee, th_ed)
                assert tuple(g.var_order) == tuple(key[1])
                truth = S.restricted_top(g, inputs, cut, configs[i], m + 1)
                assert min(S.MB.gaps_of([s for s, _, _ in truth])) >= S.GAP, (key, i)      # no instance is left out
                want = S.listed_mbest(g, inputs, cut, configs[i], m)
                assert rows == want['rows'] == [r for _, _, r in truth[:m]], (key, i)
                np.testing.assert_allclose(sc, want['scores'], rtol=1e-12)
                sizes.add(len(key[1]))
    assert 5 in sizes and min(sizes) <= 4 and len(sizes) >= 3       # K5 and up are ranked, beside the shapes exact_nbest takes
    assert totals == (seen, [int(v) for v in want_recall], int(n_bp))
    skipped = tt.exact_nbest(m)[2]
    assert skipped and all('configurations' in s[2] for s in skipped)      # (what exact_nbest() skips it still skips)
    with pytest.raises(ValueError):
        tt.search_nbest(17)


# ---- 12: capture and replay ------------------------------------------------------------------------------------------
def test_capture_and_replay_with_changed_tables():
    """After one eager call cutset_mbest is captured; a replay gives the bits of the eager call, and after the tables are
    overwritten in place the bits of an eager call on the new tables."""
    spec, inputs, cut, lists, m, _ = S.family('k5_x64_n7_m4')
    more = [C.make_inputs(spec, 70 + s) for s in range(3)]
    fb = _batch(spec, inputs)
    first = _run(fb, lists, m, kernels=(X64, X64))
    other = _run(_batch(spec, more), lists, m, kernels=(X64, X64))
    assert not np.array_equal(first['score'], other['score'])
    configs = _configs(fb, lists)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x, score, n, entries = fb.cutset_mbest(configs, m, entries=True)
    pair, unary = batch_tables(spec, fb.topo, more)
    for want in (first, other):
        x.fill_(-5)
        score.fill_(float('nan'))
        n.fill_(-5)
        entries.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        _same_bits(dict(x=x.cpu().numpy(), score=score.cpu().numpy(), n=n.cpu().numpy(), entries=entries.cpu().numpy()), want)
        fb.pair_tables.copy_(torch.from_numpy(pair))
        fb.unary_tables.copy_(torch.from_numpy(unary))
