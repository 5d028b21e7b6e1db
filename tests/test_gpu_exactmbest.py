"""Exact M-best decoding by cutset conditioning on the GPU (libmlbp_exactmbest.so) against the NumPy statement of
include/mlbp_exactmbest.h (tests/test_exactmbest_cpu.py), which is pinned on enumeration there.

Bars.  Every input whose rows are compared is listed in test_exactmbest_cpu.INPUTS, where ranks 0 .. M of every graph are
asserted to lie 1e-6 nats apart (no case left out); given that, rows are compared exactly and scores at rtol 1e-12 (the bars
of test_gpu_exactmap).  Every reported score is also recomputed on the host from the tables at the reported row.  Ties are
tested on tables whose entries are powers of two, where every product is exact: rows pairwise distinct, the scores
enumeration's as a multiset.  Bit-for-bit claims hold across batch sizes, chunk counts and M: the header makes a graph's bits a
function of the graph, the cutset and M's prefix alone."""
import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_exactmap_cpu as E
import test_exactmbest_cpu as S
import test_map_cpu as W
from helpers import batch_tables, tidir_gold, write_tidir
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

VALUES_X64, VALUES_GENERIC = ('exactmbest_values_x64_kernel', ()), ('exactmbest_values_generic_kernel', ())
LISTS_X64, LISTS_GENERIC = ('exactmbest_lists_x64_kernel', ()), ('exactmbest_lists_generic_kernel', ())
SELECT, MERGE = ('exactmbest_select_kernel', ()), ('exactmbest_merge_kernel', ())
_X64_TESTS = ['test_x64_families', 'test_branching_forest_x64', 'test_m1_is_exact_map_and_a_list_is_the_prefix_of_a_longer_one', 'test_trees_and_redundant_cutsets',
              'test_batch_position_batch_size_and_shared_tables_give_the_same_bits', 'test_power_of_two_scaling', 'test_wide_range_tables',
              'test_dyadic_ties', 'test_bad_entries_and_a_bad_index', 'test_capture_and_replay_with_changed_tables', 'test_tidir_exact_nbest']
_GENERIC_TESTS = ['test_generic_families', 'test_branching_forests_generic', 'test_k3_x1024_two_rows_everything_in_the_workspace',
                  'test_m1_is_exact_map_and_a_list_is_the_prefix_of_a_longer_one', 'test_trees_and_redundant_cutsets', 'test_n_found',
                  'test_batch_position_batch_size_and_shared_tables_give_the_same_bits', 'test_power_of_two_scaling', 'test_wide_range_tables',
                  'test_dyadic_ties', 'test_bad_entries_and_a_bad_index']
_ALL = sorted(set(_X64_TESTS + _GENERIC_TESTS))
# kernel -> the tests that launch it (tests/test_exactmbest_cpu.py holds this against the library's symbol table)
CASES = {VALUES_X64: _X64_TESTS, VALUES_GENERIC: _GENERIC_TESTS, SELECT: _ALL, LISTS_X64: [t for t in _X64_TESTS if t != 'test_trees_and_redundant_cutsets'],
         LISTS_GENERIC: _GENERIC_TESTS + ['test_x64_families'], MERGE: _ALL}
X64, GENERIC = 1, 2
# the families of test_exactmbest_cpu.INPUTS this module ranks (held against INPUTS there)
INPUTS_USED = ['k3_x64', 'k3_x64_lognormal', 'k4_x64', 'chain3_x64', 'chain4_x64', 'ring3_x2', 'ring3_x5', 'ring3_x65', 'ring3_x257', 'k3_x128',
               'ring5_x7', 'k5_x7', 'forest_x9', 'double_pair_x6', 'chain260_x2', 'k3_x1024', 'k3_x64_wide', 'ring5_x7_wide', 'star4_x9', 'star3_x5',
               'star2_x64', 'k3_x2_zeros']


def _M():
    from macaronicusermodeling_amd import exactmbest
    return exactmbest


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


def _run(fb, m, cutset=None, values=None):
    """exact_mbest -> dict(x [B][m][n_vars], score [B][m], n [B]); values: the values kernel the call must have taken."""
    M = _M()
    out = fb.exact_mbest(m, cutset=cutset)
    ran = M.last_kernel()
    torch.cuda.synchronize()
    assert out[0].dtype == torch.int32 and tuple(out[0].shape) == (fb.B, m, fb.topo.n_vars)
    assert out[1].dtype == torch.float64 and tuple(out[1].shape) == (fb.B, m)
    assert out[2].dtype == torch.int32 and tuple(out[2].shape) == (fb.B,)
    topo = fb.topo
    pl = M.plan(topo, None if cutset is None else [topo.var_index[v] for v in cutset], fb.X, fb.device)
    assert ran == M.pick_kernel(fb.X, topo.n_vars, topo.P, topo.U, pl.n_forest, m)
    if values is not None:                                      # the lists kernel: by the rule of the header
        assert M.kernels(ran) == (values, S.lists_rule(fb.X, topo.n_vars, topo.P, topo.U, pl.n_forest, m)), ran
    return dict(x=out[0].cpu().numpy(), score=out[1].cpu().numpy(), n=out[2].cpu().numpy())


def _compare(name, got, g, inputs, stated, m, index=None):
    """stated: [(rows, scores)] per graph, the statement's (index: the graph of batch position b)."""
    worst = 0.0
    for b in range(got['x'].shape[0]):
        i = b if index is None else index[b]
        rows, scores = stated[i]
        rows, scores = rows[:m], scores[:m]
        n = len(rows)
        assert got['n'][b] == n, (name, b, got['n'][b])
        assert got['x'][b, :n].tolist() == rows, (name, b)
        np.testing.assert_allclose(got['score'][b, :n], scores, rtol=1e-12, err_msg='%s graph %d' % (name, b))
        assert (got['x'][b, n:] == -1).all() and (got['score'][b, n:] == -np.inf).all(), (name, b)
        for r in range(n):                                      # the score is the row's own log-potential
            host = W.score_of(g, inputs[i], dict(zip(g.var_order, (int(v) for v in got['x'][b, r]))))
            np.testing.assert_allclose(got['score'][b, r], host, rtol=1e-12)
            worst = max(worst, abs(got['score'][b, r] - host) / max(abs(host), 1e-300))
        assert (np.diff(got['score'][b, :n]) <= 0).all(), (name, b)
    print('%s: %d lists of %d rows equal, scores within %.1e relative' % (name, got['x'].shape[0], m, worst))


def _case(name, values, pick=None, cutset=None, m=None):
    """Family `name` of test_exactmbest_cpu.INPUTS (pick: which of its graphs), M rows (the family's own unless given)."""
    spec, inputs, M, stated, _ = S.family(name)
    m = M if m is None else m
    pick = [i for i in (range(len(inputs)) if pick is None else pick) if i < len(inputs)]
    g = O.Graph(spec)
    fb = _batch(spec, [inputs[i] for i in pick])
    got = _run(fb, m, cutset=cutset, values=values)
    _compare(name, got, g, [inputs[i] for i in pick], [stated[i] for i in pick], m)
    return fb, got


# ---- against the statement --------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['k3_x64', 'k3_x64_lognormal', 'k4_x64', 'chain3_x64'])
def test_x64_families(name):
    """The X = 64 values kernel: one cutset variable (64 configurations), two (4096, the pairwise constant inside the cutset),
    none (a chain: one configuration, the whole answer from the list form).  K3 and K4 take the X = 64 lists kernel; the
    chain's two forest tables leave no room for four waves' 16-lists, so its lists pass is the generic one -- and the X = 64
    one at M = 3."""
    M = _M()
    _, got = _case(name, X64)
    want = M.KERNEL_GENERIC if name == 'chain3_x64' else M.KERNEL_X64
    assert M.kernels(M.last_kernel())[1] == want
    if name == 'chain3_x64':
        _case(name, X64, m=3)
        assert M.kernels(M.last_kernel()) == (M.KERNEL_X64, M.KERNEL_X64)


@pytest.mark.parametrize('name', ['ring3_x2', 'ring3_x5', 'ring3_x65', 'ring3_x257', 'k3_x128', 'ring5_x7', 'k5_x7', 'forest_x9',
                                  'double_pair_x6', 'chain260_x2', 'chain4_x64'])
def test_generic_families(name):
    """X = 2 (eight assignments: the lists end at n_found = 8), odd sizes, sizes past a wave and past the workgroup's 256
    threads; lists in LDS (X = 65 and below) and in the workspace (X = 257, the chain of 260); a forest of two chains (two roots)
    and an isolated variable; a double factor; three cutset variables (K5).  No variable here has two children: that is
    test_branching_forests_generic and test_branching_forest_x64."""
    spec, _, M, _, _ = S.family(name)
    topo = _batch(spec, S.family(name)[1][:1]).topo
    in_workspace = S.lists_in_workspace(spec['X'], topo.n_vars, topo.P, topo.U, M)
    assert in_workspace == (name in ('ring3_x257', 'k3_x128', 'chain260_x2')), name
    _case(name, GENERIC)


def test_k3_x1024_two_rows_everything_in_the_workspace():
    M = _M()
    assert S.lists_in_workspace(1024, 3, 3, 3, 2)
    want = 1024 * 2 + 3 + 8 + 6 + M.chunks(1, 1024) * 17 * 1024 + 2 * S.lists_bytes(1024, 3, 2) // 8
    assert M.workspace_bytes(1, 1024, 3, 3, 3, 1, 1, 2) == want * 8
    _case('k3_x1024', GENERIC)


# ---- against exact_map, and a list against a longer one ----------------------------------------------------
@pytest.mark.parametrize('name,values', [('k3_x64_lognormal', X64), ('k4_x64', X64), ('ring5_x7', GENERIC)], ids=['k3_x64', 'k4_x64', 'generic'])
def test_m1_is_exact_map_and_a_list_is_the_prefix_of_a_longer_one(name, values):
    spec, inputs, _, _, _ = S.family(name)
    fb = _batch(spec, inputs)
    x, score = fb.exact_map()
    one, four, sixteen = _run(fb, 1, values=values), _run(fb, 4, values=values), _run(fb, 16, values=values)
    assert np.array_equal(one['x'][:, 0], x.cpu().numpy()) and np.array_equal(one['score'][:, 0], score.cpu().numpy())
    for key in ('x', 'score'):
        assert np.array_equal(sixteen[key][:, :4], four[key]) and np.array_equal(four[key][:, :1], one[key]), key
    assert (one['n'] == 1).all() and (four['n'] == 4).all() and (sixteen['n'] == 16).all()


# ---- the cutset is a choice, not a result -----------------------------------------------------------------
def test_trees_and_redundant_cutsets():
    """A tree with the empty cutset is one configuration: the list form alone, held to enumeration.  A redundant cutset
    conditions on what need not be: the same rows."""
    M = _M()
    for name, values in (('chain3_x64', X64), ('forest_x9', GENERIC)):
        spec, inputs, m, stated, enumerated = S.family(name)
        g = O.Graph(spec)
        assert R.chosen_ids(spec) == []
        fb, got = _case(name, values)
        for b, want in enumerate(enumerated):
            assert got['x'][b].tolist() == S.as_rows(g, [x for _, x in want[:m]]), (name, b)
    _case('chain3_x64', X64, cutset=[1])
    _case('forest_x9', GENERIC, cutset=[4, 1])
    fb, _ = _case('k3_x64', X64, pick=(1, 2), cutset=[1])
    _case('k3_x64', X64, pick=(1, 2), cutset=[2, 0])             # 4096 configurations of a single free variable
    with pytest.raises(ValueError):
        fb.exact_mbest(4, cutset=[9])
    with pytest.raises(M.ExactMbestError, match='cycle'):
        fb.exact_mbest(4, cutset=[])


# ---- fewer than M assignments ----------------------------------------------------------------------------
def test_n_found():
    """X = 2 with zeroed entries (family k3_x2_zeros: 8, 4, 2 and 0 assignments of positive potential): rows from n_found on
    read -1 and -inf; an all-zero table leaves n_found = 0 -- not exact_map's all-zero assignment."""
    spec, inputs, _, stated, _ = S.family('k3_x2_zeros')
    g = O.Graph(spec)
    assert [len(rows) for rows, _ in stated] == [8, 4, 2, 0]
    fb = _batch(spec, inputs)
    for m in (1, 3, 16):
        got = _run(fb, m, values=GENERIC)
        _compare('n_found m = %d' % m, got, g, inputs, stated, m)
        assert got['n'].tolist() == [min(m, k) for k in (8, 4, 2, 0)]


# ---- branching: a parent that already holds a folded list takes another child ------------------------------------------
@pytest.mark.parametrize('name', ['star4_x9', 'star3_x5'])
def test_branching_forests_generic(name):
    """A hub with three and four children under the empty cutset: the second child on is folded list against list into a list
    that is itself the result of a fold -- pairs with a > 0 under the (a + 1)(b + 1) <= M bound -- and the decode threads the
    hub's rank through one fold record per child.  M = 16, 5 and 2."""
    assert R.chosen_ids(S.family(name)[0]) == []
    for m in (16, 5, 2):
        _case(name, GENERIC, m=m)
    _case(name, GENERIC, cutset=[1])                            # a leaf conditioned on: the hub keeps its other children


def test_branching_forest_x64():
    """The hub with two children at X = 64 (two forest tables).  Up to M = 5 the X = 64 lists kernel takes it: the hub's list
    comes back out of the wave's LDS for the second fold (lslot >= 0, every rank may hold an entry).  At M = 16 the generic lists
    kernel runs behind the X = 64 values kernel."""
    M = _M()
    for m, lists in ((5, M.KERNEL_X64), (4, M.KERNEL_X64), (2, M.KERNEL_X64), (16, M.KERNEL_GENERIC), (6, M.KERNEL_GENERIC)):
        _case('star2_x64', X64, m=m)
        assert M.kernels(M.last_kernel()) == (M.KERNEL_X64, lists), m


# ---- what the bits depend on ------------------------------------------------------------------------------
@pytest.mark.parametrize('name,values', [('k3_x64', X64), ('ring5_x7', GENERIC)], ids=['x64', 'generic'])
def test_batch_position_batch_size_and_shared_tables_give_the_same_bits(name, values):
    spec, inputs, m, _, _ = S.family(name)
    fb = _batch(spec, inputs)                                    # B = 8
    full = _run(fb, m, values=values)
    pair, unary = batch_tables(spec, fb.topo, inputs)
    P, U = fb.topo.P, fb.topo.U
    ptab = np.arange(8 * P).reshape(8, P)
    utab = np.arange(8 * U).reshape(8, U)
    ptab[0], utab[0] = ptab[2], utab[2]                          # graphs 0 and 2 both read the tables of graph 2
    shared = _run(_batch(spec, inputs, (pair, unary), ptab, utab), m, values=values)
    alone = _run(_batch(spec, inputs[5:6]), m, values=values)    # B = 1: another number of chunks per graph
    back = _run(_batch(spec, inputs[::-1]), m, values=values)    # every graph at another position
    for key in ('x', 'score', 'n'):
        assert np.array_equal(shared[key][0], full[key][2]) and np.array_equal(shared[key][1:], full[key][1:]), key
        assert np.array_equal(alone[key][0], full[key][5]), key
        assert np.array_equal(back[key][::-1], full[key]), key


def test_power_of_two_scaling():
    """Tables times 2^+-400, unary rows times 2^+-500: the same rows; the scores move by k ln 2."""
    for name, values, moves in (('k3_x64_lognormal', X64, [({0: 400}, {}), ({2: -400}, {}), ({}, {0: 500}), ({}, {1: -500}),
                                                           ({0: 37, 1: -5, 2: 400}, {0: -300, 1: 3, 2: 500})]),
                                ('ring5_x7', GENERIC, [({0: 400}, {}), ({4: -400}, {}), ({}, {0: 500}), ({1: -400, 3: 400}, {2: -500})])):
        spec, inputs, m, _, _ = S.family(name)
        inputs = inputs[:2]
        fb = _batch(spec, inputs)
        base = _run(fb, m, values=values)
        pair, unary = batch_tables(spec, fb.topo, inputs)
        P, U = fb.topo.P, fb.topo.U
        for pk, uk in moves:
            p2, u2 = pair.copy(), unary.copy()
            for b in range(2):
                for p, k in pk.items():
                    p2[b * P + p] = np.ldexp(p2[b * P + p], k)
                for u, k in uk.items():
                    u2[b * U + u] = np.ldexp(u2[b * U + u], k)
            got = _run(_batch(spec, inputs, (p2, u2)), m, values=values)
            shift = (sum(pk.values()) + sum(uk.values())) * np.log(2.0)
            assert np.array_equal(got['x'], base['x']) and np.array_equal(got['n'], base['n']), (name, pk, uk)
            assert E.close(got['score'], base['score'] + shift, 1e-12), (name, pk, uk)


def test_wide_range_tables():
    """exp(8 N(0, 1)) at K3, X = 64 and exp(20 N(0, 1)) on the ring: the M-th best within 600 nats of the best (asserted with
    the gaps), so the 2^-1000 rule drops nothing that is ranked."""
    _case('k3_x64_wide', X64)
    _case('ring5_x7_wide', GENERIC)


# ---- ties -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('X,values', [(64, X64), (5, GENERIC)], ids=['x64', 'generic'])
def test_dyadic_ties(X, values):
    """Entries in {1/2, 1, 2}: products are exact and most values tie.  Rows pairwise distinct, each score its row's own, the
    scores enumeration's M best as a multiset; all-ones tables give 16 distinct rows of score 0."""
    spec = R.kn_spec(3, X)
    g = O.Graph(spec)
    inputs = [E.ones_inputs(spec)] + [E.power_of_two_inputs(spec, s, -1, 1) for s in range(3)]
    got = _run(_batch(spec, inputs), 16, values=values)
    assert (got['n'] == 16).all() and (got['score'][0] == 0.0).all()
    for b, i in enumerate(inputs):
        want = [s for s, _ in S.enum_top(g, i, 16)]
        assert len({tuple(r) for r in got['x'][b].tolist()}) == 16, b
        np.testing.assert_allclose(sorted(got['score'][b]), sorted(want), rtol=1e-12, atol=1e-12)
        assert (np.diff(got['score'][b]) <= 1e-12).all()
        for r in range(16):
            host = W.score_of(g, i, dict(zip(g.var_order, (int(v) for v in got['x'][b, r]))))
            np.testing.assert_allclose(got['score'][b, r], host, rtol=1e-12, atol=1e-12)


# ---- edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,values', [('k3_x64', X64), ('ring5_x7', GENERIC)], ids=['x64', 'generic'])
def test_bad_entries_and_a_bad_index(name, values):
    spec, inputs, m, _, _ = S.family(name)
    X, inputs = spec['X'], inputs[:7]
    fb = _batch(spec, inputs)
    base = _run(fb, m, values=values)
    pair, unary = batch_tables(spec, fb.topo, inputs)
    P = fb.topo.P
    p2 = pair.copy()
    p2[0 * P + 1][:] = 0.0                                       # graph 0: an all-zero table
    p2[1 * P + 0][3 % X, 1] = np.nan                             # graph 1: a NaN entry
    p2[2 * P + 2][0, 2 % X] = np.inf                             # graph 2: +inf
    p2[4 * P + 1][1, 0] = -1.0                                   # graph 4: a negative entry
    p2[5 * P + 0][:] = np.nan                                    # graph 5: a table of NaN
    fb2 = _batch(spec, inputs, (p2, unary))
    fb2.pair_tab[3, 1] = fb2.pair_tables.shape[0]                # graph 3: a table index outside the array
    got = _run(fb2, m, values=values)
    x, score, n = got['x'], got['score'], got['n']
    assert n[0] == 0 and (x[0] == -1).all() and (score[0] == -np.inf).all()
    assert n[3] == -1 and (x[3] == -1).all() and np.isnan(score[3]).all()
    for b in (1, 2, 4, 5):
        assert ((x[b] >= -1) & (x[b] < X)).all(), b
    for key in ('x', 'score', 'n'):
        assert np.array_equal(got[key][6], base[key][6]), key


def test_refusals_come_before_any_launch():
    M = _M()
    spec = R.kn_spec(3, 64)
    fb = _batch(spec, [C.make_inputs(spec, 1)])
    _run(fb, 2, values=X64)
    for m in (0, 17):
        with pytest.raises(ValueError):
            fb.exact_mbest(m)
    spec5 = R.kn_spec(5, 64)
    fb5 = _batch(spec5, [C.make_inputs(spec5, 1)])
    with pytest.raises(M.ExactMbestError, match='configurations') as err:
        fb5.exact_mbest(4)
    from macaronicusermodeling_amd import _ffi
    assert err.value.code == _ffi.MLBP_EUNSUPPORTED
    spec32 = C.user_spec(10, [1, 4, 7], 256, 64, seed=1)
    fb32 = _batch(spec32, [C.make_inputs(spec32, 1)])
    fb32.set_pair_tables(fb32.pair_tables, dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        fb32.exact_mbest(4)


def test_capture_and_replay_with_changed_tables():
    """After one eager call the call is captured; a replay gives the bits of the eager call, and after the tables are
    overwritten in place the bits of an eager call on the new tables."""
    spec, inputs, m, _, _ = S.family('k3_x64')
    fb = _batch(spec, inputs[:3])
    first = _run(fb, m, values=X64)
    other = _run(_batch(spec, inputs[3:6]), m, values=X64)
    assert not np.array_equal(first['x'], other['x'])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x, score, n = fb.exact_mbest(m)
    pair, unary = batch_tables(spec, fb.topo, inputs[3:6])
    for want in (first, other):
        x.fill_(-5)
        score.fill_(float('nan'))
        n.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(x.cpu().numpy(), want['x']) and np.array_equal(score.cpu().numpy(), want['score'])
        assert np.array_equal(n.cpu().numpy(), want['n'])
        fb.pair_tables.copy_(torch.from_numpy(pair))
        fb.unary_tables.copy_(torch.from_numpy(unary))


# ---- trainer --------------------------------------------------------------------------------------------
def test_tidir_exact_nbest(tmp_path):
    """TiDirTrainer.exact_nbest(4) on the clique fixture (K1 to K12 at X = 64, its own thetas): K1 to K4 against every
    instance's own graph by the statement (test_exactmbest_cpu.tidir_instances: its ranks 0 .. 4 are asserted GAP apart on the
    CPU, no instance left out), K5 and up listed as skipped; logp against exact_inference's joint_logp of every row; the totals recomputed on the host; rank 0 against
    exact_decode()."""
    from test_gpu_cliques import _trainer
    m = S.TIDIR_M
    instances, _ = S.tidir_instances()
    gold = tidir_gold('tidir_cliques_reference')
    paths = write_tidir(gold, str(tmp_path))
    tt = _trainer(paths, gold)
    per_sentence, totals, skipped = tt.exact_nbest(m)
    _, counts, report, skipped_decode = tt.exact_decode()
    seen, too_large, want_recall, want_covered = 0, {}, np.zeros(m, dtype=np.int64), 0.0
    for key, b in sorted(tt.buckets.items()):
        tr = tt.trainers[key]
        if len(key[1]) >= 5:
            too_large[tuple(key[1])] = len(b['rows'])
            for row in b['rows']:
                assert per_sentence[row['index']] == (tuple(key[1]), None, None, None)
            continue
        x, score, logp, covered, label_rank, bp_rank = tr.exact_nbest(m)
        assert x.dtype == np.int64 and x.shape == (len(b['rows']), m, len(key[1])) and label_rank.dtype == np.int64
        agrees = tr.exact_decode()[3]
        assert np.array_equal(bp_rank == 0, agrees), key
        bp_x = tr.decode()[0]
        have = min(m, 64 ** len(key[1]))
        for r in range(have):                                   # the true log-probability of every row
            joint = tr.batch.exact_inference(labels=torch.from_numpy(x[:, r].astype(np.int32)).to(tr.device))[2].cpu().numpy()
            assert np.abs(logp[:, r] - joint).max() <= 1e-10, (key, r)
        assert (covered <= 1.0 + 1e-10).all() and (covered > 0).all()
        np.testing.assert_allclose(covered, np.exp(logp[:, :have]).sum(axis=1), rtol=1e-12)
        for i, row in enumerate(b['rows']):
            g, rows, scores = instances[(key, i)]
            rows = rows[:m]
            positions, words, sc, lp = per_sentence[row['index']]
            assert positions == tuple(key[1]) == tuple(g.var_order)
            assert x[i, :len(rows)].tolist() == rows, (key, i)
            assert words == [[tt.en[w] for w in r] for r in rows]
            np.testing.assert_allclose(sc, scores[:m], rtol=1e-12)
            np.testing.assert_allclose(lp, logp[i, :len(rows)], rtol=0, atol=0)
            label = [int(v) for v in b['var_labels'][i]]
            assert label_rank[i] == (rows.index(label) if label in rows else -1), (key, i)
            assert bp_rank[i] == (rows.index(bp_x[i].tolist()) if bp_x[i].tolist() in rows else -1), (key, i)
            if label in rows:
                want_recall[rows.index(label):] += 1
            want_covered += float(covered[i])
            seen += 1
    assert seen >= 4 and too_large
    n_compared, covered_sum, recall, n_bp = totals
    assert n_compared == seen == report[0] and len(recall) == m and recall == [int(v) for v in want_recall]
    assert all(a <= b for a, b in zip(recall[:-1], recall[1:])) and recall[-1] <= seen
    assert recall[0] == counts[0]                               # the labelled set is the best set: exact_decode's exact matches
    np.testing.assert_allclose(covered_sum, want_covered, rtol=1e-12)
    assert n_bp >= report[1]                                    # decode()'s set is in the list wherever it is the best set
    assert sorted(s[0] for s in skipped) == sorted(too_large) == sorted(s[0] for s in skipped_decode)
    assert all('configurations' in s[2] for s in skipped) and sum(s[1] for s in skipped) == sum(too_large.values())
    with pytest.raises(ValueError):
        tt.exact_nbest(17)
