"""Exact MAP decoding and max-marginals by cutset conditioning on the GPU (libmlbp_exactmap.so) against the float64 references
of tests/test_exactmap_cpu.py: enumeration in the log domain (one slice of the first variable at a time where X^n is large),
the max form of the forward algorithm for the long chain, and the NumPy statement of the header for the tie rule.

Bars.  Every input whose assignment is compared is listed in test_exactmap_cpu.INPUTS, where its best score is asserted to lead
the second best by 1e-6 nats (no case left out); given that, assignments are compared exactly, scores at rtol 1e-12 (the bar of
test_map_cpu) and max-marginals at 1e-10 relative to max(1, |value|).  The tie rule is tested on tables whose entries are
powers of two, where every product is exact.  Bit-for-bit claims hold across batch sizes and chunk counts: the header makes a
graph's bits a function of the graph and the cutset alone."""
import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_exactmap_cpu as E
import test_map_cpu as W
from helpers import batch_tables, tidir_gold, tidir_oracle_graph, write_tidir
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

X64, X64_MM = ('exactmap_x64_kernel', (False,)), ('exactmap_x64_kernel', (True,))
GENERIC, GENERIC_MM = ('exactmap_generic_kernel', (False,)), ('exactmap_generic_kernel', (True,))
FINAL = ('exactmap_final_kernel', ())
# kernel instance -> the tests that launch it (tests/test_exactmap_cpu.py holds this against the library's symbol table); every
# _case runs the call with and without max-marginals
_X64_TESTS = ['test_k3_x64_against_enumeration', 'test_k4_x64_against_elimination', 'test_both_sides_of_the_x64_lds_budget',
              'test_trees_equal_map_sweep', 'test_cutset_override_and_redundant_cutset',
              'test_shared_tables_and_batch_position_give_the_same_bits', 'test_power_of_two_scaling', 'test_wide_range_tables',
              'test_tie_rule', 'test_zero_nan_inf_tables_and_bad_index', 'test_capture_and_replay_with_changed_tables',
              'test_tidir_exact_decode']
_GENERIC_TESTS = ['test_small_loopy_graphs', 'test_generic_sizes_on_ring3', 'test_k3_x1024_vectors_in_the_workspace', 'test_chain260_x2',
                  'test_both_sides_of_the_x64_lds_budget', 'test_trees_equal_map_sweep', 'test_cutset_override_and_redundant_cutset',
                  'test_shared_tables_and_batch_position_give_the_same_bits', 'test_power_of_two_scaling', 'test_tie_rule',
                  'test_zero_nan_inf_tables_and_bad_index']
CASES = {X64: _X64_TESTS, X64_MM: _X64_TESTS, GENERIC: _GENERIC_TESTS, GENERIC_MM: _GENERIC_TESTS,
         FINAL: ['test_k3_x64_against_enumeration', 'test_small_loopy_graphs']}
KERNEL_OF = {X64: 1, GENERIC: 2}


def _M():
    from macaronicusermodeling_amd import exactmap
    return exactmap


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


def _run(fb, mm=False, cutset=None, kernel=None):
    """exact_map with (mm: True or a tensor) or without max-marginals -> dict(x, score[, mm])."""
    out = fb.exact_map(max_marginals=mm if mm is not False else None, cutset=cutset)
    ran = _M().last_kernel()
    torch.cuda.synchronize()
    assert len(out) == (3 if mm is not False else 2)
    assert out[0].dtype == torch.int32 and tuple(out[0].shape) == (fb.B, fb.topo.n_vars)
    assert out[1].dtype == torch.float64 and tuple(out[1].shape) == (fb.B,)
    if kernel is not None:
        assert ran == KERNEL_OF[kernel], ran
    got = dict(x=out[0].cpu().numpy(), score=out[1].cpu().numpy(), kernel=ran)
    if mm is not False:
        got['mm'] = out[2].cpu().numpy()
    return got


def _both(fb, cutset=None, kernel=None):
    """The call without and with max-marginals: the assignment and the score have the same bits."""
    plain, full = _run(fb, cutset=cutset, kernel=kernel), _run(fb, mm=True, cutset=cutset, kernel=kernel)
    assert np.array_equal(plain['x'], full['x']) and np.array_equal(plain['score'], full['score'])
    return full


def _compare(name, got, g, refs, index=None):
    """refs: [(x, best, max-marginals)] per graph (index: the reference of batch position b)."""
    worst_s = worst_m = 0.0
    for b in range(got['x'].shape[0]):
        x, best, mm = refs[b if index is None else index[b]]
        assert [int(v) for v in got['x'][b]] == [x[v] for v in g.var_order], (name, b)
        np.testing.assert_allclose(got['score'][b], best, rtol=1e-12, err_msg='%s graph %d' % (name, b))
        worst_s = max(worst_s, abs(got['score'][b] - best) / abs(best))
        assert E.close(got['mm'][b], mm, 1e-10), (name, b, np.nanmax(np.abs(got['mm'][b] - mm)))
        assert E.close(got['mm'][b].max(axis=1), np.full(len(x), got['score'][b]), 1e-12), (name, b)
        finite = np.isfinite(mm)
        worst_m = max(worst_m, float((np.abs(got['mm'][b] - mm)[finite] / np.maximum(1.0, np.abs(mm[finite]))).max()))
    print('%s: %d assignments equal, score within %.1e relative, max-marginals within %.1e' % (name, got['x'].shape[0], worst_s, worst_m))


def _case(name, kernel, pick=None, cutset=None):
    """Family `name` of test_exactmap_cpu.INPUTS (pick: which of its graphs) on `kernel`, with and without max-marginals."""
    spec, inputs, refs = E.family(name)
    pick = [i for i in (range(len(inputs)) if pick is None else pick) if i < len(inputs)]
    g = O.Graph(spec)
    fb = _batch(spec, [inputs[i] for i in pick])
    got = _both(fb, cutset=cutset, kernel=kernel)
    _compare(name, got, g, [refs[i] for i in pick])
    return fb, got


# ---- against enumeration --------------------------------------------------------------------------------
def test_k3_x64_against_enumeration():
    """The X = 64 kernel with one cutset variable.  B = 3: the 64 configurations spread over 64 chunks, a wave walks at most one;
    B = 600: one chunk, every wave walks 16.  The same graphs at both batch sizes give the same bits."""
    M = _M()
    assert (M.chunks(3, 64), M.chunks(600, 64)) == (64, 1)
    spec, inputs, refs = E.family('user_k3')
    g = O.Graph(spec)
    _, small = _case('user_k3', X64, pick=range(3))
    topo = _batch(spec, inputs[:1]).topo
    pair, unary = batch_tables(spec, topo, inputs)
    index = np.arange(600) % len(inputs)
    ptab = np.arange(len(inputs) * topo.P).reshape(-1, topo.P)[index]
    utab = np.arange(len(inputs) * topo.U).reshape(-1, topo.U)[index]
    big = _both(_batch(spec, inputs, (pair, unary), ptab, utab, B=600), kernel=X64)
    _compare('user_k3 B = 600', big, g, refs, index=index)
    for key in ('x', 'score', 'mm'):
        assert np.array_equal(big[key][:3], small[key]), key
        assert np.array_equal(big[key][64:128], big[key][:64]), key
    _case('k3_x64', X64, pick=range(3))


def test_k4_x64_against_elimination():
    """4096 configurations of two cutset variables: 256 chunks per graph, the pairwise constant inside the cutset."""
    assert _M().chunks(2, 4096) == 256
    _case('k4_x64', X64)


SMALL = ['ring5_x8', 'ring5_x7', 'k4_x8', 'k4_x16', 'k5_x4', 'shuffled_x5', 'double_pair_x6', 'forest_x9']


@pytest.mark.parametrize('name', SMALL)
def test_small_loopy_graphs(name):
    _case(name, GENERIC, pick=range(8))


@pytest.mark.parametrize('X', [2, 257, 301])
def test_generic_sizes_on_ring3(X):
    """X = 2 and the odd sizes past a workgroup's 256 threads (masked tails), vectors in LDS."""
    _case('ring3_x%d' % X, GENERIC)


def test_k3_x1024_vectors_in_the_workspace():
    M = _M()
    assert M.workspace_bytes(1, 1024, 3, 3, 3, 1, 1, True) == (512 * (4 + 3 * 1024 + 17 * 1024) + 7 * 1024) * 8
    _case('k3_x1024', GENERIC)


def test_chain260_x2():
    """259 forest edges at X = 2 against the max form of the forward algorithm; the empty cutset, one configuration."""
    _case('chain260_x2', GENERIC)


def test_both_sides_of_the_x64_lds_budget():
    """A chain of three at X = 64 keeps its two tables on chip; a chain of four (three tables) streams them."""
    M = _M()
    assert M.pick_kernel(64, 3, 2, 3, 2) == M.KERNEL_X64 and M.pick_kernel(64, 4, 3, 4, 3) == M.KERNEL_GENERIC
    _case('chain3_x64', X64)
    _case('chain4_x64', GENERIC)


def test_trees_equal_map_sweep():
    """On a tree one max-product sweep is exact: the assignment of map_sweep, its score at 1e-12."""
    for name, kernel in (('chain3_x64', X64), ('star4_x8', GENERIC), ('chain5_x8', GENERIC)):
        fb, got = _case(name, kernel)
        fb.initialize()
        x, score = fb.map_sweep([fb.topo.var_ids[0]], init=True)
        assert np.array_equal(x.cpu().numpy(), got['x']), name
        np.testing.assert_allclose(got['score'], score.cpu().numpy(), rtol=1e-12)


# ---- the cutset is a choice, not a result -----------------------------------------------------------------
def test_cutset_override_and_redundant_cutset():
    M = _M()
    fb, base = _case('k3_x64', X64, pick=(1, 2))
    _case('k3_x64', X64, pick=(1, 2), cutset=[1])
    _case('k3_x64', X64, pick=(1, 2), cutset=[2, 0])             # redundant: 4096 configurations of a single free variable
    with pytest.raises(ValueError):
        fb.exact_map(cutset=[9])
    with pytest.raises(M.ExactMapError, match='cycle'):
        fb.exact_map(cutset=[])
    with pytest.raises(ValueError):
        fb.exact_map(max_marginals=torch.empty(1, dtype=torch.float64, device=fb.device))
    _case('chain5_x8', GENERIC, cutset=[2, 0])


def test_shared_tables_and_batch_position_give_the_same_bits():
    for name, kernel in (('k3_x64', X64), ('ring5_x7', GENERIC)):
        spec, inputs, _ = E.family(name)
        inputs = inputs[:4]
        fb = _batch(spec, inputs)
        full = _both(fb, kernel=kernel)
        pair, unary = batch_tables(spec, fb.topo, inputs)
        P, U = fb.topo.P, fb.topo.U
        ptab = np.arange(4 * P).reshape(4, P)
        utab = np.arange(4 * U).reshape(4, U)
        ptab[0], utab[0] = ptab[2], utab[2]                      # graphs 0 and 2 both read the tables of graph 2
        shared = _both(_batch(spec, inputs, (pair, unary), ptab, utab), kernel=kernel)
        alone = _both(_batch(spec, inputs[1:2]), kernel=kernel)  # B = 1: another number of chunks per graph at ring5
        for key in ('x', 'score', 'mm'):
            assert np.array_equal(shared[key][0], full[key][2]) and np.array_equal(shared[key][1:], full[key][1:]), key
            assert np.array_equal(alone[key][0], full[key][1]), key


# ---- range ----------------------------------------------------------------------------------------------
def test_power_of_two_scaling():
    """Tables times 2^+-400, unary rows times 2^+-500: the same assignment; score and max-marginals move by k ln 2."""
    for name, kernel, moves in (('user_k3_lognormal', X64, [({0: 400}, {}), ({2: -400}, {}), ({}, {0: 500}), ({}, {1: -500}),
                                                             ({0: 37, 1: -5, 2: 400}, {0: -300, 1: 3, 2: 500})]),
                                ('ring5_x7', GENERIC, [({0: 400}, {}), ({4: -400}, {}), ({}, {0: 500}), ({1: -400, 3: 400}, {2: -500})])):
        spec, inputs, _ = E.family(name)
        inputs = inputs[:2]
        fb = _batch(spec, inputs)
        base = _both(fb, kernel=kernel)
        pair, unary = batch_tables(spec, fb.topo, inputs)
        P, U = fb.topo.P, fb.topo.U
        for pk, uk in moves:
            p2, u2 = pair.copy(), unary.copy()
            for b in range(2):
                for p, k in pk.items():
                    p2[b * P + p] = np.ldexp(p2[b * P + p], k)
                for u, k in uk.items():
                    u2[b * U + u] = np.ldexp(u2[b * U + u], k)
            got = _both(_batch(spec, inputs, (p2, u2)), kernel=kernel)
            shift = (sum(pk.values()) + sum(uk.values())) * np.log(2.0)
            assert np.array_equal(got['x'], base['x']), (name, pk, uk)
            assert E.close(got['score'], base['score'] + shift, 1e-12), (name, pk, uk)
            assert E.close(got['mm'], base['mm'] + shift, 1e-12), (name, pk, uk)


def test_wide_range_tables():
    """K3 at X = 64 on exp(20 N(0, 1)) tables -- 170 decades each -- against the log-domain reference."""
    _case('k3_x64_wide', X64)


# ---- ties -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('X,kernel', [(64, X64), (5, GENERIC)], ids=['x64', 'generic'])
def test_tie_rule(X, kernel):
    """Powers of two: all-ones tables give the all-zero assignment; two configurations that tie go to the lower c; a tie inside
    a forest variable goes to the lower state; tables full of ties decode as the NumPy statement of the header does."""
    spec = R.kn_spec(3, X)
    g = O.Graph(spec)
    cut = R.chosen_ids(spec)
    assert cut == [0]
    ones = E.ones_inputs(spec)
    two_configs = E.ones_inputs(spec)
    two_configs['tables'][0][[X - 1, 2], 0] = 2.0                # the cutset variable's unary row: states 2 and X - 1 tie
    in_forest = E.ones_inputs(spec)
    in_forest['tables'][0][[3, 1], 0] = 2.0
    in_forest['tables'][1][[X - 2, 2], 0] = 4.0                  # the forest's root: states 2 and X - 2 tie
    in_forest['tables'][2][[4, 3], 0] = 8.0                      # its child
    inputs = [ones, two_configs, in_forest] + [E.power_of_two_inputs(spec, s, -1, 1) for s in range(5)]
    want = [E.condition_max(g, i, cut) for i in inputs]
    assert [want[k][0][v] for k in range(3) for v in g.var_order] == [0, 0, 0, 2, 0, 0, 1, 2, 3]
    got = _both(_batch(spec, inputs), kernel=kernel)
    for b, (x, score, mm) in enumerate(want):
        assert [int(v) for v in got['x'][b]] == [x[v] for v in g.var_order], b
        assert E.close(got['score'][b], score, 1e-12) and E.close(got['mm'][b], mm, 1e-12), b
    assert got['score'][0] == 0.0 and (got['mm'][0] == 0.0).all()


# ---- edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel', [('k3_x64', X64), ('ring5_x7', GENERIC)], ids=['x64', 'generic'])
def test_zero_nan_inf_tables_and_bad_index(name, kernel):
    spec, inputs, _ = E.family(name)
    X, inputs = spec['X'], inputs[:7]
    fb = _batch(spec, inputs)
    base = _both(fb, kernel=kernel)
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
    for with_mm in (False, True):
        mm = torch.full((fb2.B, fb2.topo.n_vars, X), -7.0, dtype=torch.float64, device=fb2.device)
        got = _run(fb2, mm=mm if with_mm else False, kernel=kernel)
        x, score = got['x'], got['score']
        assert (x[0] == 0).all() and score[0] == -np.inf
        assert (x[3] == -1).all() and np.isnan(score[3])
        for b in (1, 2, 4, 5):
            assert ((x[b] >= 0) & (x[b] < X)).all(), b
        assert np.array_equal(x[6], base['x'][6]) and score[6] == base['score'][6]
        if with_mm:
            assert (got['mm'][0] == -np.inf).all() and (got['mm'][3] == -7.0).all()
            assert np.array_equal(got['mm'][6], base['mm'][6])


def test_float32_tables_are_refused():
    spec = C.user_spec(10, [1, 4, 7], 256, 64, seed=1)
    fb = _batch(spec, [C.make_inputs(spec, 1)])
    fb.set_pair_tables(fb.pair_tables, dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        fb.exact_map()


def test_capture_and_replay_with_changed_tables():
    """After one eager call the call is captured; a replay gives the bits of the eager call, and after the tables are
    overwritten in place the bits of an eager call on the new tables."""
    spec, inputs, _ = E.family('k3_x64')
    fb = _batch(spec, inputs[:3])
    first = _both(fb, kernel=X64)
    other = _both(_batch(spec, inputs[3:6]), kernel=X64)
    assert not np.array_equal(first['x'], other['x'])
    mm = torch.empty(fb.B, fb.topo.n_vars, fb.X, dtype=torch.float64, device=fb.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x, score, _ = fb.exact_map(max_marginals=mm)
    pair, unary = batch_tables(spec, fb.topo, inputs[3:6])
    for want in (first, other):
        x.fill_(-5)
        score.fill_(float('nan'))
        mm.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(x.cpu().numpy(), want['x']) and np.array_equal(score.cpu().numpy(), want['score'])
        assert np.array_equal(mm.cpu().numpy(), want['mm'])
        fb.pair_tables.copy_(torch.from_numpy(pair))
        fb.unary_tables.copy_(torch.from_numpy(unary))


# ---- trainer --------------------------------------------------------------------------------------------
def test_tidir_exact_decode(tmp_path):
    """TiDirTrainer.exact_decode() on the clique fixture (K1 to K12 at X = 64, its own thetas): K1 to K4 against every
    instance's own graph by enumeration, K5 and up listed as skipped; the report recomputed on the host from decode()."""
    from macaronicusermodeling_amd import tidir
    from test_gpu_cliques import _trainer
    gold = tidir_gold('tidir_cliques_reference')
    paths = write_tidir(gold, str(tmp_path))
    tt = _trainer(paths, gold)
    phi_ee, phi_w1, phi_ed = tidir.load_features(paths['phi.pmi'], paths['phi.pmi_w1'], paths['phi.ed'], paths['phi.ped'])
    th_ee, th_ed = np.array(gold['theta_en_en']).reshape(1, -1), np.array(gold['theta_en_de']).reshape(1, -1)
    bp_guesses, _ = tt.decode()
    guesses, counts, report, skipped = tt.exact_decode()
    want_counts, want_report, too_large, seen = np.zeros(4, dtype=np.int64), [0, 0, 0.0, 0.0], {}, 0
    for key, b in sorted(tt.buckets.items()):
        for i, row in enumerate(b['rows']):
            got = guesses[row['index']]
            if len(key[1]) >= 5:
                too_large[tuple(key[1])] = too_large.get(tuple(key[1]), 0) + 1
                assert got == (tuple(key[1]), None, None, None, None)
                continue
            g, inputs, _, _ = tidir_oracle_graph(key, b, i, phi_ee, phi_w1, phi_ed, th_ee, th_ed)
            x, best, mm = E.reference(g, inputs)
            gap = E.gap_of(best, mm) if g.X ** len(key[1]) > 1 else np.inf
            assert gap >= E.GAP, (key, gap)                     # no instance is left out
            log_z = R.logsumexp(W.brute_force(g, inputs)[2]) if len(key[1]) <= 3 else R.eliminate(g, inputs)[0]
            positions, words, score, margin, joint = got
            assert positions == tuple(key[1]) == tuple(g.var_order)
            assert words == [tt.en[x[v]] for v in key[1]], (key, gap)
            np.testing.assert_allclose(score, best, rtol=1e-12)
            assert abs(margin - gap) <= 2e-10 * max(1.0, abs(best)), (key, margin, gap)      # two max-marginals at their bar
            assert abs(joint - (best - log_z)) <= 2e-10 * max(1.0, abs(log_z)), (key, joint)   # the bar of exact_inference's log_z
            hit = [x[v] == int(b['var_labels'][i][k]) for k, v in enumerate(key[1])]
            want_counts += np.array([all(hit), 1, sum(hit), len(hit)])
            bp_words, bp_score = bp_guesses[row['index']][1:]
            agrees = bp_words == words
            short = 0.0 if agrees else max(score - bp_score, 0.0)
            assert bp_score <= score + 1e-9 * abs(score)
            want_report = [want_report[0] + 1, want_report[1] + agrees, want_report[2] + short, max(want_report[3], short)]
            seen += 1
    assert seen >= 4 and too_large
    assert tuple(int(v) for v in want_counts) == tuple(counts)
    assert report[:2] == (want_report[0], want_report[1])
    np.testing.assert_allclose(report[2:], want_report[2:], rtol=1e-9, atol=1e-12)
    assert sorted(s[0] for s in skipped) == sorted(too_large) and all('configurations' in s[2] for s in skipped)
    assert sum(s[1] for s in skipped) == sum(too_large.values())
    x, score, margin, agrees, shortfall, joint = tt.trainers[next(iter(tt.trainers))].exact_decode()
    assert x.dtype == np.int64 and agrees.dtype == np.bool_ and (shortfall >= 0).all() and margin.shape == score.shape == joint.shape
