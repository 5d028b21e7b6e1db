"""The forest shapes the cutset walk (csrc/mlbp_cutset_walk.h) branches on, without a GPU: the graph families, the plan each
must reach -- asserted through GraphTopology, cutset.choose and cutset.plan_words, so that a change of planner cannot move a
case off its path --, the six libraries' NumPy statements pinned on enumeration for every family, and the rules that make the
discrete outputs comparable, asserted for every input tests/test_gpu_walk_shapes.py uses.

Families (every second pairwise factor turned, so that both table orientations occur on forest edges and on cutset-incident
items) and the walk path each reaches:

  star2                  0-1, 0-2, unary factors on 1 and 2 only; no cutset.  Root 0 with the children 1 and 2: the sibling product
                         ("the parent's other children") of x64_down_step and of generic_down; variable 0 has an empty item
                         range (base == 1).
  diamond                K4 without the edge 2-3; cutset [0].  Root 1 with the children 2 and 3 under 64 configurations: the
                         sibling product with a cutset-incident item on every free variable, ROW and COL.
  bowtie                 the triangles 0-1-2 and 0-3-4; cutset [0].  Two roots with a child each: the second Alg::root of x64_up,
                         parent == {-1, -1} in the middle of `order`.
  two_edges_and_a_loner  0-1, 2-3, variable 4 with two unary factors; no cutset.  Three roots, one without a forest factor; one
                         configuration, so three of the four waves of the X = 64 workgroup have none.
  pair2                  two factors over (0, 1) on opposite axes, a unary factor on 1.  Cutset [0]: n_forest == 0, a cutset
                         variable without a unary factor.  Cutset [0, 1]: n_free == 0 -- both walk loops empty, constants only.
  k3_two_cut             K3 under the cutset [0, 1]: one free variable, no forest, 4096 configurations.
  unary12, unary13       12 / 13 variables with a unary factor each, P == 0 (pair_tables NULL), every variable a root.  At X = 64
                         the table-free term of the LDS rule decides alone: 12 variables fit, 13 go to the generic kernel.
  caterpillar            0-1, 1-2, 1-3, 3-4, 5-2, 5-4.  Under [5]: root 0, its child 1 with the children 2 and 3, 3 with the child
                         4 -- a hub below a root: generic_down multiplies dn[par] and the siblings' up into one vector.  Four
                         forest tables: never the X = 64 kernel.  Under the chosen [1]: the chain 2-5-4-3 and the lone root 0.

References.  Enumeration (the other CPU modules' enumerate_exact, brute_force, pair_marginals_enum, enum_top) at X = 5 (X = 3 for
the unary families: 3^13 entries) holds every statement at the bar its own module uses; that licenses the statements as the
reference at X = 64 where X^n cannot be enumerated.  refs_*() pick the reference of a (case, X): enumeration where X^n <= 64^3,
the slice-wise enumeration or the elimination up to four variables (as k4_x64 is handled in the six modules), the statement
beyond, and for the unary families' sums the closed form (normalised rows, log Z = the sum of the logs of the row sums).

The rules.  A MAP row is compared only where the best score leads by GAP = 1e-6 nats (test_exactmap_cpu.gap_of), an M-best list
where ranks 0 .. M are GAP apart (test_exactmbest_cpu.gaps_of), a draw where its margin is 1e-8 (test_exactsample_cpu
.check_margin).  No graph of these families is exempted: test_no_graph_is_exempted asserts all three on the reference alone for
every (case, X) the GPU module runs; the seeds were chosen so that it holds."""
import functools

import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_cutsetis_cpu as SI
import test_exactgrad_cpu as SG
import test_exactmap_cpu as SM
import test_exactmbest_cpu as SB
import test_exactsample_cpu as SS
import test_map_cpu as W
from oracle import lbp_oracle as O

SMALL_X = 5                      # the generic kernel's run of every family: odd, as the six modules' small sizes
UNARY_SMALL_X = 3                # 3^13 assignments can still be enumerated
MBEST_M = 5                      # the longest list the GPU module asks for
N_SAMPLES = 3


# ------------------------------------------------------------------------------------------------
# the families
# ------------------------------------------------------------------------------------------------
def shape_spec(name, X, n, unary_on, pairs):
    """One pairwise factor per pair -- the first variable on axis 0, every second factor turned --, then unary factors on
    `unary_on` (a variable may repeat).  The pairs come first and name the variables in ascending order, so that a variable's
    position in GraphTopology.var_ids (the order of first appearance) is its id also where it has no unary factor."""
    factors = [dict(id=k, vars=[a, b], dims=[0, 1] if k % 2 == 0 else [1, 0], table=k) for k, (a, b) in enumerate(pairs)]
    factors += [dict(id=len(pairs) + i, vars=[v], dims=[0], table=len(pairs) + i) for i, v in enumerate(unary_on)]
    return dict(name='%s_x%d' % (name, X), style='explicit', X=X, var_ids=list(range(n)), labels=[(2 * i + 1) % X for i in range(n)],
                factors=factors)


SHAPES = {
    'star2': lambda X: shape_spec('star2', X, 3, [1, 2], [(0, 1), (0, 2)]),
    'diamond': lambda X: shape_spec('diamond', X, 4, [0, 1, 2, 3], [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)]),
    'bowtie': lambda X: shape_spec('bowtie', X, 5, [0, 1, 2, 3, 4], [(0, 1), (0, 2), (1, 2), (0, 3), (0, 4), (3, 4)]),
    'two_edges_and_a_loner': lambda X: shape_spec('two_edges_and_a_loner', X, 5, [0, 1, 2, 3, 4, 4], [(0, 1), (2, 3)]),
    'pair2': lambda X: shape_spec('pair2', X, 2, [1], [(0, 1), (0, 1)]),
    'k3_two_cut': lambda X: R.kn_spec(3, X, name='k3_two_cut_x%d' % X),
    'unary12': lambda X: shape_spec('unary12', X, 12, list(range(12)), []),
    'unary13': lambda X: shape_spec('unary13', X, 13, list(range(13)), []),
    'caterpillar': lambda X: shape_spec('caterpillar', X, 6, [0, 1, 2, 3, 4, 5], [(0, 1), (1, 2), (1, 3), (3, 4), (5, 2), (5, 4)]),
}
UNARY = ('unary12', 'unary13')

# case -> (family, the cutset given as variable ids or None: cutset.choose, the cutset the plan must hold,
#          {root: its children in the order the walk meets them ...}, n_forest, n_items, n_consts)
CASES = {
    'star2': ('star2', None, [], {0: [1, 2]}, 2, 2, 0),
    'diamond': ('diamond', None, [0], {1: [2, 3]}, 2, 6, 1),
    'bowtie': ('bowtie', None, [0], {1: [2], 3: [4]}, 2, 8, 1),
    'two_edges_and_a_loner': ('two_edges_and_a_loner', None, [], {0: [1], 2: [3], 4: []}, 2, 6, 0),
    'pair2': ('pair2', None, [0], {1: []}, 0, 3, 0),
    'pair2_cut01': ('pair2', [0, 1], [0, 1], {}, 0, 0, 3),
    'k3_two_cut': ('k3_two_cut', [0, 1], [0, 1], {2: []}, 0, 3, 3),
    'unary12': ('unary12', None, [], {v: [] for v in range(12)}, 0, 12, 0),
    'unary13': ('unary13', None, [], {v: [] for v in range(13)}, 0, 13, 0),
    'caterpillar_cut5': ('caterpillar', [5], [5], {0: [1], 1: [2, 3], 3: [4]}, 4, 7, 1),
    'caterpillar': ('caterpillar', None, [1], {0: [], 2: [5], 5: [4], 4: [3]}, 3, 8, 1),
}
ROOTS = {'star2': [0], 'diamond': [1], 'bowtie': [1, 3], 'two_edges_and_a_loner': [0, 2, 4], 'pair2': [1], 'pair2_cut01': [], 'k3_two_cut': [2],
         'unary12': list(range(12)), 'unary13': list(range(13)), 'caterpillar_cut5': [0], 'caterpillar': [0, 2]}
N_CONFIGS_64 = {'star2': 1, 'diamond': 64, 'bowtie': 64, 'two_edges_and_a_loner': 1, 'pair2': 64, 'pair2_cut01': 4096, 'k3_two_cut': 4096,
                'unary12': 1, 'unary13': 1}
BOTH_ITEM_KINDS = ('diamond', 'bowtie', 'pair2', 'caterpillar_cut5', 'caterpillar')      # a ROW and a COL item among the cutset-incident ones
X64_CASES = [c for c in CASES if not c.startswith('caterpillar')]
X64_LDS = {'star2': 98960, 'diamond': 109744, 'bowtie': 120496, 'two_edges_and_a_loner': 120480, 'unary12': 129200, 'unary13': 139968}


def small_x(case):
    return UNARY_SMALL_X if CASES[case][0] in UNARY else SMALL_X


def runs():
    """Every (case, X) the GPU module runs: X = 64 for all but the caterpillar, and the small size for all."""
    return [(c, 64) for c in X64_CASES] + [(c, small_x(c)) for c in CASES]


def run_id(run):
    return '%s-x%d' % run


def spec_of(case, X):
    return SHAPES[CASES[case][0]](X)


def cut_of(case):
    """The cutset of the case as variable ids (what the plan must hold; the GPU module passes CASES[case][1])."""
    return list(CASES[case][2])


# ------------------------------------------------------------------------------------------------
# the plans
# ------------------------------------------------------------------------------------------------
def _S():
    from macaronicusermodeling_amd import cutset
    return cutset


def plan_of(case, X):
    """(topology, plan words, {section: (offset, length)}) through the real planner."""
    from macaronicusermodeling_amd.topology import GraphTopology
    S = _S()
    topo = GraphTopology.from_spec(spec_of(case, X))
    assert topo.var_ids == list(O.Graph(spec_of(case, X)).var_order) == list(range(topo.n_vars))      # ids are positions in these families
    given = CASES[case][1]
    words = S.plan_words(topo, S.choose(topo) if given is None else given)
    return topo, words, R._sections(S, words)


def lds_rule(n_vars, P, U, n_forest):
    """MLBP_CUTSET_X64_LDS_BYTES' left-hand side, as include/mlbp_cutset.h states it."""
    return n_forest * 33280 + 21 * n_vars * 512 + 64 + 4 * ((P + U + 16 + 3) // 4 * 4)


@pytest.mark.parametrize('case', sorted(CASES))
def test_the_plan_reaches_the_path(case):
    S = _S()
    family, given, cut, tree, n_forest, n_items, n_consts = CASES[case]
    for X in (64, small_x(case)):
        topo, words, sec = plan_of(case, X)
        if given is None:
            assert S.choose(topo) == cut, (case, S.choose(topo))
        S.check_plan(words, X)
        n, P, U, n_cut, n_free = (int(w) for w in words[:5])
        assert (n, n_cut, n_free) == (topo.n_vars, len(cut), topo.n_vars - len(cut))
        assert [int(w) for w in words[sec['cutset'][0]:sec['cutset'][0] + n_cut]] == cut
        assert (int(words[7]), int(words[5]), int(words[6])) == (n_forest, n_items, n_consts), (case, words[:8])
        order = [int(w) for w in words[sec['order'][0]:sec['order'][0] + n_free]]
        parent = {v: (int(words[sec['parent'][0] + 2 * v]), int(words[sec['parent'][0] + 2 * v + 1])) for v in range(n)}
        roots = [v for v in order if parent[v] == (-1, -1)]
        assert sorted(roots) == ROOTS[case] and all(parent[v] == (-1, -1) for v in cut)
        children = {v: sorted(w for w in order if parent[w][1] == v) for v in order}
        assert {v: kids for v, kids in children.items() if kids or v in roots} == {v: sorted(kids) for v, kids in tree.items()}, (case, children)
        assert len(order) - len(roots) == n_forest
        assert S.Plan(topo, cut, X, None).n_configs == X ** len(cut) and (X != 64 or case not in N_CONFIGS_64 or 64 ** len(cut) == N_CONFIGS_64[case])
        if len(roots) > 1 and n_forest:                          # a root in the middle of `order`: another tree's variable follows it
            assert any(parent[v] == (-1, -1) for v in order[:-1])
        # both orientations on forest edges and on cutset-incident items, wherever the family has two of them
        pav = [(int(words[sec['pav'][0] + 2 * p]), int(words[sec['pav'][0] + 2 * p + 1])) for p in range(P)]
        child_axes = {pav[parent[v][0]].index(v) for v in order if parent[v][0] >= 0}
        kinds = {int(words[sec['items'][0] + 3 * i]) for i in range(n_items)} - {S.ITEM_UNARY}
        assert n_forest < 2 or child_axes == {0, 1}, (case, child_axes)
        assert case not in BOTH_ITEM_KINDS or kinds == {S.ITEM_COL, S.ITEM_ROW}, (case, kinds)
        # the kernel
        want = S.KERNEL_X64 if X == 64 and case in X64_CASES and case != 'unary13' else S.KERNEL_GENERIC
        assert S.pick_kernel(X, n, P, U, n_forest) == want, case
        if X == 64 and family in X64_LDS:
            assert lds_rule(n, P, U, n_forest) == X64_LDS[family]
            assert (X64_LDS[family] <= S.X64_LDS_BYTES) == (family != 'unary13')
    if family == 'caterpillar':                                 # three or more forest tables: X = 64 never takes the X = 64 kernel
        topo, words, _ = plan_of(case, 64)
        assert int(words[7]) >= 3 and S.pick_kernel(64, topo.n_vars, topo.P, topo.U, int(words[7])) == S.KERNEL_GENERIC
        assert lds_rule(topo.n_vars, topo.P, topo.U, int(words[7])) > S.X64_LDS_BYTES


def test_the_families_hold_what_the_docstring_says():
    """A variable without any factor of its own in the plan (an empty item range), a cutset variable without a unary factor,
    P == 0, n_free == 0 and a single configuration on the X = 64 kernel."""
    S = _S()
    topo, words, sec = plan_of('star2', 64)
    off = [int(w) for w in words[sec['item_off'][0]:sec['item_off'][0] + topo.n_vars + 1]]
    assert off[1] - off[0] == 0 and topo.U == 2                  # variable 0: the root, no item
    topo, words, sec = plan_of('pair2', 64)
    assert [int(w) for w in words[sec['uvar'][0]:sec['uvar'][0] + topo.U]] == [1] and int(words[6]) == 0
    topo, words, _ = plan_of('pair2_cut01', 64)
    assert int(words[4]) == 0 and 64 ** int(words[3]) == 4096   # n_free == 0
    topo, words, _ = plan_of('unary12', 64)
    assert topo.P == 0 and int(words[7]) == 0
    topo, words, _ = plan_of('two_edges_and_a_loner', 64)
    assert int(words[3]) == 0 and S.chunks(2, 1) == 1           # one configuration: one chunk, one of its four waves walks


# ------------------------------------------------------------------------------------------------
# the inputs of the GPU module, and their references
# ------------------------------------------------------------------------------------------------
SEEDS = {}                       # (case, X) -> table seeds, where the default's reference does not satisfy the rules
DEFAULT_SEEDS = (1, 2)


@functools.lru_cache(maxsize=None)
def inputs_of(case, X):
    """(spec, [inputs]): lognormal tables, two graphs."""
    spec = spec_of(case, X)
    return spec, [C.make_inputs(spec, s, 'lognormal') for s in SEEDS.get((case, X), DEFAULT_SEEDS)]


def enumerable(case, X):
    return X ** len(spec_of(case, X)['var_ids']) <= 64 ** 3


def unary_closed_form(g, inputs):
    """(log_z, marginals) of a graph of unary factors alone: normalised rows, the sum of the logs of the row sums."""
    rows = {vs[0]: T for vs, T in R._factor_arrays(g, inputs)}
    assert len(rows) == len(g.var_order)
    return float(sum(np.log(rows[v].sum()) for v in g.var_order)), np.stack([rows[v] / rows[v].sum() for v in g.var_order])


@functools.lru_cache(maxsize=None)
def refs_cutset(case, X):
    """[(log_z, marginals)] per graph."""
    spec, inputs = inputs_of(case, X)
    g, n = O.Graph(spec), len(spec['var_ids'])
    if CASES[case][0] in UNARY:
        return [unary_closed_form(g, i) for i in inputs]
    if enumerable(case, X):
        return [R.enumerate_exact(g, i)[:2] for i in inputs]
    if n <= 4:
        return [R.eliminate(g, i) for i in inputs]
    return [R.condition(g, i, cut_of(case)) for i in inputs]


@functools.lru_cache(maxsize=None)
def refs_map(case, X):
    """[(x, best, max-marginals)] per graph."""
    spec, inputs = inputs_of(case, X)
    g = O.Graph(spec)
    if len(spec['var_ids']) <= 4:
        return [SM.reference(g, i) for i in inputs]
    return [SM.condition_max(g, i, cut_of(case)) for i in inputs]


@functools.lru_cache(maxsize=None)
def refs_pairs(case, X):
    """[(log_z, marginals, {factor id: M})] per graph."""
    spec, inputs = inputs_of(case, X)
    g, n = O.Graph(spec), len(spec['var_ids'])
    if CASES[case][0] in UNARY:
        return [unary_closed_form(g, i) + ({},) for i in inputs]
    if enumerable(case, X):
        return [SG.pair_marginals_enum(g, i) for i in inputs]
    if n <= 4:
        return [R.eliminate(g, i) + (SG.eliminate_pairs(g, i),) for i in inputs]
    return [SG.condition_pairs(g, i, cut_of(case)) for i in inputs]


@functools.lru_cache(maxsize=None)
def refs_mbest(case, X):
    """[(rows, scores)] per graph, MBEST_M + 1 long: enumeration's up to four variables, the statement's beyond."""
    spec, inputs = inputs_of(case, X)
    g = O.Graph(spec)
    out = []
    for i in inputs:
        if len(spec['var_ids']) <= 4:
            top = SB.enum_top(g, i, MBEST_M + 1)
            out.append((SB.as_rows(g, [x for _, x in top]), [s for s, _ in top]))
        else:
            xs, scores = SB.statement(g, i, cut_of(case), MBEST_M + 1)
            out.append((SB.as_rows(g, xs), scores))
    return out


@functools.lru_cache(maxsize=None)
def refs_sample(case, X):
    """(uniforms [S][B][n_vars], {(s, b): walk}, [Statement per graph]): the statement is the reference of a draw."""
    spec, inputs = inputs_of(case, X)
    uniforms = np.random.RandomState(4000 + sorted(CASES).index(case) + X).rand(N_SAMPLES, len(inputs), len(spec['var_ids']))
    stmts = [SS.statement(spec, i, cut_of(case)) for i in inputs]
    return uniforms, {(s, b): stmts[b].walk(uniforms[s, b]) for s in range(N_SAMPLES) for b in range(len(inputs))}, stmts


@functools.lru_cache(maxsize=None)
def refs_listed(case, X):
    """(configs [B][N][n_cut], log_q [B][N], [the statement's outputs per graph]) of the full list with q = X^-|C|."""
    spec, inputs = inputs_of(case, X)
    g, cut = O.Graph(spec), cut_of(case)
    full = SI.full_list(X, len(cut))
    log_q = np.full(len(full), -np.log(float(len(full))))
    stated = [SI.Statement(g, i, cut).run(full, log_q) for i in inputs]
    return np.tile(full[None], (len(inputs), 1, 1)), np.tile(log_q[None], (len(inputs), 1)), stated


RAGGED_B = 100                   # diamond at X = 64: chunks(100, 64) = 6, 24 wave-walkers for 64 configurations


@functools.lru_cache(maxsize=None)
def ragged():
    """(spec, three graphs' inputs, [(log_z, marginals, {factor id: M})] by elimination) of the ragged-chunk tests."""
    spec = spec_of('diamond', 64)
    inputs = [C.make_inputs(spec, s, 'lognormal') for s in (1, 2, 3)]
    g = O.Graph(spec)
    return spec, inputs, [R.eliminate(g, i) + (SG.eliminate_pairs(g, i),) for i in inputs]


# ------------------------------------------------------------------------------------------------
# the statements on enumeration, at the small size
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(CASES))
def test_the_six_statements_equal_enumeration(case):
    X = small_x(case)
    spec, inputs = inputs_of(case, X)
    g, cut, order = O.Graph(spec), cut_of(case), list(spec['var_ids'])
    assert X ** len(order) <= 7 ** 6 or CASES[case][0] in UNARY
    for b, i in enumerate(inputs):
        want_z, want_m, grid = R.enumerate_exact(g, i)
        # cutset
        z, m = R.condition(g, i, cut)
        assert abs(z - want_z) <= 1e-12 * max(1.0, abs(want_z)) and np.abs(m - want_m).max() <= 1e-12, (case, b)
        if CASES[case][0] in UNARY:
            cz, cm = unary_closed_form(g, i)
            assert abs(cz - want_z) <= 1e-12 * max(1.0, abs(want_z)) and np.abs(cm - want_m).max() <= 1e-12
        # exactmap
        x, best, _ = W.brute_force(g, i)
        want_mm = SM.grid_max_marginals(grid)
        sx, sscore, smm = SM.condition_max(g, i, cut)
        assert SM.gap_of(best, want_mm) >= SM.GAP and sx == x, (case, b)
        np.testing.assert_allclose(sscore, best, rtol=1e-12)
        assert SM.close(smm, want_mm, 1e-10) and SM.close(smm.max(axis=1), np.full(len(x), best), 1e-12)
        # exactgrad
        _, _, want_p = SG.pair_marginals_enum(g, i)
        pz, pm, pp = SG.condition_pairs(g, i, cut)
        assert set(pp) == set(want_p) and (not want_p or SG.worst_gap(pp, want_p) <= 1e-12), (case, b)
        assert abs(pz - want_z) <= 1e-12 * max(1.0, abs(want_z)) and np.abs(pm - want_m).max() <= 1e-12
        # exactsample: log Z, and the logp of draws and of other assignments
        st = SS.Statement(g, i, cut)
        assert abs(st.log_z - want_z) <= 1e-12 * max(1.0, abs(want_z))
        rs = np.random.RandomState(b)
        for k in range(24):
            if k % 2:
                xs = dict(zip(order, (int(s) for s in rs.randint(0, X, size=len(order)))))
                logp = st.forced(xs)
            else:
                w = st.walk(rs.rand(len(order)))
                xs, logp = w['x'], w['logp']
                assert abs(logp - st.forced(xs)) <= 1e-13 * max(1.0, abs(logp))
            want = grid[tuple(xs[v] for v in order)] - want_z
            assert abs(logp - want) <= 1e-12 * max(1.0, abs(want)), (case, b, xs)
        # exactmbest
        top = SB.enum_top(g, i, SB.MAX_M + 1)
        assert min(SB.gaps_of([s for s, _ in top])) >= SB.GAP
        for M in (1, MBEST_M, 16):
            xs, scores = SB.statement(g, i, cut, M)
            assert SB.as_rows(g, xs) == SB.as_rows(g, [r for _, r in top[:M]]), (case, b, M)
            np.testing.assert_allclose(scores, [s for s, _ in top[:M]], rtol=1e-12)
        # cutsetis: the full list with uniform q is the exact sum; ess as the header states it
        configs, log_q, stated = refs_listed(case, X)
        out = stated[b]
        assert abs(out['log_z_hat'] - want_z) <= 1e-10 * max(1.0, abs(want_z)) and np.abs(out['marg'] - want_m).max() <= 1e-10, (case, b)
        Zc = np.exp(out['log_w'] + log_q[b])
        assert abs(out['ess'] - Zc.sum() ** 2 / (Zc * Zc).sum()) <= 1e-10 * out['ess']


# ------------------------------------------------------------------------------------------------
# the rules, on the reference alone, for every input of the GPU module
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', runs(), ids=run_id)
def test_no_graph_is_exempted(run):
    case, X = run
    spec, inputs = inputs_of(case, X)
    gaps = [SM.gap_of(best, mm) for _, best, mm in refs_map(case, X)]
    total = X ** len(spec['var_ids'])
    lists = refs_mbest(case, X)
    assert all(len(scores) == min(MBEST_M + 1, total) for _, scores in lists)
    list_gaps = [min(SB.gaps_of(scores)) for _, scores in lists]
    print('%s X = %d: smallest MAP gap %.1e nats, smallest gap among ranks 0 .. %d %.1e nats' % (case, X, min(gaps), MBEST_M, min(list_gaps)))
    assert min(gaps) >= SM.GAP and min(list_gaps) >= SB.GAP, (case, X, gaps, list_gaps)
    for (rows, scores), (x, best, _) in zip(lists, refs_map(case, X)):          # row 0 is the MAP assignment
        assert rows[0] == [x[v] for v in spec['var_ids']] and abs(scores[0] - best) <= 1e-12 * max(1.0, abs(best))
    _, walks, stmts = refs_sample(case, X)
    assert all(s.usable for s in stmts) and SS.MARGIN == 1e-8 and SS.MAY_OMIT == 0
    SS.check_margin('%s X = %d' % (case, X), walks)


@pytest.mark.parametrize('run', [r for r in runs() if not enumerable(*r)], ids=run_id)
def test_the_references_beyond_enumeration_agree(run):
    """Where X^n cannot be enumerated the sums' reference (the elimination, the statement or the closed form) and the listed
    statement's exact sum are two computations: they agree at the statement's own bar."""
    case, X = run
    _, _, stated = refs_listed(case, X)
    for (z, m), out, (pz, pm, _) in zip(refs_cutset(case, X), stated, refs_pairs(case, X)):
        assert abs(out['log_z_hat'] - z) <= 1e-10 * max(1.0, abs(z)) and np.abs(out['marg'] - m).max() <= 1e-10
        assert abs(pz - z) <= 1e-12 * max(1.0, abs(z)) and np.abs(pm - m).max() <= 1e-12
