"""The listed modes of the four exact cutset libraries (exactmap: cutset_map; exactmbest: cutset_mbest; exactsample:
cutset_resample; exactgrad: cutset_gradient / cutset_pair_marginals) on every forest shape of tests/test_walk_shapes_cpu.py,
without a GPU: the lists tests/test_gpu_listed_shapes.py walks, the four NumPy statements (test_searchmap_cpu.listed_map,
test_searchmbest_cpu.listed_mbest, test_resample_cpu.Listed, test_estgrad_cpu.listed_pairs) pinned on enumeration for every
family -- they were pinned on K_n, a ring, a tree and two components before --, and the rules that make the discrete outputs
comparable, asserted on the reference alone for every (case, X, list) the GPU module compares.

The graphs, the plans and the kernel every (case, X) must reach are test_walk_shapes_cpu's (T.CASES, T.runs(), T.inputs_of,
T.cut_of, T.small_x) and are asserted there.

Lists (lists_of).  full: every configuration once in configuration-index order with log_q = 0 -- (1, 0) without cutset
variables.  short: five rows drawn from a RandomState, then rows 1 and 3 once more (N = 7: duplicates and arbitrary order are part
of the contract), log_q = -3 rand(N) -- a proposal that is no distribution, which the headers admit; without cutset variables the
rows are empty, configs (7, 0).  one: the first row of short alone.

References.  At the small X every statement is held to enumeration restricted to the listed states (test_searchmbest_cpu
.restricted_top), to the tilted model (test_estgrad_cpu.tilted_enum; the unary families, whose grid of pairs cannot be built
at 12 / 13 variables, to T.unary_closed_form) and to the probability of the draw on the grid of log-potentials; that licenses
the statements as the reference at X = 64.

The rules.  listed_map(margins=True): the winner leads every other configuration and its own runner-up completion by GAP =
1e-6 nats; listed_mbest: ranks 0 .. min(M, n_found) lie GAP apart; Listed.run: every draw's margin, the entry draw included, is
at least MARGIN = 1e-8.  test_no_list_is_exempted asserts all three for every (case, X) of T.runs() and every list: the share
left out is 0.  The default seeds (tables (1, 2), lists 7, uniforms 3) satisfy them everywhere.

pair2 under [0, 1] (n_free == 0): a listed row admits one assignment, so n_found is the number of distinct rows.  At X = 64
short's five drawn rows are distinct in both graphs: at m = MBEST_M = 5 the list is just full and ends at 5 of the reference's
m = 6.  The list shorter than the m the GPU module asks for, padded with -1 / -inf, is the one of `one` (n_found == 1) at both
sizes and short's at X = 5 in graph 0 (four distinct rows).  test_a_list_without_free_variables_ends_at_n_found asserts these."""
import functools

import numpy as np
import pytest

import test_cutset_cpu as R
import test_cutsetis_cpu as SI
import test_estgrad_cpu as LG
import test_exactgrad_cpu as SG
import test_exactmap_cpu as SM
import test_exactmbest_cpu as SB
import test_exactsample_cpu as SS
import test_resample_cpu as LR
import test_searchmap_cpu as LM
import test_searchmbest_cpu as LB
import test_walk_shapes_cpu as T
from oracle import lbp_oracle as O

LISTS = ('full', 'short', 'one')
N_SHORT = 7
LIST_SEEDS = {}                  # (case, X) -> seed of the lists, where the default's reference does not satisfy the rules
DEFAULT_LIST_SEED = 7
UNIFORM_SEEDS = {}               # (case, X) -> seed of the uniforms, likewise
DEFAULT_UNIFORM_SEED = 3
MBEST_M = T.MBEST_M
M_VALUES = (1, MBEST_M)          # the m of the GPU module: both lists kernels are reached (test_both_lists_kernels_are_reached)
X64_RUNS = [r for r in T.runs() if r[1] == 64]


# ------------------------------------------------------------------------------------------------
# the lists, and the statements' outputs on them
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lists_of(case, X):
    """{'full' | 'short' | 'one': (configs int32 [B][N][n_cut], log_q float64 [B][N])}, a list per graph of T.inputs_of(case, X)."""
    B, n_cut = len(T.inputs_of(case, X)[1]), len(T.cut_of(case))
    rs = np.random.RandomState(LIST_SEEDS.get((case, X), DEFAULT_LIST_SEED))
    full = SI.full_list(X, n_cut)
    configs, log_q = [], []
    for _ in range(B):
        five = rs.randint(0, X, size=(5, n_cut)).astype(np.int32)
        configs.append(np.concatenate([five, five[[1, 3]]]))
        log_q.append(-3.0 * rs.rand(N_SHORT))
    configs, log_q = np.ascontiguousarray(np.stack(configs), dtype=np.int32), np.stack(log_q)
    assert configs.shape == (B, N_SHORT, n_cut)
    return {'full': (np.ascontiguousarray(np.tile(full[None], (B, 1, 1))), np.zeros((B, len(full)))), 'short': (configs, log_q),
            'one': (np.ascontiguousarray(configs[:, :1]), np.ascontiguousarray(log_q[:, :1]))}


def _graph(case, X):
    spec, inputs = T.inputs_of(case, X)
    return O.Graph(spec), inputs, T.cut_of(case)


@functools.lru_cache(maxsize=None)
def refs_map(case, X, name):
    """[listed_map(..., margins=True)] per graph."""
    g, inputs, cut = _graph(case, X)
    return [LM.listed_map(g, i, cut, c, margins=True) for i, c in zip(inputs, lists_of(case, X)[name][0])]


@functools.lru_cache(maxsize=None)
def refs_mbest(case, X, name):
    """[listed_mbest(..., MBEST_M + 1)] per graph."""
    g, inputs, cut = _graph(case, X)
    return [LB.listed_mbest(g, i, cut, c, MBEST_M + 1) for i, c in zip(inputs, lists_of(case, X)[name][0])]


@functools.lru_cache(maxsize=None)
def uniforms_of(case, X):
    """[S][B][n_vars], T.N_SAMPLES draws per graph."""
    spec, inputs = T.inputs_of(case, X)
    return np.random.RandomState(UNIFORM_SEEDS.get((case, X), DEFAULT_UNIFORM_SEED)).rand(T.N_SAMPLES, len(inputs), len(spec['var_ids']))


@functools.lru_cache(maxsize=None)
def listed_statements(case, X):
    g, inputs, cut = _graph(case, X)
    return [LR.Listed(g, i, cut) for i in inputs]


@functools.lru_cache(maxsize=None)
def refs_resample(case, X, name):
    """[Listed.run] per graph on uniforms_of(case, X)."""
    configs, log_q = lists_of(case, X)[name]
    u = uniforms_of(case, X)
    return [st.run(configs[b], log_q[b], u[:, b]) for b, st in enumerate(listed_statements(case, X))]


def test_the_lists_are_what_the_docstring_says():
    for case, X in T.runs():
        lists = lists_of(case, X)
        n_cut, B = len(T.cut_of(case)), len(T.inputs_of(case, X)[1])
        configs, log_q = lists['full']
        assert configs.shape == (B, X ** n_cut, n_cut) and configs.dtype == np.int32 and not log_q.any()
        assert all(int(sum(int(s) * X ** q for q, s in enumerate(row))) == c for c, row in enumerate(configs[0]))
        configs, log_q = lists['short']
        assert configs.shape == (B, 7, n_cut) and configs.dtype == np.int32 and log_q.shape == (B, 7)
        assert np.array_equal(configs[:, 5], configs[:, 1]) and np.array_equal(configs[:, 6], configs[:, 3])
        assert ((configs >= 0) & (configs < X)).all() and ((log_q <= 0) & (log_q > -3)).all()
        one = lists['one']
        assert np.array_equal(one[0], configs[:, :1]) and np.array_equal(one[1], log_q[:, :1]) and one[0].shape == (B, 1, n_cut)
        again = lists_of.__wrapped__(case, X)                    # deterministic
        assert all(np.array_equal(a, b) for k in LISTS for a, b in zip(lists[k], again[k]))
        if n_cut:                                               # the two graphs walk lists of their own
            assert not np.array_equal(configs[0], configs[1])


# ------------------------------------------------------------------------------------------------
# the four statements on enumeration, at the small size
# ------------------------------------------------------------------------------------------------
def check_draws_on_the_grid(g, inputs, cut, configs, log_q, uniforms, out, grid):
    """test_resample_cpu's check of a Listed.run: p(draw | list, entry) = (w_i / sum w) p(x_free | c_i) with w_i = Z_{c_i} / q_i,
    every factor from the grid of summed log-potentials, at 1e-12; logp = score - log_q[entry] - ln sum w at 1e-10; log_z_hat
    and ess from the same weights."""
    order, N = list(g.var_order), len(log_q)

    def clamped(row):                                           # the grid with the cutset's axes fixed at the entry's states
        return np.asarray(grid[tuple(int(row[cut.index(v)]) if v in cut else slice(None) for v in order)])
    log_zc = np.array([R.logsumexp(clamped(configs[i])) for i in range(N)])
    log_w = log_zc - log_q
    log_sum_w = R.logsumexp(log_w)
    assert abs(out['log_z_hat'] + np.log(N) - log_sum_w) <= 1e-12 * max(1.0, abs(log_sum_w))
    w = np.exp(log_w - log_sum_w)
    assert abs(out['ess'] - 1.0 / (w * w).sum()) <= 1e-10 * N
    for s in range(len(uniforms)):
        i, x = int(out['entry'][s]), dict(zip(order, (int(v) for v in out['samples'][s])))
        assert 0 <= i < N and all(x[v] == configs[i][q] for q, v in enumerate(cut))
        at = grid[tuple(x[v] for v in order)]
        want = (log_w[i] - log_sum_w) + (at - log_zc[i])
        if not cut:                                             # every entry is the empty configuration: entry 0, the exact call's logp
            assert i == 0
            want = at - log_zc[0]
        assert abs(out['logp'][s] - want) <= 1e-12 * max(1.0, abs(want)), (s, out['logp'][s], want)
        assert abs(out['score'][s] - at) <= 1e-12 * max(1.0, abs(at))
        identity = out['score'][s] - log_q[i] - (out['log_z_hat'] + np.log(N)) if cut else out['score'][s] - log_zc[0]
        assert abs(out['logp'][s] - identity) <= 1e-10 * max(1.0, abs(identity))


@pytest.mark.parametrize('case', sorted(T.CASES))
def test_the_four_statements_equal_enumeration(case):
    X = T.small_x(case)
    g, inputs, cut = _graph(case, X)
    order, unary = list(g.var_order), T.CASES[case][0] in T.UNARY
    for name in ('short', 'one'):
        configs, log_q = lists_of(case, X)[name]
        for b, i in enumerate(inputs):
            c, q = configs[b], log_q[b]
            N = len(q)
            distinct = len({tuple(r) for r in c.tolist()})
            # exactmbest, exactmap: enumeration restricted to the listed states
            want = LB.restricted_top(g, i, cut, c, MBEST_M + 1)
            assert len(want) == min(MBEST_M + 1, distinct * X ** (len(order) - len(cut))), (case, name, b)
            got = refs_mbest(case, X, name)[b]
            assert got['n_found'] == len(want) and got['rows'] == [x for _, _, x in want], (case, name, b)
            assert got['entries'] == [e for _, e, _ in want], (case, name, b)
            np.testing.assert_allclose(got['scores'], [s for s, _, _ in want], rtol=1e-12)
            for m in M_VALUES:                                  # a shorter call is the prefix
                less = LB.listed_mbest(g, i, cut, c, m)
                assert less['rows'] == got['rows'][:m] and less['entries'] == got['entries'][:m] and less['n_found'] == min(m, got['n_found'])
            top = refs_map(case, X, name)[b]
            assert [top['x'][v] for v in order] == want[0][2] and top['entry'] == want[0][1], (case, name, b)
            np.testing.assert_allclose(top['score'], want[0][0], rtol=1e-12)
            assert top['entry'] == min(k for k, row in enumerate(c) if np.array_equal(row, c[top['entry']]))      # a repeat: the lower index
            # exactgrad: the tilted model, or the closed form of the unary families
            pairs = LG.listed_pairs(g, i, cut, c, q)
            assert not pairs['refused']
            if unary:
                z, marg = T.unary_closed_form(g, i)
                want_z, want_m, want_p = z + np.log(np.exp(-q).mean()), marg, {}
            else:
                want_z, want_m, want_p = LG.tilted_enum(g, i, cut, c, q)
            assert abs(pairs['log_z_hat'] - want_z) <= 1e-10 * max(1.0, abs(want_z)), (case, name, b)
            assert np.abs(pairs['marg'] - want_m).max() <= 1e-10 and set(pairs['pairs']) == set(want_p), (case, name, b)
            assert not want_p or SG.worst_gap(pairs['pairs'], want_p) <= 1e-10, (case, name, b)
            # exactsample: the probability of the draw given the list
            _, _, grid = R.enumerate_exact(g, i)
            out = refs_resample(case, X, name)[b]
            assert (out['samples'] >= 0).all() and len(out['samples']) == T.N_SAMPLES
            check_draws_on_the_grid(g, i, cut, c, q, uniforms_of(case, X)[:, b], out, grid)
            if not cut:                                         # no uniform is spent on an entry: uniform k draws the k-th variable of the walk
                assert (out['entry'] == 0).all() and all(len(per) == len(order) for per in out['margin'])
                assert abs(out['log_z_hat'] - (R.logsumexp(grid) + np.log(np.exp(-q).mean()))) <= 1e-12 * max(1.0, abs(out['log_z_hat']))
            else:
                assert all(len(per) == len(order) - len(cut) + 1 for per in out['margin'])


@pytest.mark.parametrize('case', sorted(T.CASES))
def test_the_full_list_with_log_q_zero_is_the_exact_statement(case):
    """As the four modules assert for K_n: rows, entries (the configuration numbers) and scores of the exact statements; the
    exact draws bit for bit; the exact pair marginals (bits in the statement's own order of walking, 1e-13 in index order)."""
    X = T.small_x(case)
    g, inputs, cut = _graph(case, X)
    order = list(g.var_order)
    configs, log_q = lists_of(case, X)['full']
    N = configs.shape[1]
    number = lambda x: sum(x[v] * X ** q for q, v in enumerate(cut))      # noqa: E731
    for b, i in enumerate(inputs):
        x, score, _ = SM.condition_max(g, i, cut)
        top = refs_map(case, X, 'full')[b]
        assert top['x'] == x and top['score'] == score and top['entry'] == number(x), (case, b)
        xs, scores = SB.statement(g, i, cut, MBEST_M + 1)
        got = refs_mbest(case, X, 'full')[b]
        assert got['rows'] == SB.as_rows(g, xs) and got['scores'] == scores and got['entries'] == [number(r) for r in xs], (case, b)
        exact = SS.Statement(g, i, cut)
        out = refs_resample(case, X, 'full')[b]
        for s, u in enumerate(uniforms_of(case, X)[:, b]):
            w = exact.walk(u)
            assert [int(v) for v in out['samples'][s]] == [w['x'][v] for v in order] and out['entry'][s] == number(w['x'])
            assert out['logp'][s] == w['logp'] and out['margin'][s] == w['margin']
        assert abs(out['log_z_hat'] - (exact.log_z - np.log(N))) <= 1e-12 * max(1.0, abs(exact.log_z))
        log_z, marg, pairs = SG.condition_pairs(g, i, cut)
        bits = LG.listed_pairs(g, i, cut, LG.product_list(X, len(cut)), np.zeros(N))
        assert np.array_equal(bits['marg'], marg) and all(np.array_equal(bits['pairs'][f], pairs[f]) for f in pairs), (case, b)
        other = LG.listed_pairs(g, i, cut, configs[b], log_q[b])
        assert np.abs(other['marg'] - marg).max() <= 1e-13 and (not pairs or SG.worst_gap(other['pairs'], pairs) <= 1e-13)
        assert abs(other['log_z_hat'] - (log_z - np.log(N))) <= 1e-12 * max(1.0, abs(log_z))


# ------------------------------------------------------------------------------------------------
# the rules, on the reference alone, for every input of the GPU module
# ------------------------------------------------------------------------------------------------
def rule_figures(case, X, name):
    """(the smallest lead over another configuration, over the runner-up completion, the smallest gap among ranks 0 .. min(M,
    n_found), the smallest margin of a draw) over the graphs of one (case, X, list)."""
    tops, ranked, runs = refs_map(case, X, name), refs_mbest(case, X, name), refs_resample(case, X, name)
    assert all(np.isfinite(r['score']) and r['entry'] >= 0 for r in tops)
    assert all(r['n_found'] >= 1 and len(r['scores']) == r['n_found'] for r in ranked)
    assert all((r['samples'] >= 0).all() and np.isfinite(r['logp']).all() for r in runs)
    n_draws = len(T.inputs_of(case, X)[0]['var_ids']) - len(T.cut_of(case)) + (1 if T.cut_of(case) else 0)
    assert all(len(per) == n_draws for r in runs for per in r['margin'])                   # the entry draw included
    return (min(r['config_margin'] for r in tops), min(r['completion_margin'] for r in tops),
            min([np.inf] + [gap for r in ranked for gap in SB.gaps_of(r['scores'])]),
            min([np.inf] + [m for r in runs for per in r['margin'] for m in per]))


@pytest.mark.parametrize('name', LISTS)
@pytest.mark.parametrize('run', T.runs(), ids=T.run_id)
def test_no_list_is_exempted(run, name):
    case, X = run
    assert LM.GAP == LB.GAP == 1e-6 and LR.MARGIN == 1e-8
    lead, completion, gap, margin = rule_figures(case, X, name)
    print('%s X = %d %s: configuration lead %.1e nats, completion lead %.1e nats, smallest gap among ranks 0 .. %d %.1e nats, '
          'smallest margin of a draw %.1e' % (case, X, name, lead, completion, MBEST_M, gap, margin))
    assert lead >= LM.GAP and completion >= LM.GAP, (case, X, name, lead, completion)
    assert gap >= LB.GAP, (case, X, name, gap)
    assert margin >= LR.MARGIN, (case, X, name, margin)
    for top, ranked in zip(refs_map(case, X, name), refs_mbest(case, X, name)):            # row 0 is the listed MAP answer
        order = T.inputs_of(case, X)[0]['var_ids']
        assert ranked['rows'][0] == [top['x'][v] for v in order] and ranked['entries'][0] == top['entry']


# ------------------------------------------------------------------------------------------------
# facts that keep the cases on their path
# ------------------------------------------------------------------------------------------------
def shape_of(case, X):
    """(X, n_vars, P, U, n_forest): the arguments of every library's pick_kernel."""
    topo, words, _ = T.plan_of(case, X)
    return X, topo.n_vars, topo.P, topo.U, int(words[7])


@pytest.mark.parametrize('run', T.runs(), ids=T.run_id)
def test_a_list_without_free_variables_ends_at_n_found(run):
    """n_free == 0: a listed row admits one assignment, so n_found is the number of distinct rows."""
    case, X = run
    for name in ('short', 'one'):
        for c, r in zip(lists_of(case, X)[name][0], refs_mbest(case, X, name)):
            distinct = len({tuple(row) for row in c.tolist()})
            admitted = distinct * X ** (len(T.inputs_of(case, X)[0]['var_ids']) - len(T.cut_of(case)))
            assert r['n_found'] == min(MBEST_M + 1, admitted)
            if case == 'pair2_cut01':
                assert r['n_found'] == distinct <= 5 < MBEST_M + 1 and (name == 'short' or distinct == 1)
                assert r['rows'] and len({tuple(row) for row in r['rows']}) == distinct
                assert name == 'short' or r['n_found'] < MBEST_M                                 # `one`: shorter than the m the GPU module asks for
    if case == 'pair2_cut01':                                   # short: full at m = 5 at X = 64 (five distinct rows), one row short of it at X = 5
        found = [r['n_found'] for r in refs_mbest(case, X, 'short')]
        assert found == ([5, 5] if X == 64 else [4, 5]), found


def test_every_library_takes_its_x64_walk_kernel():
    from macaronicusermodeling_amd import exactgrad, exactmap, exactmbest, exactsample
    for case, X in X64_RUNS:
        shape = shape_of(case, X)
        x64 = case != 'unary13'
        for M in (exactmap, exactsample, exactgrad):
            assert (M.pick_kernel(*shape) == M.KERNEL_X64) == x64 and (x64 or M.pick_kernel(*shape) == M.KERNEL_GENERIC), (case, M.__name__)
        for m in M_VALUES:
            assert (exactmbest.kernels(exactmbest.pick_kernel(*shape, m))[0] == exactmbest.KERNEL_X64) == x64, (case, m)
    for case, X in T.runs():
        if X != 64:
            shape = shape_of(case, X)
            assert exactmap.pick_kernel(*shape) == exactsample.pick_kernel(*shape) == exactgrad.pick_kernel(*shape) == exactmap.KERNEL_GENERIC
            assert all(exactmbest.kernels(exactmbest.pick_kernel(*shape, m)) == (2, 2) for m in M_VALUES)


def test_both_lists_kernels_are_reached():
    """Across the X = 64 cases exactmbest's listed calls take the X = 64 lists kernel and the generic one behind the X = 64 values
    kernel, at the m the GPU module uses."""
    from macaronicusermodeling_amd import exactmbest as M
    seen = {M.kernels(M.pick_kernel(*shape_of(case, X), m)) for case, X in X64_RUNS for m in M_VALUES}
    assert {(M.KERNEL_X64, M.KERNEL_X64), (M.KERNEL_X64, M.KERNEL_GENERIC), (M.KERNEL_GENERIC, M.KERNEL_GENERIC)} <= seen, seen
    assert M.kernels(M.pick_kernel(*shape_of('diamond', 64), 1)) == (M.KERNEL_X64, M.KERNEL_X64)
    assert M.kernels(M.pick_kernel(*shape_of('diamond', 64), MBEST_M)) == (M.KERNEL_X64, M.KERNEL_GENERIC)


def test_the_two_slot_gradient_kernel_is_reached_with_a_cutset():
    """n_forest == 2 at X = 64: star2, diamond, bowtie, two_edges_and_a_loner; diamond and bowtie walk 64 listed configurations
    into both R[f] slots."""
    two = [case for case, X in X64_RUNS if T.CASES[case][4] == 2]
    assert two == ['star2', 'diamond', 'bowtie', 'two_edges_and_a_loner']
    assert [case for case in two if T.cut_of(case)] == ['diamond', 'bowtie']
    assert all(T.CASES[case][4] == 0 for case, X in X64_RUNS if case not in two)


RAGGED_N = 29


def ragged_walkers(B=T.RAGGED_B, N=RAGGED_N):
    """{library: the walkers of a graph's list}: a wave per entry on the X = 64 kernels, four waves a chunk."""
    from macaronicusermodeling_amd import exactgrad, exactmap, exactmbest, exactsample
    return {'exactmap': 4 * exactmap.chunks(B, N), 'exactmbest': 4 * exactmbest.chunks(B, N), 'exactsample': 4 * exactsample.chunks(B, N),
            'exactgrad': 4 * exactgrad.chunks(B, N, exactgrad.KERNEL_X64)}


def test_the_ragged_list_leaves_walkers_with_unequal_shares():
    """diamond at X = 64, B = T.RAGGED_B: a list of RAGGED_N entries gives every library 1 < walkers < N with N % walkers != 0."""
    from macaronicusermodeling_amd import exactgrad, exactmap, exactmbest, exactsample
    shape = shape_of('diamond', 64)
    for walkers in ragged_walkers().values():
        assert 1 < walkers < RAGGED_N and RAGGED_N % walkers != 0, ragged_walkers()
    assert exactmap.pick_kernel(*shape) == exactsample.pick_kernel(*shape) == exactgrad.pick_kernel(*shape) == 1
    assert exactmbest.kernels(exactmbest.pick_kernel(*shape, MBEST_M))[0] == 1


@functools.lru_cache(maxsize=None)
def ragged_lists():
    """(configs int32 [3][RAGGED_N][1], log_q [3][RAGGED_N], uniforms [S][3][4]) for the three graphs of T.ragged(): distinct
    rows first (so that the ranks are those of 22 configurations), then repeats."""
    rs = np.random.RandomState(DEFAULT_LIST_SEED)
    configs = np.stack([np.concatenate([rs.permutation(64)[:22], rs.randint(0, 64, size=RAGGED_N - 22)]) for _ in range(3)])
    return (np.ascontiguousarray(configs[:, :, None], dtype=np.int32), -3.0 * rs.rand(3, RAGGED_N),
            np.random.RandomState(DEFAULT_UNIFORM_SEED).rand(T.N_SAMPLES, 3, 4))


@functools.lru_cache(maxsize=None)
def ragged_refs():
    """([listed_map], [listed_mbest], [Listed.run]) of the three graphs of the ragged tests."""
    spec, inputs, _ = T.ragged()
    g, cut = O.Graph(spec), T.cut_of('diamond')
    configs, log_q, u = ragged_lists()
    return ([LM.listed_map(g, i, cut, c, margins=True) for i, c in zip(inputs, configs)],
            [LB.listed_mbest(g, i, cut, c, MBEST_M + 1) for i, c in zip(inputs, configs)],
            [LR.Listed(g, i, cut).run(configs[b], log_q[b], u[:, b]) for b, i in enumerate(inputs)])


def test_the_ragged_lists_clear_the_rules():
    tops, ranked, runs = ragged_refs()
    assert min(min(r['config_margin'], r['completion_margin']) for r in tops) >= LM.GAP
    assert min(gap for r in ranked for gap in SB.gaps_of(r['scores'])) >= LB.GAP and all(r['n_found'] == MBEST_M + 1 for r in ranked)
    LR.check_margin('diamond X = 64 ragged', runs)
    assert all(len(per) == 4 for r in runs for per in r['margin'])


# ------------------------------------------------------------------------------------------------
# the refused list of the GPU module
# ------------------------------------------------------------------------------------------------
def refused_lists(X):
    """diamond: graph 0's short list with a state of X in its last row; graph 1's as it is."""
    configs, log_q = lists_of('diamond', X)['short']
    bad = configs.copy()
    bad[0, N_SHORT - 1, 0] = X
    return bad, log_q


@pytest.mark.parametrize('X', [64, 5])
def test_the_statements_refuse_the_bad_list(X):
    g, inputs, cut = _graph('diamond', X)
    bad, log_q = refused_lists(X)
    assert (bad[1] < X).all() and (bad[0] == X).sum() == 1 and bad[0, -1, 0] == X
    top = LM.listed_map(g, inputs[0], cut, bad[0])
    assert set(top['x'].values()) == {-1} and np.isnan(top['score']) and top['entry'] == -1
    assert LB.listed_mbest(g, inputs[0], cut, bad[0], MBEST_M)['n_found'] == -1
    out = LR.Listed(g, inputs[0], cut).run(bad[0], log_q[0], uniforms_of('diamond', X)[:, 0])
    assert (out['samples'] == -1).all() and (out['entry'] == -1).all() and np.isnan(out['logp']).all() and np.isnan(out['log_z_hat'])
    assert LG.listed_pairs(g, inputs[0], cut, bad[0], log_q[0])['refused']
