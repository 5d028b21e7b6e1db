"""Draws beyond the exact limit without a GPU: the NumPy statement of the LISTED mode of include/mlbp_exactsample.h pinned on
exhaustive enumeration and on the exact statement, the margin that makes a draw comparable, and the host side of the listed
call -- struct, constant, workspace rule, refusals.

The statement.  Listed(g, inputs, cut) is built from the existing statements: the forest, the pass up and a free variable's
vector are test_exactsample_cpu.Statement's (without its enumeration of every configuration: a listed call never counts
them), the SEGMENTED prefix sums and the draw rule are that module's prefix() and draw(), the split of exp(-log_q) into r 2^k
is test_cutsetis_cpu.split.  run() states the header: every entry's weight as a (mantissa, exponent) pair, the weights under
the largest exponent with the floor of 2^-4000, their prefix sums in list order, log_z_hat, ess, the entry drawn by the first
uniform, the free variables from the roots down.  Bringing the weights under E multiplies them by a power of two, which moves
no prefix sum's mantissa: with the full list in index order and log_q = 0 the statement's draws are the exact statement's bit
for bit, which test_the_full_list_is_the_exact_statement asserts.

The margin.  As in test_exactsample_cpu: a draw's margin is min_i |A_i - t| / total, the entry draw included, and samples and
entries are compared exactly with the device's only where every draw clears MARGIN = 1e-8.  INPUTS lists every input of
tests/test_gpu_resample.py whose samples are compared with the statement's; test_every_gpu_input_has_its_margin asserts the
margin for all of them, none left out; the seeds were chosen so that it holds.

No test asserts a statistical accuracy: every assertion is a deterministic function of its inputs."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_cutsetis_cpu as K
import test_exactsample_cpu as E
import test_map_cpu as W
from oracle import lbp_oracle as O

MARGIN = E.MARGIN
LN2 = K.LN2
MAX_ABS_LOG_Q = 1.0e6           # include/mlbp_cutsetis.h MLBP_CUTSETIS_MAX_ABS_LOG_Q
MIN_SHIFT = -4000


# ------------------------------------------------------------------------------------------------
# the statement
# ------------------------------------------------------------------------------------------------
class Listed(E.Statement):
    """The listed mode of include/mlbp_exactsample.h in NumPy for one graph and the cutset `cut` (variable ids; column q of a
    list is the state of cut[q]).  A configuration is its row of states, not a number."""

    def __init__(self, g, inputs, cut):
        forest = K.Statement(g, inputs, cut)                    # the forest of cutset.plan_words, nothing enumerated
        self.g, self.inputs, self.cut, self.X, self.order = g, inputs, list(cut), g.X, list(g.var_order)
        self.free, self.facs, self.edges, self.parent, self.walk_order = forest.free, forest.facs, forest.edges, forest.parent, forest.walk
        self._up = {}

    def states(self, row):
        return {v: int(s) for v, s in zip(self.cut, row)}

    def up(self, row):
        key = tuple(int(s) for s in row)
        if key not in self._up:
            with np.errstate(invalid='ignore', over='ignore'):
                self._up[key] = E.Statement.up(self, key)
        return self._up[key]

    def weights(self, configs, log_q):
        """(terms [N]: every weight under the largest exponent E of a positive one, E) -- NaN terms for a list that is refused."""
        N = len(log_q)
        configs = np.asarray(configs).reshape(N, len(self.cut))
        log_q = np.asarray(log_q, dtype=np.float64)
        ok = np.abs(log_q) <= MAX_ABS_LOG_Q                      # False for a NaN
        ok &= ((configs >= 0) & (configs < self.X)).all(axis=1)
        Zc = np.array([self.up(configs[i])[0] if ok[i] else np.nan for i in range(N)])
        with np.errstate(invalid='ignore', over='ignore'):
            r, k = K.split(np.where(ok, log_q, 0.0))
            zm, ze = np.frexp(Zc)                               # Z_c = zm 2^ze
            wm, we = np.frexp(zm * r)                           # w = wm 2^(we + ze + k)
        e = we + ze + k
        live = wm > 0
        top = int(e[live].max()) if live.any() else 0
        with np.errstate(invalid='ignore', over='ignore'):
            terms = np.ldexp(wm, np.maximum(e - top, MIN_SHIFT).astype(np.int64))
        return terms, top

    def run(self, configs, log_q, uniforms):
        """uniforms [S][n_vars] -> dict(samples int [S][n_vars] in g.var_order, logp [S], log_z_hat, score [S], entry [S],
        ess, margin [[per draw] per sample])."""
        N, S, n = len(log_q), len(uniforms), len(self.order)
        configs = np.asarray(configs).reshape(N, len(self.cut))
        terms, top = self.weights(configs, log_q)
        with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
            A = E.prefix(terms)
            last = A[-1]
            log_z_hat = float(top * LN2 + np.log(last / N)) if last != 0 else -np.inf
            ess = float(last * last / (terms * terms).sum()) if last != 0 else 0.0
        out = dict(samples=np.full((S, n), -1, dtype=np.int64), logp=np.full(S, np.nan), log_z_hat=log_z_hat, score=np.full(S, np.nan),
                   entry=np.full(S, -1, dtype=np.int64), ess=ess, margin=[[] for _ in range(S)], terms=terms)
        if not (last > 0 and np.isfinite(last)):
            return out
        for s, u in enumerate(uniforms):
            i, logp, margins = 0, 0.0, out['margin'][s]
            if self.cut:
                i, p, m = E.draw(terms, u[0])
                margins.append(m)
                logp = float(np.log(p))
            x = self.states(configs[i])
            bel = self.up(configs[i])[1]
            for k, v in enumerate(self.walk_order):             # roots to leaves: every variable after its parent
                x[v], p, m = E.draw(self.vector(v, bel, x), u[len(self.cut) + k])
                margins.append(m)
                logp += float(np.log(p))
            out['samples'][s] = [x[v] for v in self.order]
            out['logp'][s], out['entry'][s] = logp, i
            out['score'][s] = W.score_of(self.g, self.inputs, x)
        return out


def listed(spec, inputs, cut=None):
    return Listed(O.Graph(spec), inputs, R.chosen_ids(spec) if cut is None else cut)


# ------------------------------------------------------------------------------------------------
# every input of the GPU module whose samples are compared with the statement's:
# name -> (spec, table kind, table seeds (one graph each), N, list: 'full' (index order, log_q = 0) or the seed of make_list,
#          S, seed of the uniforms)
# ------------------------------------------------------------------------------------------------
INPUTS = {
    # the X = 64 kernel
    'k3_x64_full': (lambda: R.kn_spec(3, 64), 'uniform', (1, 2, 3), 64, 'full', 3, 0),
    'k3_x64_n7': (lambda: R.kn_spec(3, 64), 'lognormal', (1, 2, 3), 7, 11, 3, 1),
    'k5_x64_n5': (lambda: R.kn_spec(5, 64), 'uniform', (1, 2, 3), 5, 12, 3, 2),
    'k5_x64_n37': (lambda: R.kn_spec(5, 64), 'lognormal', (4, 5, 6), 37, 13, 5, 3),
    # the generic kernel
    'k4_x5_full': (lambda: R.kn_spec(4, 5), 'uniform', (1, 2), 25, 'full', 3, 4),
    'k4_x5_n300': (lambda: R.kn_spec(4, 5), 'lognormal', (3, 4), 300, 14, 3, 5),
    'k6_x3': (lambda: R.kn_spec(6, 3), 'uniform', (1, 2, 3), 20, 15, 3, 6),
    'chain4_x64': (lambda: C.chain_spec(4, 64), 'uniform', (1, 2), 4, 16, 2, 7),
    'star4_x8': (lambda: C.star_spec(4, 8), 'uniform', (1, 2, 3), 6, 17, 3, 8),
}


def make_list(g, inputs, cut, N, how, b=0):
    """(configs int32 [N][n_cut], log_q [N]) of one graph: the full list with log_q = 0, or test_cutsetis_cpu.make_list from
    seed `how` + 100 b; without cutset variables the log_q of a proposal that is no distribution, which the header admits."""
    if how == 'full':
        assert N == g.X ** len(cut)
        return K.full_list(g.X, len(cut)), np.zeros(N)
    if not cut:
        return np.zeros((N, 0), dtype=np.int32), -np.random.RandomState(how + 100 * b).rand(N) * 3.0
    return K.make_list(g, inputs, cut, N, how + 100 * b)


@functools.lru_cache(maxsize=None)
def family(name):
    """(spec, [inputs], cutset ids, configs [B][N][n_cut], log_q [B][N], uniforms [S][B][n_vars], [run per graph], [Listed per
    graph]) of INPUTS[name]: computed once per process and shared."""
    make, kind, seeds, N, how, S, u_seed = INPUTS[name]
    spec = make()
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    inputs = [C.make_inputs(spec, s, kind) for s in seeds]
    lists = [make_list(g, inp, cut, N, how, b) for b, inp in enumerate(inputs)]
    configs = np.stack([c for c, _ in lists]).astype(np.int32).reshape(len(inputs), N, len(cut))
    log_q = np.stack([q for _, q in lists])
    uniforms = np.random.RandomState(2000 + u_seed).rand(S, len(inputs), len(spec['var_ids']))
    stmts = [Listed(g, inp, cut) for inp in inputs]
    runs = [st.run(configs[b], log_q[b], uniforms[:, b]) for b, st in enumerate(stmts)]
    return spec, inputs, cut, configs, log_q, uniforms, runs, stmts


def check_margin(name, runs):
    """The rule of test_exactsample_cpu.check_margin: no (graph, sample) pair is left out."""
    margins = [m for r in runs for per in r['margin'] for m in per]
    smallest = min([np.inf] + margins)
    print('%s: %d graphs, %d draws, smallest margin of the statement %.2e' % (name, len(runs), len(margins), smallest))
    assert smallest >= MARGIN, (name, smallest)


@pytest.mark.parametrize('name', sorted(INPUTS))
def test_every_gpu_input_has_its_margin(name):
    assert MARGIN == 1e-8
    spec, _, cut, _, _, uniforms, runs, _ = family(name)
    assert all((r['samples'] >= 0).all() and np.isfinite(r['logp']).all() for r in runs)
    assert all(len(per) == len(spec['var_ids']) - len(cut) + (1 if cut else 0) for r in runs for per in r['margin'])      # the entry draw included
    check_margin(name, runs)


@functools.lru_cache(maxsize=None)
def shared_tables_family(B=600, N=3, S=2):
    """(spec, [3 inputs], cutset ids, configs [B][N][n_cut], log_q [B][N], uniforms [S][B][n_vars], [run per graph]): K5 at
    X = 64, graph b on the tables of inputs[b % 3] with a list of its own -- the GPU module's batch of 600 with one chunk."""
    spec = R.kn_spec(5, 64)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    inputs = [C.make_inputs(spec, 30 + s, 'lognormal' if s else 'uniform') for s in range(3)]
    lists = [make_list(g, inputs[b % 3], cut, N, 50, b) for b in range(B)]
    configs, log_q = np.stack([c for c, _ in lists]), np.stack([q for _, q in lists])
    uniforms = np.random.RandomState(5).rand(S, B, 5)
    stmts = [Listed(g, i, cut) for i in inputs]
    runs = [stmts[b % 3].run(configs[b], log_q[b], uniforms[:, b]) for b in range(B)]
    return spec, inputs, cut, configs, log_q, uniforms, runs


def test_the_batch_of_600_has_its_margin():
    runs = shared_tables_family()[-1]
    assert len(runs) == 600 and all((r['samples'] >= 0).all() for r in runs)
    check_margin('k5_x64_b600', runs)


def test_the_gpu_inputs_reach_what_the_issue_names():
    """N against the 4 C waves of the X = 64 kernel and the L = 2 of the SEGMENTED scan; K5 at X = 64 is beyond the exact limit."""
    from macaronicusermodeling_amd import cutset as S
    assert 64 ** len(family('k5_x64_n5')[2]) > S.MAX_CONFIGS and len(family('k5_x64_n5')[2]) == 3
    assert INPUTS['k5_x64_n5'][3] % 4 and INPUTS['k5_x64_n37'][3] % 4
    assert -(-INPUTS['k4_x5_n300'][3] // 256) == 2
    assert family('chain4_x64')[2] == [] and family('star4_x8')[2] == [] and family('star4_x8')[3].shape == (3, 6, 0)
    assert len(family('k6_x3')[2]) == 4


# ------------------------------------------------------------------------------------------------
# the statement against exhaustive enumeration
# ------------------------------------------------------------------------------------------------
SMALL = [('k3', lambda X: R.kn_spec(3, X)), ('k4', lambda X: R.kn_spec(4, X)), ('k5', lambda X: R.kn_spec(5, X)),
         ('tree', lambda X: C.star_spec(4, X))]


@pytest.mark.parametrize('X', [3, 4])
@pytest.mark.parametrize('name,make', SMALL, ids=[s[0] for s in SMALL])
def test_the_probability_of_a_draw_given_the_list_equals_enumeration(name, make, X):
    """p(draw | list, entry) = (w_i / sum w) p(x_free | c_i) with w_i = Z_{c_i} / q_i, every factor of it from the grid of
    summed log-potentials, at 1e-12; and logp = score - log_q[entry] - ln sum w at 1e-10."""
    spec = make(X)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    order = list(g.var_order)
    for kind, seed in (('uniform', 3), ('lognormal', 4)):
        inputs = C.make_inputs(spec, seed, kind)
        _, _, grid = W.brute_force(g, inputs)
        N = 9
        configs, log_q = make_list(g, inputs, cut, N, 20 + seed)
        st = Listed(g, inputs, cut)
        uniforms = np.random.RandomState(seed).rand(12, len(order))
        out = st.run(configs, log_q, uniforms)

        def clamped(row):                                       # the grid with the cutset's axes fixed at the entry's states
            return np.asarray(grid[tuple(int(row[cut.index(v)]) if v in cut else slice(None) for v in order)])
        log_zc = np.array([R.logsumexp(clamped(configs[i])) for i in range(N)])
        log_w = log_zc - log_q
        log_sum_w = R.logsumexp(log_w)
        assert abs(out['log_z_hat'] + np.log(N) - log_sum_w) <= 1e-12 * max(1.0, abs(log_sum_w))
        w = np.exp(log_w - log_sum_w)
        assert abs(out['ess'] - 1.0 / (w * w).sum()) <= 1e-10 * N
        worst = 0.0
        for s in range(len(uniforms)):
            i, x = int(out['entry'][s]), dict(zip(order, (int(v) for v in out['samples'][s])))
            assert 0 <= i < N and all(x[v] == configs[i][q] for q, v in enumerate(cut))
            want = (log_w[i] - log_sum_w) + (grid[tuple(x[v] for v in order)] - log_zc[i])
            if not cut:                                         # every entry is the empty configuration: entry 0, the exact call's logp
                assert i == 0
                want = grid[tuple(x[v] for v in order)] - log_zc[0]
            worst = max(worst, abs(out['logp'][s] - want) / max(1.0, abs(want)))
            assert abs(out['score'][s] - grid[tuple(x[v] for v in order)]) <= 1e-12 * max(1.0, abs(out['score'][s]))
            identity = out['score'][s] - log_q[i] - (out['log_z_hat'] + np.log(N)) if cut else out['score'][s] - log_zc[0]
            assert abs(out['logp'][s] - identity) <= 1e-10 * max(1.0, abs(identity))
        print('%s X = %d %s: logp of 12 draws within %.1e of enumeration' % (name, X, kind, worst))
        assert worst <= 1e-12


# ------------------------------------------------------------------------------------------------
# the full list in index order with log_q = 0 is the exact call
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,make,X', [('k3', lambda X: R.kn_spec(3, X), 4), ('k3_x64', lambda X: R.kn_spec(3, X), 64),
                                         ('k4', lambda X: R.kn_spec(4, X), 5), ('ring5', lambda X: C.ring_spec(5, X), 3)],
                         ids=['k3', 'k3_x64', 'k4', 'ring5'])
def test_the_full_list_is_the_exact_statement(name, make, X):
    """Samples, entry (= the configuration number), logp and score: the exact statement's, bit for bit; log_z_hat = log_z - ln N."""
    spec = make(X)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    for kind, seed in (('uniform', 5), ('lognormal', 6)):
        inputs = C.make_inputs(spec, seed, kind)
        exact = E.Statement(g, inputs, cut)
        N = X ** len(cut)
        uniforms = np.random.RandomState(seed).rand(6, len(g.var_order))
        out = Listed(g, inputs, cut).run(K.full_list(X, len(cut)), np.zeros(N), uniforms)
        for s, u in enumerate(uniforms):
            w = exact.walk(u)
            assert [int(v) for v in out['samples'][s]] == [w['x'][v] for v in g.var_order]
            assert out['entry'][s] == sum(w['x'][v] * X ** q for q, v in enumerate(cut))
            assert out['logp'][s] == w['logp'] and out['margin'][s] == w['margin']
            assert out['score'][s] == W.score_of(g, inputs, w['x'])
        assert abs(out['log_z_hat'] - (exact.log_z - np.log(N))) <= 1e-12 * max(1.0, abs(exact.log_z))


# ------------------------------------------------------------------------------------------------
# other statement cases
# ------------------------------------------------------------------------------------------------
def test_the_weights_are_the_cutsetis_statements():
    """exp(log_w) of test_cutsetis_cpu.Statement.run, entry by entry, and its log_z_hat and ess; also at large |log_q|."""
    spec = R.kn_spec(5, 4)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    inputs = C.make_inputs(spec, 7, 'lognormal')
    configs, log_q = K.make_list(g, inputs, cut, 40, 3)
    for lq in (log_q, log_q * 200.0 - 3000.0, log_q + 9000.0):
        ref = K.Statement(g, inputs, cut).run(configs, lq)
        st = Listed(g, inputs, cut)
        terms, top = st.weights(configs, lq)
        assert np.array_equal(terms, ref['terms'])
        live = terms > 0
        np.testing.assert_allclose(top * LN2 + np.log(terms[live]), ref['log_w'][live], rtol=1e-13)
        out = st.run(configs, lq, np.full((1, 5), 0.5))
        assert abs(out['log_z_hat'] - ref['log_z_hat']) <= 1e-12 * max(1.0, abs(ref['log_z_hat']))
        assert abs(out['ess'] - ref['ess']) <= 1e-12 * ref['ess']


def test_the_statement_refuses_what_the_header_refuses():
    spec = R.kn_spec(4, 3)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    inputs = C.make_inputs(spec, 2)
    configs, log_q = K.make_list(g, inputs, cut, 6, 1)
    u = np.full((2, 4), 0.5)
    good = Listed(g, inputs, cut).run(configs, log_q, u)
    assert (good['samples'] >= 0).all() and np.isfinite(good['logp']).all() and (good['entry'] >= 0).all()
    for bad_state in (-1, 3):
        c2 = configs.copy()
        c2[4, 1] = bad_state
        out = Listed(g, inputs, cut).run(c2, log_q, u)
        assert (out['samples'] == -1).all() and (out['entry'] == -1).all()
        assert np.isnan(out['logp']).all() and np.isnan(out['score']).all() and np.isnan(out['log_z_hat']) and np.isnan(out['ess'])
    for bad_q in (np.nan, np.inf, -np.inf, 1.5e6, -1.5e6):
        q2 = log_q.copy()
        q2[2] = bad_q
        out = Listed(g, inputs, cut).run(configs, q2, u)
        assert (out['samples'] == -1).all() and (out['entry'] == -1).all() and np.isnan(out['logp']).all()
        assert np.isnan(out['log_z_hat']) and np.isnan(out['ess'])
    dead = C.make_inputs(spec, 2)
    pair = next(f['table'] for f in spec['factors'] if len(f['vars']) == 2)
    dead['tables'][pair][:] = 0.0
    out = Listed(g, dead, cut).run(configs, log_q, u)
    assert (out['samples'] == -1).all() and (out['entry'] == -1).all() and np.isnan(out['logp']).all() and np.isnan(out['score']).all()
    assert out['log_z_hat'] == -np.inf and out['ess'] == 0.0


def test_a_list_of_one_and_a_list_of_copies():
    """N = 1: the entry is drawn with probability one, logp is the conditionals' alone, ess = 1.  N copies of one state: the
    same draws of the free variables whatever entry is picked, ess = N, log_z_hat the single entry's."""
    spec = R.kn_spec(4, 4)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    inputs = C.make_inputs(spec, 9, 'lognormal')
    st = Listed(g, inputs, cut)
    u = np.random.RandomState(3).rand(5, 4)
    one = st.run([[2, 1]], [-0.7], u)
    assert (one['entry'] == 0).all() and abs(one['ess'] - 1.0) <= 1e-15
    assert abs(one['log_z_hat'] - (np.log(st.up((2, 1))[0]) + 0.7)) <= 1e-12
    many = st.run(np.tile([[2, 1]], (7, 1)), np.full(7, -0.7), u)
    assert abs(many['ess'] - 7.0) <= 1e-12 and abs(many['log_z_hat'] - one['log_z_hat']) <= 1e-12
    assert np.array_equal(many['samples'], one['samples'])
    np.testing.assert_allclose(many['logp'], one['logp'] - np.log(7.0), rtol=1e-12)
    assert np.array_equal(many['entry'], np.minimum((u[:, 0] * 7).astype(int), 6))
    _, _, grid = W.brute_force(g, inputs)
    fixed = dict(zip(cut, (2, 1)))
    sub = np.asarray(grid[tuple(fixed.get(v, slice(None)) for v in g.var_order)])
    for s in range(5):                                          # N = 1: logp is the product of the conditionals p(x_free | c)
        x = dict(zip(g.var_order, (int(v) for v in one['samples'][s])))
        assert abs(one['logp'][s] - (grid[tuple(x[v] for v in g.var_order)] - R.logsumexp(sub))) <= 1e-12 * max(1.0, abs(one['logp'][s]))


def test_power_of_two_scaling_moves_no_sample():
    spec = R.kn_spec(5, 3)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    inputs = C.make_inputs(spec, 4, 'lognormal')
    configs, log_q = K.make_list(g, inputs, cut, 15, 2)
    u = np.random.RandomState(1).rand(6, 5)
    base = Listed(g, inputs, cut).run(configs, log_q, u)
    for k in (300, -300):
        moved = dict(inputs, tables=[np.ldexp(T, k) if i in (0, 7) else T for i, T in enumerate(inputs['tables'])])
        got = Listed(g, moved, cut).run(configs, log_q, u)
        assert np.array_equal(got['samples'], base['samples']) and np.array_equal(got['entry'], base['entry'])
        assert np.array_equal(got['logp'], base['logp']) and got['ess'] == base['ess']
        np.testing.assert_allclose(got['log_z_hat'], base['log_z_hat'] + 2 * k * LN2, rtol=1e-12)
        np.testing.assert_allclose(got['score'], base['score'] + 2 * k * LN2, rtol=1e-12)


# ------------------------------------------------------------------------------------------------
# the host side of the listed call
# ------------------------------------------------------------------------------------------------
def _M():
    from macaronicusermodeling_amd import exactsample
    return exactsample


def _ffi():
    from macaronicusermodeling_amd import _ffi
    return _ffi


def test_struct_constant_and_header_words():
    M = _M()
    names = [n for n, _ in M.ExactSampleArgs._fields_]
    assert names.index('N') == names.index('S') + 1
    assert {'configs', 'log_q', 'entry', 'ess'} <= set(names)
    assert M.MAX_LISTED == 65536 == K.MAX_LISTED
    text = open(E.HEADER).read()
    assert '#define MLBP_EXACTSAMPLE_MAX_LISTED 65536' in text
    for word in ('LISTED MODE', 'log_z_hat', 'ess', 'MLBP_CUTSETIS_MAX_ABS_LOG_Q', 'N == 0'):
        assert word in text, word
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.train import TiDirTrainer, UserGraphTrainer
    assert callable(FactorGraphBatch.cutset_resample) and callable(FactorGraphBatch.estimate_sample)
    assert callable(UserGraphTrainer.estimated_sample) and callable(TiDirTrainer.estimated_sample)


def test_listed_workspace_bytes_is_the_headers_formula():
    from macaronicusermodeling_amd import cutset as S
    M = _M()

    def ints(P, U):
        return 4 * ((P + U + 16 + 3) // 4 * 4)

    def vectors(n_vars, X):
        return (5 * n_vars + 2) * ((X + 1) // 2 * 2)

    def x64(X, n_vars, P, U, n_forest):
        return X == 64 and n_forest * 33280 + 21 * n_vars * 512 + 64 + ints(P, U) <= S.X64_LDS_BYTES

    def chunks(B, n):
        return min(n, -(-S.MIN_WORKGROUPS // B))
    shapes = ((64, 3, 3, 3, 1), (64, 5, 10, 5, 1), (64, 8, 28, 8, 1), (64, 12, 66, 12, 1), (64, 4, 3, 4, 3), (5, 4, 6, 4, 1), (3, 6, 15, 6, 1),
              (301, 3, 3, 3, 1), (1024, 3, 3, 3, 1), (1024, 5, 10, 5, 1), (8, 5, 4, 4, 4))
    spilled = 0
    for B, shape, N, n_samples in itertools.product((1, 3, 600, 8192), shapes, (1, 3, 37, 300, 65536), (1, 9, 64)):
        X, n_vars, P, U, n_forest = shape
        is_x64 = x64(*shape)
        assert (M.pick_kernel(*shape) == M.KERNEL_X64) == is_x64
        spill = not is_x64 and vectors(n_vars, X) * 8 + 64 + ints(P, U) > S.GENERIC_LDS_BYTES
        spilled += spill
        cw, cd = chunks(B, N), chunks(B, -(-n_samples // 4) if is_x64 else n_samples)
        want = B * N * 3 + B * M.HEAD + (B * max(cw, cd) * vectors(n_vars, X) if spill else 0)
        assert M.listed_workspace_bytes(B, n_samples, X, n_vars, P, U, n_forest, N) == want * 8, (B, shape, N, n_samples)
    assert spilled
    # the full list needs what the exact call needs
    assert M.listed_workspace_bytes(3, 5, 64, 3, 3, 3, 1, 64) == M.workspace_bytes(3, 5, 64, 3, 3, 3, 1, 1)
    assert M.listed_workspace_bytes(2, 5, 1024, 3, 3, 3, 1, 1024) == M.workspace_bytes(2, 5, 1024, 3, 3, 3, 1, 1)


def _listed_args(M, N=7, n=3, n_cut=1):
    """Arguments of a listed call on K_n at X = 64 that pass every host-side check."""
    from macaronicusermodeling_amd import cutset
    topo = R._topo(R.kn_spec(n, 4))
    words = cutset.plan_words(topo, list(range(n_cut)))
    a = M.ExactSampleArgs()
    a.B, a.X, a.n_vars, a.P, a.U, a.S, a.N = 2, 64, n, topo.P, topo.U, 5, N
    a.n_cut, a.n_free, a.n_items, a.n_consts, a.n_forest = (int(w) for w in words[3:8])
    a.n_pair_tables, a.n_unary_tables, a.plan_words = 6, 6, len(words)
    for name, typ in M.ExactSampleArgs._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, name, 4096)
    a.workspace_bytes = M.listed_workspace_bytes(a.B, a.S, a.X, a.n_vars, a.P, a.U, a.n_forest, max(1, min(N, M.MAX_LISTED)))
    return a


def test_listed_bad_arguments_on_a_cpu_only_machine():
    import torch
    M, F = _M(), _ffi()
    call = lambda a: M.lib.mlbp_exactsample_f64(ctypes.byref(a), None)
    a = _listed_args(M, N=-1)
    assert call(a) == F.MLBP_EINVAL and 'N = -1' in M.last_error()
    a = _listed_args(M, N=M.MAX_LISTED + 1)
    assert call(a) == F.MLBP_EINVAL and '65536' in M.last_error()
    a = _listed_args(M)
    a.configs = None
    assert call(a) == F.MLBP_EINVAL and 'configs' in M.last_error()
    a = _listed_args(M)
    a.log_q = None
    assert call(a) == F.MLBP_EINVAL and 'log_q' in M.last_error()
    a = _listed_args(M)
    a.workspace_bytes -= 8
    assert call(a) == F.MLBP_EINVAL and 'workspace' in M.last_error()
    a = _listed_args(M, n=19, n_cut=17)                         # 17 cutset variables: the remainder of K19 is one edge
    assert call(a) == F.MLBP_EUNSUPPORTED and '16' in M.last_error()
    assert M.lib.mlbp_exactsample_last_kernel() == M.KERNEL_NONE
    if torch.cuda.is_available():
        return                                                  # (the GPU module runs the entry for real)
    for n, n_cut, N in ((3, 1, 7), (5, 3, 37), (5, 3, M.MAX_LISTED), (12, 10, 1)):     # K5 and K12: beyond the exact limit
        for opt in (4096, None):                                # log_z, score, entry and ess are optional
            a = _listed_args(M, N=N, n=n, n_cut=n_cut)
            a.log_z = a.score = a.entry = a.ess = opt
            assert call(a) == F.MLBP_ENODEVICE, (n, M.last_error())
            assert 'no CPU fallback' in M.last_error() and M.lib.mlbp_exactsample_last_kernel() == M.KERNEL_NONE
    a = _listed_args(M, N=4)                                    # without cutset variables configs may be NULL
    a.n_cut, a.n_free = 0, 3
    from macaronicusermodeling_amd import cutset
    words = cutset.plan_words(R._topo(C.chain_spec(3, 4)), [])
    a.P, a.U, a.n_cut, a.n_free, a.n_items, a.n_consts, a.n_forest, a.plan_words = 2, 3, *(int(w) for w in words[3:8]), len(words)
    a.configs = None
    assert call(a) == F.MLBP_ENODEVICE, M.last_error()


def test_n_zero_is_the_exact_call_whatever_the_new_pointers_hold():
    """N == 0: the checks, the error words and the workspace of the exact call, with NULL or junk in configs, log_q, entry, ess."""
    import torch
    M, F = _M(), _ffi()
    call = lambda a: M.lib.mlbp_exactsample_f64(ctypes.byref(a), None)
    for junk in (None, 4096, 12345):
        a = E._valid_args(M)
        assert a.N == 0
        a.configs = a.log_q = a.entry = a.ess = junk
        a.workspace_bytes = M.workspace_bytes(a.B, a.S, a.X, a.n_vars, a.P, a.U, a.n_forest, a.n_cut)
        if not torch.cuda.is_available():
            assert call(a) == F.MLBP_ENODEVICE and 'no CPU fallback' in M.last_error()
        a.workspace_bytes -= 8
        assert call(a) == F.MLBP_EINVAL and 'workspace' in M.last_error()
        a = E._valid_args(M, X=1024, n_cut=2)                   # the exact call's limit, in its words
        a.configs = a.log_q = a.entry = a.ess = junk
        assert call(a) == F.MLBP_EUNSUPPORTED and 'configurations' in M.last_error()
    a = E._valid_args(M, X=1024, n_cut=2)                       # the same plan, listed: no bound on X^|C|
    a.N = 5
    a.workspace_bytes = 1 << 40
    if not torch.cuda.is_available():
        assert call(a) == F.MLBP_ENODEVICE, M.last_error()


def test_the_listed_plan_check_is_the_estimates():
    """A listed call validates its plan through cutsetis.plan: K5 at X = 64 passes there and raises 'configurations' here."""
    from macaronicusermodeling_amd import cutsetis
    M = _M()
    topo = R._topo(R.kn_spec(5, 4))
    with pytest.raises(M.ExactSampleError, match='configurations'):
        M.Plan(topo, [0, 1, 2], 64, None)
    assert cutsetis.Plan(topo, [0, 1, 2], 64, None).n_cut == 3
