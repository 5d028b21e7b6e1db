"""Cutset importance sampling without a GPU: the NumPy statement of include/mlbp_cutsetis.h pinned on exhaustive enumeration,
the C ABI of libmlbp_cutsetis.so, its host functions and the kernel inventory rule applied to the eleventh library.

References.  The statement solves the conditioned forest of one listed entry the way test_cutset_cpu.condition does for every
configuration -- the same breadth-first forest, one pass up, one pass down -- and then states the header: the split of
exp(-log_q) into r 2^k, the weights as (mantissa, exponent) pairs, S1, S2 and the marginal accumulators under the largest
exponent, one logarithm per output.  Enumeration is test_cutset_cpu.enumerate_exact's log-domain grid; nothing of the algorithm
under test is in it.

Lists.  make_list() draws every cutset variable's state from the normalised product of its unary rows (uniform where it has
none) with NumPy from a fixed seed, so log_q is exact on the host.  No test here or in the GPU module asserts a statistical
accuracy: every assertion is a deterministic function of its inputs.  INPUTS lists every input family the GPU module holds
against the statement; test_every_gpu_input_is_finite_where_claimed asserts for each that the outputs are finite where claimed
and that the smallest live term of S1 has not left the range S1 is summed in."""
import ctypes
import functools
import itertools
import os
import re

import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
from conftest import ROOT
from oracle import lbp_oracle as O

LN2 = float(np.log(2.0))
MAX_LISTED = 65536


# ------------------------------------------------------------------------------------------------
# the statement
# ------------------------------------------------------------------------------------------------
def split(log_q):
    """exp(-log_q) = r * 2^k by the header's formula: (r, k)."""
    k = np.rint(-log_q / LN2)
    return np.exp(-log_q - k * LN2), k.astype(np.int64)


class Statement:
    """include/mlbp_cutsetis.h in NumPy for one graph and the cutset `cut` (variable ids; column q of a list is the state of
    cut[q]).  The forest is the one of cutset.plan_words: breadth-first from the lowest free variable of every tree."""

    def __init__(self, g, inputs, cut):
        self.g, self.cut, self.X = g, list(cut), g.X
        self.free = [v for v in g.var_order if v not in self.cut]
        self.facs = R._factor_arrays(g, inputs)
        self.edges = [(vs, T) for vs, T in self.facs if len(vs) == 2 and vs[0] not in self.cut and vs[1] not in self.cut]
        self.parent, self.walk = {}, []
        for root in self.free:
            if root in self.parent:
                continue
            self.parent[root] = None
            queue = [root]
            while queue:
                v = queue.pop(0)
                self.walk.append(v)
                for k, (vs, T) in enumerate(self.edges):
                    if v in vs:
                        w = vs[1] if vs[0] == v else vs[0]
                        if w not in self.parent:
                            self.parent[w] = (v, k)
                            queue.append(w)
        assert len(self.edges) == sum(1 for v in self.free if self.parent[v] is not None), 'the remainder has a cycle'
        self._solved = {}

    def _toward(self, k, frm, vec):
        vs, T = self.edges[k]
        return vec.dot(T) if vs[0] == frm else T.dot(vec)

    def solve(self, states):
        """(Z_c, m_c [n_vars][X] in g.var_order: the conditional marginals of the free variables, the indicator of its state
        for a cutset variable) of the configuration `states` (one state per cut position)."""
        key = tuple(int(s) for s in states)
        if key in self._solved:
            return self._solved[key]
        X, free, parent = self.X, self.free, self.parent
        s = dict(zip(self.cut, key))
        const, phi = 1.0, {v: np.ones(X) for v in free}
        for vs, T in self.facs:
            if len(vs) == 1:
                if vs[0] in s:
                    const = const * T[s[vs[0]]]
                else:
                    phi[vs[0]] = phi[vs[0]] * T
            elif vs[0] in s and vs[1] in s:
                const = const * T[s[vs[0]], s[vs[1]]]
            elif vs[0] in s:
                phi[vs[1]] = phi[vs[1]] * T[s[vs[0]], :]
            elif vs[1] in s:
                phi[vs[0]] = phi[vs[0]] * T[:, s[vs[1]]]
        bel, up, dn = {v: phi[v].copy() for v in free}, {}, {}
        Zc = const
        for v in reversed(self.walk):
            if parent[v] is None:
                Zc = Zc * bel[v].sum()
            else:
                par, k = parent[v]
                up[v] = self._toward(k, v, bel[v])
                bel[par] = bel[par] * up[v]
        for v in self.walk:
            if parent[v] is not None:
                par, k = parent[v]
                excl = phi[par] * (dn[par] if par in dn else 1.0)
                for w in free:
                    if w != v and parent[w] is not None and parent[w][0] == par:
                        excl = excl * up[w]
                dn[v] = self._toward(k, par, excl)
                bel[v] = bel[v] * dn[v]
        m = np.zeros((len(self.g.var_order), X))
        for i, v in enumerate(self.g.var_order):
            if v in s:
                m[i, s[v]] = 1.0
            elif Zc > 0:
                m[i] = bel[v] / bel[v].sum()
        self._solved[key] = (float(Zc), m)
        return self._solved[key]

    def run(self, configs, log_q):
        """The outputs of the header for the list (configs [N][n_cut], log_q [N]): dict(log_z_hat, ess, marg [n_vars][X], log_w
        [N], terms [N]: every entry's share of S1's mantissa, 0 for a dead entry)."""
        configs = np.asarray(configs).reshape(len(log_q), len(self.cut))
        log_q = np.asarray(log_q, dtype=np.float64)
        N, nv, X = len(log_q), len(self.g.var_order), self.X
        rows, index = {}, np.zeros(N, dtype=np.int64)
        for i in range(N):
            index[i] = rows.setdefault(tuple(int(s) for s in configs[i]), len(rows))
        solved = [self.solve(key) for key in rows]
        Zc = np.array([z for z, _ in solved])[index]
        live = Zc > 0
        r, k = split(log_q)
        zm, ze = np.frexp(Zc)                                   # Z_c = zm 2^ze
        wm, we = np.frexp(zm * r)                               # w = wm 2^(we + ze + k)
        e = we + ze + k
        log_w = np.where(live, e * LN2 + np.log(np.where(live, wm, 1.0)), -np.inf)
        if not live.any():
            return dict(log_z_hat=-np.inf, ess=0.0, marg=np.full((nv, X), 1.0 / X), log_w=log_w, terms=np.zeros(N))
        emax = int(e[live].max())
        terms = np.where(live, np.ldexp(wm, np.maximum(e - emax, -4000).astype(np.int64)), 0.0)
        S1, S2 = terms.sum(), (terms * terms).sum()
        acc = np.zeros((nv, X))
        for j, (_, m) in enumerate(solved):
            acc += terms[index == j].sum() * m
        return dict(log_z_hat=float(emax * LN2 + np.log(S1 / N)), ess=float(S1 * S1 / S2), marg=acc / S1, log_w=log_w, terms=terms)


def proposal_rows(g, inputs, cut):
    """[n_cut][X]: per cutset variable the normalised product of its unary rows, uniform where it has none."""
    rows = []
    for v in cut:
        p = np.ones(g.X)
        for vs, T in R._factor_arrays(g, inputs):
            if vs == (v,):
                p = p * T
        rows.append(p / p.sum())
    return rows


def make_list(g, inputs, cut, N, seed):
    """(configs int32 [N][n_cut], log_q float64 [N]): states drawn from proposal_rows, log_q the exact log-probability."""
    rs = np.random.RandomState(seed)
    rows = proposal_rows(g, inputs, cut)
    configs = np.zeros((N, len(cut)), dtype=np.int32)
    log_q = np.zeros(N)
    for q, p in enumerate(rows):
        configs[:, q] = rs.choice(g.X, size=N, p=p)
        log_q += np.log(p[configs[:, q]])
    return configs, log_q


def full_list(X, n_cut):
    """Every configuration once, in the exact libraries' order: configuration c's digit q is the state of cut position q."""
    return np.array([[(c // X ** q) % X for q in range(n_cut)] for c in range(X ** n_cut)], dtype=np.int32).reshape(X ** n_cut, n_cut)


# ------------------------------------------------------------------------------------------------
# the statement against enumeration
# ------------------------------------------------------------------------------------------------
def two_components_spec(X):
    """A triangle 0 - 1 - 2 and, apart from it, the pair 3 - 4."""
    factors = [dict(id=i, vars=[i], dims=[0], table=i) for i in range(5)]
    for k, (a, b) in enumerate(((0, 1), (1, 2), (0, 2), (3, 4))):
        factors.append(dict(id=5 + k, vars=[a, b], dims=[0, 1] if k % 2 else [1, 0], table=5 + k))
    return dict(name='two_components_x%d' % X, style='explicit', X=X, var_ids=list(range(5)), labels=[0] * 5, factors=factors)


SMALL = [('k3', lambda X: R.kn_spec(3, X)), ('k4', lambda X: R.kn_spec(4, X)), ('k5', lambda X: R.kn_spec(5, X)),
         ('k6', lambda X: R.kn_spec(6, X)), ('ring5', lambda X: C.ring_spec(5, X)), ('star4', lambda X: C.star_spec(4, X)),
         ('two_components', two_components_spec)]


@pytest.mark.parametrize('name,make', SMALL, ids=[n for n, _ in SMALL])
@pytest.mark.parametrize('X', [2, 3, 4])
def test_statement_equals_enumeration(name, make, X):
    """ln Z_c of every configuration against the grid with the cutset clamped at 1e-12; sum_c q(c) Z_c / q(c) = Z and
    sum_c Z_c m_c / Z = the enumerated marginals at 1e-10 for a q that is not uniform; the zero-variance proposal."""
    spec = make(X)
    g = O.Graph(spec)
    cut = R.chosen_ids(spec)
    order = list(g.var_order)
    for seed in (1, 2):
        inputs = C.make_inputs(spec, seed, 'lognormal')
        log_z, marg, grid = R.enumerate_exact(g, inputs)
        st = Statement(g, inputs, cut)
        configs = full_list(X, len(cut))
        N = len(configs)
        rows = proposal_rows(g, inputs, cut)
        log_q = np.zeros(N)
        for q in range(len(cut)):
            log_q += np.log(rows[q][configs[:, q]])
        assert abs(np.exp(log_q).sum() - 1) <= 1e-12 and (not cut or np.ptp(log_q) > 1e-3)      # a distribution, not uniform
        out = st.run(configs, log_q)
        # ln Z_c: the grid with the cutset's axes fixed
        for i, c in enumerate(configs):
            ix = tuple(int(c[cut.index(v)]) if v in cut else slice(None) for v in order)
            want = R.logsumexp(np.asarray(grid[ix]))
            assert abs(out['log_w'][i] + log_q[i] - want) <= 1e-12 * max(1.0, abs(want)), (name, X, i)
        # sum_c q(c) w(c) = Z, and the q-weighted weights carry the marginals
        w = np.exp(out['log_w'] - log_z)
        assert abs((np.exp(log_q) * w).sum() - 1) <= 1e-10
        m = sum(np.exp(log_q[i]) * w[i] * st.solve(configs[i])[1] for i in range(N))
        assert np.abs(m - marg).max() <= 1e-10
        # the uniform full list is the exact sum
        uni = st.run(configs, np.full(N, -np.log(N)))
        assert abs(uni['log_z_hat'] - log_z) <= 1e-10 * max(1.0, abs(log_z)) and np.abs(uni['marg'] - marg).max() <= 1e-10
        # q = Z_c / Z: every weight is Z, ess = N -- also for a list that repeats entries
        pick = np.random.RandomState(seed).randint(0, N, size=3 * N + 1)
        zero = st.run(configs[pick], (out['log_w'] + log_q - log_z)[pick])
        assert np.abs(zero['log_w'] - log_z).max() <= 1e-12 * max(1.0, abs(log_z))
        assert abs(zero['ess'] - len(pick)) <= 1e-9 * len(pick) and abs(zero['log_z_hat'] - log_z) <= 1e-10 * max(1.0, abs(log_z))


def test_split_is_the_headers_formula():
    lq = np.array([0.0, -1e-3, -0.3, -0.35, -41.6, 3.0, 700.0, -700.0, 1e6, -1e6])
    r, k = split(lq)
    assert (r >= 2 ** -0.5 - 1e-9).all() and (r <= 2 ** 0.5 + 1e-9).all()
    small = np.abs(lq) < 700
    assert np.allclose(np.ldexp(r[small], k[small]), np.exp(-lq[small]), rtol=1e-12)


def test_repeated_entry_and_dead_entries():
    """One configuration N times: every weight equal, so ess = N and log_z_hat = log_w.  Dead entries add nothing; an all-dead
    list gives -inf, uniform marginals and ess = 0."""
    spec = R.kn_spec(4, 3)
    g, inputs = O.Graph(spec), C.make_inputs(spec, 3, 'lognormal')
    st = Statement(g, inputs, [0, 1])
    out = st.run(np.tile([[2, 1]], (7, 1)), np.full(7, -1.25))
    assert np.ptp(out['log_w']) == 0 and abs(out['ess'] - 7) <= 1e-12 and abs(out['log_z_hat'] - out['log_w'][0]) <= 1e-12
    dead = dead_inputs(spec, 3, (0, 2))
    st = Statement(g, dead, [0, 1])
    configs = np.array([[0, 1], [1, 1], [2, 0], [1, 2]], dtype=np.int32)
    out = st.run(configs, np.full(4, -1.0))
    assert np.isneginf(out['log_w'][[0, 2]]).all() and np.isfinite(out['log_w'][[1, 3]]).all()
    live = st.run(configs[[1, 3]], np.full(2, -1.0))
    assert abs(out['log_z_hat'] - (live['log_z_hat'] + np.log(2.0 / 4.0))) <= 1e-12 and np.abs(out['marg'] - live['marg']).max() <= 1e-15
    none = st.run(configs[[0, 2]], np.full(2, -1.0))
    assert none['log_z_hat'] == -np.inf and none['ess'] == 0.0 and (none['marg'] == 1.0 / 3).all()


# ------------------------------------------------------------------------------------------------
# every input of the GPU module: name -> (spec, [inputs], cutset ids or None, N, seed of the lists)
# ------------------------------------------------------------------------------------------------
def dead_inputs(spec, seed, states, kind='lognormal'):
    """Inputs under which Z_c = 0 exactly where variable 0 takes one of `states`: those entries of a pairwise table on
    variable 0 are zero along variable 0's axis."""
    inputs = C.make_inputs(spec, seed, kind)
    f = [f for f in spec['factors'] if len(f['vars']) == 2 and 0 in f['vars']][0]
    axis = f['dims'][f['vars'].index(0)]
    for s in states:
        if axis == 0:
            inputs['tables'][f['table']][s, :] = 0.0
        else:
            inputs['tables'][f['table']][:, s] = 0.0
    return inputs


def wide_inputs(spec, seed, sigma):
    rs = np.random.RandomState(seed)
    n = 1 + max(f['table'] for f in spec['factors'])
    shape = {f['table']: (spec['X'], spec['X']) if len(f['vars']) == 2 else (spec['X'], 1) for f in spec['factors']}
    return dict(tables=[np.exp(sigma * rs.randn(*shape[t])) for t in range(n)])


def _family(make, seeds, N, kind='lognormal', cutset=None, inputs=None, lists=7):
    spec = make()
    return spec, ([C.make_inputs(spec, s, kind) for s in seeds] if inputs is None else inputs(spec)), cutset, N, lists


INPUTS = {
    'k5_x64': lambda: _family(lambda: R.kn_spec(5, 64), (1, 2, 3), 24),                    # the first shape the exact family refuses
    'k8_x64': lambda: _family(lambda: R.kn_spec(8, 64), (1, 2), 12),                       # six cut positions: 36 bits of configuration
    'k9_x64': lambda: _family(lambda: R.kn_spec(9, 64), (1, 2), 8),                        # the last shape on the X = 64 kernel
    'chain3_x64': lambda: _family(lambda: C.chain_spec(3, 64), (1, 2, 3), 6),              # a tree on the X = 64 kernel: the empty cutset
    'k3_x64': lambda: _family(lambda: R.kn_spec(3, 64), (1, 2, 3, 4), 64),
    'k3_x64_n1': lambda: _family(lambda: R.kn_spec(3, 64), (1, 2), 1),
    'k3_x64_n5': lambda: _family(lambda: R.kn_spec(3, 64), (1, 2), 5),                     # waves without an entry, empty partials
    'k3_x64_b1': lambda: _family(lambda: R.kn_spec(3, 64), (5,), 65536),                   # the longest list
    'k10_x64': lambda: _family(lambda: R.kn_spec(10, 64), (1, 2), 4),                      # X = 64 beyond the LDS rule: generic
    'k5_x7': lambda: _family(lambda: R.kn_spec(5, 7), (1, 2, 3), 64),
    'ring5_x7': lambda: _family(lambda: C.ring_spec(5, 7), (1, 2, 3, 4), 64, kind='uniform'),
    'ring5_x7_n1': lambda: _family(lambda: C.ring_spec(5, 7), (1, 2), 1, kind='uniform'),
    'ring3_x2': lambda: _family(lambda: C.ring_spec(3, 2), (7, 8), 16),
    'ring3_x65': lambda: _family(lambda: C.ring_spec(3, 65), (7, 8), 16),
    'ring3_x257': lambda: _family(lambda: C.ring_spec(3, 257), (7, 8), 16),
    'k3_x1024': lambda: _family(lambda: R.kn_spec(3, 1024), (9,), 2, kind='uniform'),     # vectors in the workspace
    'star4_x9_cut': lambda: _family(lambda: C.star_spec(4, 9), (1, 2, 3), 16, cutset=[2]),  # a branching forest under one cut leaf
    'star4_x9': lambda: _family(lambda: C.star_spec(4, 9), (1, 2, 3), 4),                  # a tree: the empty cutset
    'k3_x64_dead': lambda: _family(lambda: R.kn_spec(3, 64), (1, 2), 48, inputs=lambda s: [dead_inputs(s, 1, range(0, 64, 2)), dead_inputs(s, 2, range(64))]),
    'ring5_x7_dead': lambda: _family(lambda: C.ring_spec(5, 7), (1, 2), 32, inputs=lambda s: [dead_inputs(s, 1, (0, 3, 4)), dead_inputs(s, 2, range(7))]),
    'k3_x64_wide': lambda: _family(lambda: R.kn_spec(3, 64), (21, 22), 32, inputs=lambda s: [wide_inputs(s, k, 20.0) for k in (21, 22)]),
    'ring5_x7_wide': lambda: _family(lambda: C.ring_spec(5, 7), (21, 22), 32, inputs=lambda s: [wide_inputs(s, k, 20.0) for k in (21, 22)]),
}
ALL_DEAD = {'k3_x64_dead': (1,), 'ring5_x7_dead': (1,)}          # graphs whose every entry is dead


@functools.lru_cache(maxsize=None)
def family(name):
    """(spec, [inputs], cutset ids, configs int32 [B][N][n_cut], log_q [B][N], [the statement's outputs per graph]): computed once
    per process and shared; nothing in it is changed by a test."""
    spec, inputs, cutset, N, seed = INPUTS[name]()
    g = O.Graph(spec)
    cut = R.chosen_ids(spec) if cutset is None else list(cutset)
    lists = [make_list(g, i, cut, N, seed + b) for b, i in enumerate(inputs)]
    stated = [Statement(g, i, cut).run(c, lq) for i, (c, lq) in zip(inputs, lists)]
    return spec, inputs, cut, np.stack([c for c, _ in lists]), np.stack([lq for _, lq in lists]), stated


@pytest.mark.parametrize('name', sorted(INPUTS))
def test_every_gpu_input_is_finite_where_claimed(name):
    """No family is left out: log_z_hat, ess, the marginals and every live log_w finite; the marginal rows sum to one; the smallest
    live term of S1 is a positive normal number under S1's exponent -- no live entry is lost to the running exponent."""
    spec, inputs, cut, configs, log_q, stated = family(name)
    assert configs.shape[:2] == log_q.shape and configs.shape[2] == len(cut) and np.isfinite(log_q).all()
    smallest = np.inf
    for b, out in enumerate(stated):
        if b in ALL_DEAD.get(name, ()):
            assert out['log_z_hat'] == -np.inf and out['ess'] == 0.0 and np.isneginf(out['log_w']).all()
            continue
        live = out['terms'] > 0
        assert live.any() and (name.endswith('_dead') or live.all()), (name, b)
        assert np.isfinite(out['log_z_hat']) and 1.0 - 1e-9 <= out['ess'] <= log_q.shape[1] * (1 + 1e-9), (name, b, out['ess'])
        assert np.isfinite(out['marg']).all() and np.abs(out['marg'].sum(axis=1) - 1).max() <= 1e-12
        assert np.isfinite(out['log_w'][live]).all() and np.isneginf(out['log_w'][~live]).all()
        smallest = min(smallest, float(out['terms'][live].min() / out['terms'].sum()))
    print('%s: N = %d, smallest live term of S1 / S1 = %.1e' % (name, log_q.shape[1], smallest))
    assert smallest > 2.0 ** -1000, (name, smallest)


# ------------------------------------------------------------------------------------------------
# C ABI of libmlbp_cutsetis.so
# ------------------------------------------------------------------------------------------------
HEADER = os.path.join(ROOT, 'include', 'mlbp_cutsetis.h')


def _M():
    from macaronicusermodeling_amd import cutsetis
    return cutsetis


def _ffi():
    from macaronicusermodeling_amd import _ffi
    return _ffi


def test_every_declared_symbol_is_exported_and_bound_and_nothing_else():
    """What this library adds to the shared contract (tests/test_side_libraries_cpu.py: the bound functions are the declared
    and the exported ones, the integer constants and the struct are the header's)."""
    from macaronicusermodeling_amd import cutset
    M = _M()
    text = open(HEADER).read()
    assert float(re.search(r'#define MLBP_CUTSETIS_MAX_ABS_LOG_Q (\S+)', text).group(1)) == M.MAX_ABS_LOG_Q
    assert M.MAX_LISTED == MAX_LISTED and M.MIN_WORKGROUPS == cutset.MIN_WORKGROUPS
    for word in ('k = rint(-log_q / ln 2)', 'ess = 0', 'sqrt(1 / ess - 1 / N)', 'consistent, not unbiased', 'n_vars * X + 3', 'n_cut = 0'):
        assert word in text, word                               # what the issue asks the header to state


def _valid_args(M, X=64, n=3, n_cut=None, N=16):
    """Arguments of K_n that pass every host-side check (the pointers are never dereferenced on the host)."""
    from macaronicusermodeling_amd import cutset
    words = cutset.plan_words(R._topo(R.kn_spec(n, 4)), list(range(n - 2 if n_cut is None else n_cut)))
    a = M.CutsetisArgs()
    a.B, a.X, a.n_vars, a.P, a.U, a.N = 2, X, n, n * (n - 1) // 2, n, N
    a.n_cut, a.n_free, a.n_items, a.n_consts, a.n_forest = (int(w) for w in words[3:8])
    a.n_pair_tables, a.n_unary_tables, a.plan_words = 2 * a.P, 2 * a.U, len(words)
    for name, typ in M.CutsetisArgs._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, name, 4096)
    a.workspace_bytes = 1 << 40
    return a


def test_library_identity_and_bad_arguments():
    M, E_ = _M(), _ffi()
    assert M.lib.mlbp_cutsetis_arch() == b'gfx950'
    assert M.lib.mlbp_cutsetis_f64(None, None) == E_.MLBP_EINVAL and 'NULL' in M.last_error()
    for field, value, word in (('B', 0, 'sizes'), ('X', 1, 'two states'), ('n_free', 0, 'sizes'), ('N', 0, 'list'), ('N', 65537, 'list'), ('N', -1, 'list'),
                               ('plan', None, 'plan'), ('plan_words', 5, 'plan'), ('pair_tab', None, 'pair_tab'), ('n_unary_tables', 0, 'unary_tables'),
                               ('configs', None, 'configs'), ('log_q', None, 'log_q'), ('log_z_hat', None, 'log_z_hat'), ('marginals', None, 'marginals'),
                               ('ess', None, 'ess'), ('labels', None, 'labels'), ('workspace', None, 'workspace'), ('workspace_bytes', 8, 'workspace')):
        a = _valid_args(M)
        setattr(a, field, value)
        assert M.lib.mlbp_cutsetis_f64(ctypes.byref(a), None) == E_.MLBP_EINVAL, field
        assert word in M.last_error(), (field, M.last_error())
        assert M.lib.mlbp_cutsetis_last_kernel() == M.KERNEL_NONE
    a = _valid_args(M, X=1025)
    assert M.lib.mlbp_cutsetis_f64(ctypes.byref(a), None) == E_.MLBP_EUNSUPPORTED and '1024' in M.last_error()
    a = _valid_args(M, n=19, n_cut=17)
    assert M.lib.mlbp_cutsetis_f64(ctypes.byref(a), None) == E_.MLBP_EUNSUPPORTED and 'at most 16' in M.last_error()
    with pytest.raises(M.CutsetisError):
        M.check(E_.MLBP_EINVAL)


def test_compute_entry_fails_loudly_without_a_gpu():
    """After its argument checks: shapes the exact libraries refuse (K5, K8 at X = 64, K3 at X = 1024 squared) get this far."""
    import torch
    M = _M()
    if torch.cuda.is_available():
        return                                                  # (the GPU module runs the entry for real)
    for X, n, N in ((64, 3, 1), (64, 5, 16), (64, 8, 65536), (64, 10, 4), (7, 5, 64), (1024, 4, 2)):
        a = _valid_args(M, X=X, n=n, N=N)
        a.configs = 4096 if n > 2 else None
        assert M.lib.mlbp_cutsetis_f64(ctypes.byref(a), None) == _ffi().MLBP_ENODEVICE, (X, n, N, M.last_error())
        assert 'no CPU fallback' in M.last_error() and M.lib.mlbp_cutsetis_last_kernel() == M.KERNEL_NONE
    a = _valid_args(M, n=3, n_cut=0)                            # a cyclic remainder is the plan check's to refuse; n_cut = 0 needs no configs
    a.configs = None
    assert M.lib.mlbp_cutsetis_f64(ctypes.byref(a), None) == _ffi().MLBP_ENODEVICE


def test_check_plan_is_the_shared_check_without_the_configuration_bound():
    from macaronicusermodeling_amd import cutset as S
    M, E_ = _M(), _ffi()
    topo = R._topo(R.kn_spec(4, 4))
    good = S.plan_words(topo, [0, 1])
    ring = S.plan_words(R._topo(C.ring_spec(5, 4)), [])
    bad = good.copy()
    bad[S.PLAN_HEADER] = 9
    for words, X in ((good, 4), (good, 64), (good, 1), (good[:-1], 4), (ring, 4), (bad, 4), (S.plan_words(topo, [0]), 4), (good, 1025)):
        w = np.ascontiguousarray(words, dtype=np.int32)
        rc = M.lib.mlbp_cutsetis_check_plan(E_.i32ptr(w), len(w), X)
        assert rc == S.lib.mlbp_cutset_check_plan(E_.i32ptr(w), len(w), X)
        if rc:
            assert M.last_error() == S.last_error() and M.last_error()
    # what the exact libraries refuse for their size and this one takes
    for n in (5, 8, 12):
        words = S.plan_words(R._topo(R.kn_spec(n, 4)), list(range(n - 2)))
        w = np.ascontiguousarray(words, dtype=np.int32)
        assert S.lib.mlbp_cutset_check_plan(E_.i32ptr(w), len(w), 64) == E_.MLBP_EUNSUPPORTED and 'configurations' in S.last_error()
        assert M.lib.mlbp_cutsetis_check_plan(E_.i32ptr(w), len(w), 64) == E_.MLBP_OK, M.last_error()
        M.check_plan(words, 1024)
    w = np.ascontiguousarray(S.plan_words(R._topo(R.kn_spec(19, 2)), list(range(17))), dtype=np.int32)
    assert M.lib.mlbp_cutsetis_check_plan(E_.i32ptr(w), len(w), 2) == E_.MLBP_EUNSUPPORTED and 'at most 16' in M.last_error()
    assert S.lib.mlbp_cutset_check_plan(E_.i32ptr(w), len(w), 2) == E_.MLBP_EUNSUPPORTED and 'configurations' in S.last_error()
    w = np.ascontiguousarray(S.plan_words(R._topo(R.kn_spec(18, 2)), list(range(16))), dtype=np.int32)
    assert M.lib.mlbp_cutsetis_check_plan(E_.i32ptr(w), len(w), 2) == E_.MLBP_OK
    assert M.lib.mlbp_cutsetis_check_plan(None, 16, 4) == E_.MLBP_EINVAL and 'NULL' in M.last_error()
    with pytest.raises(M.CutsetisError, match='cycle'):
        M.Plan(R._topo(C.ring_spec(5, 4)), [], 4, None)
    with pytest.raises(M.CutsetisError, match='cycle'):
        M.Plan(R._topo(R.kn_spec(5, 4)), [0, 1], 64, None)
    with pytest.raises(ValueError):
        M.Plan(topo, [0, 0], 4, None)
    big = M.plan(R._topo(R.kn_spec(12, 4)), None, 64, None)
    assert big.n_cut == 10 and big.n_configs == 64 ** 10
    assert M.plan(topo, [0, 1], 4, None) is M.plan(topo, [0, 1], 4, None) is not S.plan(topo, [0, 1], 4, None)


def ints(P, U):
    return 4 * ((P + U + 16 + 3) // 4 * 4)


def kn_shape(n, X=64):
    return (X, n, n * (n - 1) // 2, n, 1)


def test_kernel_choice_chunks_and_workspace_are_the_rules_of_the_header():
    from macaronicusermodeling_amd import cutset as S
    M, E_ = _M(), _ffi()

    def vectors(n_vars, X):
        return (5 * n_vars + 2) * ((X + 1) // 2 * 2) * 8

    def rule(X, n_vars, P, U, n_forest):
        return M.KERNEL_X64 if X == 64 and n_forest * 33280 + 21 * n_vars * 512 + 64 + ints(P, U) <= S.X64_LDS_BYTES else M.KERNEL_GENERIC

    def in_workspace(X, n_vars, P, U, n_forest):
        return rule(X, n_vars, P, U, n_forest) == M.KERNEL_GENERIC and vectors(n_vars, X) + 64 + ints(P, U) > S.GENERIC_LDS_BYTES

    def chunks(B, N):
        return min(N, -(-M.MIN_WORKGROUPS // B))
    shapes = tuple(kn_shape(n) for n in range(3, 13)) + ((64, 3, 2, 3, 2), (64, 4, 3, 4, 3), (63, 3, 3, 3, 1), (2, 260, 259, 260, 259), (257, 3, 3, 3, 1),
                                                         (1024, 3, 3, 3, 1), (7, 5, 5, 5, 3), (7, 5, 10, 5, 1), (9, 5, 4, 4, 3))
    for shape in shapes:
        assert M.pick_kernel(*shape) == rule(*shape) == S.pick_kernel(*shape), shape
    assert M.pick_kernel(*kn_shape(9)) == M.KERNEL_X64 and M.pick_kernel(*kn_shape(10)) == M.KERNEL_GENERIC      # both sides of the LDS rule
    assert M.lib.mlbp_cutsetis_pick_kernel(1025, 3, 3, 3, 1) == E_.MLBP_EUNSUPPORTED
    assert M.lib.mlbp_cutsetis_pick_kernel(1, 3, 3, 3, 1) == E_.MLBP_EINVAL
    for B, N in ((1, 64), (1, 65536), (2, 4096), (3, 64), (8192, 64), (600, 64), (600, 7), (256, 3), (511, 4), (512, 4), (1, 1), (9, 65536), (1024, 1024)):
        assert M.chunks(B, N) == chunks(B, N) == S.chunks(B, N), (B, N)
    for B, N in ((0, 1), (1, 0), (1, MAX_LISTED + 1), (1, -3)):
        assert M.lib.mlbp_cutsetis_chunks(B, N) == E_.MLBP_EINVAL and 'N' in M.last_error()
        assert M.lib.mlbp_cutsetis_workspace_bytes(B, 64, 3, 3, 3, 1, N) == E_.MLBP_EINVAL
    assert not in_workspace(*kn_shape(10)) and in_workspace(1024, 3, 3, 3, 1) and in_workspace(*kn_shape(12, 1024))
    for B in (1, 3, 8192):
        for shape in shapes:
            X, n_vars, P, U, n_forest = shape
            for N in (1, 5, 64, 65536):
                per = n_vars * X + 3
                want = B * chunks(B, N) * (4 * per if rule(*shape) == M.KERNEL_X64 else per + (vectors(n_vars, X) // 8 if in_workspace(*shape) else 0))
                assert M.workspace_bytes(B, X, n_vars, P, U, n_forest, N) == want * 8, (B, shape, N)
    assert M.workspace_bytes(8192, 1024, 40, 39, 40, 39, 65536) > 2 ** 31                      # 64-bit


# ------------------------------------------------------------------------------------------------
# kernel inventory: tests/test_side_libraries_cpu.py holds the shared rule; what the eleventh library added to it
# ------------------------------------------------------------------------------------------------
def test_cutsetis_library_kernels_are_the_sources_kernels_and_each_has_a_case():
    import test_gpu_cutsetis as G
    assert set(G.INPUTS_USED) == set(INPUTS), set(G.INPUTS_USED) ^ set(INPUTS)       # every input compared there is checked here


def test_the_other_libraries_hold_no_cutsetis_kernel_and_the_sources_stay_apart():
    pkg = os.path.join(ROOT, 'macaronicusermodeling_amd')
    for shared in ('mlbp_cutset_plan.h', 'mlbp_cutset_walk.h'):
        assert '__global__' not in open(os.path.join(pkg, 'csrc', shared)).read()      # helpers only
