"""Exact posterior sampling by cutset conditioning without a GPU: the NumPy statement of include/mlbp_exactsample.h pinned on
exhaustive enumeration, the margin that makes a draw comparable, the C ABI of libmlbp_exactsample.so and the kernel inventory
rule applied to the ninth library.

The statement.  Statement(g, inputs, cut) conditions on every joint state of the cutset and keeps every Z_c; walk() draws the
configuration from the SEGMENTED prefix sums of the header and the free variables from the roots down (the forest is the one
of cutset.plan_words: breadth-first from the lowest free variable of every tree, so the k-th free variable of the reverse
`order` is the k-th of that walk); forced() returns log p(x) of a given assignment by the same factors.  Nothing is rescaled:
the header's rescaling is by powers of two and changes no ratio.  The statement's prefix sums over a variable's states are the
plain running sum; the X = 64 kernel's WAVE order differs from it by roundings, which is what the margin is for.

The margin.  A draw lands where the prefix sums cross t = u * total; its margin is min_i |A_i - t| / total.  Samples are
compared exactly only where every draw of the (graph, sample) pair has a margin of at least MARGIN = 1e-8 -- the value and the
reasoning of tests/test_gpu_sample.py: two decades above the 1e-10 the sums are held to, and one differing draw changes every
later one.  The cap on left-out pairs is 0: INPUTS lists every input of the GPU module whose samples are compared with the
statement's, and test_every_gpu_input_has_its_margin asserts the margin for all of them here, before any device is involved;
the seeds were chosen so that it holds.  (The dyadic inputs sit ON the boundaries on purpose: there every sum is exact in any
order, which test_the_dyadic_inputs_are_exact asserts instead.)"""
import ctypes
import functools
import itertools
import os

import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_map_cpu as W
from conftest import ROOT
from oracle import lbp_oracle as O

MARGIN = 1e-8
MAY_OMIT = 0


# ------------------------------------------------------------------------------------------------
# the statement
# ------------------------------------------------------------------------------------------------
def prefix(a):
    """The SEGMENTED inclusive prefix sums of the header: segments of L = ceil(n / 256), each added left to right on top of
    the running sum of the segments before it.  For n <= 256 the plain running sum."""
    a = np.asarray(a, dtype=np.float64)
    n = len(a)
    L = -(-n // 256)
    n_seg = -(-n // L)
    padded = np.zeros(n_seg * L)
    padded[:n] = a
    local = np.cumsum(padded.reshape(n_seg, L), axis=1)
    off = np.concatenate([[0.0], np.cumsum(local[:, -1])[:-1]])
    return (off[:, None] + local).reshape(-1)[:n]


def draw(a, u):
    """The draw rule of the header on weights a with uniform u: (index, a[index] / total, margin)."""
    a = np.asarray(a, dtype=np.float64)
    A = prefix(a)
    total = A[-1]
    t = u * total
    live = a > 0
    cross = np.nonzero((A > t) & live)[0]
    x = int(cross[0]) if len(cross) else int(np.nonzero(live)[0][-1])
    return x, a[x] / total, float(np.abs(A - t).min() / total)


class Statement:
    """include/mlbp_exactsample.h in NumPy for one graph and the cutset `cut` (variable ids; digit q of a configuration is
    the state of cut[q])."""

    def __init__(self, g, inputs, cut):
        self.g, self.cut, self.X, self.order = g, list(cut), g.X, list(g.var_order)
        X = self.X
        self.free = [v for v in self.order if v not in self.cut]
        self.facs = R._factor_arrays(g, inputs)
        self.edges = [(vs, T) for vs, T in self.facs if len(vs) == 2 and vs[0] not in self.cut and vs[1] not in self.cut]
        self.parent, self.walk_order = {}, []
        for root in self.free:                                  # breadth-first over every tree of the remainder
            if root in self.parent:
                continue
            self.parent[root] = None
            queue = [root]
            while queue:
                v = queue.pop(0)
                self.walk_order.append(v)
                for k, (vs, T) in enumerate(self.edges):
                    if v in vs:
                        w = vs[1] if vs[0] == v else vs[0]
                        if w not in self.parent:
                            self.parent[w] = (v, k)
                            queue.append(w)
        assert len(self.edges) == sum(1 for v in self.free if self.parent[v] is not None), 'the remainder has a cycle'
        self.n_configs = X ** len(self.cut)
        with np.errstate(invalid='ignore', over='ignore'):
            self.w = np.array([self.up(c)[0] for c in range(self.n_configs)])
            self.W = prefix(self.w)
        self.Z = self.W[-1]
        self.usable = bool(np.isfinite(self.Z) and self.Z > 0)
        with np.errstate(divide='ignore', invalid='ignore'):
            self.log_z = float(np.log(self.Z))

    def states(self, c):
        return {v: (c // self.X ** q) % self.X for q, v in enumerate(self.cut)}

    def up(self, c):
        """(Z_c, every free variable's vector on the way up) under configuration c."""
        s = self.states(c)
        const, bel = 1.0, {v: np.ones(self.X) for v in self.free}
        for vs, T in self.facs:
            if len(vs) == 1:
                if vs[0] in s:
                    const = const * T[s[vs[0]]]
                else:
                    bel[vs[0]] = bel[vs[0]] * T
            elif vs[0] in s and vs[1] in s:
                const = const * T[s[vs[0]], s[vs[1]]]
            elif vs[0] in s:
                bel[vs[1]] = bel[vs[1]] * T[s[vs[0]], :]
            elif vs[1] in s:
                bel[vs[0]] = bel[vs[0]] * T[:, s[vs[1]]]
        Zc = const
        for v in reversed(self.walk_order):                     # leaves to roots
            if self.parent[v] is None:
                Zc = Zc * bel[v].sum()
            else:
                par, k = self.parent[v]
                vs, T = self.edges[k]
                bel[par] = bel[par] * (bel[v].dot(T) if vs[0] == v else T.dot(bel[v]))
        return Zc, bel

    def vector(self, v, bel, x):
        """b of the header for free variable v, its parent (if any) drawn already."""
        if self.parent[v] is None:
            return bel[v]
        par, k = self.parent[v]
        vs, T = self.edges[k]
        return bel[v] * (T[:, x[par]] if vs[0] == v else T[x[par], :])

    def walk(self, uniforms):
        """uniforms: [n_vars] -> dict(x {v: state} or None, logp, margin [per draw])."""
        if not self.usable:
            return dict(x=None, logp=float('nan'), margin=[])
        margins, logp, c = [], 0.0, 0
        if self.cut:
            c, p, m = draw(self.w, uniforms[0])
            margins.append(m)
            logp = float(np.log(p))
        x = self.states(c)
        bel = self.up(c)[1]
        for k, v in enumerate(self.walk_order):                 # roots to leaves: every variable after its parent
            x[v], p, m = draw(self.vector(v, bel, x), uniforms[len(self.cut) + k])
            margins.append(m)
            logp += float(np.log(p))
        return dict(x=x, logp=logp, margin=margins)

    def forced(self, x):
        """log p(x) of the assignment x {v: state} by the factors the walk would have used."""
        c = sum(x[v] * self.X ** q for q, v in enumerate(self.cut))
        with np.errstate(divide='ignore'):
            logp = float(np.log(self.w[c] / self.W[-1])) if self.cut else 0.0
            bel = self.up(c)[1]
            for v in self.walk_order:
                b = self.vector(v, bel, x)
                logp += float(np.log(b[x[v]] / prefix(b)[-1]))
        return logp


def statement(spec, inputs, cut=None):
    return Statement(O.Graph(spec), inputs, R.chosen_ids(spec) if cut is None else cut)


# ------------------------------------------------------------------------------------------------
# every input of the GPU module whose samples are compared with the statement's:
# name -> (spec, table kind, table seeds, cutset ids or None, S, seed of the uniforms)
# ------------------------------------------------------------------------------------------------
INPUTS = {
    'k3_x64': (lambda: R.kn_spec(3, 64), 'uniform', range(5), None, 4, 0),
    'k3_x64_lognormal': (lambda: R.kn_spec(3, 64), 'lognormal', range(2), None, 3, 1),
    'k4_x64': (lambda: R.kn_spec(4, 64), 'lognormal', (1, 2), None, 3, 2),
    'chain3_x64': (lambda: C.chain_spec(3, 64), 'uniform', (1, 2), None, 3, 3),
    'chain3_x64_cut1': (lambda: C.chain_spec(3, 64), 'uniform', (1, 2), [1], 3, 3),
    'chain4_x64': (lambda: C.chain_spec(4, 64), 'uniform', (1, 2), None, 2, 4),
    'ring3_x2': (lambda: C.ring_spec(3, 2), 'uniform', (7, 8, 9), None, 3, 5),
    'ring3_x5': (lambda: C.ring_spec(3, 5), 'uniform', (7, 8, 9), None, 3, 6),
    'ring3_x65': (lambda: C.ring_spec(3, 65), 'uniform', (7, 8, 9), None, 3, 7),
    'ring5_x7': (lambda: C.ring_spec(5, 7), 'uniform', range(4), None, 3, 8),
    'k3_x128': (lambda: R.kn_spec(3, 128), 'uniform', (1, 2), None, 2, 9),
    'k3_x1024': (lambda: R.kn_spec(3, 1024), 'uniform', (9,), None, 1, 10),
    'chain260_x2': (lambda: C.chain_spec(260, 2), 'uniform', (1, 2), None, 2, 11),
    'chain5_x8': (lambda: C.chain_spec(5, 8), 'uniform', (1, 2, 3), None, 3, 12),
    'chain5_x8_cut2': (lambda: C.chain_spec(5, 8), 'uniform', (1, 2, 3), [2, 0], 3, 12),
    'star4_x8': (lambda: C.star_spec(4, 8), 'uniform', (1, 2, 3), None, 3, 13),
    'forest_x9': (lambda: R.forest_spec(9), 'uniform', (3, 4, 5), None, 3, 14),
    'double_pair_x6': (lambda: R.double_pair_spec(6), 'uniform', (3, 4, 5), None, 3, 15),
    'shuffled_x5': (lambda: C.shuffled_ids_spec(5), 'uniform', (3, 4, 5), None, 3, 16),
}


@functools.lru_cache(maxsize=None)
def family(name):
    """(spec, [inputs], cutset ids or None, uniforms [S][B][n_vars], {(s, b): walk}, [Statement per graph]) of INPUTS[name]:
    computed once per process and shared."""
    make, kind, seeds, cut, S, u_seed = INPUTS[name]
    spec = make()
    inputs = [C.make_inputs(spec, s, kind) for s in seeds]
    uniforms = np.random.RandomState(1000 + u_seed).rand(S, len(inputs), len(spec['var_ids']))
    stmts = [statement(spec, i, cut) for i in inputs]
    walks = {(s, b): stmts[b].walk(uniforms[s, b]) for s in range(S) for b in range(len(inputs))}
    return spec, inputs, cut, uniforms, walks, stmts


def smallest_margin(walks):
    return min([np.inf] + [m for w in walks.values() for m in w['margin']])


def check_margin(name, walks):
    """The rule of tests/test_gpu_sample.py: no (graph, sample) pair is left out."""
    omitted = sum(1 for w in walks.values() if w['margin'] and min(w['margin']) < MARGIN)
    smallest = smallest_margin(walks)
    print('%s: %d (graph, sample) pairs, %d draws, smallest margin of the statement %.2e, %d pairs left out (cap %d)'
          % (name, len(walks), sum(len(w['margin']) for w in walks.values()), smallest, omitted, MAY_OMIT))
    assert omitted <= MAY_OMIT and smallest >= MARGIN, (name, smallest)


@pytest.mark.parametrize('name', sorted(INPUTS))
def test_every_gpu_input_has_its_margin(name):
    assert MARGIN == 1e-8 and MAY_OMIT == 0
    _, _, _, _, walks, stmts = family(name)
    assert all(s.usable for s in stmts)
    check_margin(name, walks)


def dyadic_inputs(X):
    """K3 (cutset [0]) on tables whose entries are 0, 1, 2 or 4 and whose totals are powers of two: every sum and product of
    the walk is exact in any order.  The cutset variable's weights are [1, 0, 2, 1, 0 ...]: prefix sums / total = 1/4, 1/4,
    3/4, 1; the root (variable 1) has [0, 2, 1, 1, 0 ...] and the leaf (variable 2) [1, 1, 0, 2, 0 ...] whatever its parent."""
    spec = R.kn_spec(3, X)
    tables = [np.ones((X, X)) if len(f['vars']) == 2 else np.zeros((X, 1)) for f in sorted(spec['factors'], key=lambda f: f['table'])]
    tables[0][:4, 0] = [1, 0, 2, 1]
    tables[1][:4, 0] = [0, 2, 1, 1]
    tables[2][:4, 0] = [1, 1, 0, 2]
    # [S][n_vars]: on a boundary (the rule is A_i > t: the next index), at zero, just below a boundary, the zero-weight
    # index skipped, and u = 1 (outside the contract: none crosses, the highest index of positive weight)
    uniforms = np.array([[0.25, 0.5, 0.5], [0.0, 0.0, 0.0], [0.75, 0.75, 0.25], [0.25 - 2.0 ** -54, 0.5 - 2.0 ** -54, 0.5 - 2.0 ** -54],
                         [0.5, 0.25, 0.75], [1.0, 1.0, 1.0]])
    want = [[2, 2, 3], [0, 1, 0], [3, 3, 1], [0, 1, 1], [2, 1, 3], [3, 3, 3]]
    return spec, dict(tables=tables), uniforms, want


@pytest.mark.parametrize('X', [4, 5, 64])
def test_the_dyadic_inputs_are_exact(X):
    """The boundary, zero-weight and fallback rules on the statement; logp is the logarithm of a product of dyadic numbers."""
    spec, inputs, uniforms, want = dyadic_inputs(X)
    st = statement(spec, inputs)
    assert st.cut == [0] and st.walk_order == [1, 2]
    assert np.array_equal(st.W / st.W[-1], np.concatenate([[0.25, 0.25, 0.75], np.ones(X - 3)]))
    probs = [np.array([1, 0, 2, 1]) / 4.0, np.array([0, 2, 1, 1]) / 4.0, np.array([1, 1, 0, 2]) / 4.0]
    for u, x in zip(uniforms, want):
        w = st.walk(u)
        assert [w['x'][v] for v in st.order] == x, (u, w['x'])
        assert w['logp'] == sum(np.log(probs[i][x[i]]) for i in range(3))
        assert all(p[x[i]] > 0 for i, p in enumerate(probs))     # a zero-weight configuration or state is never drawn
    assert min(st.walk(uniforms[0])['margin']) == 0.0            # on the boundary
    assert draw([1, 2, 0], 1.0)[0] == 1 and draw([0, 0, 4, 0], 0.0)[0] == 2 and draw([1, 1], 0.5)[0] == 1


# ------------------------------------------------------------------------------------------------
# the statement against exhaustive enumeration
# ------------------------------------------------------------------------------------------------
SMALL = [('k3', lambda X: R.kn_spec(3, X)), ('k4', lambda X: R.kn_spec(4, X)), ('ring5', lambda X: C.ring_spec(5, X)),
         ('tree', lambda X: C.star_spec(4, X)), ('two_components', lambda X: R.forest_spec(X))]


@pytest.mark.parametrize('X', [2, 3, 4])
@pytest.mark.parametrize('name,make', SMALL, ids=[s[0] for s in SMALL])
def test_forced_logp_equals_enumeration(name, make, X):
    """log p(x) of EVERY assignment at 1e-12, exp(logp) sums to 1, and a drawn assignment's logp is its forced logp."""
    spec = make(X)
    g = O.Graph(spec)
    for kind, seed in (('uniform', 3), ('lognormal', 4)):
        inputs = C.make_inputs(spec, seed, kind)
        _, _, grid = W.brute_force(g, inputs)
        log_z = R.logsumexp(grid)
        st = statement(spec, inputs)
        assert abs(st.log_z - log_z) <= 1e-12 * max(1.0, abs(log_z))
        total, worst = 0.0, 0.0
        for a in itertools.product(range(X), repeat=len(g.var_order)):
            want = grid[a] - log_z
            got = st.forced(dict(zip(g.var_order, a)))
            worst = max(worst, abs(got - want) / max(1.0, abs(want)))
            total += np.exp(got)
        print('%s X = %d %s: %d assignments, forced logp within %.1e of enumeration, sum of p %.15f' % (name, X, kind, X ** len(g.var_order), worst, total))
        assert worst <= 1e-12 and abs(total - 1.0) <= 1e-12
        rs = np.random.RandomState(seed)
        for _ in range(8):
            w = st.walk(rs.rand(len(g.var_order)))
            assert abs(w['logp'] - st.forced(w['x'])) <= 1e-13 * max(1.0, abs(w['logp']))
            want = grid[tuple(w['x'][v] for v in g.var_order)] - log_z
            assert abs(w['logp'] - want) <= 1e-12 * max(1.0, abs(want))


def test_any_valid_cutset_gives_the_same_logp():
    spec = R.kn_spec(3, 4)
    g, inputs = O.Graph(spec), C.make_inputs(spec, 8)
    base = statement(spec, inputs)
    for cut in ([0], [1], [2], [0, 1], [2, 0], [0, 1, 2]):
        st = Statement(g, inputs, cut)
        for a in itertools.product(range(4), repeat=3):
            x = dict(zip(g.var_order, a))
            assert abs(st.forced(x) - base.forced(x)) <= 1e-12 * max(1.0, abs(base.forced(x))), (cut, a)
    spec = C.chain_spec(4, 3)
    g, inputs = O.Graph(spec), C.make_inputs(spec, 9)
    for a in itertools.product(range(3), repeat=4):
        x = dict(zip(g.var_order, a))
        assert abs(Statement(g, inputs, []).forced(x) - Statement(g, inputs, [2]).forced(x)) <= 1e-12


def test_the_draws_follow_the_model():
    """Not a proof -- the identity above is -- but a statement that drew from another distribution with the right logp would
    pass everything else: 20000 draws of K3 at X = 2 against the enumerated probabilities, at five standard deviations."""
    spec = R.kn_spec(3, 2)
    g, inputs = O.Graph(spec), C.make_inputs(spec, 5)
    _, _, grid = W.brute_force(g, inputs)
    p = np.exp(grid - R.logsumexp(grid))
    st = statement(spec, inputs)
    rs = np.random.RandomState(0)
    n, counts = 20000, np.zeros_like(p)
    for _ in range(n):
        w = st.walk(rs.rand(3))
        counts[tuple(w['x'][v] for v in g.var_order)] += 1
    assert (np.abs(counts / n - p) <= 5 * np.sqrt(p * (1 - p) / n)).all()


def test_the_segmented_prefix_sums():
    rs = np.random.RandomState(1)
    for n in (1, 2, 64, 256, 257, 4096, 65536):
        a = rs.rand(n)
        A = prefix(a)
        assert len(A) == n and (np.diff(A) >= 0).all() and abs(A[-1] - a.sum()) <= 1e-12 * a.sum()
        if n <= 256:
            assert np.array_equal(A, np.cumsum(a))
    a = np.zeros(600)
    a[[3, 599]] = 1.0
    assert np.array_equal(prefix(a), np.concatenate([np.zeros(3), np.ones(596), [2.0]]))


def test_bad_graphs_are_refused_by_the_statement():
    spec = C.ring_spec(5, 3)
    pair = next(f['table'] for f in spec['factors'] if len(f['vars']) == 2)
    for value in (0.0, np.nan, np.inf):
        inputs = C.make_inputs(spec, 1)
        if value == 0.0:
            inputs['tables'][pair][:] = 0.0
        else:
            inputs['tables'][pair][1, 2] = value
        st = statement(spec, inputs)
        w = st.walk(np.full(5, 0.5))
        assert not st.usable and w['x'] is None and np.isnan(w['logp'])
        assert st.log_z == -np.inf if value == 0.0 else not np.isfinite(st.log_z)


# ------------------------------------------------------------------------------------------------
# C ABI of libmlbp_exactsample.so
# ------------------------------------------------------------------------------------------------
HEADER = os.path.join(ROOT, 'include', 'mlbp_exactsample.h')


def _M():
    from macaronicusermodeling_amd import exactsample
    return exactsample


def _ffi():
    from macaronicusermodeling_amd import _ffi
    return _ffi


def test_every_declared_symbol_is_exported_and_bound_and_nothing_else():
    """What this library adds to the shared contract (tests/test_side_libraries_cpu.py: the bound functions are the declared
    and the exported ones, the constants and the struct are the header's)."""
    text = open(HEADER).read()
    for word in ('given=', 'float32', 'grouped', 'MLBP_CUTSET_MAX_CONFIGS'):      # the "not done" list
        assert word in text[text.index('Not done'):text.index('#ifndef')], word


def _valid_args(M, X=64, n_cut=1):
    """Arguments of K3 that pass every host-side check (the pointers are never dereferenced on the host)."""
    from macaronicusermodeling_amd import cutset
    words = cutset.plan_words(R._topo(R.kn_spec(3, 4)), list(range(n_cut)))
    a = M.ExactSampleArgs()
    a.B, a.X, a.n_vars, a.P, a.U, a.S = 2, X, 3, 3, 3, 5
    a.n_cut, a.n_free, a.n_items, a.n_consts, a.n_forest = (int(w) for w in words[3:8])
    a.n_pair_tables, a.n_unary_tables, a.plan_words = 6, 6, len(words)
    for name, typ in M.ExactSampleArgs._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, name, 4096)
    a.workspace_bytes = 1 << 40
    return a


def test_library_identity_and_bad_arguments():
    M, E = _M(), _ffi()
    assert M.lib.mlbp_exactsample_arch() == b'gfx950'
    assert M.lib.mlbp_exactsample_f64(None, None) == E.MLBP_EINVAL and 'NULL' in M.last_error()
    for field, value, word in (('B', 0, 'sizes'), ('X', 1, 'two states'), ('n_free', 1, 'sizes'), ('S', 0, 'sizes'), ('plan', None, 'plan'),
                               ('plan_words', 5, 'plan'), ('pair_tab', None, 'pair_tab'), ('n_unary_tables', 0, 'unary_tables'),
                               ('uniforms', None, 'uniforms'), ('samples', None, 'samples'), ('logp', None, 'logp'),
                               ('workspace', None, 'workspace'), ('workspace_bytes', 8, 'workspace')):
        a = _valid_args(M)
        setattr(a, field, value)
        assert M.lib.mlbp_exactsample_f64(ctypes.byref(a), None) == E.MLBP_EINVAL, field
        assert word in M.last_error(), (field, M.last_error())
        assert M.lib.mlbp_exactsample_last_kernel() == M.KERNEL_NONE
    a = _valid_args(M, X=1025)
    assert M.lib.mlbp_exactsample_f64(ctypes.byref(a), None) == E.MLBP_EUNSUPPORTED and '1024' in M.last_error()
    a = _valid_args(M, X=1024, n_cut=2)
    assert M.lib.mlbp_exactsample_f64(ctypes.byref(a), None) == E.MLBP_EUNSUPPORTED and 'configurations' in M.last_error()
    with pytest.raises(M.ExactSampleError):
        M.check(E.MLBP_EINVAL)


def test_compute_entry_fails_loudly_without_a_gpu():
    import torch
    M = _M()
    if torch.cuda.is_available():
        return                                                  # (the GPU module runs the entry for real)
    for X in (64, 128, 1024):
        for opt in (4096, None):                                # log_z and score are optional
            a = _valid_args(M, X=X)
            a.log_z = a.score = opt
            assert M.lib.mlbp_exactsample_f64(ctypes.byref(a), None) == _ffi().MLBP_ENODEVICE
            assert 'no CPU fallback' in M.last_error() and M.lib.mlbp_exactsample_last_kernel() == M.KERNEL_NONE


def test_check_plan_is_the_shared_check():
    """The plan's validation is stated once (csrc/mlbp_cutset_plan.h): the libraries refuse the same plans in the same words."""
    from macaronicusermodeling_amd import cutset as S
    M, E = _M(), _ffi()
    topo = R._topo(R.kn_spec(4, 4))
    good = S.plan_words(topo, [0, 1])
    ring = S.plan_words(R._topo(C.ring_spec(5, 4)), [])
    bad = good.copy()
    bad[S.PLAN_HEADER] = 9
    for words, X in ((good, 4), (good, 64), (good, 1024), (good, 1), (good[:-1], 4), (ring, 4), (bad, 4), (S.plan_words(topo, [0]), 4)):
        w = np.ascontiguousarray(words, dtype=np.int32)
        rc = M.lib.mlbp_exactsample_check_plan(E.i32ptr(w), len(w), X)
        assert rc == S.lib.mlbp_cutset_check_plan(E.i32ptr(w), len(w), X)
        if rc:
            assert M.last_error() == S.last_error() and M.last_error()
    assert M.lib.mlbp_exactsample_check_plan(None, 16, 4) == E.MLBP_EINVAL and 'NULL' in M.last_error()
    with pytest.raises(M.ExactSampleError, match='cycle'):
        M.Plan(R._topo(C.ring_spec(5, 4)), [], 4, None)
    with pytest.raises(M.ExactSampleError, match='configurations') as err:
        M.Plan(R._topo(R.kn_spec(5, 4)), [0, 1, 2], 64, None)
    assert err.value.code == E.MLBP_EUNSUPPORTED
    with pytest.raises(ValueError):
        M.Plan(topo, [0, 0], 4, None)
    assert M.plan(topo, [0, 1], 4, None) is M.plan(topo, [0, 1], 4, None) is not S.plan(topo, [0, 1], 4, None)


def test_kernel_choice_chunks_and_workspace_are_the_rules_of_the_header():
    from macaronicusermodeling_amd import cutset as S
    M, E = _M(), _ffi()

    def ints(P, U):
        return 4 * ((P + U + 16 + 3) // 4 * 4)

    def vectors(n_vars, X):
        return (5 * n_vars + 2) * ((X + 1) // 2 * 2) * 8

    def rule(X, n_vars, P, U, n_forest):
        if X == 64 and n_forest * 33280 + 21 * n_vars * 512 + 64 + ints(P, U) <= S.X64_LDS_BYTES:
            return M.KERNEL_X64
        return M.KERNEL_GENERIC

    def in_workspace(X, n_vars, P, U, n_forest):
        return rule(X, n_vars, P, U, n_forest) == M.KERNEL_GENERIC and vectors(n_vars, X) + 64 + ints(P, U) > S.GENERIC_LDS_BYTES

    def chunks(B, n):
        return min(n, -(-S.MIN_WORKGROUPS // B))
    shapes = ((64, 3, 3, 3, 1), (64, 4, 6, 4, 1), (64, 3, 2, 3, 2), (64, 4, 3, 4, 3), (64, 3, 3, 12, 1), (63, 3, 3, 3, 1), (2, 260, 259, 260, 259),
              (257, 3, 3, 3, 1), (301, 3, 3, 3, 1), (1024, 3, 3, 3, 1), (7, 5, 5, 5, 3), (64, 5, 4, 5, 2), (64, 6, 5, 6, 2), (64, 9, 8, 9, 1), (64, 10, 9, 10, 1))
    for shape in shapes:
        assert M.pick_kernel(*shape) == rule(*shape) == S.pick_kernel(*shape), shape           # the rule of mlbp_cutset_pick_kernel
    # both sides of the X = 64 budget: two forest tables fit, three do not; with two, 5 variables fit and 6 do not; with one, 9 and 10
    assert M.pick_kernel(64, 3, 2, 3, 2) == M.KERNEL_X64 and M.pick_kernel(64, 4, 3, 4, 3) == M.KERNEL_GENERIC
    assert M.pick_kernel(64, 5, 4, 5, 2) == M.KERNEL_X64 and M.pick_kernel(64, 6, 5, 6, 2) == M.KERNEL_GENERIC
    assert M.pick_kernel(64, 9, 8, 9, 1) == M.KERNEL_X64 and M.pick_kernel(64, 10, 9, 10, 1) == M.KERNEL_GENERIC
    # K3 and K4 at two workgroups per CU of 160 KB
    assert 33280 + 21 * 3 * 512 + 64 + ints(3, 3) <= 81920 and 33280 + 21 * 4 * 512 + 64 + ints(6, 4) <= 81920
    assert not in_workspace(301, 3, 3, 3, 1) and in_workspace(1024, 3, 3, 3, 1)
    assert M.lib.mlbp_exactsample_pick_kernel(1025, 3, 3, 3, 1) == E.MLBP_EUNSUPPORTED
    assert M.lib.mlbp_exactsample_pick_kernel(1, 3, 3, 3, 1) == E.MLBP_EINVAL
    assert M.lib.mlbp_exactsample_pick_kernel(64, 3, 3, 3, 4) == E.MLBP_EINVAL
    for B, n in ((1, 64), (1, 4096), (2, 4096), (3, 64), (8192, 64), (600, 64), (600, 7), (256, 3), (511, 4), (512, 4), (1, 1), (9, 65536)):
        assert M.chunks(B, n) == chunks(B, n) == S.chunks(B, n), (B, n)
    assert (M.chunks(3, 64), M.chunks(600, 64), M.chunks(2, 4096)) == (64, 1, 256)
    assert M.lib.mlbp_exactsample_chunks(0, 1) == E.MLBP_EINVAL and M.lib.mlbp_exactsample_chunks(1, 0) == E.MLBP_EINVAL
    for B in (1, 3, 8192):
        for shape in shapes:
            X, n_vars, P, U, n_forest = shape
            for n_cut in (0, 1, 2):
                if X ** n_cut > S.MAX_CONFIGS or n_cut > n_vars:
                    continue
                for n_samples in (1, 2, 5, 64):
                    cw = chunks(B, X ** n_cut)
                    cd = chunks(B, -(-n_samples // 4) if rule(*shape) == M.KERNEL_X64 else n_samples)
                    want = B * X ** n_cut * 3 + B * M.HEAD + (B * max(cw, cd) * vectors(n_vars, X) // 8 if in_workspace(*shape) else 0)
                    assert M.workspace_bytes(B, n_samples, X, n_vars, P, U, n_forest, n_cut) == want * 8, (B, shape, n_cut, n_samples)
    assert M.lib.mlbp_exactsample_workspace_bytes(1, 1, 64, 4, 6, 4, 1, 3) == E.MLBP_EUNSUPPORTED and 'configurations' in M.last_error()
    assert M.lib.mlbp_exactsample_workspace_bytes(0, 1, 64, 3, 3, 3, 1, 1) == E.MLBP_EINVAL
    assert M.lib.mlbp_exactsample_workspace_bytes(1, 0, 64, 3, 3, 3, 1, 1) == E.MLBP_EINVAL
    assert M.workspace_bytes(8192, 64, 1024, 40, 39, 40, 39, 0) > 2 ** 31                        # 64-bit


# ------------------------------------------------------------------------------------------------
# kernel inventory: tests/test_side_libraries_cpu.py holds the shared rule; what the ninth library added to it
# ------------------------------------------------------------------------------------------------
def test_the_other_libraries_hold_no_exactsample_kernel_and_the_sources_stay_apart():
    pkg = os.path.join(ROOT, 'macaronicusermodeling_amd')
    for shared in ('mlbp_cutset_plan.h', 'mlbp_cutset_walk.h'):
        assert '__global__' not in open(os.path.join(pkg, 'csrc', shared)).read()      # helpers only
