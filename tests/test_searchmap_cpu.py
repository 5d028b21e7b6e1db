"""Search decoding beyond the exact limit without a GPU: the listed mode of libmlbp_exactmap.so (include/mlbp_exactmap.h) -- the
max over LISTED cutset states -- stated in NumPy and pinned on enumeration, every input of tests/test_gpu_searchmap.py with its
margins, and the C ABI of the mode.

listed_map() states the header: for every entry of the list the conditioned forest is solved by one max pass up, the values
are compared as (mantissa, exponent) pairs -- every rescaling a power of two, so ties are ties on power-of-two tables exactly
as in the kernels --, the entry of the largest value wins (ties: the lowest entry index) and is decoded by back-pointers with
the tie rule of the exact call.

Margins.  An assignment is compared exactly only where (a) the winner's value leads the best entry of any OTHER configuration
by GAP = 1e-6 nats and (b) within the winner's configuration the best completion leads the runner-up by GAP: the project's bars
for exact_map.  INPUTS lists every input the GPU module compares; test_every_gpu_input_clears_the_margins asserts both for every
graph: the share left out is 0."""
import ctypes
import functools
import itertools
import os

import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_cutsetis_cpu as IS
import test_exactmap_cpu as E
import test_map_cpu as W
from conftest import ROOT
from oracle import lbp_oracle as O

GAP = E.GAP
LN2 = float(np.log(2.0))


# ------------------------------------------------------------------------------------------------
# the statement
# ------------------------------------------------------------------------------------------------
def forest_of(g, facs, cut):
    """(free, edges, parent, walk) of the remainder: the forest of cutset.plan_words, breadth-first from the lowest free variable
    of every tree (E.condition_max's)."""
    free = [v for v in g.var_order if v not in cut]
    edges = [(vs, T) for vs, T in facs if len(vs) == 2 and vs[0] not in cut and vs[1] not in cut]
    parent, walk = {}, []
    for root in free:
        if root in parent:
            continue
        parent[root] = None
        queue = [root]
        while queue:
            v = queue.pop(0)
            walk.append(v)
            for k, (vs, T) in enumerate(edges):
                if v in vs:
                    w = vs[1] if vs[0] == v else vs[0]
                    if w not in parent:
                        parent[w] = (v, k)
                        queue.append(w)
    assert len(edges) == sum(1 for v in free if parent[v] is not None), 'the remainder has a cycle'
    return free, edges, parent, walk


def _norm(vec):
    """(vec * 2^-e, e), e the exponent of the largest entry: exact."""
    top = float(np.max(vec)) if np.size(vec) else 0.0
    if not (top > 0.0 and np.isfinite(top)):
        return vec, 0
    e = int(np.frexp(top)[1])
    return np.ldexp(vec, -e), e


def _products(edges, k, frm, vec):
    """[state of the other end][state of frm]."""
    vs, T = edges[k]
    return (vec[:, None] * T).T if vs[0] == frm else T * vec[None, :]


def _times(m, e, c):
    """(m, e) times the scalar c, renormalised: exact but for the one product."""
    (m,), de = _norm(np.array([m * c]))
    return float(m), e + de


def solve_entry(X, facs, cut, forest, states):
    """One entry, leaves to roots: ((mantissa in [1/2, 1) or 0, exponent) of V, phi, bel, up) under cutset states `states`.
    Every vector is rescaled by the power of two of its largest entry and the exponents are tallied, as the header says."""
    free, edges, parent, walk = forest
    s = dict(zip(cut, (int(v) for v in states)))
    m, e = 1.0, 0
    phi = {v: np.ones(X) for v in free}
    for vs, T in facs:
        if len(vs) == 1:
            if vs[0] in s:
                m, e = _times(m, e, T[s[vs[0]]])
            else:
                phi[vs[0]] = phi[vs[0]] * T
        elif vs[0] in s and vs[1] in s:
            m, e = _times(m, e, T[s[vs[0]], s[vs[1]]])
        elif vs[0] in s:
            phi[vs[1]] = phi[vs[1]] * T[s[vs[0]], :]
        elif vs[1] in s:
            phi[vs[0]] = phi[vs[0]] * T[:, s[vs[1]]]
        for v in vs:
            if v in phi:
                phi[v], de = _norm(phi[v])
                e += de
    bel, up = {v: phi[v].copy() for v in free}, {}
    for v in reversed(walk):
        if parent[v] is None:
            m, e = _times(m, e, float(bel[v].max()))
        else:
            par, k = parent[v]
            up[v], de = _norm(_products(edges, k, v, bel[v]).max(axis=1))
            bel[par], de2 = _norm(bel[par] * up[v])
            e += de + de2
    return ((float(m), int(e)) if m > 0.0 else (0.0, 0)), phi, bel, up


def log_of(V):
    return -np.inf if not V[0] > 0.0 else float(np.log(V[0]) + V[1] * LN2)


def completion_margin(facs, forest, phi, bel, up):
    """Within one configuration: the best completion's lead in nats over the best completion that differs in a free variable
    (inf without free variables)."""
    free, edges, parent, walk = forest
    dn, lead = {}, np.inf
    for v in walk:
        full = bel[v]
        if parent[v] is not None:
            par, k = parent[v]
            excl = phi[par] * (dn[par] if par in dn else 1.0)
            for w in free:
                if w != v and parent[w] is not None and parent[w][0] == par:
                    excl = excl * up[w]
            excl, _ = _norm(excl)
            dn[v], _ = _norm(_products(edges, k, par, excl).max(axis=1))
            full = bel[v] * dn[v]
        ratio = np.sort(full / full.max())
        with np.errstate(divide='ignore'):
            lead = min(lead, float(-np.log(ratio[-2])))
    return lead


def listed_map(spec, inputs, cut, configs, margins=False):
    """include/mlbp_exactmap.h's listed mode in NumPy (spec: a spec or an oracle Graph): dict(x {v: state}, score, entry,
    log_v [N]) of the list `configs` ([N][n_cut] integers; column q is the state of cut[q]); with margins also config_margin
    and completion_margin in nats."""
    g = spec if isinstance(spec, O.Graph) else O.Graph(spec)
    X, order = g.X, list(g.var_order)
    configs = np.asarray(configs)
    N = configs.shape[0]
    configs = configs.reshape(N, len(cut))
    assert N >= 1
    if ((configs < 0) | (configs >= X)).any():
        return dict(x={v: -1 for v in order}, score=np.nan, entry=-1, log_v=np.full(N, np.nan))
    facs = R._factor_arrays(g, inputs)
    forest = forest_of(g, facs, cut)
    free, edges, parent, walk = forest
    best, solved = None, []
    for i in range(N):
        V, phi, bel, up = solve_entry(X, facs, cut, forest, configs[i])
        solved.append(V)
        key = (V[0] > 0.0, V[1] if V[0] > 0.0 else 0, V[0])      # zero below every positive value; then (exponent, mantissa)
        if best is None or key > best[0]:                       # ties: the lowest entry index
            best = (key, i, phi, bel, up)
    _, i, phi, bel, up = best
    x = dict(zip(cut, (int(v) for v in configs[i])))
    positive = solved[i][0] > 0.0
    for v in walk:                                              # every root, then every child given its parent: the lowest maximiser
        if not positive:
            x[v] = 0
        elif parent[v] is None:
            x[v] = int(np.argmax(bel[v]))
        else:
            par, k = parent[v]
            x[v] = int(np.argmax(_products(edges, k, v, bel[v])[x[par]]))
    if not positive:
        x = {v: 0 for v in order}
    out = dict(x=x, score=W.score_of(g, inputs, x), entry=i, log_v=np.array([log_of(V) for V in solved]))
    if margins:
        other = [out['log_v'][j] for j in range(N) if not np.array_equal(configs[j], configs[i])]
        out['config_margin'] = float(out['log_v'][i] - max(other)) if other else np.inf
        out['completion_margin'] = completion_margin(facs, forest, phi, bel, up) if positive else 0.0
    return out


# ------------------------------------------------------------------------------------------------
# the statement against enumeration
# ------------------------------------------------------------------------------------------------
def tree_spec(X):
    """0 - 1, 1 - 2, 1 - 3, 3 - 4: a tree that is no chain; nothing to cut."""
    factors = [dict(id=i, vars=[i], dims=[0], table=i) for i in range(5)]
    for k, (a, b) in enumerate(((0, 1), (1, 2), (1, 3), (3, 4))):
        factors.append(dict(id=5 + k, vars=[a, b], dims=[0, 1] if k % 2 else [1, 0], table=5 + k))
    return dict(name='tree_x%d' % X, style='explicit', X=X, var_ids=list(range(5)), labels=[0] * 5, factors=factors)


SMALL = [('k3', lambda X: R.kn_spec(3, X)), ('k4', lambda X: R.kn_spec(4, X)), ('k5', lambda X: R.kn_spec(5, X)),
         ('ring5', lambda X: C.ring_spec(5, X)), ('tree', tree_spec), ('two_components', IS.two_components_spec)]


def _restricted_argmax(g, grid, cut, configs, walk):
    """Enumeration's answer: among the assignments whose cutset state is listed, the maximum of the grid; ties by the header's
    order -- the lowest entry index, then the forest from its roots down."""
    order = list(g.var_order)
    first = {}
    for i, row in enumerate(configs):
        first.setdefault(tuple(int(v) for v in row), i)
    allowed = [a for a in itertools.product(range(g.X), repeat=len(order)) if tuple(a[order.index(v)] for v in cut) in first]
    top = max(grid[a] for a in allowed)
    ties = [a for a in allowed if grid[a] == top]
    key = lambda a: (first[tuple(a[order.index(v)] for v in cut)],) + tuple(a[order.index(v)] for v in walk)     # noqa: E731
    return min(ties, key=key), top, len(ties)


@pytest.mark.parametrize('X', [2, 3, 4])
@pytest.mark.parametrize('name,make', SMALL, ids=[n for n, _ in SMALL])
def test_statement_equals_enumeration(name, make, X):
    """The full list in index order is the enumerated argmax; a partial list the argmax over the assignments it admits; with
    entry 0 taken from any assignment x the score is at least score(x)."""
    spec = make(X)
    g = O.Graph(spec)
    cut = R.chosen_ids(spec)
    order = list(g.var_order)
    full = IS.full_list(X, len(cut))
    walk = forest_of(g, R._factor_arrays(g, C.make_inputs(spec, 1)), cut)[3]
    rs = np.random.RandomState(X + len(name))
    for seed in (3, 4, 5):
        inputs = C.make_inputs(spec, seed, 'lognormal' if seed == 4 else 'uniform')
        x, best, grid = W.brute_force(g, inputs)
        got = listed_map(spec, inputs, cut, full, margins=True)
        assert got['x'] == x, (name, X, seed)
        np.testing.assert_allclose(got['score'], best, rtol=1e-12)
        ex, escore, _ = E.condition_max(g, inputs, cut)
        assert got['x'] == ex and got['score'] == escore
        if len(cut):
            assert tuple(full[got['entry']]) == tuple(x[v] for v in cut)
            lists = [full[rs.permutation(len(full))[:max(1, len(full) // 2)]], full[rs.randint(0, len(full), size=5)]]
        else:
            assert got['entry'] == 0 and len(full) == 1
            lists = [np.zeros((3, 0), dtype=np.int32)]           # a tree: the one empty configuration, three times
        for configs in lists:
            want, top, n_ties = _restricted_argmax(g, grid, cut, configs, walk)
            part = listed_map(spec, inputs, cut, configs, margins=True)
            assert n_ties == 1 and tuple(part['x'][v] for v in order) == want, (name, X, seed)
            np.testing.assert_allclose(part['score'], top, rtol=1e-12)
            assert part['score'] <= best + 1e-12 * max(1.0, abs(best))
            assert tuple(configs[part['entry']]) == tuple(want[order.index(v)] for v in cut)
            assert part['entry'] == min(i for i, row in enumerate(configs) if np.array_equal(row, configs[part['entry']]))
        # the guarantee: any assignment's cutset state as entry 0
        a = {v: int(rs.randint(X)) for v in order}
        configs = np.concatenate([np.array([[a[v] for v in cut]], dtype=np.int32).reshape(1, len(cut)), full[rs.randint(0, len(full), size=3)]])
        got = listed_map(spec, inputs, cut, configs)
        assert got['score'] >= W.score_of(g, inputs, a) - 1e-12 * max(1.0, abs(got['score']))
        one = listed_map(spec, inputs, cut, configs[:1])
        assert one['entry'] == 0 and one['score'] >= W.score_of(g, inputs, a) - 1e-12 * max(1.0, abs(one['score']))
        assert all(one['x'][v] == a[v] for v in cut)


@pytest.mark.parametrize('name,make', SMALL, ids=[n for n, _ in SMALL])
def test_the_tie_rule_of_the_statement(name, make):
    """Power-of-two tables: every product is exact, so ties are ties.  The full list decodes as enumeration under the header's
    order; among tying entries the lowest wins, whatever configuration it names."""
    for X in (2, 3):
        spec = make(X)
        g = O.Graph(spec)
        cut = R.chosen_ids(spec)
        order = list(g.var_order)
        full = IS.full_list(X, len(cut))
        walk = forest_of(g, R._factor_arrays(g, E.ones_inputs(spec)), cut)[3]
        seen_ties = 0
        for seed in range(8):
            inputs = E.power_of_two_inputs(spec, seed, -1, 1)
            grid = np.rint(W.brute_force(g, inputs)[2] / LN2).astype(np.int64)      # log2 of the potentials: whole numbers, ties exact
            rs = np.random.RandomState(seed)
            for configs in (full, full[::-1], full[rs.randint(0, len(full), size=6)]):
                want, top, n_ties = _restricted_argmax(g, grid, cut, configs, walk)
                got = listed_map(spec, inputs, cut, configs)
                assert tuple(got['x'][v] for v in order) == want, (name, X, seed)
                np.testing.assert_allclose(got['score'], top * LN2, rtol=1e-12, atol=1e-12)
                seen_ties += n_ties > 1
        assert seen_ties >= 4, (name, X, seen_ties)
        ones = listed_map(spec, E.ones_inputs(spec), cut, full[::-1])
        assert ones['entry'] == 0 and ones['score'] == 0.0
        assert all(ones['x'][v] == (int(full[::-1][0][cut.index(v)]) if v in cut else 0) for v in order)


def test_bad_states_and_all_zero_lists():
    spec = R.kn_spec(4, 3)
    inputs = C.make_inputs(spec, 2)
    cut = R.chosen_ids(spec)
    for bad in (3, -1):
        got = listed_map(spec, inputs, cut, [[0, 1], [bad, 2]])
        assert set(got['x'].values()) == {-1} and np.isnan(got['score']) and got['entry'] == -1
    pair_table = next(f['table'] for f in spec['factors'] if len(f['vars']) == 2)
    inputs['tables'][pair_table] = np.zeros_like(inputs['tables'][pair_table])
    got = listed_map(spec, inputs, cut, [[2, 1], [0, 2]])
    assert set(got['x'].values()) == {0} and got['score'] == -np.inf and got['entry'] == 0


# ------------------------------------------------------------------------------------------------
# every input of the GPU module whose assignment is compared: name -> (spec, [inputs], cut, [configs [N][n_cut]])
# ------------------------------------------------------------------------------------------------
def random_lists(X, n_cut, N, B, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, X, size=(N, n_cut)).astype(np.int32) for _ in range(B)]


def shuffled_lists(X, n_cut, B, seed):
    """The full list permuted, with a quarter of it repeated behind."""
    rs = np.random.RandomState(seed)
    full = IS.full_list(X, n_cut)
    out = []
    for _ in range(B):
        perm = full[rs.permutation(len(full))]
        out.append(np.ascontiguousarray(np.concatenate([perm, perm[rs.randint(0, len(full), size=max(1, len(full) // 4))]]), dtype=np.int32))
    return out


def _family(spec, seeds, lists, kind='uniform'):
    cut = R.chosen_ids(spec)
    inputs = [C.make_inputs(spec, s, kind) for s in seeds]
    return spec, inputs, cut, lists(spec['X'], len(cut), len(inputs))


INPUTS = {
    'k3_x64_full': lambda: _family(R.kn_spec(3, 64), (0, 1, 2), lambda X, q, B: [IS.full_list(X, q)] * B),
    'k4_x4_full': lambda: _family(R.kn_spec(4, 4), (0, 1, 2), lambda X, q, B: [IS.full_list(X, q)] * B),
    'k3_x64_shuffled': lambda: _family(R.kn_spec(3, 64), (0, 1, 2), lambda X, q, B: shuffled_lists(X, q, B, 11)),
    'k4_x4_shuffled': lambda: _family(R.kn_spec(4, 4), (0, 1, 2), lambda X, q, B: shuffled_lists(X, q, B, 12)),
    'k5_x64_n1': lambda: _family(R.kn_spec(5, 64), (0, 1, 2), lambda X, q, B: random_lists(X, q, 1, B, 21)),
    'k5_x64_n7': lambda: _family(R.kn_spec(5, 64), (0, 1, 2), lambda X, q, B: random_lists(X, q, 7, B, 22)),
    'k5_x64_n64': lambda: _family(R.kn_spec(5, 64), (0, 1, 2), lambda X, q, B: random_lists(X, q, 64, B, 23), 'lognormal'),
    'k9_x64': lambda: _family(R.kn_spec(9, 64), (0, 1), lambda X, q, B: random_lists(X, q, 6, B, 24)),
    'k10_x64': lambda: _family(R.kn_spec(10, 64), (0, 1), lambda X, q, B: random_lists(X, q, 6, B, 25)),
    'k5_x7': lambda: _family(R.kn_spec(5, 7), (0, 1, 2), lambda X, q, B: random_lists(X, q, 9, B, 26)),
    'k3_x257': lambda: _family(R.kn_spec(3, 257), (0, 1), lambda X, q, B: random_lists(X, q, 5, B, 27)),
}


@functools.lru_cache(maxsize=None)
def family(name):
    """(spec, [inputs], cut, [configs], [listed_map(..., margins=True)]) of INPUTS[name]: computed once per process and shared."""
    spec, inputs, cut, lists = INPUTS[name]()
    return spec, inputs, cut, lists, [listed_map(spec, i, cut, c, margins=True) for i, c in zip(inputs, lists)]


@pytest.mark.parametrize('name', sorted(INPUTS))
def test_every_gpu_input_clears_the_margins(name):
    """No graph is left out of the assignment comparison: the winner leads every other configuration's entry, and its own
    runner-up completion, by GAP."""
    spec, inputs, cut, lists, refs = family(name)
    assert len(cut) == len(O.Graph(spec).var_order) - 2          # K_n: all but two variables are cut
    a = min(r['config_margin'] for r in refs)
    b = min(r['completion_margin'] for r in refs)
    print('%s: %d graphs, smallest lead over another configuration %.1e nats, over the runner-up completion %.1e nats' % (name, len(refs), a, b))
    assert a >= GAP and b >= GAP, (name, a, b)
    assert all(np.isfinite(r['score']) for r in refs)


def test_the_full_lists_are_the_exact_answer():
    for name in ('k3_x64_full', 'k4_x4_full', 'k4_x4_shuffled'):
        spec, inputs, cut, lists, refs = family(name)
        g = O.Graph(spec)
        for i, c, r in zip(inputs, lists, refs):
            x, best, _ = E.reference(g, i)
            assert r['x'] == x, name
            np.testing.assert_allclose(r['score'], best, rtol=1e-12)
            assert r['entry'] == min(k for k, row in enumerate(c) if np.array_equal(row, c[r['entry']]))


# ------------------------------------------------------------------------------------------------
# C ABI of the listed mode
# ------------------------------------------------------------------------------------------------
HEADER = os.path.join(ROOT, 'include', 'mlbp_exactmap.h')


def _M():
    from macaronicusermodeling_amd import exactmap
    return exactmap


def _ffi():
    from macaronicusermodeling_amd import _ffi
    return _ffi


def _valid_args(M, X=64, n=3, n_cut=None, N=16, mm=False):
    """Arguments of K_n with a list of N entries that pass every host-side check (the pointers are never dereferenced on the host)."""
    from macaronicusermodeling_amd import cutset
    words = cutset.plan_words(R._topo(R.kn_spec(n, 4)), list(range(n - 2 if n_cut is None else n_cut)))
    a = M.ExactMapArgs()
    a.B, a.X, a.n_vars, a.P, a.U, a.N = 2, X, n, n * (n - 1) // 2, n, N
    a.n_cut, a.n_free, a.n_items, a.n_consts, a.n_forest = (int(w) for w in words[3:8])
    a.n_pair_tables, a.n_unary_tables, a.plan_words = 2 * a.P, 2 * a.U, len(words)
    for name, typ in M.ExactMapArgs._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, name, 4096)
    if not mm:
        a.max_marginals = None
    a.workspace_bytes = 1 << 40
    return a


def test_the_binding_mirrors_the_new_fields_and_constants():
    M = _M()
    names = [n for n, _ in M.ExactMapArgs._fields_]
    assert names.index('N') == names.index('plan_words') + 1 and names[-1] == 'entry' and 'configs' in names
    assert (M.MAX_LISTED, M.MAX_CUT) == (65536, 16)
    text = open(HEADER).read()
    for word in ('MLBP_EXACTMAP_MAX_LISTED', 'MLBP_EXACTMAP_MAX_CUT', 'lowest entry index', 'Workspace of a listed call',
                 'B * parts * MLBP_EXACTMAP_PARTIAL_HEADER', 'mlbp_cutsetis_check_plan'):
        assert word in text, word


def test_bad_arguments_of_the_listed_mode():
    M, F = _M(), _ffi()
    for field, value, word in (('N', -1, 'list'), ('N', 65537, 'list'), ('configs', None, 'configs')):
        a = _valid_args(M)
        setattr(a, field, value)
        assert M.lib.mlbp_exactmap_f64(ctypes.byref(a), None) == F.MLBP_EINVAL, field
        assert word in M.last_error(), (field, M.last_error())
        assert M.lib.mlbp_exactmap_last_kernel() == M.KERNEL_NONE
    a = _valid_args(M, mm=True)
    assert M.lib.mlbp_exactmap_f64(ctypes.byref(a), None) == F.MLBP_EUNSUPPORTED and 'max_marginals' in M.last_error()
    a = _valid_args(M, n=19, n_cut=17)
    assert M.lib.mlbp_exactmap_f64(ctypes.byref(a), None) == F.MLBP_EUNSUPPORTED and 'at most 16' in M.last_error()
    for field, value, word in (('assignment', None, 'assignment'), ('plan', None, 'plan'), ('workspace_bytes', 8, 'workspace')):
        a = _valid_args(M, n=5)
        setattr(a, field, value)
        assert M.lib.mlbp_exactmap_f64(ctypes.byref(a), None) == F.MLBP_EINVAL and word in M.last_error(), field


def test_shapes_beyond_the_exact_limit_reach_the_device_check():
    """K5, K8 and K12 at X = 64 and K5 at X = 7 with a list get as far as the device; the same arguments without one are refused
    for their configurations, as before."""
    import torch
    M, F = _M(), _ffi()
    for X, n in ((64, 5), (64, 8), (64, 12), (7, 5)):
        a = _valid_args(M, X=X, n=n, N=0)
        if X ** (n - 2) > 65536:                                # (K5 at X = 7 has 343 configurations: the exact call takes it)
            assert M.lib.mlbp_exactmap_f64(ctypes.byref(a), None) == F.MLBP_EUNSUPPORTED and 'configurations' in M.last_error(), (X, n)
        if torch.cuda.is_available():
            continue                                            # (the GPU module runs the entry for real)
        for N in (1, 7, 65536):
            a = _valid_args(M, X=X, n=n, N=N)
            assert M.lib.mlbp_exactmap_f64(ctypes.byref(a), None) == F.MLBP_ENODEVICE, (X, n, N, M.last_error())
            assert 'no CPU fallback' in M.last_error() and M.lib.mlbp_exactmap_last_kernel() == M.KERNEL_NONE
    if not torch.cuda.is_available():
        a = _valid_args(M, n=3, n_cut=0)                        # n_cut = 0 needs no configs (a cyclic remainder is the plan check's)
        a.configs = None
        assert M.lib.mlbp_exactmap_f64(ctypes.byref(a), None) == F.MLBP_ENODEVICE


def test_listed_workspace_bytes_is_what_the_entry_checks():
    import torch
    from macaronicusermodeling_amd import cutset as S
    M, F = _M(), _ffi()

    def want(B, X, n, N):
        P, U, Xp = n * (n - 1) // 2, n, (X + 1) // 2 * 2
        ints = 4 * ((P + U + 16 + 3) // 4 * 4)
        vectors = (5 * n + 2) * Xp
        x64 = X == 64 and 33280 + 21 * n * 512 + 64 + ints <= S.X64_LDS_BYTES
        C_ = min(N, -(-S.MIN_WORKGROUPS // B))
        per = 4 * M.PARTIAL_HEADER if x64 else M.PARTIAL_HEADER + (vectors if vectors * 8 + 64 + ints > S.GENERIC_LDS_BYTES else 0)
        return (B * C_ * per + B * (2 * n + 1) * Xp) * 8
    for X, n, N in ((64, 3, 64), (64, 5, 1), (64, 5, 7), (64, 9, 256), (64, 10, 256), (64, 12, 65536), (7, 5, 9), (257, 3, 5), (1024, 4, 3)):
        for B in (1, 2, 600):
            need = M.listed_workspace_bytes(B, X, n, n * (n - 1) // 2, n, 1, N)
            assert need == want(B, X, n, N), (B, X, n, N)
        a = _valid_args(M, X=X, n=n, N=N)
        need = M.listed_workspace_bytes(a.B, X, n, a.P, a.U, a.n_forest, N)
        a.workspace_bytes = need - 8
        assert M.lib.mlbp_exactmap_f64(ctypes.byref(a), None) == F.MLBP_EINVAL and 'workspace' in M.last_error(), (X, n, N)
        a.workspace_bytes = need
        rc = M.lib.mlbp_exactmap_f64(ctypes.byref(a), None)
        if not torch.cuda.is_available():
            assert rc == F.MLBP_ENODEVICE, (X, n, N, M.last_error())
    assert M.pick_kernel(64, 9, 36, 9, 1) == M.KERNEL_X64 and M.pick_kernel(64, 10, 45, 10, 1) == M.KERNEL_GENERIC
    assert M.pick_kernel(64, 5, 10, 5, 1) == M.KERNEL_X64 and M.pick_kernel(64, 12, 66, 12, 1) == M.KERNEL_GENERIC


def test_a_listed_plan_is_validated_by_the_listed_check():
    """mlbp_exactmap_check_plan keeps the exact call's bound; cutsetis.plan's check admits K5 at X = 64."""
    from macaronicusermodeling_amd import cutsetis
    M = _M()
    topo = R._topo(R.kn_spec(5, 4))
    with pytest.raises(M.ExactMapError, match='configurations'):
        M.Plan(topo, [0, 1, 2], 64, None)
    assert cutsetis.Plan(topo, [0, 1, 2], 64, None).n_cut == 3


def test_the_gpu_module_names_the_three_kernels_of_a_listed_call():
    import test_gpu_searchmap as G
    import test_side_libraries_cpu as L
    assert set(G.CASES) == {('exactmap_x64_kernel', (False,)), ('exactmap_generic_kernel', (False,)), ('exactmap_final_kernel', ())}
    assert set(G.CASES) <= L.INSTANCES['exactmap']
    for kern, tests in G.CASES.items():
        assert tests, kern
        for t in tests:
            assert callable(getattr(G, t, None)), (kern, t)
