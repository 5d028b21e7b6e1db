"""Exact MAP decoding and max-marginals by cutset conditioning without a GPU: the float64 references the GPU tests compare
against, the NumPy statement of include/mlbp_exactmap.h pinned on exhaustive enumeration, the gap that makes an assignment
comparable, the C ABI of libmlbp_exactmap.so and the kernel inventory rule applied to the seventh library.

References.  test_map_cpu.brute_force is the log-domain grid and its argmax.  reference() is the same enumeration one slice of
the first variable at a time (so that X^n need not fit in memory) and also gives the max-marginals -- the grid's maxima with
one variable held -- and is pinned on the grid here; viterbi() is the max form of the forward algorithm for chains.
condition_max() states the header in NumPy -- condition on every joint state of the cutset, solve the forest by one max pass
up, decode by back-pointers with the tie rule, one max pass down for the max-marginals -- and must equal the grid for every
graph family the GPU module uses.

The tie cap.  An assignment is compared exactly only where the reference's best score leads its second best by at least GAP =
1e-6 nats; INPUTS lists every input of the GPU module and test_every_gpu_input_has_a_gap asserts the lead for all of them:
none is left out."""
import ctypes
import functools
import itertools
import os

import numpy as np
import pytest

import cases as C
import kernel_inventory as K
import test_cutset_cpu as R
import test_map_cpu as W
from conftest import ROOT
from oracle import lbp_oracle as O

GAP = 1e-6


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def reference(g, inputs):
    """(x {v: state}, best score, max-marginals [n_vars][X] in g.var_order) by enumeration in the log domain, one slice of the
    first variable at a time; the first (lowest, row-major) assignment at the maximum, as brute_force."""
    order = list(g.var_order)
    n, X = len(order), g.X
    with np.errstate(divide='ignore'):
        logs = [(vs, np.log(T)) for vs, T in R._factor_arrays(g, inputs)]
    v0, rest = order[0], order[1:]
    mm = np.full((n, X), -np.inf)
    best, arg = -np.inf, None

    def along(vec, v):
        shape = [1] * (n - 1)
        shape[rest.index(v)] = X
        return vec.reshape(shape)
    for s in range(X):
        grid = np.zeros((X,) * (n - 1))
        for vs, L in logs:
            if len(vs) == 1:
                grid = grid + (L[s] if vs[0] == v0 else along(L, vs[0]))
            elif vs[0] == v0:
                grid = grid + along(L[s, :], vs[1])
            elif vs[1] == v0:
                grid = grid + along(L[:, s], vs[0])
            else:
                ia, ib = rest.index(vs[0]), rest.index(vs[1])
                shape = [1] * (n - 1)
                shape[ia] = shape[ib] = X
                grid = grid + (L if ia < ib else L.T).reshape(shape)
        top = float(grid.max())
        mm[0, s] = top
        for i in range(n - 1):
            mm[i + 1] = np.maximum(mm[i + 1], grid.max(axis=tuple(a for a in range(n - 1) if a != i)))
        if top > best:
            best, arg = top, (s,) + tuple(int(k) for k in np.unravel_index(int(np.argmax(grid)), grid.shape))
    return (None if arg is None else dict(zip(order, arg))), best, mm


def viterbi(g, inputs):
    """(x, best score, max-marginals) of C.chain_spec graphs by the max form of the forward and the backward recursion, in the
    log domain."""
    n, X = len(g.var_order), g.X
    with np.errstate(divide='ignore'):
        tabs = {vs: np.log(T) for vs, T in R._factor_arrays(g, inputs)}
    fwd, back = [tabs[(0,)]], [None]
    for i in range(1, n):
        cand = fwd[-1][:, None] + tabs[(i - 1, i)]
        back.append(cand.argmax(axis=0))
        fwd.append(cand.max(axis=0) + tabs[(i,)])
    bwd = [None] * n
    bwd[n - 1] = np.zeros(X)
    for i in range(n - 1, 0, -1):
        bwd[i - 1] = (tabs[(i - 1, i)] + (bwd[i] + tabs[(i,)])[None, :]).max(axis=1)
    x = [0] * n
    x[n - 1] = int(fwd[-1].argmax())
    for i in range(n - 1, 0, -1):
        x[i - 1] = int(back[i][x[i]])
    return dict(zip(g.var_order, x)), float(fwd[-1].max()), np.stack([fwd[i] + bwd[i] for i in range(n)])


def gap_of(best, mm):
    """best minus the best score of any assignment that differs in at least one variable."""
    second = np.sort(mm, axis=1)[:, -2]
    return float((best - second).min())


def condition_max(g, inputs, cut):
    """include/mlbp_exactmap.h in NumPy: (x {v: state}, score, max-marginals [n_vars][X] in g.var_order, natural log) for the
    cutset `cut` (variable ids; digit q of a configuration is the state of cut[q]).  The forest is the one of
    cutset.plan_words: breadth-first from the lowest free variable of every tree."""
    X, order = g.X, list(g.var_order)
    free = [v for v in order if v not in cut]
    facs = R._factor_arrays(g, inputs)
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

    def products(k, frm, vec):                                  # [state of the other end][state of frm]
        vs, T = edges[k]
        return (vec[:, None] * T).T if vs[0] == frm else T * vec[None, :]
    best = None
    mm = {v: np.zeros(X) for v in order}
    for c in range(X ** len(cut)):
        s = {v: (c // X ** q) % X for q, v in enumerate(cut)}
        const, phi = 1.0, {v: np.ones(X) for v in free}
        for vs, T in facs:
            if len(vs) == 1:
                if vs[0] in s:
                    const *= T[s[vs[0]]]
                else:
                    phi[vs[0]] = phi[vs[0]] * T
            elif vs[0] in s and vs[1] in s:
                const *= T[s[vs[0]], s[vs[1]]]
            elif vs[0] in s:
                phi[vs[1]] = phi[vs[1]] * T[s[vs[0]], :]
            elif vs[1] in s:
                phi[vs[0]] = phi[vs[0]] * T[:, s[vs[1]]]
        bel, up = {v: phi[v].copy() for v in free}, {}
        V = const
        for v in reversed(walk):                                # leaves to roots
            if parent[v] is None:
                V *= bel[v].max()
            else:
                par, k = parent[v]
                up[v] = products(k, v, bel[v]).max(axis=1)
                bel[par] = bel[par] * up[v]
        if best is None or V > best[0]:                         # ties: the lowest c
            best = (V, s, {v: bel[v].copy() for v in free})
        if not V > 0:
            continue
        dn, full = {}, dict(bel)
        for v in walk:                                          # roots to leaves
            if parent[v] is not None:
                par, k = parent[v]
                excl = phi[par] * (dn[par] if par in dn else 1.0)
                for w in free:
                    if w != v and parent[w] is not None and parent[w][0] == par:
                        excl = excl * up[w]
                dn[v] = products(k, par, excl).max(axis=1)
                full[v] = bel[v] * dn[v]
            mm[v] = np.maximum(mm[v], V * (full[v] / full[v].max()))
        for v in cut:
            mm[v][s[v]] = max(mm[v][s[v]], V)
    V, x, bel = best[0], dict(best[1]), best[2]
    for v in walk:                                              # every root, then every child given its parent: the lowest maximiser
        if not V > 0:                                           # every assignment has potential zero: every state is a maximiser
            x[v] = 0
        elif parent[v] is None:
            x[v] = int(np.argmax(bel[v]))
        else:
            par, k = parent[v]
            x[v] = int(np.argmax(products(k, v, bel[v])[x[par]]))
    with np.errstate(divide='ignore'):
        return x, W.score_of(g, inputs, x), np.log(np.stack([mm[v] for v in order]))


def power_of_two_inputs(spec, seed, lo=-3, hi=3):
    """Tables whose entries are powers of two: every product of the walk is exact, so ties are ties."""
    rs = np.random.RandomState(seed)
    n = 1 + max(f['table'] for f in spec['factors'])
    shape = {f['table']: (spec['X'], spec['X']) if len(f['vars']) == 2 else (spec['X'], 1) for f in spec['factors']}
    return dict(tables=[np.ldexp(1.0, rs.randint(lo, hi + 1, size=shape[t])) for t in range(n)])


def ones_inputs(spec):
    return power_of_two_inputs(spec, 0, 0, 0)


# ------------------------------------------------------------------------------------------------
# every input of the GPU module whose assignment is compared: name -> (spec, [inputs], how the reference is computed)
# ------------------------------------------------------------------------------------------------
def _family(make, seeds, kind='uniform', how=reference):
    spec = make()
    return spec, [C.make_inputs(spec, s, kind) for s in seeds], how


INPUTS = {
    'user_k3': lambda: _family(lambda: C.user_spec(10, [1, 4, 7], 64, 64, seed=1), range(500, 564)),
    'user_k3_lognormal': lambda: _family(lambda: C.user_spec(10, [1, 4, 7], 64, 64, seed=1), range(32), 'lognormal'),
    'k3_x64': lambda: _family(lambda: R.kn_spec(3, 64), range(16)),
    'k3_x64_wide': lambda: (R.kn_spec(3, 64), [R.wide_inputs(R.kn_spec(3, 64), s) for s in (21, 22)], reference),
    'k4_x64': lambda: _family(lambda: R.kn_spec(4, 64), (1, 2), 'lognormal'),
    'ring5_x8': lambda: _family(lambda: C.ring_spec(5, 8), range(40)),
    'ring5_x7': lambda: _family(lambda: C.ring_spec(5, 7), range(40)),
    'k4_x8': lambda: _family(lambda: R.kn_spec(4, 8), range(40)),
    'k4_x16': lambda: _family(lambda: R.kn_spec(4, 16), range(8)),
    'k5_x4': lambda: _family(lambda: R.kn_spec(5, 4), (3, 4, 5)),
    'shuffled_x5': lambda: _family(lambda: C.shuffled_ids_spec(5), (3, 4, 5)),
    'double_pair_x6': lambda: _family(lambda: R.double_pair_spec(6), (3, 4, 5)),
    'forest_x9': lambda: _family(lambda: R.forest_spec(9), (3, 4, 5)),
    'ring3_x2': lambda: _family(lambda: C.ring_spec(3, 2), (7, 8)),
    'ring3_x257': lambda: _family(lambda: C.ring_spec(3, 257), (7, 8)),
    'ring3_x301': lambda: _family(lambda: C.ring_spec(3, 301), (7, 8)),
    'k3_x1024': lambda: _family(lambda: R.kn_spec(3, 1024), (9,)),
    'chain260_x2': lambda: _family(lambda: C.chain_spec(260, 2), (1, 2), how=viterbi),
    'chain3_x64': lambda: _family(lambda: C.chain_spec(3, 64), (1, 2)),
    'chain4_x64': lambda: _family(lambda: C.chain_spec(4, 64), (1,)),
    'star4_x8': lambda: _family(lambda: C.star_spec(4, 8), (1, 2, 3)),
    'chain5_x8': lambda: _family(lambda: C.chain_spec(5, 8), (1, 2, 3)),
}


@functools.lru_cache(maxsize=None)
def family(name):
    """(spec, [inputs], [(x, best, max-marginals)]) of INPUTS[name]: computed once per process and shared."""
    spec, inputs, how = INPUTS[name]()
    g = O.Graph(spec)
    return spec, inputs, [how(g, i) for i in inputs]


@pytest.mark.parametrize('name', sorted(INPUTS))
def test_every_gpu_input_has_a_gap(name):
    """No case is left out (cap 0): every graph the GPU module decodes leads its second-best assignment by GAP."""
    _, _, refs = family(name)
    gaps = [gap_of(best, mm) for _, best, mm in refs]
    print('%s: smallest gap over %d graphs %.1e nats' % (name, len(gaps), min(gaps)))
    assert min(gaps) >= GAP, (name, gaps)


# ------------------------------------------------------------------------------------------------
# the statement and the references against the grid
# ------------------------------------------------------------------------------------------------
def grid_max_marginals(grid):
    n = grid.ndim
    return np.stack([grid.max(axis=tuple(a for a in range(n) if a != i)) for i in range(n)])


def close(got, want, rel):
    """Both -inf, or within rel * max(1, |want|)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    same_inf = np.isneginf(got) & np.isneginf(want)
    with np.errstate(invalid='ignore'):
        near = np.abs(got - want) <= rel * np.maximum(1.0, np.abs(want))
    return bool((same_inf | near).all())


SMALL = [('k3_x5', lambda: R.kn_spec(3, 5)), ('k4_x4', lambda: R.kn_spec(4, 4)), ('k5_x3', lambda: R.kn_spec(5, 3)),
         ('ring6_x4', lambda: C.ring_spec(6, 4)), ('ring5_x7', lambda: C.ring_spec(5, 7)), ('double_pair_x5', lambda: R.double_pair_spec(5)),
         ('forest_x4', lambda: R.forest_spec(4)), ('chain5_x8', lambda: C.chain_spec(5, 8)), ('star4_x8', lambda: C.star_spec(4, 8)),
         ('shuffled_x5', lambda: C.shuffled_ids_spec(5)), ('user_p3', lambda: C.user_spec(6, [0, 2, 5], 16, 16))]


@pytest.mark.parametrize('name,make', SMALL, ids=[s[0] for s in SMALL])
def test_statement_and_reference_equal_brute_force(name, make):
    spec = make()
    g = O.Graph(spec)
    cut = R.chosen_ids(spec)
    for kind in ('uniform',) if spec['style'] == 'trainmp' else ('uniform', 'lognormal'):
        for seed in (3, 4, 5):
            inputs = C.make_inputs(spec, seed, kind)
            x, best, grid = W.brute_force(g, inputs)
            want_mm = grid_max_marginals(grid)
            assert gap_of(best, want_mm) >= GAP
            rx, rbest, rmm = reference(g, inputs)
            assert rx == x and rbest == best and np.array_equal(rmm, want_mm), (name, kind, seed)
            sx, sscore, smm = condition_max(g, inputs, cut)
            assert sx == x, (name, kind, seed, cut)
            np.testing.assert_allclose(sscore, best, rtol=1e-12)
            assert close(smm, want_mm, 1e-10), (name, kind, seed)
            assert close(smm.max(axis=1), np.full(len(x), best), 1e-12)


def test_any_valid_cutset_gives_the_same_assignment():
    spec = R.kn_spec(3, 5)
    g, inputs = O.Graph(spec), C.make_inputs(spec, 8)
    x, best, grid = W.brute_force(g, inputs)
    for cut in ([0], [1], [2], [0, 1], [2, 0], [0, 1, 2]):
        sx, sscore, smm = condition_max(g, inputs, cut)
        assert sx == x and close(smm, grid_max_marginals(grid), 1e-10), cut
        np.testing.assert_allclose(sscore, best, rtol=1e-12)
    spec = C.chain_spec(4, 3)
    g, inputs = O.Graph(spec), C.make_inputs(spec, 9)
    assert condition_max(g, inputs, [])[0] == condition_max(g, inputs, [2])[0] == W.brute_force(g, inputs)[0]


def test_viterbi_equals_the_statement_and_the_grid():
    for n, X, seed in ((7, 3, 13), (6, 2, 14)):
        spec = C.chain_spec(n, X)
        g, inputs = O.Graph(spec), C.make_inputs(spec, seed)
        x, best, grid = W.brute_force(g, inputs)
        vx, vbest, vmm = viterbi(g, inputs)
        sx, sscore, smm = condition_max(g, inputs, [])
        assert vx == x == sx
        np.testing.assert_allclose([vbest, sscore], best, rtol=1e-12)
        assert close(vmm, grid_max_marginals(grid), 1e-12) and close(smm, vmm, 1e-10)


def test_the_tie_rule_of_the_statement():
    """On power-of-two tables every product is exact: all-ones tables decode to the all-zero assignment, and among equal
    maxima the statement returns the lowest configuration, then the lowest root state, then the lowest child states."""
    for spec in (R.kn_spec(3, 4), C.ring_spec(5, 3), C.chain_spec(4, 3), R.forest_spec(3)):
        g = O.Graph(spec)
        x, score, mm = condition_max(g, ones_inputs(spec), R.chosen_ids(spec))
        assert set(x.values()) == {0} and score == 0.0 and (mm == 0.0).all()
    spec = C.ring_spec(5, 3)                                     # an all-zero table: every assignment ties at -inf
    inputs = C.make_inputs(spec, 1)
    pair_table = next(f['table'] for f in spec['factors'] if len(f['vars']) == 2)
    inputs['tables'][pair_table] = np.zeros_like(inputs['tables'][pair_table])
    x, score, mm = condition_max(O.Graph(spec), inputs, R.chosen_ids(spec))
    assert set(x.values()) == {0} and score == -np.inf and np.isneginf(mm).all()
    spec = R.kn_spec(3, 4)
    g = O.Graph(spec)
    for seed in range(20):
        inputs = power_of_two_inputs(spec, seed, -1, 1)
        _, best, grid = W.brute_force(g, inputs)
        cut = R.chosen_ids(spec)
        x, score, _ = condition_max(g, inputs, cut)
        assert score == best                                    # sums of integers times ln 2: exact enough to compare
        # the statement's order: configuration, then the forest from its root down = lexicographic in (cut, walk) order
        ties = [a for a in itertools.product(range(4), repeat=3) if grid[a] == best]
        walk = [v for v in g.var_order if v not in cut]         # K3: the root is the lower free variable
        key = lambda a: tuple(a[g.var_order.index(v)] for v in list(cut)[::-1] + walk)     # noqa: E731
        want = min(ties, key=key)
        assert tuple(x[v] for v in g.var_order) == want, (seed, ties)


# ------------------------------------------------------------------------------------------------
# C ABI of libmlbp_exactmap.so
# ------------------------------------------------------------------------------------------------
def _M():
    from macaronicusermodeling_amd import exactmap
    return exactmap


def _ffi():
    from macaronicusermodeling_amd import _ffi
    return _ffi


def _valid_args(M, X=64, n_cut=1):
    """Arguments of K3 that pass every host-side check (the pointers are never dereferenced on the host)."""
    from macaronicusermodeling_amd import cutset
    words = cutset.plan_words(R._topo(R.kn_spec(3, 4)), list(range(n_cut)))
    a = M.ExactMapArgs()
    a.B, a.X, a.n_vars, a.P, a.U = 2, X, 3, 3, 3
    a.n_cut, a.n_free, a.n_items, a.n_consts, a.n_forest = (int(w) for w in words[3:8])
    a.n_pair_tables, a.n_unary_tables, a.plan_words = 6, 6, len(words)
    for name, typ in M.ExactMapArgs._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, name, 4096)
    a.workspace_bytes = 1 << 40
    return a


def test_library_identity_and_bad_arguments():
    M, E = _M(), _ffi()
    assert M.lib.mlbp_exactmap_arch() == b'gfx950'
    assert M.lib.mlbp_exactmap_f64(None, None) == E.MLBP_EINVAL and 'NULL' in M.last_error()
    for field, value, word in (('B', 0, 'sizes'), ('X', 1, 'two states'), ('n_free', 1, 'sizes'), ('plan', None, 'plan'), ('plan_words', 5, 'plan'),
                               ('pair_tab', None, 'pair_tab'), ('n_unary_tables', 0, 'unary_tables'), ('assignment', None, 'assignment'),
                               ('score', None, 'score'), ('workspace', None, 'workspace'), ('workspace_bytes', 8, 'workspace')):
        a = _valid_args(M)
        setattr(a, field, value)
        assert M.lib.mlbp_exactmap_f64(ctypes.byref(a), None) == E.MLBP_EINVAL, field
        assert word in M.last_error(), (field, M.last_error())
        assert M.lib.mlbp_exactmap_last_kernel() == M.KERNEL_NONE
    a = _valid_args(M, X=1025)
    assert M.lib.mlbp_exactmap_f64(ctypes.byref(a), None) == E.MLBP_EUNSUPPORTED and '1024' in M.last_error()
    a = _valid_args(M, X=1024, n_cut=2)
    assert M.lib.mlbp_exactmap_f64(ctypes.byref(a), None) == E.MLBP_EUNSUPPORTED and 'configurations' in M.last_error()
    with pytest.raises(M.ExactMapError):
        M.check(E.MLBP_EINVAL)


def test_compute_entry_fails_loudly_without_a_gpu():
    import torch
    M = _M()
    if torch.cuda.is_available():
        return                                                  # (the GPU module runs the entry for real)
    for X in (64, 128, 1024):
        for mm in (4096, None):                                 # max_marginals is optional
            a = _valid_args(M, X=X)
            a.max_marginals = mm
            assert M.lib.mlbp_exactmap_f64(ctypes.byref(a), None) == _ffi().MLBP_ENODEVICE
            assert 'no CPU fallback' in M.last_error() and M.lib.mlbp_exactmap_last_kernel() == M.KERNEL_NONE


def test_check_plan_is_the_shared_check():
    """The plan's validation is stated once (csrc/mlbp_cutset_plan.h): both libraries refuse the same plans in the same words."""
    from macaronicusermodeling_amd import cutset as S
    M, E = _M(), _ffi()
    topo = R._topo(R.kn_spec(4, 4))
    good = S.plan_words(topo, [0, 1])
    ring = S.plan_words(R._topo(C.ring_spec(5, 4)), [])
    bad = good.copy()
    bad[S.PLAN_HEADER] = 9
    for words, X in ((good, 4), (good, 64), (good, 1024), (good, 1), (good[:-1], 4), (ring, 4), (bad, 4), (S.plan_words(topo, [0]), 4)):
        w = np.ascontiguousarray(words, dtype=np.int32)
        rc = M.lib.mlbp_exactmap_check_plan(E.i32ptr(w), len(w), X)
        assert rc == S.lib.mlbp_cutset_check_plan(E.i32ptr(w), len(w), X)
        if rc:
            assert M.last_error() == S.last_error() and M.last_error()
    assert M.lib.mlbp_exactmap_check_plan(None, 16, 4) == E.MLBP_EINVAL and 'NULL' in M.last_error()
    with pytest.raises(M.ExactMapError, match='cycle'):
        M.Plan(R._topo(C.ring_spec(5, 4)), [], 4, None)
    with pytest.raises(M.ExactMapError, match='configurations') as err:
        M.Plan(R._topo(R.kn_spec(5, 4)), [0, 1, 2], 64, None)
    assert err.value.code == E.MLBP_EUNSUPPORTED
    with pytest.raises(ValueError):
        M.Plan(topo, [0, 0], 4, None)


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

    def chunks(B, n_configs):
        return min(n_configs, -(-S.MIN_WORKGROUPS // B))
    shapes = ((64, 3, 3, 3, 1), (64, 4, 6, 4, 1), (64, 3, 2, 3, 2), (64, 4, 3, 4, 3), (64, 3, 3, 12, 1), (63, 3, 3, 3, 1), (2, 260, 259, 260, 259),
              (257, 3, 3, 3, 1), (301, 3, 3, 3, 1), (1024, 3, 3, 3, 1), (7, 5, 5, 5, 3), (64, 5, 4, 5, 2), (64, 6, 5, 6, 2), (64, 9, 8, 9, 1), (64, 10, 9, 10, 1))
    for shape in shapes:
        assert M.pick_kernel(*shape) == rule(*shape) == S.pick_kernel(*shape), shape           # the rule of mlbp_cutset_pick_kernel
    # both sides of the X = 64 budget: two forest tables fit, three do not; with two, 5 variables fit and 6 do not; with one, 9 and 10
    assert M.pick_kernel(64, 3, 2, 3, 2) == M.KERNEL_X64 and M.pick_kernel(64, 4, 3, 4, 3) == M.KERNEL_GENERIC
    assert M.pick_kernel(64, 5, 4, 5, 2) == M.KERNEL_X64 and M.pick_kernel(64, 6, 5, 6, 2) == M.KERNEL_GENERIC
    assert M.pick_kernel(64, 9, 8, 9, 1) == M.KERNEL_X64 and M.pick_kernel(64, 10, 9, 10, 1) == M.KERNEL_GENERIC
    assert not in_workspace(301, 3, 3, 3, 1) and in_workspace(1024, 3, 3, 3, 1)
    assert M.lib.mlbp_exactmap_pick_kernel(1025, 3, 3, 3, 1) == E.MLBP_EUNSUPPORTED
    assert M.lib.mlbp_exactmap_pick_kernel(1, 3, 3, 3, 1) == E.MLBP_EINVAL
    assert M.lib.mlbp_exactmap_pick_kernel(64, 3, 3, 3, 4) == E.MLBP_EINVAL
    for B, n in ((1, 64), (1, 4096), (2, 4096), (3, 64), (8192, 64), (600, 64), (600, 7), (256, 3), (511, 4), (512, 4), (1, 1), (9, 65536)):
        assert M.chunks(B, n) == chunks(B, n) == S.chunks(B, n), (B, n)
    assert (M.chunks(3, 64), M.chunks(600, 64), M.chunks(2, 4096)) == (64, 1, 256)
    assert M.lib.mlbp_exactmap_chunks(0, 1) == E.MLBP_EINVAL and M.lib.mlbp_exactmap_chunks(1, 0) == E.MLBP_EINVAL
    for B in (1, 3, 8192):
        for shape in shapes:
            X, n_vars, P, U, n_forest = shape
            Xp = (X + 1) // 2 * 2
            for n_cut in (0, 1, 2):
                if X ** n_cut > S.MAX_CONFIGS or n_cut > n_vars:
                    continue
                for mm in (False, True):
                    per = (M.PARTIAL_HEADER + (n_vars * X if mm else 0)) * (4 if rule(*shape) == M.KERNEL_X64 else 1)
                    per += vectors(n_vars, X) // 8 if in_workspace(*shape) else 0
                    want = (B * chunks(B, X ** n_cut) * per + B * (2 * n_vars + 1) * Xp) * 8
                    assert M.workspace_bytes(B, X, n_vars, P, U, n_forest, n_cut, mm) == want, (B, shape, n_cut, mm)
    assert M.lib.mlbp_exactmap_workspace_bytes(1, 64, 4, 6, 4, 1, 3, 0) == E.MLBP_EUNSUPPORTED and 'configurations' in M.last_error()
    assert M.lib.mlbp_exactmap_workspace_bytes(0, 64, 3, 3, 3, 1, 1, 1) == E.MLBP_EINVAL
    assert M.workspace_bytes(8192, 1024, 40, 39, 40, 39, 0, True) > 2 ** 31                    # 64-bit


# ------------------------------------------------------------------------------------------------
# kernel inventory: tests/test_side_libraries_cpu.py holds the shared rule; what the seventh library added to it
# ------------------------------------------------------------------------------------------------
def test_the_other_libraries_hold_no_exactmap_kernel_and_the_sources_stay_apart():
    pkg = os.path.join(ROOT, 'macaronicusermodeling_amd')
    assert not K.kernel_names(csrc=os.path.join(pkg, 'csrc')) & {'check_packed_plan'}
    shared = open(os.path.join(pkg, 'csrc', 'mlbp_cutset_plan.h')).read()
    assert '__global__' not in shared                           # helpers only: the first library's inventory scans csrc/
