"""Exact inference by cutset conditioning without a GPU: the float64 references the GPU tests compare against, the NumPy
statement of include/mlbp_cutset.h pinned on exhaustive enumeration, the cutset choice and the host checks of libmlbp_cutset.so
(the contract it shares with the other side libraries is in tests/test_side_libraries_cpu.py).

References.  enumerate_exact() is the log-domain grid of test_map_cpu.brute_force, then log-sum-exp and axis sums: nothing of
the algorithm under test is in it.  Where X^n is too large, eliminate() sums variables out one at a time with einsum / matmul
on max-rescaled tables, and chain_forward_backward() is the forward algorithm; both are pinned on the grid here.
condition() states the header's semantics in NumPy -- condition on every joint state of the cutset, solve the forest by one pass
up and one pass down, combine -- and must equal the grid for every graph family the GPU module uses."""
import ctypes
import itertools

import numpy as np
import pytest

import cases as C
import helpers
import test_map_cpu as W
from oracle import lbp_oracle as O


# ------------------------------------------------------------------------------------------------
# graph families
# ------------------------------------------------------------------------------------------------
def kn_spec(n, X, name=None):
    """K_n: one unary factor per variable, one pairwise factor per pair (lower id on axis 0, every third one turned)."""
    factors = [dict(id=i, vars=[i], dims=[0], table=i) for i in range(n)]
    for a in range(n):
        for b in range(a + 1, n):
            k = len(factors)
            factors.append(dict(id=k, vars=[a, b], dims=[0, 1] if k % 3 else [1, 0], table=k))
    return dict(name=name or 'k%d_x%d' % (n, X), style='explicit', X=X, var_ids=list(range(n)), labels=[(2 * i + 1) % X for i in range(n)],
                factors=factors)


def double_pair_spec(X):
    """Two factors over the pair (0, 1) -- a cycle of two -- with a tail 1 - 2."""
    factors = [dict(id=0, vars=[0], dims=[0], table=0), dict(id=1, vars=[0, 1], dims=[0, 1], table=1),
               dict(id=2, vars=[1, 0], dims=[0, 1], table=2), dict(id=3, vars=[1, 2], dims=[1, 0], table=3), dict(id=4, vars=[2], dims=[0], table=4)]
    return dict(name='double_pair_x%d' % X, style='explicit', X=X, var_ids=[0, 1, 2], labels=[0, 1 % X, 0], factors=factors)


def forest_spec(X):
    """Two trees (0 - 1 - 2 and 3 - 4) and variable 5 with unary factors only."""
    factors = [dict(id=0, vars=[0, 1], dims=[0, 1], table=0), dict(id=1, vars=[2, 1], dims=[0, 1], table=1), dict(id=2, vars=[1], dims=[0], table=2),
               dict(id=3, vars=[3, 4], dims=[1, 0], table=3), dict(id=4, vars=[4], dims=[0], table=4), dict(id=5, vars=[5], dims=[0], table=5),
               dict(id=6, vars=[5], dims=[0], table=6)]
    return dict(name='forest_x%d' % X, style='explicit', X=X, var_ids=[0, 1, 2, 3, 4, 5], labels=[0] * 6, factors=factors)


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def logsumexp(a, axis=None):
    top = np.max(a, axis=axis, keepdims=True)
    with np.errstate(invalid='ignore'):
        out = np.log(np.sum(np.exp(a - top), axis=axis, keepdims=True)) + top
    return float(out.reshape(-1)[0]) if axis is None else np.squeeze(out, axis=axis)


def enumerate_exact(g, inputs):
    """(log_z, marginals [n_vars][X] in g.var_order, grid) by exhaustive enumeration in the log domain."""
    _, _, grid = W.brute_force(g, inputs)
    log_z = logsumexp(grid)
    n = grid.ndim
    marg = np.stack([np.exp(logsumexp(grid, axis=tuple(a for a in range(n) if a != i)) - log_z) if n > 1 else np.exp(grid - log_z)
                     for i in range(n)])
    return log_z, marg, grid


def _factor_arrays(g, inputs):
    """[(variables in axis order, table)] of every factor."""
    out = []
    for f in g.factors:
        T = O.factor_table(g, inputs, f)
        if len(f['vars']) == 1:
            out.append(((f['vars'][0],), T.reshape(-1)))
        else:
            by_axis = {g.dim_of(f, v): v for v in f['vars']}
            out.append(((by_axis[0], by_axis[1]), T))
    return out


def eliminate(g, inputs):
    """(log_z, marginals) by summing the other variables out one at a time (einsum, BLAS where it can); every intermediate is
    divided by its largest entry and the logarithms are tallied."""
    letters = {v: chr(ord('a') + i) for i, v in enumerate(g.var_order)}
    margs, log_zs = [], []
    for target in g.var_order:
        fs, shift = [], 0.0
        for vs, T in _factor_arrays(g, inputs):
            top = T.max()
            fs.append((vs, T / top))
            shift += np.log(top)
        for u in [v for v in g.var_order if v != target]:
            mine = [f for f in fs if u in f[0]]
            rest = [f for f in fs if u not in f[0]]
            keep = tuple(sorted({v for vs, _ in mine for v in vs if v != u}, key=g.var_order.index))
            expr = ','.join(''.join(letters[v] for v in vs) for vs, _ in mine) + '->' + ''.join(letters[v] for v in keep)
            T = np.einsum(expr, *[t for _, t in mine], optimize=True)
            top = T.max()
            shift += np.log(top)
            fs = rest + [(keep, T / top)]
        vec = np.ones(g.X)
        for vs, T in fs:
            vec = vec * (T if vs else float(T))
        margs.append(vec / vec.sum())
        log_zs.append(float(np.log(vec.sum()) + shift))
    assert np.ptp(log_zs) <= 1e-11 * max(1.0, abs(log_zs[0])), log_zs
    return log_zs[0], np.stack(margs)


def chain_forward_backward(g, inputs):
    """(log_z, marginals) of C.chain_spec graphs by the forward and the backward recursion, rescaled at every step."""
    n, X = len(g.var_order), g.X
    tabs = {vs: T for vs, T in _factor_arrays(g, inputs)}
    fwd, bwd, shift = [None] * n, [None] * n, 0.0
    a = tabs[(0,)].copy()
    for i in range(n):
        if i:
            a = a.dot(tabs[(i - 1, i)]) * tabs[(i,)]
        shift += np.log(a.sum())
        a = a / a.sum()
        fwd[i] = a
    b = np.ones(X)
    for i in range(n - 1, -1, -1):
        bwd[i] = b
        if i:
            b = tabs[(i - 1, i)].dot(b * tabs[(i,)])
            b = b / b.sum()
    marg = np.stack([fwd[i] * bwd[i] / (fwd[i] * bwd[i]).sum() for i in range(n)])
    return float(shift), marg


def condition(g, inputs, cut):
    """include/mlbp_cutset.h in NumPy: (log_z, marginals [n_vars][X] in g.var_order) for the cutset `cut` (variable ids)."""
    X, order = g.X, g.var_order
    free = [v for v in order if v not in cut]
    facs = _factor_arrays(g, inputs)
    edges = [(vs, T) for vs, T in facs if len(vs) == 2 and vs[0] not in cut and vs[1] not in cut]
    parent, walk = {}, []
    for root in free:                                           # breadth-first over every tree of the remainder
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

    def toward(k, frm, vec):                                    # the message through forest factor k away from variable `frm`
        vs, T = edges[k]
        return vec.dot(T) if vs[0] == frm else T.dot(vec)
    Z, acc = 0.0, {v: np.zeros(X) for v in order}
    for states in itertools.product(range(X), repeat=len(cut)):
        s = dict(zip(cut, states))
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
                phi[vs[1]] = phi[vs[1]] * T[s[vs[0]], :]        # a row of the table on the free variable
            elif vs[1] in s:
                phi[vs[0]] = phi[vs[0]] * T[:, s[vs[1]]]        # a column
        bel, up = {v: phi[v].copy() for v in free}, {}
        Zc = const
        for v in reversed(walk):                                # leaves to roots
            if parent[v] is None:
                Zc *= bel[v].sum()
            else:
                par, k = parent[v]
                up[v] = toward(k, v, bel[v])
                bel[par] = bel[par] * up[v]
        dn = {}
        for v in walk:                                          # roots to leaves
            if parent[v] is not None:
                par, k = parent[v]
                excl = phi[par] * (dn[par] if par in dn else 1.0)
                for w in free:
                    if w != v and parent[w] is not None and parent[w][0] == par:
                        excl = excl * up[w]
                dn[v] = toward(k, par, excl)
                bel[v] = bel[v] * dn[v]
        Z += Zc
        for v in free:
            acc[v] += Zc * bel[v] / bel[v].sum() if Zc > 0 else 0.0
        for v in cut:
            acc[v][s[v]] += Zc                                  # the indicator of its state, unconditionally
    if Z == 0:
        return -np.inf, np.full((len(order), X), 1.0 / X)
    return float(np.log(Z)), np.stack([acc[v] / Z for v in order])


def chosen_ids(spec):
    """cutset.choose of the spec's topology, as variable ids."""
    from macaronicusermodeling_amd import cutset as S
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(spec)
    return [topo.var_ids[i] for i in S.choose(topo)]


def bp_marginals(spec, inputs):
    """The oracle's sweeps rooted at every variable in turn: [n_vars][X] in g.var_order."""
    g, msgs, _ = helpers.oracle_msgs(spec, inputs, list(O.Graph(spec).var_order))
    return np.stack([O.marginal(g, msgs, v) for v in g.var_order])


SMALL = [('k3_x5', lambda: kn_spec(3, 5)), ('k4_x4', lambda: kn_spec(4, 4)), ('k5_x3', lambda: kn_spec(5, 3)),
         ('ring6_x4', lambda: C.ring_spec(6, 4)), ('chain5_x8', lambda: C.chain_spec(5, 8)), ('shuffled_x5', lambda: C.shuffled_ids_spec(5)),
         ('user_p3', lambda: C.user_spec(6, [0, 2, 5], 16, 16)), ('user_p4', lambda: C.user_spec(8, [1, 2, 5, 7], 6, 6)),
         ('double_pair_x5', lambda: double_pair_spec(5)), ('forest_x4', lambda: forest_spec(4))]


@pytest.mark.parametrize('name,make', SMALL, ids=[s[0] for s in SMALL])
def test_conditioning_equals_enumeration(name, make):
    spec = make()
    g = O.Graph(spec)
    cut = chosen_ids(spec)
    kinds = ('uniform',) if spec['style'] == 'trainmp' else ('uniform', 'lognormal')
    for kind in kinds:
        for seed in (3, 4, 5):
            inputs = C.make_inputs(spec, seed, kind)
            want_z, want_m, _ = enumerate_exact(g, inputs)
            got_z, got_m = condition(g, inputs, cut)
            err_z, err_m = abs(got_z - want_z), float(np.abs(got_m - want_m).max())
            print('%s %s seed %d cutset %r: |log_z - enumeration| %.1e, marginals %.1e' % (name, kind, seed, cut, err_z, err_m))
            assert err_z <= 1e-12 * max(1.0, abs(want_z)) and err_m <= 1e-12
            if name.startswith('user'):
                off = float(np.abs(bp_marginals(spec, inputs) - want_m).max())
                print('    loopy BP is %.1e away from the exact marginals' % off)
                assert off > 1e-6                                # the GPU bar of 1e-10 separates exact from BP


def test_any_valid_cutset_gives_the_same_answer():
    spec = kn_spec(3, 5)
    g, inputs = O.Graph(spec), C.make_inputs(spec, 8)
    want_z, want_m, _ = enumerate_exact(g, inputs)
    for cut in ([0], [1], [2], [0, 1], [2, 0], [0, 1, 2]):
        z, m = condition(g, inputs, cut)
        assert abs(z - want_z) <= 1e-12 and np.abs(m - want_m).max() <= 1e-12, cut
    spec = C.chain_spec(4, 3)
    g, inputs = O.Graph(spec), C.make_inputs(spec, 9)
    z0, m0 = condition(g, inputs, [])
    z1, m1 = condition(g, inputs, [2])
    assert abs(z0 - z1) <= 1e-12 and np.abs(m0 - m1).max() <= 1e-12


def test_the_large_size_references_equal_enumeration():
    for spec in (kn_spec(4, 4), C.ring_spec(3, 7), kn_spec(3, 6), C.shuffled_ids_spec(5)):
        g, inputs = O.Graph(spec), C.make_inputs(spec, 12, 'lognormal')
        want_z, want_m, _ = enumerate_exact(g, inputs)
        z, m = eliminate(g, inputs)
        assert abs(z - want_z) <= 1e-12 * max(1.0, abs(want_z)) and np.abs(m - want_m).max() <= 1e-13, spec['name']
    spec = C.chain_spec(7, 3)
    g, inputs = O.Graph(spec), C.make_inputs(spec, 13)
    want_z, want_m, _ = enumerate_exact(g, inputs)
    z, m = chain_forward_backward(g, inputs)
    assert abs(z - want_z) <= 1e-12 * max(1.0, abs(want_z)) and np.abs(m - want_m).max() <= 1e-13


def wide_inputs(spec, seed):
    """Tables exp(20 N(0, 1)): 170 decades."""
    rs = np.random.RandomState(seed)
    n = 1 + max(f['table'] for f in spec['factors'])
    shape = {f['table']: (spec['X'], spec['X']) if len(f['vars']) == 2 else (spec['X'], 1) for f in spec['factors']}
    return dict(tables=[np.exp(20.0 * rs.randn(*shape[t])) for t in range(n)])


def test_the_wide_range_grid_is_finite():
    spec = kn_spec(3, 64)
    z, m, grid = enumerate_exact(O.Graph(spec), wide_inputs(spec, 21))
    assert np.isfinite(grid).all() and np.isfinite(z) and np.isfinite(m).all()
    assert np.abs(m.sum(axis=1) - 1).max() <= 1e-12


# ------------------------------------------------------------------------------------------------
# the cutset choice
# ------------------------------------------------------------------------------------------------
def _S():
    from macaronicusermodeling_amd import cutset
    return cutset


def _topo(spec):
    from macaronicusermodeling_amd.topology import GraphTopology
    return GraphTopology.from_spec(spec)


def _is_forest(n_vars, edges, removed):
    root = list(range(n_vars))

    def find(v):
        while root[v] != v:
            v = root[v]
        return v
    for a, b in edges:
        if a in removed or b in removed:
            continue
        ra, rb = find(a), find(b)
        if ra == rb:
            return False
        root[ra] = rb
    return True


def test_choose_returns_the_documented_cutsets():
    S = _S()
    for n in (3, 4, 5, 6):
        assert S.choose(_topo(kn_spec(n, 4))) == list(range(n - 2))
    for n in (3, 5, 6):
        assert S.choose(_topo(C.ring_spec(n, 4))) == [0]
    assert S.choose(_topo(C.chain_spec(5, 4))) == [] and S.choose(_topo(C.star_spec(4, 4))) == [] and S.choose(_topo(forest_spec(4))) == []
    assert S.choose(_topo(double_pair_spec(4))) == [0]          # two factors over one pair are a cycle; the tie goes to the first
    topo = _topo(C.shuffled_ids_spec(5))                         # the triangle 7 - 2 - 11 with the tail 11 - 5: 11 has degree 2 in the core too
    assert [topo.var_ids[i] for i in S.choose(topo)] == [7]
    assert S.choose(_topo(C.user_spec(10, [1, 4, 7], 64, 64, seed=1))) == [0]


def test_the_remainder_of_choose_is_a_forest_on_random_graphs():
    S = _S()
    rs = np.random.RandomState(7)
    loopy = 0
    for i in range(60):
        spec = helpers.random_spec(rs, 'random%d' % i, X=4)
        topo = _topo(spec)
        cut = S.choose(topo)
        edges = S.pair_edges(topo)
        assert _is_forest(topo.n_vars, edges, set(cut)), spec['name']
        assert S.choose(topo) == cut                             # deterministic
        assert bool(cut) == (not _is_forest(topo.n_vars, edges, set())), spec['name']
        for drop in range(len(cut)):                             # no chosen variable is redundant at the time it is taken
            assert not _is_forest(topo.n_vars, edges, set(cut[:drop])), spec['name']
        words = S.plan_words(topo, cut)
        assert S.lib.mlbp_cutset_check_plan(_ffi().i32ptr(words), len(words), 4) == 0, S.last_error()
        loopy += bool(cut)
    assert loopy >= 10


def _ffi():
    from macaronicusermodeling_amd import _ffi
    return _ffi


# ------------------------------------------------------------------------------------------------
# C ABI of libmlbp_cutset.so
# ------------------------------------------------------------------------------------------------
def test_every_declared_symbol_is_exported_and_bound_and_nothing_else():
    """What this library adds to the shared contract (tests/test_side_libraries_cpu.py: the bound functions are the declared
    and the exported ones, the constants and the struct are the header's)."""
    assert _S().MAX_CONFIGS == 65536


def _valid_args(S, X=64, n_cut=1):
    """Arguments of K3 that pass every host-side check (the pointers are never dereferenced on the host)."""
    topo = _topo(kn_spec(3, 4))
    words = S.plan_words(topo, list(range(n_cut)))
    a = S.CutsetArgs()
    a.B, a.X, a.n_vars, a.P, a.U = 2, X, 3, 3, 3
    a.n_cut, a.n_free, a.n_items, a.n_consts, a.n_forest = (int(w) for w in words[3:8])
    a.n_pair_tables, a.n_unary_tables, a.plan_words = 6, 6, len(words)
    for name, typ in S.CutsetArgs._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, name, 4096)
    a.workspace_bytes = 1 << 40
    return a


def test_library_identity_and_bad_arguments():
    S = _S()
    E = _ffi()
    assert S.lib.mlbp_cutset_arch() == b'gfx950'
    assert S.lib.mlbp_cutset_f64(None, None) == E.MLBP_EINVAL and 'NULL' in S.last_error()
    for field, value, word in (('B', 0, 'sizes'), ('X', 1, 'two states'), ('n_free', 1, 'sizes'), ('plan', None, 'plan'), ('plan_words', 5, 'plan'),
                               ('pair_tab', None, 'pair_tab'), ('n_unary_tables', 0, 'unary_tables'), ('log_z', None, 'log_z'),
                               ('marginals', None, 'marginals'), ('labels', None, 'labels'), ('workspace', None, 'workspace'),
                               ('workspace_bytes', 8, 'workspace')):
        a = _valid_args(S)
        setattr(a, field, value)
        assert S.lib.mlbp_cutset_f64(ctypes.byref(a), None) == E.MLBP_EINVAL, field
        assert word in S.last_error(), (field, S.last_error())
        assert S.lib.mlbp_cutset_last_kernel() == S.KERNEL_NONE
    a = _valid_args(S, X=1025)
    assert S.lib.mlbp_cutset_f64(ctypes.byref(a), None) == E.MLBP_EUNSUPPORTED and '1024' in S.last_error()
    a = _valid_args(S, X=1024, n_cut=2)
    assert S.lib.mlbp_cutset_f64(ctypes.byref(a), None) == E.MLBP_EUNSUPPORTED and 'configurations' in S.last_error()
    with pytest.raises(S.CutsetError):
        S.check(E.MLBP_EINVAL)


def test_compute_entry_fails_loudly_without_a_gpu():
    import torch
    S = _S()
    if torch.cuda.is_available():
        return                                                  # (the GPU module runs the entry for real)
    for X in (64, 128, 1024):
        a = _valid_args(S, X=X)
        a.labels = a.score = a.joint_logp = None                # all three are optional
        assert S.lib.mlbp_cutset_f64(ctypes.byref(a), None) == _ffi().MLBP_ENODEVICE
        assert 'no CPU fallback' in S.last_error() and S.lib.mlbp_cutset_last_kernel() == S.KERNEL_NONE


def test_kernel_choice_chunks_and_workspace_are_the_rules_of_the_header():
    S = _S()
    E = _ffi()

    def ints(P, U):
        return 4 * ((P + U + 16 + 3) // 4 * 4)

    def vectors(n_vars, X):
        return (5 * n_vars + 2) * ((X + 1) // 2 * 2) * 8

    def rule(X, n_vars, P, U, n_forest):
        if X == 64 and n_forest * 33280 + 21 * n_vars * 512 + 64 + ints(P, U) <= S.X64_LDS_BYTES:
            return S.KERNEL_X64
        return S.KERNEL_GENERIC

    def in_workspace(X, n_vars, P, U, n_forest):
        return rule(X, n_vars, P, U, n_forest) == S.KERNEL_GENERIC and vectors(n_vars, X) + 64 + ints(P, U) > S.GENERIC_LDS_BYTES

    def chunks(B, n_configs):
        return min(n_configs, -(-S.MIN_WORKGROUPS // B))
    shapes = ((64, 3, 3, 3, 1), (64, 4, 6, 4, 1), (64, 3, 2, 3, 2), (64, 4, 3, 4, 3), (64, 3, 3, 12, 1), (63, 3, 3, 3, 1), (2, 260, 259, 260, 259),
              (257, 3, 3, 3, 1), (301, 3, 3, 3, 1), (1024, 3, 3, 3, 1), (7, 5, 5, 5, 3), (64, 5, 4, 5, 2), (64, 6, 5, 6, 2), (64, 9, 8, 9, 1), (64, 10, 9, 10, 1))
    for shape in shapes:
        assert S.pick_kernel(*shape) == rule(*shape), shape
    # both sides of the X = 64 budget: two forest tables fit, three do not; with two, 5 variables fit and 6 do not; with one, 9 and 10
    assert S.pick_kernel(64, 3, 2, 3, 2) == S.KERNEL_X64 and S.pick_kernel(64, 4, 3, 4, 3) == S.KERNEL_GENERIC
    assert S.pick_kernel(64, 5, 4, 5, 2) == S.KERNEL_X64 and S.pick_kernel(64, 6, 5, 6, 2) == S.KERNEL_GENERIC
    assert S.pick_kernel(64, 9, 8, 9, 1) == S.KERNEL_X64 and S.pick_kernel(64, 10, 9, 10, 1) == S.KERNEL_GENERIC
    assert not in_workspace(301, 3, 3, 3, 1) and in_workspace(1024, 3, 3, 3, 1)
    assert S.lib.mlbp_cutset_pick_kernel(1025, 3, 3, 3, 1) == E.MLBP_EUNSUPPORTED
    assert S.lib.mlbp_cutset_pick_kernel(1, 3, 3, 3, 1) == E.MLBP_EINVAL
    assert S.lib.mlbp_cutset_pick_kernel(64, 3, 3, 3, 4) == E.MLBP_EINVAL            # more forest tables than pairwise factors
    for B, n in ((1, 64), (1, 4096), (2, 4096), (3, 64), (8192, 64), (600, 7), (256, 3), (511, 4), (512, 4), (1, 1), (9, 65536)):
        assert S.chunks(B, n) == chunks(B, n), (B, n)
    assert (S.chunks(1, 4096), S.chunks(2, 4096), S.chunks(8192, 64), S.chunks(3, 64)) == (512, 256, 1, 64)
    assert S.lib.mlbp_cutset_chunks(0, 1) == E.MLBP_EINVAL and S.lib.mlbp_cutset_chunks(1, 0) == E.MLBP_EINVAL
    for B in (1, 3, 8192):
        for shape in shapes:
            X, n_vars, P, U, n_forest = shape
            for n_cut in (0, 1, 2):
                if X ** n_cut > S.MAX_CONFIGS or n_cut > n_vars:
                    continue
                per = (n_vars * X + 2) * (4 if rule(*shape) == S.KERNEL_X64 else 1) + (vectors(n_vars, X) // 8 if in_workspace(*shape) else 0)
                assert S.workspace_bytes(B, X, n_vars, P, U, n_forest, n_cut) == B * chunks(B, X ** n_cut) * per * 8, (B, shape, n_cut)
    assert S.lib.mlbp_cutset_workspace_bytes(1, 64, 4, 6, 4, 1, 3) == E.MLBP_EUNSUPPORTED and 'configurations' in S.last_error()
    assert S.lib.mlbp_cutset_workspace_bytes(1, 1024, 3, 3, 3, 1, 2) == E.MLBP_EUNSUPPORTED
    assert S.lib.mlbp_cutset_workspace_bytes(0, 64, 3, 3, 3, 1, 1) == E.MLBP_EINVAL
    assert S.workspace_bytes(8192, 1024, 40, 39, 40, 39, 0) > 2 ** 31                   # 64-bit


def _sections(S, words):
    """{name: (offset, length)} of a packed plan."""
    n, P, U, n_cut, n_free, n_items, n_consts = (int(w) for w in words[:7])
    out, at = {}, S.PLAN_HEADER
    for name, length in (('cutset', n_cut), ('order', n_free), ('parent', 2 * n), ('item_off', n + 1), ('items', 3 * n_items),
                         ('consts', 4 * n_consts), ('pav', 2 * P), ('uvar', U), ('fslot', P)):
        out[name] = (at, length)
        at += length
    assert at == len(words)
    return out


def test_check_plan_refuses_each_of_its_cases():
    S = _S()
    E = _ffi()

    def check(words, X=4):
        w = np.ascontiguousarray(words, dtype=np.int32)
        return S.lib.mlbp_cutset_check_plan(E.i32ptr(w), len(w), X)
    topo = _topo(kn_spec(4, 4))
    good = S.plan_words(topo, [0, 1])
    sec = _sections(S, good)
    assert check(good) == E.MLBP_OK
    assert check(good, 64) == E.MLBP_OK                                     # 64^2 = 4096 configurations
    assert check(good, 1024) == E.MLBP_EUNSUPPORTED and 'configurations' in S.last_error()      # 1024^2
    assert check(S.plan_words(topo, [0, 1, 2, 3]), 64) == E.MLBP_EUNSUPPORTED and 'configurations' in S.last_error()   # 64^4
    assert check(S.plan_words(topo, [0, 1, 2, 3]), 16) == E.MLBP_OK         # 16^4 = 65536: the limit itself
    assert check(good, 1025) == E.MLBP_EUNSUPPORTED and check(good, 1) == E.MLBP_EINVAL
    assert S.lib.mlbp_cutset_check_plan(None, 16, 4) == E.MLBP_EINVAL and 'NULL' in S.last_error()
    assert check(good[:-1]) == E.MLBP_EINVAL and 'words' in S.last_error()

    def poke(section, index, value, word, base=good, secs=sec):
        bad = base.copy()
        bad[secs[section][0] + index] = value
        assert check(bad) == E.MLBP_EINVAL, (section, index, value)
        assert word in S.last_error(), (section, index, value, S.last_error())
    poke('cutset', 0, 4, 'out of range')
    poke('cutset', 0, -1, 'out of range')
    poke('cutset', 1, 0, 'repeated')
    poke('order', 0, 0, 'order')                                             # a cutset variable
    poke('order', 0, int(good[sec['order'][0] + 1]), 'order')                # repeated
    poke('order', 1, 9, 'order')
    child = int(good[sec['order'][0]])
    poke('parent', 2 * child, 6, 'parent link')                              # a factor outside [0, P)
    poke('parent', 2 * child, 0, 'parent link')                              # a factor that does not join the two
    poke('parent', 2 * child + 1, child, 'parent link')                      # its own parent
    poke('parent', 0, 5, 'cutset variable')
    poke('item_off', 0, 1, 'item_off')
    poke('item_off', 4, 99, 'item_off')
    poke('items', 0, 7, 'unknown kind')
    poke('items', 1, 3, 'unary factor')
    poke('items', 1, -1, 'unary factor')
    first_pair_item = next(i for i in range(int(good[5])) if good[sec['items'][0] + 3 * i] != S.ITEM_UNARY)
    poke('items', 3 * first_pair_item + 1, 6, 'pair factor')
    poke('items', 3 * first_pair_item + 2, 2, 'cut position')
    poke('consts', 0, 9, 'unknown kind')
    poke('consts', 2, 2, 'cut position')
    poke('consts', 1, 2, 'unary factor')
    poke('pav', 0, 4, 'out of range')
    poke('pav', 0, int(good[sec['pav'][0] + 1]), 'itself')
    poke('uvar', 0, -1, 'out of range')
    poke('fslot', 0, 0, 'forest_slot')
    forest_factor = int(good[sec['parent'][0] + 2 * child])
    poke('fslot', forest_factor, 1, 'forest_slot')
    # a factor used twice; a factor left out
    items0 = sec['items'][0]
    bad = good.copy()
    bad[items0 + 3:items0 + 6] = bad[items0:items0 + 3]
    assert check(bad) == E.MLBP_EINVAL and ('twice' in S.last_error() or 'is not on' in S.last_error())
    # a remainder with a cycle: the message names the cycle's variables
    ring = _topo(C.ring_spec(5, 4))
    assert check(S.plan_words(ring, [])) == E.MLBP_EINVAL
    assert 'cycle' in S.last_error() and '2 - 1 - 0 - 4 - 3 - 2' in S.last_error(), S.last_error()
    assert check(S.plan_words(ring, [3])) == E.MLBP_OK                       # any variable of the ring will do
    k4 = S.plan_words(topo, [0])
    assert check(k4) == E.MLBP_EINVAL and 'cycle' in S.last_error()
    assert check(S.plan_words(_topo(double_pair_spec(4)), [])) == E.MLBP_EINVAL and 'cycle' in S.last_error() and '1 - 0 - 1' in S.last_error()     # from the closing factor's axis-0 variable
    with pytest.raises(S.CutsetError, match='cycle'):
        S.Plan(ring, [], 4, None)
    with pytest.raises(ValueError):
        S.Plan(ring, [0, 0], 4, None)
    with pytest.raises(ValueError):
        S.Plan(ring, [5], 4, None)
