"""Exact pair marginals, expected features and the true gradient by cutset conditioning without a GPU: the float64 references
the GPU tests compare against, the NumPy statement of include/mlbp_exactgrad.h pinned on exhaustive enumeration, the
derivative identity, the gap that tells exact from BP and the host checks of libmlbp_exactgrad.so
(the contract it shares with the other side libraries is in tests/test_side_libraries_cpu.py).

References.  pair_marginals_enum() is the log-domain grid of test_cutset_cpu.enumerate_exact summed over the axes of the other
variables: nothing of the algorithm under test is in it.  condition_pairs() states the header in NumPy -- condition on every
joint state of the cutset, one pass up, one pass down, a rank-1 update per forest factor with the table applied once at the end,
a row or column per cutset-incident factor, a cell per cutset-internal factor -- and must equal the grid.  features_of() is the
header's contraction of pair marginals and marginals with phi."""
import ctypes
import itertools

import numpy as np
import pytest

import cases as C
import helpers
import test_cutset_cpu as R
import test_map_cpu as W
from oracle import lbp_oracle as O


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def pair_factors(g):
    """[(factor id, variable on table axis 0, variable on axis 1)] of every pairwise factor, in id order."""
    out = []
    for f in g.factors:
        if len(f['vars']) == 2:
            by_axis = {g.dim_of(f, v): v for v in f['vars']}
            out.append((f['id'], by_axis[0], by_axis[1]))
    return out


def pair_marginals_enum(g, inputs):
    """(log_z, marginals [n_vars][X] in g.var_order, {factor id: M [X][X] in the table's axes}) by exhaustive enumeration."""
    log_z, marg, grid = R.enumerate_exact(g, inputs)
    order, n = list(g.var_order), grid.ndim
    pairs = {}
    for fid, va, vb in pair_factors(g):
        a, b = order.index(va), order.index(vb)
        rest = tuple(k for k in range(n) if k not in (a, b))
        M = np.exp((R.logsumexp(grid, axis=rest) if rest else grid) - log_z)
        pairs[fid] = M if a < b else M.T
    return log_z, marg, pairs


def eliminate_pairs(g, inputs):
    """{factor id: M} where X^n is too large for the grid: every other variable summed out by einsum (BLAS where it can) over
    tables divided by their largest entry; pinned on the grid below."""
    letters = {v: chr(ord('a') + i) for i, v in enumerate(g.var_order)}
    facs = [(vs, T / T.max()) for vs, T in R._factor_arrays(g, inputs)]
    out = {}
    for fid, va, vb in pair_factors(g):
        expr = ','.join(''.join(letters[v] for v in vs) for vs, _ in facs) + '->' + letters[va] + letters[vb]
        M = np.einsum(expr, *[T for _, T in facs], optimize=True)
        out[fid] = M / M.sum()
    return out


def condition_pairs(g, inputs, cut):
    """include/mlbp_exactgrad.h in NumPy: (log_z, marginals [n_vars][X] in g.var_order, {factor id: M}) for the cutset `cut`
    (variable ids).  The walk is test_cutset_cpu.condition's; a forest factor accumulates (Z_c / a^T T b) a b^T and takes its
    table once, at the end."""
    X, order = g.X, list(g.var_order)
    free = [v for v in order if v not in cut]
    facs = [(f['id'],) + fa for f, fa in zip(g.factors, R._factor_arrays(g, inputs))]
    edges = [(fid, vs, T) for fid, vs, T in facs if len(vs) == 2 and vs[0] not in cut and vs[1] not in cut]
    parent, walk = {}, []
    for root in free:
        if root in parent:
            continue
        parent[root] = None
        queue = [root]
        while queue:
            v = queue.pop(0)
            walk.append(v)
            for k, (_, vs, T) in enumerate(edges):
                if v in vs:
                    w = vs[1] if vs[0] == v else vs[0]
                    if w not in parent:
                        parent[w] = (v, k)
                        queue.append(w)
    assert len(edges) == sum(1 for v in free if parent[v] is not None), 'the remainder has a cycle'

    def toward(k, frm, vec):
        _, vs, T = edges[k]
        return vec.dot(T) if vs[0] == frm else T.dot(vec)
    Z, acc = 0.0, {v: np.zeros(X) for v in order}
    pacc = {fid: np.zeros((X, X)) for fid, vs, _ in facs if len(vs) == 2}
    forest = set()
    for states in itertools.product(range(X), repeat=len(cut)):
        s = dict(zip(cut, states))
        const, phi = 1.0, {v: np.ones(X) for v in free}
        for _, vs, T in facs:
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
        Zc = const
        for v in reversed(walk):                                # leaves to roots
            if parent[v] is None:
                Zc *= bel[v].sum()
            else:
                par, k = parent[v]
                up[v] = toward(k, v, bel[v])
                bel[par] = bel[par] * up[v]
        if not Zc > 0:
            continue
        dn = {}
        for v in walk:                                          # roots to leaves
            if parent[v] is not None:
                par, k = parent[v]
                excl = phi[par] * (dn[par] if par in dn else 1.0)
                for w in free:
                    if w != v and parent[w] is not None and parent[w][0] == par:
                        excl = excl * up[w]
                dn[v] = toward(k, par, excl)
                fid, vs, T = edges[k]
                a = bel[v]                                      # v's vector on the way up
                norm = float(a.dot(dn[v]))                      # a^T T b
                pacc[fid] += (Zc / norm) * (np.outer(a, excl) if vs[0] == v else np.outer(excl, a))
                forest.add(fid)
                bel[v] = bel[v] * dn[v]
        Z += Zc
        m_c = {v: bel[v] / bel[v].sum() for v in free}
        for v in free:
            acc[v] += Zc * m_c[v]
        for v in cut:
            acc[v][s[v]] += Zc
        for fid, vs, T in facs:
            if len(vs) != 2:
                continue
            if vs[0] in s and vs[1] in s:
                pacc[fid][s[vs[0]], s[vs[1]]] += Zc            # a cell
            elif vs[0] in s:
                pacc[fid][s[vs[0]], :] += Zc * m_c[vs[1]]      # a row
            elif vs[1] in s:
                pacc[fid][:, s[vs[1]]] += Zc * m_c[vs[0]]      # a column
    if Z == 0:
        return -np.inf, np.full((len(order), X), 1.0 / X), {fid: np.full((X, X), 1.0 / X ** 2) for fid in pacc}
    tables = {fid: T for fid, vs, T in facs if len(vs) == 2}
    pairs = {fid: (A * tables[fid] if fid in forest else A) / Z for fid, A in pacc.items()}
    return float(np.log(Z)), np.stack([acc[v] / Z for v in order]), pairs


# ---- features -------------------------------------------------------------------------------------
def make_features(g, seed, F_ee=3, F_ed=6, Vde=None, kinds=None):
    """phi tensors drawn in [-1, 1] and, per factor id, the selector (pair_phi in {0, 1} / unary_kind in {0, 1, 2}) and the
    observed column of every unary factor."""
    rs = np.random.RandomState(seed)
    X = g.X
    Vde = X + 3 if Vde is None else Vde
    feat = dict(phi_en_en=rs.uniform(-1, 1, (X, X, F_ee)), phi_en_en_w1=rs.uniform(-1, 1, (X, X, F_ee)),
                phi_en_de=rs.uniform(-1, 1, (X, Vde, F_ed)), sel={}, obs={})
    n_unary = 0
    for f in g.factors:
        if len(f['vars']) == 2:
            feat['sel'][f['id']] = int(rs.randint(0, 2))
        else:
            kind = int(rs.randint(0, 3)) if kinds is None else kinds[n_unary % len(kinds)]
            n_unary += 1
            feat['sel'][f['id']] = kind
            feat['obs'][f['id']] = int(rs.randint(0, Vde if kind == 2 else X))
    return feat


def unary_phi(feat, fid):
    """([X][F] slab of unary factor fid at its observed column, 'ee' or 'ed')."""
    kind = feat['sel'][fid]
    phi = (feat['phi_en_en'], feat['phi_en_en_w1'], feat['phi_en_de'])[kind]
    return phi[:, feat['obs'][fid], :], 'ed' if kind == 2 else 'ee'


def features_of(g, feat, marg, pairs):
    """(ee [F_ee], ed [F_ed]): the header's contraction of pair marginals {factor id: [X][X]} and marginals [n_vars][X] (in
    g.var_order) with phi.  With indicators in place of both it is the observed feature vector."""
    order = list(g.var_order)
    out = dict(ee=np.zeros(feat['phi_en_en'].shape[2]), ed=np.zeros(feat['phi_en_de'].shape[2]))
    for f in g.factors:
        if len(f['vars']) == 2:
            phi = feat['phi_en_en_w1'] if feat['sel'][f['id']] else feat['phi_en_en']
            out['ee'] += np.tensordot(pairs[f['id']], phi, axes=([0, 1], [0, 1]))
        else:
            slab, which = unary_phi(feat, f['id'])
            out[which] += marg[order.index(f['vars'][0])].dot(slab)
    return out['ee'], out['ed']


def observed_of(g, feat, labels):
    """The observed features at labels {variable id: state}."""
    X, order = g.X, list(g.var_order)
    marg = np.zeros((len(order), X))
    for i, v in enumerate(order):
        marg[i, labels[v]] = 1.0
    pairs = {}
    for fid, va, vb in pair_factors(g):
        pairs[fid] = np.zeros((X, X))
        pairs[fid][labels[va], labels[vb]] = 1.0
    return features_of(g, feat, marg, pairs)


def theta_inputs(g, feat, th_ee, th_ed):
    """The explicit-style inputs whose tables are exp(phi . theta), as the trainer builds them."""
    n = 1 + max(f['table'] for f in g.factors)
    tables = [None] * n
    for f in g.factors:
        if len(f['vars']) == 2:
            phi = feat['phi_en_en_w1'] if feat['sel'][f['id']] else feat['phi_en_en']
            tables[f['table']] = np.exp(phi.dot(th_ee))
        else:
            slab, which = unary_phi(feat, f['id'])
            tables[f['table']] = np.exp(slab.dot(th_ed if which == 'ed' else th_ee)).reshape(-1, 1)
    return dict(tables=tables)


# ------------------------------------------------------------------------------------------------
# the statement against the grid
# ------------------------------------------------------------------------------------------------
SMALL = [('k3_x4', lambda: R.kn_spec(3, 4)), ('k4_x4', lambda: R.kn_spec(4, 4)), ('ring5_x3', lambda: C.ring_spec(5, 3)),
         ('double_pair_x5', lambda: R.double_pair_spec(5)), ('forest_x4', lambda: R.forest_spec(4)), ('chain3_x5', lambda: C.chain_spec(3, 5)),
         ('shuffled_x4', lambda: C.shuffled_ids_spec(4))]


def worst_gap(got, want):
    return max(float(np.abs(got[fid] - want[fid]).max()) for fid in want)


@pytest.mark.parametrize('name,make', SMALL, ids=[s[0] for s in SMALL])
def test_statement_equals_enumeration(name, make):
    spec = make()
    g = O.Graph(spec)
    cut = R.chosen_ids(spec)
    for kind in ('uniform', 'lognormal'):
        for seed in (3, 4, 5):
            inputs = C.make_inputs(spec, seed, kind)
            want_z, want_m, want_p = pair_marginals_enum(g, inputs)
            z, m, p = condition_pairs(g, inputs, cut)
            err = worst_gap(p, want_p)
            print('%s %s seed %d cutset %r: pair marginals within %.1e of enumeration' % (name, kind, seed, cut, err))
            assert set(p) == set(want_p) and err <= 1e-12
            assert abs(z - want_z) <= 1e-12 * max(1.0, abs(want_z)) and np.abs(m - want_m).max() <= 1e-12
            order = list(g.var_order)
            for fid, va, vb in pair_factors(g):                 # every block sums to 1, rows and columns to the marginals
                assert abs(p[fid].sum() - 1) <= 1e-12
                assert np.abs(p[fid].sum(axis=1) - m[order.index(va)]).max() <= 1e-12
                assert np.abs(p[fid].sum(axis=0) - m[order.index(vb)]).max() <= 1e-12


def test_any_valid_cutset_gives_the_same_pair_marginals():
    spec = R.kn_spec(3, 5)
    g, inputs = O.Graph(spec), C.make_inputs(spec, 8)
    want = pair_marginals_enum(g, inputs)[2]
    for cut in ([0], [1], [2], [0, 1], [2, 0], [0, 1, 2]):
        assert worst_gap(condition_pairs(g, inputs, cut)[2], want) <= 1e-12, cut
    spec = C.chain_spec(4, 3)
    g, inputs = O.Graph(spec), C.make_inputs(spec, 9)
    want = pair_marginals_enum(g, inputs)[2]
    for cut in ([], [2], [1, 3]):
        assert worst_gap(condition_pairs(g, inputs, cut)[2], want) <= 1e-12, cut


def test_the_large_size_reference_equals_enumeration():
    for spec in (R.kn_spec(4, 4), C.ring_spec(3, 7), R.double_pair_spec(5), R.forest_spec(3)):
        g, inputs = O.Graph(spec), C.make_inputs(spec, 12, 'lognormal')
        assert worst_gap(eliminate_pairs(g, inputs), pair_marginals_enum(g, inputs)[2]) <= 1e-13, spec['name']


def test_an_all_zero_table_gives_uniform_blocks():
    spec = C.ring_spec(5, 3)
    inputs = C.make_inputs(spec, 1)
    pair_table = next(f['table'] for f in spec['factors'] if len(f['vars']) == 2)
    inputs['tables'][pair_table] = np.zeros_like(inputs['tables'][pair_table])
    z, m, p = condition_pairs(O.Graph(spec), inputs, R.chosen_ids(spec))
    assert z == -np.inf and (m == 1.0 / 3).all() and all((M == 1.0 / 9).all() for M in p.values())


# ------------------------------------------------------------------------------------------------
# the derivative identity
# ------------------------------------------------------------------------------------------------
def k3_one_unary_spec(X, unary_on):
    """K3 with ONE unary factor: P + U = 4, the largest count for which the finite-difference bar below is derived."""
    factors = [dict(id=0, vars=[unary_on], dims=[0], table=0), dict(id=1, vars=[0, 1], dims=[0, 1], table=1),
               dict(id=2, vars=[0, 2], dims=[1, 0], table=2), dict(id=3, vars=[1, 2], dims=[0, 1], table=3)]
    return dict(name='k3u_x%d' % X, style='explicit', X=X, var_ids=[0, 1, 2], labels=[1 % X, 0, 2 % X], factors=factors)


@pytest.mark.parametrize('kind', [0, 1, 2])
def test_the_gradient_is_the_derivative_of_joint_logp(kind):
    """grad against the central finite difference of the ENUMERATED joint_logp in every theta component at h = 1e-5, bar 1e-8.
    The truncation term is h^2 / 6 * |d^3|, and the third derivative of log Z in one component is a third cumulant of a sum of
    P + U features bounded by 1: |d^3| <= 8 (P + U)^3 = 512 at P + U = 4, so the term stays below 1e-10 / 6 * 512 = 8.6e-9."""
    h, bar = 1e-5, 1e-8
    for X, seed in ((3, 11), (4, 12)):
        spec = k3_one_unary_spec(X, unary_on=seed % 3)
        g = O.Graph(spec)
        assert sum(1 for f in g.factors) == 4
        feat = make_features(g, seed, kinds=[kind])
        rs = np.random.RandomState(seed + 100)
        th_ee, th_ed = rs.randn(3) * 0.5, rs.randn(6) * 0.5
        labels = dict(zip(g.var_order, (int(x) for x in rs.randint(0, X, size=3))))

        def joint(te, td):
            inputs = theta_inputs(g, feat, te, td)
            return W.score_of(g, inputs, labels) - R.enumerate_exact(g, inputs)[0]
        inputs = theta_inputs(g, feat, th_ee, th_ed)
        _, marg, pairs = condition_pairs(g, inputs, R.chosen_ids(spec))
        ex = features_of(g, feat, marg, pairs)
        ob = observed_of(g, feat, labels)
        grad = np.concatenate([ob[0] - ex[0], ob[1] - ex[1]])
        _, marg_e, pairs_e = pair_marginals_enum(g, inputs)
        ex_e = features_of(g, feat, marg_e, pairs_e)
        assert np.abs(np.concatenate(ex) - np.concatenate(ex_e)).max() <= 1e-12
        fd = np.zeros(9)
        for k in range(9):
            step = np.zeros(9)
            step[k] = h
            fd[k] = (joint(th_ee + step[:3], th_ed + step[3:]) - joint(th_ee - step[:3], th_ed - step[3:])) / (2 * h)
        print('kind %d X %d: |grad - finite difference| %.1e' % (kind, X, np.abs(grad - fd).max()))
        assert np.abs(grad - fd).max() <= bar, (kind, X, grad, fd)
        if kind == 2:
            assert np.abs(grad[3:]).max() > 1e-3                # the en_de half is exercised
        else:
            assert np.abs(grad[3:]).max() == 0.0


# ------------------------------------------------------------------------------------------------
# the bar tells exact from BP
# ------------------------------------------------------------------------------------------------
def test_bp_factor_beliefs_are_not_the_pair_marginals():
    """On the K3 user-shaped inputs of test_cutset_cpu, the reference's pairwise factor beliefs after three sweeps differ from
    the exact pair marginals by more than 1e-8 in some entry.  (A row of M_p sums to the marginal; the smallest marginal gap the
    project states is 3e-5, so the largest entry gap is at least 3e-5 / 64 = 4.7e-7.)"""
    spec = C.user_spec(6, [0, 2, 5], 16, 16)
    g = O.Graph(spec)
    for seed in (3, 4, 5):
        inputs = C.make_inputs(spec, seed)
        _, _, want = pair_marginals_enum(g, inputs)
        _, msgs, _ = helpers.oracle_msgs(spec, inputs, list(g.var_order))
        off = max(float(np.abs(O.factor_beliefs(g, inputs, msgs, fid) - want[fid]).max()) for fid in want)
        print('seed %d: BP factor beliefs are %.1e away from the exact pair marginals' % (seed, off))
        assert off > 1e-8
        assert worst_gap(condition_pairs(g, inputs, R.chosen_ids(spec))[2], want) <= 1e-12


# ------------------------------------------------------------------------------------------------
# C ABI of libmlbp_exactgrad.so
# ------------------------------------------------------------------------------------------------
def _M():
    from macaronicusermodeling_amd import exactgrad
    return exactgrad


def _ffi():
    from macaronicusermodeling_amd import _ffi
    return _ffi


def test_every_declared_symbol_is_exported_and_bound_and_nothing_else():
    """What this library adds to the shared contract (tests/test_side_libraries_cpu.py: the bound functions are the declared
    and the exported ones, the constants and the struct are the header's)."""
    M = _M()
    # the layout: 16 int32, then pointers, with the one int64 among them -- no padding anywhere
    assert M.ExactGradArgs.plan.offset == 64 and M.ExactGradArgs.workspace_bytes.offset == 64 + 13 * 8
    assert ctypes.sizeof(M.ExactGradArgs) == 64 + 21 * 8


def _valid_args(M, X=64, n_cut=1):
    """Arguments of K3 that pass every host-side check (the pointers are never dereferenced on the host)."""
    from macaronicusermodeling_amd import cutset
    words = cutset.plan_words(R._topo(R.kn_spec(3, 4)), list(range(n_cut)))
    a = M.ExactGradArgs()
    a.B, a.X, a.n_vars, a.P, a.U = 2, X, 3, 3, 3
    a.n_cut, a.n_free, a.n_items, a.n_consts, a.n_forest = (int(w) for w in words[3:8])
    a.n_pair_tables, a.n_unary_tables, a.plan_words = 6, 6, len(words)
    a.F_ee, a.F_ed, a.Vde = 3, 6, 70
    for name, typ in M.ExactGradArgs._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, name, 4096)
    a.workspace_bytes = 1 << 40
    return a


def test_library_identity_and_bad_arguments():
    M, E = _M(), _ffi()
    assert M.lib.mlbp_exactgrad_arch() == b'gfx950'
    assert M.lib.mlbp_exactgrad_f64(None, None) == E.MLBP_EINVAL and 'NULL' in M.last_error()
    for field, value, word in (('B', 0, 'sizes'), ('X', 1, 'two states'), ('n_free', 1, 'sizes'), ('plan', None, 'plan'), ('plan_words', 5, 'plan'),
                               ('pair_tab', None, 'pair_tab'), ('n_unary_tables', 0, 'unary_tables'), ('log_z', None, 'log_z'),
                               ('workspace', None, 'workspace'), ('workspace_bytes', 8, 'workspace'),
                               # a requested expect_* or grad_* without the feature inputs; grad_* without labels
                               ('phi_en_en', None, 'feature inputs'), ('phi_en_en_w1', None, 'feature inputs'), ('phi_en_de', None, 'feature inputs'),
                               ('pair_phi', None, 'feature inputs'), ('unary_kind', None, 'feature inputs'), ('unary_obs', None, 'feature inputs'),
                               ('F_ee', 0, 'feature inputs'), ('F_ed', 0, 'feature inputs'), ('Vde', 0, 'feature inputs'), ('labels', None, 'labels')):
        a = _valid_args(M)
        setattr(a, field, value)
        assert M.lib.mlbp_exactgrad_f64(ctypes.byref(a), None) == E.MLBP_EINVAL, field
        assert word in M.last_error(), (field, M.last_error())
        assert M.lib.mlbp_exactgrad_last_kernel() == M.KERNEL_NONE
    outputs = ('expect_ee', 'expect_ed', 'grad_ee', 'grad_ed')

    def with_only(only):
        a = _valid_args(M)
        for name in outputs:
            if name != only:
                setattr(a, name, None)
        return a
    for only in outputs:                                        # each of the four alone asks for the feature inputs,
        a = with_only(only)
        a.phi_en_de = None
        assert M.lib.mlbp_exactgrad_f64(ctypes.byref(a), None) == E.MLBP_EINVAL and 'feature inputs' in M.last_error(), only
    for only in outputs[2:]:                                    # and each grad_* alone for labels; expect_* does not
        a = with_only(only)
        a.labels = None
        assert M.lib.mlbp_exactgrad_f64(ctypes.byref(a), None) == E.MLBP_EINVAL and 'labels' in M.last_error(), only
    a = _valid_args(M, X=1025)
    assert M.lib.mlbp_exactgrad_f64(ctypes.byref(a), None) == E.MLBP_EUNSUPPORTED and '1024' in M.last_error()
    a = _valid_args(M, X=1024, n_cut=2)
    assert M.lib.mlbp_exactgrad_f64(ctypes.byref(a), None) == E.MLBP_EUNSUPPORTED and 'configurations' in M.last_error()
    a = _valid_args(M)
    a.F_ed = M.MAX_FEATURES + 1
    assert M.lib.mlbp_exactgrad_f64(ctypes.byref(a), None) == E.MLBP_EUNSUPPORTED and 'features' in M.last_error()
    with pytest.raises(M.ExactGradError):
        M.check(E.MLBP_EINVAL)


def test_compute_entry_fails_loudly_without_a_gpu():
    import torch
    M = _M()
    if torch.cuda.is_available():
        return                                                  # (the GPU module runs the entry for real)
    optional = ('marginals', 'pair_marginals', 'expect_ee', 'expect_ed', 'grad_ee', 'grad_ed')
    for X in (64, 128, 1024):
        for drop in ((), optional, optional[2:], ('labels', 'grad_ee', 'grad_ed')):
            a = _valid_args(M, X=X)
            for name in drop:
                setattr(a, name, None)
            if drop == optional:                                # no feature output: the feature inputs are not needed
                a.phi_en_en = a.phi_en_en_w1 = a.phi_en_de = a.pair_phi = a.unary_kind = a.unary_obs = a.labels = None
                a.F_ee = a.F_ed = a.Vde = 0
            assert M.lib.mlbp_exactgrad_f64(ctypes.byref(a), None) == _ffi().MLBP_ENODEVICE, (X, drop, M.last_error())
            assert 'no CPU fallback' in M.last_error() and M.lib.mlbp_exactgrad_last_kernel() == M.KERNEL_NONE


def test_check_plan_is_the_shared_check():
    """The plan's validation is stated once (csrc/mlbp_cutset_plan.h): this library refuses what mlbp_cutset_check_plan refuses,
    case by case of tests/test_cutset_cpu.py, in the same words."""
    from macaronicusermodeling_amd import cutset as S
    M, E = _M(), _ffi()
    topo = R._topo(R.kn_spec(4, 4))
    good = S.plan_words(topo, [0, 1])
    sec = R._sections(S, good)
    ring = S.plan_words(R._topo(C.ring_spec(5, 4)), [])
    cases = [(good, 4), (good, 64), (good, 1024), (good, 1025), (good, 1), (good[:-1], 4), (ring, 4), (S.plan_words(topo, [0]), 4),
             (S.plan_words(topo, [0, 1, 2, 3]), 64), (S.plan_words(topo, [0, 1, 2, 3]), 16),
             (S.plan_words(R._topo(R.double_pair_spec(4)), []), 4)]
    child = int(good[sec['order'][0]])
    first_pair_item = next(i for i in range(int(good[5])) if good[sec['items'][0] + 3 * i] != S.ITEM_UNARY)
    for section, index, value in (('cutset', 0, 4), ('cutset', 0, -1), ('cutset', 1, 0), ('order', 0, 0), ('order', 1, 9),
                                  ('parent', 2 * child, 6), ('parent', 2 * child, 0), ('parent', 2 * child + 1, child), ('parent', 0, 5),
                                  ('item_off', 0, 1), ('item_off', 4, 99), ('items', 0, 7), ('items', 1, 3), ('items', 1, -1),
                                  ('items', 3 * first_pair_item + 1, 6), ('items', 3 * first_pair_item + 2, 2), ('consts', 0, 9),
                                  ('consts', 2, 2), ('consts', 1, 2), ('pav', 0, 4), ('pav', 0, int(good[sec['pav'][0] + 1])), ('uvar', 0, -1),
                                  ('fslot', 0, 0), ('fslot', int(good[sec['parent'][0] + 2 * child]), 1)):
        bad = good.copy()
        bad[sec[section][0] + index] = value
        cases.append((bad, 4))
    refused = 0
    for words, X in cases:
        w = np.ascontiguousarray(words, dtype=np.int32)
        rc = M.lib.mlbp_exactgrad_check_plan(E.i32ptr(w), len(w), X)
        assert rc == S.lib.mlbp_cutset_check_plan(E.i32ptr(w), len(w), X)
        if rc:
            refused += 1
            assert M.last_error() == S.last_error() and M.last_error()
    assert refused == len(cases) - 3
    assert M.lib.mlbp_exactgrad_check_plan(None, 16, 4) == E.MLBP_EINVAL and 'NULL' in M.last_error()
    with pytest.raises(M.ExactGradError, match='cycle'):
        M.Plan(R._topo(C.ring_spec(5, 4)), [], 4, None)
    with pytest.raises(M.ExactGradError, match='configurations') as err:
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
        if X == 64 and n_forest <= M.X64_MAX_FOREST and n_forest * 33280 + 21 * n_vars * 512 + 64 + ints(P, U) <= S.X64_LDS_BYTES:
            return M.KERNEL_X64
        return M.KERNEL_GENERIC

    def in_workspace(X, n_vars, P, U, n_forest):
        return rule(X, n_vars, P, U, n_forest) == M.KERNEL_GENERIC and vectors(n_vars, X) + 64 + ints(P, U) > S.GENERIC_LDS_BYTES

    def chunks(B, n_configs, kernel):
        walkers = -(-n_configs // 4) if kernel == M.KERNEL_X64 else n_configs
        return min(walkers, -(-M.MIN_WORKGROUPS // B))
    shapes = ((64, 3, 3, 3, 1), (64, 4, 6, 4, 1), (64, 3, 2, 3, 2), (64, 4, 3, 4, 3), (64, 3, 3, 12, 1), (63, 3, 3, 3, 1), (2, 260, 259, 260, 259),
              (257, 3, 3, 3, 1), (301, 3, 3, 3, 1), (1024, 3, 3, 3, 1), (7, 5, 5, 5, 3), (64, 5, 4, 5, 2), (64, 6, 5, 6, 2), (64, 9, 8, 9, 1), (64, 10, 9, 10, 1),
              (64, 2, 2, 2, 0), (64, 12, 11, 12, 0), (64, 13, 12, 13, 0))
    for shape in shapes:
        assert M.pick_kernel(*shape) == rule(*shape), shape
    # both sides of the register budget: two forest factors run on the X = 64 kernel, three do not (a chain of three / of four)
    assert M.pick_kernel(64, 3, 2, 3, 2) == M.KERNEL_X64 and M.pick_kernel(64, 4, 3, 4, 3) == M.KERNEL_GENERIC
    # both sides of the LDS budget: with two forest tables 5 variables fit and 6 do not; with one, 9 and 10; with none, 12 and 13
    assert M.pick_kernel(64, 5, 4, 5, 2) == M.KERNEL_X64 and M.pick_kernel(64, 6, 5, 6, 2) == M.KERNEL_GENERIC
    assert M.pick_kernel(64, 9, 8, 9, 1) == M.KERNEL_X64 and M.pick_kernel(64, 10, 9, 10, 1) == M.KERNEL_GENERIC
    assert M.pick_kernel(64, 12, 11, 12, 0) == M.KERNEL_X64 and M.pick_kernel(64, 13, 12, 13, 0) == M.KERNEL_GENERIC
    assert not in_workspace(301, 3, 3, 3, 1) and in_workspace(1024, 3, 3, 3, 1)
    assert M.lib.mlbp_exactgrad_pick_kernel(1025, 3, 3, 3, 1) == E.MLBP_EUNSUPPORTED
    assert M.lib.mlbp_exactgrad_pick_kernel(1, 3, 3, 3, 1) == E.MLBP_EINVAL
    assert M.lib.mlbp_exactgrad_pick_kernel(64, 3, 3, 3, 4) == E.MLBP_EINVAL
    for B, n in ((1, 64), (1, 4096), (2, 4096), (3, 64), (8192, 64), (600, 64), (600, 7), (256, 3), (255, 4), (256, 4), (128, 9), (1, 1), (9, 65536),
                 (16, 64), (17, 64), (1, 1023), (1, 1025)):
        for kernel in (M.KERNEL_X64, M.KERNEL_GENERIC):
            assert M.chunks(B, n, kernel) == chunks(B, n, kernel), (B, n, kernel)
    assert (M.chunks(3, 64, M.KERNEL_X64), M.chunks(3, 64, M.KERNEL_GENERIC), M.chunks(8192, 64, M.KERNEL_X64), M.chunks(2, 4096, M.KERNEL_X64),
            M.chunks(1, 1, M.KERNEL_X64)) == (16, 64, 1, 128, 1)
    assert M.lib.mlbp_exactgrad_chunks(0, 1, 1) == E.MLBP_EINVAL and M.lib.mlbp_exactgrad_chunks(1, 0, 1) == E.MLBP_EINVAL
    assert M.lib.mlbp_exactgrad_chunks(1, 1, 0) == E.MLBP_EINVAL and M.lib.mlbp_exactgrad_chunks(1, 1, 3) == E.MLBP_EINVAL
    for B in (1, 3, 8192):
        for shape in shapes:
            X, n_vars, P, U, n_forest = shape
            for n_cut in (0, 1, 2):
                if X ** n_cut > S.MAX_CONFIGS or n_cut > n_vars:
                    continue
                kernel = rule(*shape)
                per = (2 + n_vars * X + P * X * X) * (4 if kernel == M.KERNEL_X64 else 1) + (vectors(n_vars, X) // 8 if in_workspace(*shape) else 0)
                assert M.workspace_bytes(B, X, n_vars, P, U, n_forest, n_cut) == B * chunks(B, X ** n_cut, kernel) * per * 8, (B, shape, n_cut)
    assert M.lib.mlbp_exactgrad_workspace_bytes(1, 64, 4, 6, 4, 1, 3) == E.MLBP_EUNSUPPORTED and 'configurations' in M.last_error()
    assert M.lib.mlbp_exactgrad_workspace_bytes(1, 1024, 3, 3, 3, 1, 2) == E.MLBP_EUNSUPPORTED
    assert M.lib.mlbp_exactgrad_workspace_bytes(0, 64, 3, 3, 3, 1, 1) == E.MLBP_EINVAL
    assert M.workspace_bytes(8192, 64, 3, 3, 3, 1, 1) > 2 ** 31                              # 64-bit
