"""The gradient beyond the exact limit without a GPU: the NumPy statement of the LISTED mode of include/mlbp_exactgrad.h, pinned
on exhaustive enumeration, and the host side of the mode -- the struct, the constants, the workspace and the bad-argument table.

The statement.  listed_pairs() is tests/test_exactgrad_cpu.condition_pairs with the three substitutions the header names: a
caller's list of cutset states where the enumeration of all of them stands, the entry's weight w_i = Z_c exp(-log_q[i]) where
Z_c stands, the mean weight under the logarithm.  Every other line is that function's, so that the full list with log_q = 0 is
the exact statement bit for bit.

The reference.  The self-normalised estimator over ANY list is the expectation under the tilted model
    p~(x) ~ p(x) * sum_i [c(x) = c_i] / q_i,
a deterministic identity: sum_i w_i E[f | c_i] = sum_c (sum_{i: c_i = c} 1 / q_i) Z_c E[f | c].  tilted_enum() forms p~ on the
log-domain grid of test_cutset_cpu.enumerate_exact; nothing of the algorithm under test is in it.  No test here or in
tests/test_gpu_estgrad.py asserts a statistical accuracy."""
import ctypes
import itertools

import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_cutsetis_cpu as IS
import test_exactgrad_cpu as G
from oracle import lbp_oracle as O


# ------------------------------------------------------------------------------------------------
# the statement
# ------------------------------------------------------------------------------------------------
def listed_pairs(g, inputs, cut, configs, log_q, feat=None):
    """The listed mode of include/mlbp_exactgrad.h in NumPy: dict(log_z_hat, marg [n_vars][X] in g.var_order, pairs {factor id:
    M}, weights [N], refused) for the cutset `cut` (variable ids; column q of configs is the state of cut[q]); with `feat` also
    expect (ee, ed), contracted from the accumulators before the division, as the combine kernel does."""
    X, order = g.X, list(g.var_order)
    configs = np.asarray(configs).reshape(len(log_q), len(cut))
    log_q = np.asarray(log_q, dtype=np.float64)
    N = len(log_q)
    if ((configs < 0) | (configs >= X)).any() or not (np.abs(log_q) <= 1e6).all():
        return dict(refused=True, log_z_hat=np.nan)
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
    r, k2 = IS.split(log_q)                                     # exp(-log_q) = r 2^k: the one formula
    S1, acc = 0.0, {v: np.zeros(X) for v in order}
    pacc = {fid: np.zeros((X, X)) for fid, vs, _ in facs if len(vs) == 2}
    forest = {edges[parent[v][1]][0] for v in free if parent[v] is not None}
    weights = np.zeros(N)
    for i in range(N):
        s = dict(zip(cut, (int(x) for x in configs[i])))
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
        w = float(np.ldexp(Zc * r[i], int(k2[i])))              # where Z_c stands
        weights[i] = w
        dn = {}
        for v in walk:                                          # roots to leaves
            if parent[v] is not None:
                par, k = parent[v]
                excl = phi[par] * (dn[par] if par in dn else 1.0)
                for u in free:
                    if u != v and parent[u] is not None and parent[u][0] == par:
                        excl = excl * up[u]
                dn[v] = toward(k, par, excl)
                fid, vs, T = edges[k]
                a = bel[v]
                norm = float(a.dot(dn[v]))
                pacc[fid] += (w / norm) * (np.outer(a, excl) if vs[0] == v else np.outer(excl, a))
                bel[v] = bel[v] * dn[v]
        S1 += w
        m_c = {v: bel[v] / bel[v].sum() for v in free}
        for v in free:
            acc[v] += w * m_c[v]
        for v in cut:
            acc[v][s[v]] += w
        for fid, vs, T in facs:
            if len(vs) != 2:
                continue
            if vs[0] in s and vs[1] in s:
                pacc[fid][s[vs[0]], s[vs[1]]] += w
            elif vs[0] in s:
                pacc[fid][s[vs[0]], :] += w * m_c[vs[1]]
            elif vs[1] in s:
                pacc[fid][:, s[vs[1]]] += w * m_c[vs[0]]
    out = dict(refused=False, weights=weights)
    if S1 == 0:
        out.update(log_z_hat=-np.inf, marg=np.full((len(order), X), 1.0 / X), pairs={fid: np.full((X, X), 1.0 / X ** 2) for fid in pacc})
    else:
        tables = {fid: T for fid, vs, T in facs if len(vs) == 2}
        raw = {fid: (A * tables[fid] if fid in forest else A) for fid, A in pacc.items()}
        out.update(log_z_hat=float(np.log(S1 / N)), marg=np.stack([acc[v] / S1 for v in order]), pairs={fid: A / S1 for fid, A in raw.items()})
        if feat is not None:                                    # contracted before the division: another order of the same sum
            ee, ed = G.features_of(g, feat, np.stack([acc[v] for v in order]), raw)
            out['expect'] = (ee / S1, ed / S1)
    if feat is not None and 'expect' not in out:
        out['expect'] = G.features_of(g, feat, out['marg'], out['pairs'])
    return out


def _lse(a, axis):
    """logsumexp over `axis` that gives -inf, not NaN, for a slice that holds nothing."""
    top = np.max(a, axis=axis, keepdims=True)
    safe = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide='ignore'):
        out = np.log(np.sum(np.exp(a - safe), axis=axis, keepdims=True)) + safe
    return np.squeeze(out, axis=axis) if axis else float(out.reshape(-1)[0])


def tilted_enum(g, inputs, cut, configs, log_q):
    """(log_z_hat, marginals, {factor id: M}) of the tilted model p~ by exhaustive enumeration in the log domain."""
    X, order = g.X, list(g.var_order)
    _, _, grid = R.enumerate_exact(g, inputs)
    n = grid.ndim
    mult = np.zeros((X,) * len(cut))
    for row, lq in zip(np.asarray(configs).reshape(len(log_q), len(cut)), log_q):
        mult[tuple(int(s) for s in row)] += np.exp(-lq)
    axes = [order.index(v) for v in cut]
    shape = [1] * n
    for q, a in enumerate(axes):
        shape[a] = X
    with np.errstate(divide='ignore'):
        tilt = grid + np.log(np.transpose(mult, np.argsort(axes)).reshape(shape) if cut else mult.reshape(shape))
    every = tuple(range(n))
    lz = _lse(tilt, every)
    marg = np.stack([np.exp(_lse(tilt, tuple(a for a in every if a != i)) - lz) if n > 1 else np.exp(tilt - lz) for i in range(n)])
    pairs = {}
    for fid, va, vb in G.pair_factors(g):
        a, b = order.index(va), order.index(vb)
        rest = tuple(k for k in every if k not in (a, b))
        M = np.exp((_lse(tilt, rest) if rest else tilt) - lz)
        pairs[fid] = M if a < b else M.T
    return lz - np.log(len(log_q)), marg, pairs


def product_list(X, n_cut):
    """Every configuration once in the order the exact STATEMENT walks them (itertools.product: the last position fastest)."""
    return np.array(list(itertools.product(range(X), repeat=n_cut)), dtype=np.int32).reshape(X ** n_cut, n_cut)


SHAPES = [('k3', lambda X: R.kn_spec(3, X)), ('k4', lambda X: R.kn_spec(4, X)), ('k5', lambda X: R.kn_spec(5, X)),
          ('cycle4', lambda X: C.ring_spec(4, X)), ('tree', lambda X: R.forest_spec(X))]
CASES = [(name, make, X) for name, make in SHAPES for X in (3, 4)]
IDS = ['%s_x%d' % (c[0], c[2]) for c in CASES]


def grad_bar(g):
    return len(g.factors) * g.X * g.X * 2.0 ** -51


# ------------------------------------------------------------------------------------------------
# the statement against enumeration
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,make,X', CASES, ids=IDS)
def test_estimator_identity(name, make, X):
    """For any list the estimate is the expectation under the tilted model: pair marginals, marginals and expected features
    within 1e-10, log_z_hat within 1e-10 relative; the gradient within (P + U) X^2 2^-51 of observed - the contraction of the
    returned tensors."""
    spec = make(X)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    assert (name == 'tree') == (not cut)
    feat = G.make_features(g, 31)
    labels = dict(zip(g.var_order, (int(x) for x in np.random.RandomState(5).randint(0, X, size=len(g.var_order)))))
    for kind in ('uniform', 'lognormal'):
        for seed, N in ((3, 1), (4, 5), (5, 23)):
            inputs = C.make_inputs(spec, seed, kind)
            configs, log_q = IS.make_list(g, inputs, cut, N, seed + 40)
            got = listed_pairs(g, inputs, cut, configs, log_q, feat)
            want_z, want_m, want_p = tilted_enum(g, inputs, cut, configs, log_q)
            assert abs(got['log_z_hat'] - want_z) <= 1e-10 * max(1.0, abs(want_z))
            assert np.abs(got['marg'] - want_m).max() <= 1e-10 and G.worst_gap(got['pairs'], want_p) <= 1e-10
            want_f = np.concatenate(G.features_of(g, feat, want_m, want_p))
            assert np.abs(np.concatenate(got['expect']) - want_f).max() <= 1e-10
            ob = np.concatenate(G.observed_of(g, feat, labels))
            grad = ob - np.concatenate(got['expect'])
            contracted = ob - np.concatenate(G.features_of(g, feat, got['marg'], got['pairs']))
            assert np.abs(grad - contracted).max() <= grad_bar(g), (name, kind, seed)
            for fid, va, vb in G.pair_factors(g):               # every block sums to 1, rows and columns to the marginals
                order = list(g.var_order)
                assert abs(got['pairs'][fid].sum() - 1) <= 1e-12
                assert np.abs(got['pairs'][fid].sum(axis=1) - got['marg'][order.index(va)]).max() <= 1e-12
                assert np.abs(got['pairs'][fid].sum(axis=0) - got['marg'][order.index(vb)]).max() <= 1e-12


@pytest.mark.parametrize('name,make,X', CASES, ids=IDS)
def test_full_list_is_the_exact_statement_bit_for_bit(name, make, X):
    spec = make(X)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    inputs = C.make_inputs(spec, 9, 'lognormal')
    full = product_list(X, len(cut))
    got = listed_pairs(g, inputs, cut, full, np.zeros(len(full)))
    log_z, marg, pairs = G.condition_pairs(g, inputs, cut)
    assert np.array_equal(got['marg'], marg) and all(np.array_equal(got['pairs'][fid], pairs[fid]) for fid in pairs)
    want = log_z - np.log(len(full))
    assert abs(got['log_z_hat'] - want) <= 1e-12 * max(1.0, abs(want))
    # and the exact libraries' own order (digit q of c is the state of position q) is the same set: the same numbers to rounding
    other = listed_pairs(g, inputs, cut, IS.full_list(X, len(cut)), np.zeros(len(full)))
    assert np.abs(other['marg'] - marg).max() <= 1e-13 and G.worst_gap(other['pairs'], pairs) <= 1e-13


@pytest.mark.parametrize('name,make,X', CASES[:6], ids=IDS[:6])
def test_weights_are_those_of_the_cutset_estimate_statement(name, make, X):
    spec = make(X)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    inputs = C.make_inputs(spec, 6, 'lognormal')
    configs, log_q = IS.make_list(g, inputs, cut, 17, 2)
    got = listed_pairs(g, inputs, cut, configs, log_q)
    ref = IS.Statement(g, inputs, cut).run(configs, log_q)
    top = np.frexp(got['weights'].max())[1]                     # w = m 2^e with m in [0.5, 1): the statement's emax
    assert np.array_equal(np.ldexp(got['weights'], -top), ref['terms'])
    assert abs(got['log_z_hat'] - ref['log_z_hat']) <= 1e-12 * max(1.0, abs(ref['log_z_hat']))
    assert np.abs(got['marg'] - ref['marg']).max() <= 1e-12


def test_special_lists_and_scaling():
    """N = 1: the conditional quantities of the one entry and ln Z_c - log_q.  Four copies of one entry: the bits of one.
    A table times 2^k: no bit of a normalised output moves and log_z_hat moves by k ln 2."""
    spec = R.kn_spec(4, 4)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    inputs = C.make_inputs(spec, 3)
    one = np.array([[1, 3]], dtype=np.int32)
    got = listed_pairs(g, inputs, cut, one, np.array([-0.7]))
    z_c, m_c = IS.Statement(g, inputs, cut).solve(one[0])
    assert abs(got['log_z_hat'] - (np.log(z_c) + 0.7)) <= 1e-12 and np.abs(got['marg'] - m_c).max() <= 1e-12
    order = list(g.var_order)
    for q, v in enumerate(cut):
        assert got['marg'][order.index(v)][one[0][q]] == 1.0
    four = listed_pairs(g, inputs, cut, np.repeat(one, 4, axis=0), np.full(4, -0.7))
    assert np.array_equal(four['marg'], got['marg']) and all(np.array_equal(four['pairs'][f], got['pairs'][f]) for f in got['pairs'])
    assert abs(four['log_z_hat'] - got['log_z_hat']) <= 1e-12
    configs, log_q = IS.make_list(g, inputs, cut, 9, 1)
    base = listed_pairs(g, inputs, cut, configs, log_q)
    for table, k in ((0, 40), (5, -37), (9, 300)):
        scaled = dict(inputs, tables=list(inputs['tables']))
        scaled['tables'][table] = np.ldexp(scaled['tables'][table], k)
        moved = listed_pairs(g, scaled, cut, configs, log_q)
        assert np.array_equal(moved['marg'], base['marg']) and all(np.array_equal(moved['pairs'][f], base['pairs'][f]) for f in base['pairs'])
        assert abs(moved['log_z_hat'] - base['log_z_hat'] - k * np.log(2.0)) <= 1e-12 * max(1.0, abs(moved['log_z_hat']))


def test_edge_rules_of_a_list():
    spec = R.kn_spec(3, 4)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    inputs = C.make_inputs(spec, 2)
    configs, log_q = IS.make_list(g, inputs, cut, 6, 1)
    for bad in (4, -1):
        c2 = configs.copy()
        c2[3, 0] = bad
        assert listed_pairs(g, inputs, cut, c2, log_q)['refused']
    for bad in (np.nan, np.inf, -np.inf, 2e6):
        q2 = log_q.copy()
        q2[2] = bad
        assert listed_pairs(g, inputs, cut, configs, q2)['refused']
    zero = dict(inputs, tables=[np.zeros_like(t) if i == 0 else t for i, t in enumerate(inputs['tables'])])
    out = listed_pairs(g, zero, cut, configs, log_q)
    assert out['log_z_hat'] == -np.inf and (out['marg'] == 0.25).all() and all((M == 1.0 / 16).all() for M in out['pairs'].values())


# ------------------------------------------------------------------------------------------------
# the host side of the listed mode
# ------------------------------------------------------------------------------------------------
def _M():
    from macaronicusermodeling_amd import exactgrad
    return exactgrad


def _ffi():
    from macaronicusermodeling_amd import _ffi
    return _ffi


def test_binding_mirrors_the_listed_header():
    M = _M()
    from macaronicusermodeling_amd import cutdraw, cutsetis, exactmap, exactsample
    assert M.MAX_LISTED == 65536 == cutsetis.MAX_LISTED == exactmap.MAX_LISTED == exactsample.MAX_LISTED == cutdraw.MAX_LISTED
    assert M.MAX_CUT == 16
    # mlbp_exactgrad_args is what it was; the list lies behind it in mlbp_exactgrad_listed_args
    assert [f[0] for f in M.ExactGradArgs._fields_][-1] == 'grad_ed' and ctypes.sizeof(M.ExactGradArgs) == 64 + 21 * 8
    T = M.listed_args()
    assert T is M.listed_args() and [f[0] for f in T._fields_] == ['args', 'configs', 'log_q', 'N'] and T._fields_[0][1] is M.ExactGradArgs
    size = ctypes.sizeof(M.ExactGradArgs)
    assert (T.args.offset, T.configs.offset, T.log_q.offset, T.N.offset, ctypes.sizeof(T)) == (0, size, size + 8, size + 16, size + 24)
    t = T()
    assert t.N == 0 and ctypes.addressof(t.args) == ctypes.addressof(t)          # a zeroed tail is the exact call; `args` shares its memory
    text = open(IS.HEADER.replace('mlbp_cutsetis.h', 'mlbp_exactgrad.h')).read()
    body = text[text.index('typedef struct mlbp_exactgrad_listed_args {'):text.index('} mlbp_exactgrad_listed_args;')]
    assert [w for w in ('args;', 'configs;', 'log_q;', 'N;') if w in body] == ['args;', 'configs;', 'log_q;', 'N;']
    assert body.index('args;') < body.index('configs;') < body.index('log_q;') < body.index(' N;')


def test_listed_workspace_is_the_headers_formula():
    from macaronicusermodeling_amd import cutset as S
    M = _M()

    def ints(P, U):
        return 4 * ((P + U + 16 + 3) // 4 * 4)
    shapes = ((64, 3, 3, 3, 1), (64, 5, 10, 5, 1), (64, 8, 28, 8, 1), (64, 4, 4, 4, 2), (64, 4, 3, 4, 3), (5, 4, 6, 4, 1), (3, 6, 15, 6, 1), (7, 5, 5, 5, 3),
              (64, 12, 66, 12, 0), (512, 3, 3, 3, 1), (1024, 3, 3, 3, 1))
    for X, n_vars, P, U, n_forest in shapes:
        kernel = M.pick_kernel(X, n_vars, P, U, n_forest)
        vectors = (5 * n_vars + 2) * ((X + 1) // 2 * 2)
        spill = kernel == M.KERNEL_GENERIC and vectors * 8 + 64 + ints(P, U) > S.GENERIC_LDS_BYTES
        per = (2 + n_vars * X + P * X * X) * (4 if kernel == M.KERNEL_X64 else 1) + (vectors if spill else 0)
        for B in (1, 3, 600, 8192):
            for N in (1, 3, 5, 37, 64, 256, 65536):
                walkers = -(-N // 4) if kernel == M.KERNEL_X64 else N
                chunks = min(walkers, -(-M.MIN_WORKGROUPS // B))
                assert M.chunks(B, N, kernel) == chunks
                assert M.listed_workspace_bytes(B, X, n_vars, P, U, n_forest, N) == B * chunks * per * 8, (X, n_vars, B, N)
    # the full list asks for what the exact call asks for
    assert M.listed_workspace_bytes(3, 64, 3, 3, 3, 1, 64) == M.workspace_bytes(3, 64, 3, 3, 3, 1, 1)
    assert M.listed_workspace_bytes(2, 5, 4, 6, 4, 1, 25) == M.workspace_bytes(2, 5, 4, 6, 4, 1, 2)
    # the header's figure: a K5 partial at X = 64 is 330 256 bytes; four per graph at B = 8192 are 10.8 GB
    assert (2 + 5 * 64 + 10 * 64 * 64) * 8 == 330256
    need = M.listed_workspace_bytes(8192, 64, 5, 10, 5, 1, 256)
    assert need == 8192 * 4 * 330256 and 10.8e9 < need < 10.9e9


def _listed_args(M, n=5, X=64, N=8, n_cut=None):
    """Arguments of a listed call on K_n that pass every host-side check (no pointer is dereferenced on the host)."""
    from macaronicusermodeling_amd import cutset
    n_cut = n - 2 if n_cut is None else n_cut
    words = cutset.plan_words(R._topo(R.kn_spec(n, 4)), list(range(n_cut)))
    t = M.listed_args()()
    a = t.args                                                  # shares t's memory
    a.B, a.X, a.n_vars, a.P, a.U = 2, X, n, n * (n - 1) // 2, n
    a.n_cut, a.n_free, a.n_items, a.n_consts, a.n_forest = (int(w) for w in words[3:8])
    a.n_pair_tables, a.n_unary_tables, a.plan_words = 2 * a.P, 2 * a.U, -len(words)      # negated: the list lies behind the struct
    a.F_ee, a.F_ed, a.Vde = 3, 6, 70
    for name, typ in M.ExactGradArgs._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, name, 4096)
    t.configs, t.log_q, t.N = 4096, 4096, N
    a.workspace_bytes = M.listed_workspace_bytes(a.B, X, a.n_vars, a.P, a.U, a.n_forest, N) if N > 0 else 1 << 40
    return t


def test_listed_bad_arguments():
    import torch
    M, E = _M(), _ffi()
    call = lambda t: M.lib.mlbp_exactgrad_f64(ctypes.byref(t.args), None)   # noqa: E731

    def put(t, field, value):
        setattr(t if field in ('N', 'configs', 'log_q') else t.args, field, value)
    for field, value, status, word in (('N', -1, E.MLBP_EINVAL, 'N = -1'), ('N', M.MAX_LISTED + 1, E.MLBP_EINVAL, 'N = 65537'),
                                       ('configs', None, E.MLBP_EINVAL, 'configs'), ('log_q', None, E.MLBP_EINVAL, 'log_q'),
                                       ('workspace', None, E.MLBP_EINVAL, 'workspace'), ('log_z', None, E.MLBP_EINVAL, 'log_z'),
                                       ('labels', None, E.MLBP_EINVAL, 'labels'), ('phi_en_de', None, E.MLBP_EINVAL, 'feature inputs'),
                                       ('plan_words', -5, E.MLBP_EINVAL, 'plan')):
        t = _listed_args(M)
        put(t, field, value)
        assert call(t) == status and word in M.last_error(), (field, M.last_error())
        assert M.lib.mlbp_exactgrad_last_kernel() == M.KERNEL_NONE
    t = _listed_args(M)
    t.args.workspace_bytes -= 8                                 # one double short of the listed formula
    assert call(t) == E.MLBP_EINVAL and 'workspace' in M.last_error()
    t = _listed_args(M, N=8)
    t.args.workspace_bytes = M.listed_workspace_bytes(2, 64, 5, 10, 5, 1, 4) # enough for a shorter list, not for this one
    assert call(t) == E.MLBP_EINVAL and 'workspace' in M.last_error()
    t = _listed_args(M, n=19, n_cut=17)                         # 17 cutset variables: beyond the walk's 16
    assert call(t) == E.MLBP_EUNSUPPORTED and 'cutset variables' in M.last_error() and '16' in M.last_error()
    t = _listed_args(M, N=0)                                    # the exact call refuses K5 at X = 64 as it always has
    assert call(t) == E.MLBP_EUNSUPPORTED and 'configurations' in M.last_error()
    if torch.cuda.is_available():
        return                                                  # (what passes the checks would be enqueued: the GPU module's part)
    for n, n_cut in ((5, 3), (8, 6), (18, 16), (3, 1), (3, 0)):
        t = _listed_args(M, n=n, n_cut=n_cut)
        if n_cut == 0:
            t.configs = None                                    # not read without cutset variables
        assert call(t) == E.MLBP_ENODEVICE, (n, M.last_error())
    # N == 0 is the exact call whatever the list's fields hold: junk, NULL, and a workspace sized for the exact call alone
    for configs, log_q in ((4096, 4096), (None, None), (1, 3)):
        t = _listed_args(M, n=3, n_cut=1, N=0)
        t.configs, t.log_q = configs, log_q
        t.args.workspace_bytes = M.workspace_bytes(2, 64, 3, 3, 3, 1, 1)
        assert call(t) == E.MLBP_ENODEVICE, M.last_error()
    # and the struct alone, its plan_words as they are, is the exact call: nothing behind it is read
    t = _listed_args(M, n=3, n_cut=1, N=5)
    plain = M.ExactGradArgs.from_buffer_copy(t.args)
    plain.plan_words = -plain.plan_words
    plain.workspace_bytes = M.workspace_bytes(2, 64, 3, 3, 3, 1, 1)
    assert M.lib.mlbp_exactgrad_f64(ctypes.byref(plain), None) == E.MLBP_ENODEVICE, M.last_error()


def test_batch_calls_exist_and_check_their_lists():
    """The public names of the feature and the host-side refusals that need no device."""
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.train import TiDirTrainer, UserGraphTrainer
    for name in ('cutset_gradient', 'cutset_pair_marginals', 'estimate_gradient'):
        assert callable(getattr(FactorGraphBatch, name))
    assert callable(UserGraphTrainer.estimated_gradient)
    assert callable(TiDirTrainer.estimated_step) and callable(TiDirTrainer.estimated_gradient_report)
