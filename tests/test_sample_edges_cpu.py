"""The sampling kernels at their edges, without a GPU: the inputs of tests/test_gpu_sample_edges.py and the preconditions under
which the float64 NumPy walk (tests/test_sample_cpu.py) is ground truth for them.

Every GPU case of test_gpu_sample_edges.py is an entry of CASES here and has a twin below that asserts, on the same inputs and
the same uniforms, what the GPU test relies on before it looks at the device: the walk's smallest margin is at least MARGIN
(so the cap on left-out (graph, sample) pairs is 0), every conditional marginal of the walk is finite, for wide-range
tables every marginal entry is 0 or at least test_range_cpu.FLOOR, and log q is far enough from 0 for a relative tolerance to
be met by every correct summation order (`logq_floor`).  The GPU test calls `precondition(name)` itself, so a seed
that leaves the regime fails here, on the CPU, and never reaches the device.  Each twin prints the smallest margin and the
smallest positive marginal entry of the walk.

A. Power-of-two scaling.  With normalised messages a table times 2^k changes no bit of a message: a sum of scaled terms is the
   scaled sum, the quotient by the scaled total is the unscaled quotient (nothing leaves the normal range with the exponents
   of test_gpu_exponent_range).  The twin shows it on the walk: explicitly scaled inputs give the unscaled walk's bits.  With
   unnormalised messages the scale multiplies along every path of the sweeps and only the marginal divides it out, so the
   exponents are small: UNNORM_K.
B. Wide-range tables exp(sigma N(0,1)) (test_range_cpu.range_inputs).
C. Size edges of the generic kernel: odd X above 256, X = 257, X = 2, X = 1024.
D. The X = 64 kernel's LDS budget with real potentials: K7 (above 64 KiB of dynamic LDS), chain_spec(28, 64) (message slots
   above 64 KiB) and K8 (past the budget: generic).
E. More than 256 variables: chain_spec(260, 2).  The walk redoes a whole sweep per step (O(n^2)); a chain is a tree, so the
   reference is `chain_walks`, an O(n) float64 recursion pinned on the walk below before it is trusted.
F. Bad entries: NaN and +inf in a pairwise table, an all-zero pairwise table, and the empty marginal (include/mlbp_sample.h
   step 4: no state with m_i > 0 gives x_v = 0 and log q = -inf)."""
import functools
import types

import numpy as np
import pytest

import cases as C
import test_gpu_sample as G
import test_range_cpu as R
import test_sample_cpu as SC
from helpers import batch_tables
from oracle import lbp_oracle as O

UNNORM_K = (-60, -17, 0, 1, 33, 60)          # test_gpu_exponent_range.F32_K: the unnormalised case's exponents (see part A)
AT = (3, 9)                                  # the edited entry of part F


def _topo(spec):
    from macaronicusermodeling_amd.topology import GraphTopology
    return GraphTopology.from_spec(spec)


def _k3x():
    return R.LEAN['k3'][0]()                                                      # K3, X = 64, one table per factor


def _k4x():
    return R._explicit(C.user_spec(10, [0, 2, 5, 8], 64, 64, seed=4))


def _k3x128():
    return R._explicit(C.user_spec(10, [1, 4, 7], 128, 128, seed=1))


K8 = lambda: C.user_spec(12, [0, 1, 3, 5, 7, 9, 10, 11], 64, 64, seed=5)          # noqa: E731


def _seeded(spec, B, seed, kind='uniform'):
    return [C.make_inputs(spec, seed + 1000 * b, kind) for b in range(B)]


def _wide(spec, width, B, seed):
    """Explicit tables exp(width N(0,1)), drawn as test_range_cpu.range_inputs draws them."""
    rs = np.random.RandomState(seed + int(width))
    X = spec['X']
    ntab = 1 + max(f['table'] for f in spec['factors'])
    shape = {f['table']: (X, X) if len(f['vars']) == 2 else (X, 1) for f in spec['factors']}
    return [dict(tables=[np.exp(width * rs.randn(*shape[t])) for t in range(ntab)]) for _ in range(B)]


def _pair_table(spec, p):
    return [f for f in spec['factors'] if len(f['vars']) == 2][p]['table']


def _mk(spec, inputs, roots, instance, u_seed, n_samples=2, **kw):
    uniforms = np.random.RandomState(u_seed).rand(n_samples, len(inputs), len(spec['var_ids']))
    case = dict(spec=spec, inputs=inputs, roots=list(roots), instance=instance, uniforms=uniforms, order=None, given=None,
                normalize=True, wide=False, empty=False, reference='walk', logq_floor=True)
    case.update(kw)
    return case


def _scaling(spec, roots, instance, u_seed, seed=5300, given=False, **kw):
    inputs = _seeded(spec, 8, seed)
    giv = None
    if given:                                                    # one variable fixed for half the graphs
        giv = np.full((8, len(spec['var_ids'])), -1, dtype=np.int32)
        giv[::2, 1] = np.random.RandomState(u_seed).randint(0, spec['X'], size=4)
    return _mk(spec, inputs, roots, instance, u_seed, given=giv, **kw)


def _range(name, width, instance, u_seed=27):
    case = R.range_inputs(name, width)
    return _mk(case['spec'], case['inputs'], case['roots'], instance, u_seed, wide=True, logq_floor=False)


def _edited(spec, roots, instance, u_seed, value, graph, table, normalize=True, whole_table=False, **kw):
    inputs = _seeded(spec, 4, 5600)
    if whole_table:
        tabs = list(inputs[graph]['tables'])
        tabs[_pair_table(spec, table)] = np.full_like(tabs[_pair_table(spec, table)], value)
        inputs[graph] = dict(tables=tabs)
    elif value is not None:
        inputs[graph] = R.edit_pair_entry(inputs[graph], _pair_table(spec, table), value, at=AT)
    return _mk(spec, inputs, roots, instance, u_seed, normalize=normalize, edited=graph, **kw)


K3_ROOTS = [1, 4, 7]
INF, NAN = float('inf'), float('nan')
CASES = {
    # A
    'scale_k3': lambda: _scaling(_k3x(), K3_ROOTS, G.X64_RESIDENT, 41),
    'scale_k4': lambda: _scaling(_k4x(), [0, 2, 5], G.X64_STREAMED, 42),
    'scale_x128': lambda: _scaling(_k3x128(), K3_ROOTS, G.GENERIC, 43),
    'scale_k3_given': lambda: _scaling(_k3x(), K3_ROOTS, G.X64_RESIDENT, 44, given=True),
    'scale_x128_given': lambda: _scaling(_k3x128(), K3_ROOTS, G.GENERIC, 45, given=True),
    'scale_k3_unnormalised': lambda: _scaling(_k3x(), K3_ROOTS, G.X64_RESIDENT, 46, normalize=False, exponents=UNNORM_K),
    'scale_x128_unnormalised': lambda: _scaling(_k3x128(), K3_ROOTS, G.GENERIC, 47, normalize=False, exponents=UNNORM_K),
    # B
    'wide_k3_5': lambda: _range('k3', 5, G.X64_RESIDENT),
    'wide_k3_20': lambda: _range('k3', 20, G.X64_RESIDENT),
    'wide_chain8_20': lambda: _range('chain8', 20, G.X64_STREAMED),
    'wide_star6_20': lambda: _range('star6', 20, G.X64_STREAMED),
    'wide_x128_20': lambda: _mk(_k3x128(), _wide(_k3x128(), 20, 4, 3111), K3_ROOTS, G.GENERIC, 27, wide=True),
    # C
    'ring3_x301': lambda: _mk(C.ring_spec(3, 301), _seeded(C.ring_spec(3, 301), 2, 11), [0, 1, 2], G.GENERIC, 51),
    'chain3_x257': lambda: _mk(C.chain_spec(3, 257), _seeded(C.chain_spec(3, 257), 2, 12), [0], G.GENERIC, 52),
    'chain3_x2': lambda: _mk(C.chain_spec(3, 2), _seeded(C.chain_spec(3, 2), 8, 13), [0], G.GENERIC, 53),
    'chain2_x1024': lambda: _mk(C.chain_spec(2, 1024), _seeded(C.chain_spec(2, 1024), 1, 14), [0], G.GENERIC, 54, n_samples=1),
    # D
    'k7_lds': lambda: _mk(R.K7(), _seeded(R.K7(), 4, 900), [0, 5, 11], G.X64_STREAMED, 61, n_samples=1),
    'chain28_lds': lambda: _mk(C.chain_spec(28, 64), _seeded(C.chain_spec(28, 64), 2, 920), [0], G.X64_STREAMED, 63, n_samples=1),
    'k8_generic': lambda: _mk(K8(), _seeded(K8(), 2, 910), [0, 5, 11], G.GENERIC, 62, n_samples=1),
    # E
    'chain260_x2': lambda: _mk(C.chain_spec(260, 2), _seeded(C.chain_spec(260, 2), 2, 15), [0], G.GENERIC, 71, n_samples=1,
                               reference='chain'),
    # F: the batches without an edit (the graphs whose bits an edit must leave alone; the batches of the table-index case)
    'clean_k3': lambda: _edited(_k3x(), K3_ROOTS, G.X64_RESIDENT, 81, None, 2, 1),
    'clean_k4': lambda: _mk(_k4x(), _seeded(_k4x(), 4, 5600), [0, 2, 5], G.X64_STREAMED, 81),
    'clean_x128': lambda: _edited(_k3x128(), K3_ROOTS, G.GENERIC, 81, None, 2, 1),
    # F.1
    'nan_k3': lambda: _edited(_k3x(), K3_ROOTS, G.X64_RESIDENT, 81, NAN, 2, 1),
    'inf_k3': lambda: _edited(_k3x(), K3_ROOTS, G.X64_RESIDENT, 81, INF, 2, 1),
    'nan_x128': lambda: _edited(_k3x128(), K3_ROOTS, G.GENERIC, 81, NAN, 2, 1),
    'inf_x128': lambda: _edited(_k3x128(), K3_ROOTS, G.GENERIC, 81, INF, 2, 1),
    # F.2
    'zero_k3': lambda: _edited(_k3x(), K3_ROOTS, G.X64_RESIDENT, 81, 0.0, 1, 0, whole_table=True),
    'zero_k3_unnormalised': lambda: _edited(_k3x(), K3_ROOTS, G.X64_RESIDENT, 81, 0.0, 1, 0, normalize=False, whole_table=True),
    'zero_x128': lambda: _edited(_k3x128(), K3_ROOTS, G.GENERIC, 81, 0.0, 1, 0, whole_table=True),
    'zero_x128_unnormalised': lambda: _edited(_k3x128(), K3_ROOTS, G.GENERIC, 81, 0.0, 1, 0, normalize=False, whole_table=True),
    # F.3
    'empty_k3': lambda: _edited(_k3x(), K3_ROOTS, G.X64_RESIDENT, 81, INF, 2, 1, normalize=False, empty=True),
    'empty_x128': lambda: _edited(_k3x128(), K3_ROOTS, G.GENERIC, 81, INF, 2, 1, normalize=False, empty=True),
    'clean_k3_unnormalised': lambda: _edited(_k3x(), K3_ROOTS, G.X64_RESIDENT, 81, None, 2, 1, normalize=False),
    'clean_x128_unnormalised': lambda: _edited(_k3x128(), K3_ROOTS, G.GENERIC, 81, None, 2, 1, normalize=False),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of one case (shared by the tests of a process: read, never written)."""
    return CASES[name]()


# ------------------------------------------------------------------------------------------------
# E: the chain recursion
# ------------------------------------------------------------------------------------------------
def chain_walks(spec, inputs_list, uniforms):
    """test_gpu_sample._walks for chain_spec(n, X), roots [0], default order, normalised messages, nothing given, in O(n) per
    sample.  One sweep rooted at variable 0 is exact on a chain, and at step k only variables below k are clamped, so
      - the messages arriving from the right never see a clamp: b_k = renorm(T_k . a_{k+1}) with
        a_{k+1} = renorm((uniform * u_{k+1}) * b_{k+1}), u = renorm(unary row), computed once per graph;
      - the message arriving from the left is the row of the drawn state: variable k-1 sends the indicator of x_{k-1}
        (renorm of a vector with one positive entry), so f_k = renorm(T_{k-1}[x_{k-1}, :]);
      - m_k = renorm(((uniform * u_k) * f_k) * b_k), the products in facset order with nan_to_num after each as
        oracle.lbp_oracle._product_of_incoming takes them.
    The draw and its margin are test_sample_cpu.draw's."""
    g = O.Graph(spec)
    n, X = len(g.var_order), g.X
    assert [f['vars'] for f in spec['factors']] == [[i] for i in range(n)] + [[i, i + 1] for i in range(n - 1)]
    uni = np.full(X, 1.0 / X)
    out, smallest = {}, np.inf
    for b, inputs in enumerate(inputs_list):
        tab = [O.factor_table(g, inputs, g.by_id[i]) for i in range(2 * n - 1)]
        u = [O.renormalize(tab[i].reshape(-1)) for i in range(n)]
        back = [None] * n                                       # back[k]: the message of factor (k, k+1) to variable k
        for k in range(n - 2, -1, -1):
            a = np.nan_to_num(u[k + 1] * uni)
            if back[k + 1] is not None:
                a = np.nan_to_num(back[k + 1] * a)
            back[k] = O.renormalize(tab[n + k].dot(O.renormalize(a)))
        for s in range(uniforms.shape[0]):
            x, cm, margin, logq = {}, {}, {}, 0.0
            for k in range(n):
                acc = np.nan_to_num(u[k] * uni)
                if k > 0:
                    acc = np.nan_to_num(O.renormalize(tab[n + k - 1][x[k - 1], :]) * acc)
                if k < n - 1:
                    acc = np.nan_to_num(back[k] * acc)
                m = cm[k] = O.renormalize(acc)
                x[k], margin[k] = SC.draw(m, float(uniforms[s, b, k]))
                logq += np.log(m[x[k]])
            out[s, b] = dict(g=g, x=x, logq=float(logq), cm=cm, margin=margin)
            smallest = min([smallest] + list(margin.values()))
    return out, smallest


@pytest.mark.parametrize('n,X', [(6, 2), (5, 4), (1, 4), (2, 3)])
def test_chain_recursion_is_the_walk(n, X):
    """Before the recursion is trusted at 260 variables: conditional marginals and log q within 1e-12 of the walk, the same
    states, the same margins."""
    spec = C.chain_spec(n, X)
    inputs = _seeded(spec, 6, 30, 'lognormal' if X == 4 else 'uniform')
    uniforms = np.random.RandomState(31).rand(4, len(inputs), n)
    walks, smallest = G._walks(spec, inputs, [0], uniforms)
    fast, fast_smallest = chain_walks(spec, inputs, uniforms)
    assert sorted(fast) == sorted(walks) and smallest >= G.MARGIN
    worst = 0.0
    for key, w in walks.items():
        f = fast[key]
        assert f['x'] == w['x'], key
        np.testing.assert_allclose(f['logq'], w['logq'], rtol=1e-12)
        for v in w['cm']:
            np.testing.assert_allclose(f['cm'][v], w['cm'][v], rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(f['margin'][v], w['margin'][v], rtol=1e-9, atol=1e-15)
            worst = max(worst, float(np.abs(f['cm'][v] / w['cm'][v] - 1).max()))
    np.testing.assert_allclose(fast_smallest, smallest, rtol=1e-9)
    print('chain%d_x%d: %d walks, recursion within %.1e relative of the walk, smallest margin %.2e' % (n, X, len(walks), worst, smallest))


# ------------------------------------------------------------------------------------------------
# the reference of a case and its precondition
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name):
    """({(s, b): walk}, smallest margin) of a case, computed once per process."""
    c = case(name)
    with np.errstate(all='ignore'):
        if c['reference'] == 'chain':
            assert c['roots'] == [0] and c['order'] is None and c['given'] is None and c['normalize']
            return chain_walks(c['spec'], c['inputs'], c['uniforms'])
        return G._walks(c['spec'], c['inputs'], c['roots'], c['uniforms'], order=c['order'], given=c['given'], normalize=c['normalize'])


def smallest_positive(walks):
    return min(float(m[m > 0].min()) for w in walks.values() for m in w['cm'].values() if (m > 0).any())


def logq_floor(spec):
    """The smallest |log q| at which rtol 1e-10 on log q can be asked of a correct kernel.  A drawn probability near 1 is a quotient
    by a sum of X terms; two correct summation orders differ by up to 2 X 2^-53 relative, log q adds n_vars such logarithms, so
    its absolute error reaches n_vars 2 X 2^-53 -- inside 1e-10 |log q| only from this |log q| on.  (Wide-range tables give
    marginals that put all but 1e-6 or less on one state: log q is then a few 1e-7 and one differing last bit of a marginal
    is 1e-10 of it.)"""
    return len(spec['var_ids']) * 2 * spec['X'] * 2.0 ** -53 / 1e-10


def precondition(name):
    """What a GPU case relies on, asserted on the walk alone; returns the walks.  log q is conditioned (logq_floor) in every
    case whose inputs were chosen here; the four wide-range cases on test_range_cpu.range_inputs are compared as they are
    given -- their smallest |log q| is printed."""
    c = case(name)
    walks, smallest = reference(name)
    assert len(walks) == c['uniforms'].shape[0] * len(c['inputs'])
    G._check_margin(name, walks, smallest)
    entries = np.concatenate([m for w in walks.values() for m in w['cm'].values()])
    low = smallest_positive(walks)
    print('%s: smallest margin of the walk %.2e, smallest positive marginal entry %.2e, %d of %d entries zero'
          % (name, smallest, low, int((entries == 0).sum()), entries.size))
    assert np.isfinite(entries).all() and (entries >= 0).all(), name
    logq = np.array([w['logq'] for w in walks.values()])
    assert not np.isnan(logq).any() and not np.isposinf(logq).any(), name
    if not c['empty']:
        assert np.isfinite(logq).all(), name
    print('%s: smallest |log q| of the walk %.2e (conditioned from %.2e on%s)'
          % (name, np.abs(logq).min(), logq_floor(c['spec']), '' if c['logq_floor'] else '; not asserted'))
    if c['logq_floor']:
        assert np.abs(logq).min() >= logq_floor(c['spec']), (name, np.abs(logq).min())
    if c['wide']:
        assert low >= R.FLOOR, (name, low)
    return walks


TWINS = [n for n in CASES if not n.startswith('scale_')]


@pytest.mark.parametrize('name', TWINS)
def test_precondition(name):
    precondition(name)


# ------------------------------------------------------------------------------------------------
# A: scaling
# ------------------------------------------------------------------------------------------------
def exponents(name):
    """(topology, k per pairwise table [B * P], k per unary row [B * U]) of a scaling case: test_gpu_exponent_range._exponents
    on a stand-in for the batch (PAIR_K / UNARY_K by graph and slot), or the case's own cycle for both kinds of table."""
    import torch
    import test_gpu_exponent_range as XR
    c = case(name)
    topo, B = _topo(c['spec']), len(c['inputs'])
    if c.get('exponents'):
        cyc = c['exponents']
        kp = np.array([cyc[(i // topo.P + i % topo.P) % len(cyc)] for i in range(B * topo.P)], dtype=np.int32)
        ku = np.array([cyc[(i // topo.U + i % topo.U + 2) % len(cyc)] for i in range(B * topo.U)], dtype=np.int32)
        return topo, kp, ku
    pair, unary = batch_tables(c['spec'], topo, c['inputs'])
    stand_in = types.SimpleNamespace(topo=topo, B=B, pair_tables=torch.from_numpy(pair), unary_tables=torch.from_numpy(unary),
                                     pair_tables_shared=False)
    kp, ku = XR._exponents(stand_in)
    return topo, kp, ku


def scaled_inputs(name):
    """The case's inputs with pairwise table p of graph b times 2^kp[b P + p] and unary row u times 2^ku[b U + u], exactly."""
    c = case(name)
    topo, kp, ku = exponents(name)
    by_id = {f['id']: f for f in c['spec']['factors']}
    out = []
    for b, inp in enumerate(c['inputs']):
        tabs = list(inp['tables'])
        for slots, k, n in ((topo.pair_factors, kp, topo.P), (topo.unary_factors, ku, topo.U)):
            for i, j in enumerate(slots):
                t = by_id[topo.factor_ids[j]]['table']
                tabs[t] = np.ldexp(inp['tables'][t], int(k[b * n + i]))
                assert np.isfinite(tabs[t]).all() and (tabs[t] >= np.finfo(np.float64).tiny).all()
        out.append(dict(tables=tabs))
    return out


@pytest.mark.parametrize('name', [n for n in CASES if n.startswith('scale_')])
def test_scaled_tables_give_the_walk_the_same_bits(name):
    """The claim of part A is IEEE, not luck: the walk on explicitly scaled inputs returns the unscaled walk's states, log q and
    conditional marginals bit for bit."""
    c = case(name)
    walks = precondition(name)
    _, kp, ku = exponents(name)
    assert len(set(kp.tolist())) > 2 and len(set(ku.tolist())) > 2          # not the trivial scaling
    with np.errstate(all='ignore'):
        scaled, _ = G._walks(c['spec'], scaled_inputs(name), c['roots'], c['uniforms'], given=c['given'], normalize=c['normalize'])
    differ = 0
    for key, w in walks.items():
        s = scaled[key]
        differ += sum(int((s['cm'][v] != w['cm'][v]).sum()) for v in w['cm']) + (s['logq'] != w['logq']) + (s['x'] != w['x'])
    print('%s: exponents %d..%d (pairwise), %d..%d (unary); %d differing entries' % (name, kp.min(), kp.max(), ku.min(), ku.max(), differ))
    assert differ == 0, name


# ------------------------------------------------------------------------------------------------
# D, E: what the host says about the shapes
# ------------------------------------------------------------------------------------------------
def x64_lds_bytes(n_msgs, n_vars):
    """include/mlbp_sample.h: messages, partial sums and one raw vector, the cached marginal, the clamp states."""
    return n_msgs * 512 + 4608 + 512 + 4 * ((n_vars + 3) // 4 * 4)


def test_lds_budget_cases_sit_where_they_should():
    S = SC._S()
    k7, k8 = _topo(R.K7()), _topo(K8())
    assert (k7.n_msgs, k7.n_vars, k7.P) == (126, 7, 21) and x64_lds_bytes(126, 7) == 69664 > 65536
    assert S.pick_kernel(64, k7.n_msgs, k7.n_vars) == S.KERNEL_X64
    c28 = _topo(C.chain_spec(28, 64))
    assert (c28.n_msgs, c28.n_vars, c28.P) == (136, 28, 27) and 136 * 512 > 65536 and x64_lds_bytes(136, 28) == 74864
    assert S.pick_kernel(64, c28.n_msgs, c28.n_vars) == S.KERNEL_X64
    assert (k8.n_msgs, k8.n_vars) == (152, 8) and x64_lds_bytes(152, 8) == 82976 > S.X64_LDS_BYTES
    assert S.pick_kernel(64, k8.n_msgs, k8.n_vars) == S.KERNEL_GENERIC


def test_chain260_passes_every_host_side_check():
    """260 variables and 1296 message slots at X = 2: the topology compiles, the library's program and read-out checks accept
    it, and the generic kernel takes it with 2 x 1296 x 2 doubles of workspace."""
    from macaronicusermodeling_amd import _ffi
    S = SC._S()
    topo = _topo(case('chain260_x2')['spec'])
    assert (topo.n_vars, topo.n_msgs, topo.P, topo.U) == (260, 1296, 259, 260)
    ops, srcs, sweeps = topo.compile_program([0])
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)          # noqa: E731
    o, s, w, sv, od = i32(ops), i32(srcs), i32(sweeps), i32(S.slot_var_array(topo)), np.arange(260, dtype=np.int32)
    assert S.lib.mlbp_sample_check_program(_ffi.i32ptr(o), len(o) // 4, _ffi.i32ptr(s), len(s), _ffi.i32ptr(w), len(w) // 2, topo.n_msgs,
                                           topo.P, topo.U, topo.n_vars, _ffi.i32ptr(sv), _ffi.i32ptr(od)) == _ffi.MLBP_OK, S.last_error()
    assert S.lib.mlbp_sample_check_readout(topo.n_vars, _ffi.i32ptr(i32(topo.in_off)), _ffi.i32ptr(i32(topo.in_slots)), topo.n_msgs) == _ffi.MLBP_OK
    assert S.pick_kernel(2, topo.n_msgs, topo.n_vars) == S.KERNEL_GENERIC
    assert S.workspace_bytes(2, 1, 2, topo.n_msgs, topo.n_vars) == 2 * 1296 * 2 * 8


# ------------------------------------------------------------------------------------------------
# F: what the walk does with bad entries
# ------------------------------------------------------------------------------------------------
def _cm(walks, s, b):
    return np.stack([m for _, m in sorted(walks[s, b]['cm'].items())])


@pytest.mark.parametrize('name', ['nan_k3', 'inf_k3', 'nan_x128', 'inf_x128'])
def test_a_non_finite_entry_changes_the_walk_of_its_graph_only(name):
    c = case(name)
    walks, clean = precondition(name), precondition('clean_' + name.split('_')[1])
    for (s, b), w in walks.items():
        same = all(np.array_equal(w['cm'][v], clean[s, b]['cm'][v]) for v in w['cm'])
        assert same == (b != c['edited']), (name, s, b)


@pytest.mark.parametrize('name', ['zero_k3_unnormalised', 'zero_x128_unnormalised'])
def test_an_all_zero_table_without_normalisation_gives_uniform_marginals(name):
    c = case(name)
    walks = precondition(name)
    X = c['spec']['X']
    for s in range(c['uniforms'].shape[0]):
        assert np.array_equal(_cm(walks, s, c['edited']), np.full((3, X), 1.0 / X))
        np.testing.assert_allclose(walks[s, c['edited']]['logq'], -3 * np.log(X), rtol=1e-15)


def test_draw_on_an_empty_marginal():
    """include/mlbp_sample.h step 4: when no state has m_i > 0, x_v = 0 whatever u is (margin inf: the draw reads no uniform)."""
    for u in (0.0, 0.3, 1.0 - 2.0 ** -53):
        assert SC.draw(np.zeros(8), u) == (0, np.inf)


@pytest.mark.parametrize('name', ['empty_k3', 'empty_x128'])
def test_an_infinite_entry_without_normalisation_empties_a_marginal(name):
    """+inf survives unnormalised messages as DBL_MAX, the marginal's total overflows and every m_i is 0: the walk returns state 0
    and log q = -inf for the edited graph, and goes on to the next variable."""
    c = case(name)
    walks = precondition(name)
    for (s, b), w in walks.items():
        emptied = [v for v, m in sorted(w['cm'].items()) if not (m > 0).any()]
        if b == c['edited']:
            assert emptied and np.isneginf(w['logq']), (name, s, b)
            assert all(w['x'][v] == 0 and np.isinf(w['margin'][v]) for v in emptied)
        else:
            assert not emptied and np.isfinite(w['logq']), (name, s, b)
    print('%s: graph %d, emptied variables %r' % (name, c['edited'], [[v for v, m in sorted(walks[s, c['edited']]['cm'].items()) if not (m > 0).any()]
                                                                     for s in range(c['uniforms'].shape[0])]))
