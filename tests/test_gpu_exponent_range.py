"""The sweep kernels away from unit magnitude.  The fast paths owe their speed to how they carry magnitude -- the lean X = 64
kernel keeps messages with a power-of-two scale and normalises once, the shared-table MFMA forms store c (.) message or
sqrt(c) (.) message, the contraction normalises by a reciprocal, and each has exponent-key thresholds that hand a graph to the
exact kernel -- and every other GPU test feeds them tables within about three decades of 1.

A. Power-of-two scaling.  A table times 2^k is exact and commutes with every product, sum, FMA, division and reciprocal as long
   as nothing leaves the normal range, and with the exponents below nothing does (a contraction's results stay above 2^-420;
   unary messages are normalised before anything multiplies them).  So every case runs twice -- tables as they are, tables
   scaled -- and asserts the same BITS in messages and marginals, status 0 and the same exact_count: a differing bit is a
   scale that was not carried, a differing count a threshold compared with unscaled data.  Exponents: pairwise table p of
   graph b: PAIR_K[(b + p) % 6]; unary row u of graph b: UNARY_K[(b + u) % 5] (rows of a shared pool, and shared pairwise
   tables beyond the first two, by their index); the two shared pots: 2^-400 and 2^+257; float32 tables: |k| <= 60.
   With shared tables and 37 graphs, neighbouring graphs of one 16-graph workgroup carry unary scales 2^1000 apart.
B. Wide-range tables (tests/test_range_cpu.py: exp(sigma N(0,1)), sigma 5 and 20; train-layout thetas times 8 and 64) against
   the float64 oracle at 1e-10 and against the per-graph kernels at 1e-11, EVERY graph compared -- each graph first passes
   test_range_cpu.oracle_is_normal, so the oracle is ground truth for it.  A graph may be flagged and redone by the exact
   kernel: that is the contract; exact_count is printed, not asserted.
C. Entries the scale-free forms must hand over (a contraction result that is negative, or NaN): the edited graph goes to the
   exact kernel and only it, the untouched graphs keep their bits.
"""
import numpy as np
import pytest

import cases as C
import test_gpu_instances as TI
import test_gpu_lean_memory as TM
import test_gpu_logz as GL
import test_gpu_map as GM
import test_gpu_shared as TS
import test_range_cpu as R
from helpers import batch_tables, oracle_msgs
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

RTOL = 1e-10
RTOL_EXACT = 1e-11
EXACT, SHARED_MFMA, WIDE, GENERIC, SHARED_GEMM, LEAN = 2, 3, 4, 5, 6, 7
PAIR_K = (-400, -63, 0, 1, 257, 400)
UNARY_K = (-500, -1, 0, 64, 500)
SHARED_K = (-400, 257)
F32_K = (-60, -17, 0, 1, 33, 60)
F32_SHARED_K = (-60, 33)
LN2 = float(np.log(2.0))


# ---- scaling -----------------------------------------------------------------------------------------------------------
def _exponents(fb):
    """(k per pairwise table, k per unary row) for the tables fb holds."""
    topo, B = fb.topo, fb.B
    P, U = topo.P, topo.U
    kp, ku = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    if P:
        n = fb.pair_tables.shape[0]
        f32 = fb.pair_tables.dtype == torch.float32
        cyc = F32_K if f32 else PAIR_K
        if n == B * P and not (fb.pair_tables_shared and B > 1):
            kp = np.array([cyc[(i // P + i % P) % len(cyc)] for i in range(n)], dtype=np.int32)
        else:
            two = F32_SHARED_K if f32 else SHARED_K
            kp = np.array([two[i] if i < 2 else cyc[i % len(cyc)] for i in range(n)], dtype=np.int32)
    if U:
        n = fb.unary_tables.shape[0]
        if n == B * U:
            ku = np.array([UNARY_K[(i // U + i % U) % len(UNARY_K)] for i in range(n)], dtype=np.int32)
        else:
            ku = np.array([UNARY_K[i % len(UNARY_K)] for i in range(n)], dtype=np.int32)
    return kp, ku


def _ldexp_(t, k):
    a = t.cpu().numpy()
    scaled = np.ldexp(a, k.reshape((-1,) + (1,) * (a.ndim - 1)))
    assert scaled.dtype == a.dtype and np.isfinite(scaled).all() and (np.abs(scaled[a != 0]) >= np.finfo(a.dtype).tiny).all()
    t.copy_(torch.from_numpy(scaled))


def _scale_(fb):
    """Scales fb's tables on the device, in place and exactly; returns the sum of exponents over each graph's factors [B]."""
    kp, ku = _exponents(fb)
    total = np.zeros(fb.B)
    if len(kp):
        _ldexp_(fb.pair_tables, kp)
        total += kp[fb.pair_tab.cpu().numpy()].sum(1)
    if len(ku):
        _ldexp_(fb.unary_tables, ku)
        total += ku[fb.unary_tab.cpu().numpy()].sum(1)
    return total


def _sweep(fb, roots, init=True, start=None, variant=1, grad_shape=None):
    from macaronicusermodeling_amd import _ffi
    nan = float('nan')
    if start is None:
        fb.msgs.fill_(nan)
    else:
        fb.msgs.copy_(torch.from_numpy(start))
    marg = torch.full((fb.B, fb.topo.n_vars, fb.X), nan, dtype=torch.float64, device=fb.device)
    kw = {}
    if grad_shape:
        kw['gradient'] = tuple(torch.full((fb.B, n), nan, dtype=torch.float64, device=fb.device) for n in grad_shape)
    prog = TI._with_variant(variant, lambda: fb.sweep(roots, init=init, marginals=marg, **kw))
    kernel = _ffi.lib.mlbp_last_sweep_kernel()
    torch.cuda.synchronize()
    out = dict(msgs=fb.msgs.clone(), marg=marg, status=prog.status(), exact=prog.exact_count(fb.B), kernel=kernel)
    if grad_shape:
        out['g_ee'], out['g_ed'] = kw['gradient']
    return out


def _same_bits(name, a, b, keys=('msgs', 'marg')):
    """Prints how far the two runs are apart before it asserts that they are not."""
    for k in keys:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        differ = int((x != y).sum())
        rel = float(np.max(np.abs(x - y) / np.maximum(np.abs(x), 1e-300))) if differ else 0.0
        print('%s %s: %d of %d entries differ, largest relative difference %.3g' % (name, k, differ, x.size, rel))
    print('%s: exact_count %s unscaled, %s scaled; status %s / %s' % (name, a.get('exact'), b.get('exact'), a.get('status'), b.get('status')))
    assert a.get('status', 0) == 0 and b.get('status', 0) == 0, name
    assert a.get('exact') == b.get('exact'), '%s: a flag that follows the scale' % name
    for k in keys:
        assert torch.equal(a[k], b[k]), '%s: %s changes under power-of-two scaling' % (name, k)


def _invariant(name, fb, roots, kernel, keys=('msgs', 'marg'), **kw):
    a = _sweep(fb, roots, **kw)
    _scale_(fb)
    b = _sweep(fb, roots, **kw)
    assert a['kernel'] == b['kernel'] == kernel, (name, a['kernel'], b['kernel'])
    assert not bool(torch.isnan(a['msgs']).any()) and not bool(torch.isnan(a['marg']).any())
    _same_bits(name, a, b, keys)
    return a, b


# ---- A: the lean kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pool', [None, 192], ids=['dense', 'indexed'])
@pytest.mark.parametrize('init', [True, False])
def test_scaling_lean_user_k3(init, pool):
    bt = TM._user_k3(13, 5101, **(dict(unary_pool=pool) if pool else {}))
    _invariant('lean K3 init=%s pool=%s' % (init, pool), bt.fb, bt.roots, LEAN, init=init, start=None if init else bt.start(5102))


@pytest.mark.parametrize('shape', ['star6', 'chain8', 'ring3_x48'])
def test_scaling_lean_shapes(shape):
    """star6: products of more than four sources (carry links); chain8: the seventh table in LDS; X = 48: the padded instance."""
    spec, roots, B = {'star6': (C.star_spec(6, 64), [0, 3, 0, 5], 5), 'chain8': (C.chain_spec(8, 64), [0, 7, 3, 0], 5),
                      'ring3_x48': (C.ring_spec(3, 48), [0, 2, 1, 0], 9)}[shape]
    bt = TM._Batch(spec, roots, B, 5110)
    _invariant('lean %s init' % shape, bt.fb, roots, LEAN)
    bt = TM._Batch(spec, roots, B, 5111)
    _invariant('lean %s from messages' % shape, bt.fb, roots, LEAN, init=False, start=bt.start(5112))


def test_scaling_lean_grouped_call():
    from macaronicusermodeling_amd import _ffi
    from macaronicusermodeling_amd import batch as batch_mod
    bts = [TM._user_k3(7, 5120), TM._Batch(C.star_spec(6, 64), [0, 3, 0, 5], 5, 5121)]
    runs = []
    for scaled in (False, True):
        if scaled:
            for bt in bts:
                _scale_(bt.fb)
        margs = [torch.full((bt.B, bt.topo.n_vars, 64), float('nan'), dtype=torch.float64, device=bt.fb.device) for bt in bts]
        for bt in bts:
            bt.fb.msgs.fill_(float('nan'))
        progs = batch_mod.sweep_groups([bt.fb for bt in bts], [bt.roots for bt in bts], init=True, marginals=margs)
        torch.cuda.synchronize()
        assert _ffi.lib.mlbp_last_sweep_kernel() == LEAN
        runs.append([dict(msgs=bt.fb.msgs.clone(), marg=m, status=p.status(), exact=p.exact_count(bt.B)) for bt, m, p in zip(bts, margs, progs)])
    for k, bt in enumerate(bts):
        _same_bits('lean grouped call, group %d' % k, runs[0][k], runs[1][k])


def test_scaling_lean_fused_gradient():
    """The GRAD instance: the gradient reads normalised beliefs and the features, so it has the same bits too."""
    gr = TI._Group(dict(spec='user_k3', X=64, B=9, layout='unique', kind='sweep', grad=True), 5130)
    _invariant('lean fused gradient', gr.fb, gr.roots, LEAN, keys=('msgs', 'marg', 'g_ee', 'g_ed'), grad_shape=(3, 6))


# ---- A: the exact kernels, the shared-table forms, X > 64 -----------------------------------------------------------------
@pytest.mark.parametrize('init', [True, False])
def test_scaling_exact_kernel(init):
    bt = TM._user_k3(13, 5140)
    _invariant('exact K3 init=%s' % init, bt.fb, bt.roots, EXACT, init=init, start=None if init else bt.start(5141), variant=3)


@pytest.mark.parametrize('name', ['user_k2', 'user_k3_gaps_1_2_3', 'user_k4', 'user_k4_both_pots', 'user_k5'])
def test_scaling_shared_table_forms(name):
    """B = 37: ragged 16-graph groups, neighbouring graphs of a workgroup 2^1000 apart in their unary rows."""
    fb, topo, _ = TS._shared_batch(TS.SPECS[name](), 37)
    roots = (list(topo.var_ids) * 3)[:3]
    a, _ = _invariant('shared %s' % name, fb, roots, SHARED_MFMA)
    assert a['exact'] == 0


def _group(spec, X, B, layout, seed, f32=False):
    w = dict(spec=spec, X=X, B=B, layout=layout, kind='sweep')
    if f32:
        w['f32'] = True
    return TI._Group(w, seed)


@pytest.mark.parametrize('what', ['wide_x128', 'wide_pad_x100', 'generic_x20', 'gemm_x96', 'gemm_x200', 'gemm_chunked_x1100',
                                  'wide_f32_x256', 'gemm_f32_x256'])
def test_scaling_large_state_kernels(what):
    spec, X, B, layout, kernel, variant, f32 = {
        'wide_x128': ('ring5', 128, 3, 'unique', WIDE, 1, False),
        'wide_pad_x100': ('ring3', 100, 2, 'unique', WIDE, 1, False),
        'generic_x20': ('ring5', 20, 3, 'unique', GENERIC, 3, False),
        'gemm_x96': ('ring3', 96, 19, 'shared', SHARED_GEMM, 1, False),
        'gemm_x200': ('ring3', 200, 19, 'shared', SHARED_GEMM, 1, False),
        'gemm_chunked_x1100': ('ring3', 1100, 2, 'shared', SHARED_GEMM, 1, False),
        'wide_f32_x256': ('ring5', 256, 3, 'unique', WIDE, 1, True),
        'gemm_f32_x256': ('ring3', 256, 19, 'shared', SHARED_GEMM, 1, True),
    }[what]
    gr = _group(spec, X, B, layout, 5150, f32)
    _invariant(what, gr.fb, gr.roots, kernel, variant=variant)


# ---- A: max-product and log Z ----------------------------------------------------------------------------------------------
def _explicit_inputs(spec, B, seed):
    return [C.make_inputs(spec, seed + 1000 * b) for b in range(B)]


@pytest.mark.parametrize('what', ['k3_resident', 'k4_streamed', 'x128_generic'])
def test_scaling_map_sweep(what):
    spec, roots, kernel = {'k3_resident': (R.LEAN['k3'][0](), [1, 4, 7], 1),
                           'k4_streamed': (TM._explicit(C.user_spec(10, [0, 2, 5, 8], 64, 64, seed=4)), [0, 2, 5], 1),
                           'x128_generic': (TM._explicit(C.user_spec(10, [1, 4, 7], 128, 128, seed=1)), [1, 4, 7], 2)}[what]
    fb = GM._batch(spec, _explicit_inputs(spec, 8, 5160))
    assert (fb.topo.P <= 3) == (what != 'k4_streamed')
    a = GM._run(fb, roots)
    ksum = _scale_(fb)
    b = GM._run(fb, roots)
    assert a['kernel'] == b['kernel'] == kernel
    for k in ('msgs', 'mm', 'x'):
        print('map %s %s: %d entries differ' % (what, k, int((a[k] != b[k]).sum())))
    print('map %s score: largest |(scaled - ln2 sum k) / unscaled - 1| %.3g' % (what, float(np.max(np.abs((b['score'] - LN2 * ksum) / a['score'] - 1)))))
    for k in ('msgs', 'mm', 'x'):
        assert np.array_equal(a[k], b[k]), k
    np.testing.assert_allclose(b['score'] - LN2 * ksum, a['score'], rtol=1e-12)


@pytest.mark.parametrize('what', ['k3', 'k3_shared', 'x128'])
def test_scaling_log_partition(what):
    if what == 'k3_shared':
        spec, fb, _ = GL._shared_pair(19)
        roots = GL.K3['roots']
        assert fb.pair_tables_shared
    else:
        spec, roots = (R.LEAN['k3'][0](), [1, 4, 7]) if what == 'k3' else (TM._explicit(C.user_spec(10, [1, 4, 7], 128, 128, seed=1)), [1, 4, 7])
        fb = GL._batch(spec, _explicit_inputs(spec, 8, 5170))
    labels = GL._labels(fb, seed=5)
    a = GL._run(fb, roots, labels)
    ksum = _scale_(fb)
    b = GL._run(fb, roots, labels)
    assert a['kernel'] == b['kernel'] == {'k3': 1, 'k3_shared': 2, 'x128': 3}[what]
    atol = GL.kernel_atol(fb.topo, spec['X'])
    diff = np.abs((b['log_z'] - LN2 * ksum) - a['log_z'])
    print('log Z %s: messages differ in %d entries; worst |log_z - ln2 sum k - unscaled| %.3g (atol %.3g); joint_logp worst |diff| %.3g'
          % (what, int((a['msgs'] != b['msgs']).sum()), float(diff.max()), atol, float(np.abs(a['joint'] - b['joint']).max())))
    assert np.array_equal(a['msgs'], b['msgs'])
    assert np.isfinite(a['log_z']).all() and np.isfinite(b['log_z']).all()
    assert (diff <= atol).all(), diff.max()


# ---- B: wide-range tables, every graph -------------------------------------------------------------------------------------
def _worst(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


@pytest.mark.parametrize('name,width,init', [(n, w, i) for n in ('k3', 'star6', 'chain8') for w in R.LEAN_WIDTHS
                                             for i in ((True, False) if n == 'k3' else (True,))])
def test_wide_range_lean_shapes(name, width, init):
    case = R.range_inputs(name, width)
    spec, roots, inputs = case['spec'], case['roots'], case['inputs']
    B, X = len(inputs), spec['X']
    bt = TM._Batch(spec, roots, B, 1)
    pair, unary = batch_tables(spec, bt.topo, inputs)
    bt.pair, bt.unary = pair.reshape(B, bt.topo.P, X, X), unary.reshape(B, bt.topo.U, X)
    bt.upload()
    start = None if init else R.start_messages(spec, B, 3200 + width)
    got = _sweep(bt.fb, roots, init=init, start=start)
    ex = _sweep(bt.fb, roots, init=init, start=start, variant=3)
    msgs, marg = got['msgs'].cpu().numpy(), got['marg'].cpu().numpy()
    want = []
    for b in range(B):
        pre = R.oracle_is_normal(spec, inputs[b], roots, None if start is None else start[b])
        R.assert_normal('%s sigma %d graph %d' % (name, width, b), pre)
        want.append(pre)
    wm, wg = np.stack([p['messages'] for p in want]), np.stack([p['marginals'] for p in want])
    print('wide range lean %s sigma %d init=%s: exact_count %d of %d; worst relative error against the oracle: messages %.3g marginals %.3g; '
          'against the exact kernel: messages %.3g marginals %.3g'
          % (name, width, init, got['exact'], B, _worst(msgs, wm), _worst(marg, wg), _worst(msgs, ex['msgs'].cpu().numpy()),
             _worst(marg, ex['marg'].cpu().numpy())))
    assert got['kernel'] == LEAN and ex['kernel'] == EXACT
    assert got['status'] == 0 and ex['status'] == 0
    for b in range(B):
        np.testing.assert_allclose(msgs[b], wm[b], rtol=RTOL, atol=1e-300, err_msg='messages of graph %d' % b)
        np.testing.assert_allclose(marg[b], wg[b], rtol=RTOL, atol=1e-300, err_msg='marginals of graph %d' % b)
    np.testing.assert_allclose(msgs, ex['msgs'].cpu().numpy(), rtol=RTOL_EXACT, atol=1e-300)
    np.testing.assert_allclose(marg, ex['marg'].cpu().numpy(), rtol=RTOL_EXACT, atol=1e-300)


@pytest.mark.parametrize('width', R.SHARED_WIDTHS)
@pytest.mark.parametrize('name', ['user_k2', 'user_k3_gaps_3_6', 'user_k3_gaps_1_2_3', 'user_k4', 'user_k5', 'user_k6'])
def test_wide_range_shared_table_specs(name, width):
    spec = TS.SPECS[name]()
    B = R.SHARED_B
    fb, topo, inputs = TS._shared_batch(spec, B, seed=R.SHARED_SEED, mutate=lambda i: R.scale_thetas(i, width))
    roots = (list(topo.var_ids) * 3)[:3]
    assert roots == R.range_inputs(name, width, B=1)['roots']
    got = _sweep(fb, roots)
    ex = _sweep(fb, roots, variant=3)
    msgs, marg = got['msgs'].cpu().numpy(), got['marg'].cpu().numpy()
    want = []
    for b in range(B):
        pre = R.oracle_is_normal(spec, inputs[b], roots)
        R.assert_normal('%s thetas x %d graph %d' % (name, width, b), pre)
        want.append(pre)
    wm, wg = np.stack([p['messages'] for p in want]), np.stack([p['marginals'] for p in want])
    print('wide range shared %s thetas x %d: exact_count %d of %d; worst relative error against the oracle: messages %.3g marginals %.3g; '
          'against the exact kernel: messages %.3g marginals %.3g'
          % (name, width, got['exact'], B, _worst(msgs, wm), _worst(marg, wg), _worst(msgs, ex['msgs'].cpu().numpy()),
             _worst(marg, ex['marg'].cpu().numpy())))
    assert got['kernel'] == SHARED_MFMA and ex['kernel'] != SHARED_MFMA
    assert got['status'] == 0 and ex['status'] == 0
    for b in range(B):
        np.testing.assert_allclose(msgs[b], wm[b], rtol=RTOL, atol=1e-300, err_msg='messages of graph %d' % b)
        np.testing.assert_allclose(marg[b], wg[b], rtol=RTOL, atol=1e-300, err_msg='marginals of graph %d' % b)
    np.testing.assert_allclose(msgs, ex['msgs'].cpu().numpy(), rtol=RTOL_EXACT, atol=1e-300)
    np.testing.assert_allclose(marg, ex['marg'].cpu().numpy(), rtol=RTOL_EXACT, atol=1e-300)


@pytest.mark.parametrize('name,width', R.MAP_CASES)
def test_wide_range_map_sweep(name, width):
    case = R.range_inputs(name, width)
    fb = GM._batch(case['spec'], case['inputs'])
    got = GM._run(fb, case['roots'])
    assert got['kernel'] == 1
    GM._compare('wide range %s sigma %d' % (name, width), case['spec'], fb.topo, case['inputs'], case['roots'], got, may_omit=0)


@pytest.mark.parametrize('name,width', R.LOGZ_CASES)
def test_wide_range_log_partition(name, width):
    """log_partition against the log-domain statement on the oracle's messages (test_range_cpu.log_partition_logdomain).
    K7 at sigma 20 is past the limit of include/mlbp_logz.h (the product of d_v normalised messages must stay normal) and is
    not pinned."""
    case = R.range_inputs(name, width)
    spec, roots, inputs = case['spec'], case['roots'], case['inputs']
    fb = GL._batch(spec, inputs)
    got = GL._run(fb, roots, GL._labels(fb, seed=6))
    assert got['kernel'] == 1
    base = GL.kernel_atol(fb.topo, spec['X']) + 1e-10 * GL.message_factors(fb.topo)
    worst, fails = 0.0, []
    for b, inp in enumerate(inputs):
        pre = R.oracle_is_normal(spec, inp, roots)
        R.assert_normal('%s sigma %d graph %d' % (name, width, b), pre)
        want = R.log_partition_logdomain(pre['g'], inp, pre['msgs'])
        err = abs(got['log_z'][b] - want)
        worst = max(worst, err)
        if not err <= base + 1e-12 * abs(want):
            fails.append((b, got['log_z'][b], want, err))
    print('wide range log Z %s sigma %d: %d graphs, worst |diff| to the log-domain statement %.3g (atol %.3g + 1e-12 |log Z|)'
          % (name, width, len(inputs), worst, base))
    assert not fails, fails


# ---- C: entries the scale-free forms must hand over ----------------------------------------------------------------------------
HAND_OVER = {'negative': -100.0, 'nan': float('nan')}       # -100 among U(0,1) + 0.01: the contraction's result is negative in one state


@pytest.mark.parametrize('init', [True, False])
@pytest.mark.parametrize('what', list(HAND_OVER))
def test_hand_over_lean(what, init):
    bt = TM._user_k3(13, 5201)
    start = None if init else bt.start(5202)
    _, clean, clean_marg = bt.run(init, start)
    b_edit = 5
    bt.pair[b_edit, 1, 3, 9] = HAND_OVER[what]
    bt.upload()
    from macaronicusermodeling_amd import _ffi
    prog, msgs, marg = bt.run(init, start)
    assert _ffi.lib.mlbp_last_sweep_kernel() == LEAN and prog.status() == 0
    print('hand-over lean %s init=%s: exact_count %d' % (what, init, prog.exact_count(bt.B)))
    for b in range(bt.B):
        want, wmarg = bt.oracle(b, start)
        np.testing.assert_allclose(msgs[b], want, rtol=RTOL, atol=1e-300, err_msg='messages of graph %d' % b)
        np.testing.assert_allclose(marg[b], wmarg, rtol=RTOL, atol=1e-300, err_msg='marginals of graph %d' % b)
    assert prog.exact_count(bt.B) == 1
    others = [b for b in range(bt.B) if b != b_edit]
    assert np.array_equal(msgs[others], clean[others]) and np.array_equal(marg[others], clean_marg[others])
    assert not np.array_equal(msgs[b_edit], clean[b_edit], equal_nan=True)


@pytest.mark.parametrize('what', list(HAND_OVER))
def test_hand_over_shared(what):
    """A shared batch has one copy of each pairwise table, so an edit that belongs to ONE graph reaches the device through that
    graph's unary rows: user_k3_gaps_3_6 has no pairwise factor at gap 1, and its unary en_en factors at gap 1 read columns of the
    graph's own pot_en_en_w1 -- the edit sits in such a column."""
    spec = TS.SPECS['user_k3_gaps_3_6']()
    assert not [f for f in spec['factors'] if len(f['vars']) == 2 and f['gap'] == 1]
    col = [f for f in spec['factors'] if len(f['vars']) == 1 and f['factor_type'] == 'en_en' and f['gap'] == 1][0]['observed_dim']
    B, b_edit = 37, 21

    def mutate(inputs):
        inputs[b_edit]['pot_en_en_w1'] = inputs[b_edit]['pot_en_en_w1'].copy()
        inputs[b_edit]['pot_en_en_w1'][5, col] = HAND_OVER[what]
    fb0, topo, _ = TS._shared_batch(spec, B)
    roots = (list(topo.var_ids) * 3)[:3]
    clean = _sweep(fb0, roots)
    fb, _, inputs = TS._shared_batch(spec, B, mutate=mutate)
    got = _sweep(fb, roots)
    assert clean['kernel'] == got['kernel'] == SHARED_MFMA and got['status'] == 0 and clean['exact'] == 0
    print('hand-over shared %s: exact_count %d' % (what, got['exact']))
    msgs, marg = got['msgs'].cpu().numpy(), got['marg'].cpu().numpy()
    with np.errstate(all='ignore'):
        for b in range(B):
            g, om, want = oracle_msgs(spec, inputs[b], roots)
            np.testing.assert_allclose(msgs[b], want, rtol=RTOL, atol=1e-300, err_msg='messages of graph %d' % b)
            wmarg = np.stack([O.marginal(g, om, v).reshape(-1) for v in topo.var_ids])
            np.testing.assert_allclose(marg[b], wmarg, rtol=RTOL, atol=1e-300, err_msg='marginals of graph %d' % b)
    assert got['exact'] == 1
    others = [b for b in range(B) if b != b_edit]
    assert torch.equal(got['msgs'][others], clean['msgs'][others]) and torch.equal(got['marg'][others], clean['marg'][others])
    assert not np.array_equal(msgs[b_edit], clean['msgs'][b_edit].cpu().numpy(), equal_nan=True)
