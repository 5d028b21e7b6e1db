"""The gradient and belief kernels away from unit magnitude and at padded sizes (tests/test_gpu_exponent_range.py did this for
the sweeps).  Every path that does its own arithmetic on magnitudes -- the shared-table epilogue in its DIRECT, memory and
three-source forms (c (.) message, sqrt(c) (.) message tiles against T (.) phi_k), the standalone shared gradient (X = 64 on the
matrix cores, X > 64 as contractions with a combine launch), the per-graph kernels ((c_i r_j) T in the reference's order), the
beliefs and expectation kernels, and the gradient of a graph handed over to the exact kernel -- has a case here, and every case
asserts the kernel it ran on (mlbp_last_sweep_kernel, mlbp_last_sweep_fused_gradient, the launch log).

A. Power-of-two scaling (test_gpu_exponent_range._scale_: PAIR_K / UNARY_K per own table, 2^-400 and 2^+257 on the two shared
   pots, unary rows 2^1000 apart inside one 16-graph workgroup): beliefs are S / Z, every operand of S and Z scales exactly and
   nothing leaves the normal range, so g_ee, g_ed, messages and marginals keep their BITS, status is 0 and exact_count is equal
   in both runs (0 on the shared forms).
B. Wide-range tables (tests/test_gradient_range_cpu.py: thetas times 8 and 64) against the float64 oracle's gradient, EVERY
   graph, at the project's gradient bar (test_gpu_instances.GRAD_RTOL, atol 1e-11), and against the per-graph kernels at the
   same bar.  The CPU module proves the oracle's gradient equal to a log-domain longdouble statement to 1e-12 on the same
   inputs.  exact_count is printed, not asserted.
C. Hand-over with a gradient behind it: one entry -100 or NaN in one graph.  exact_count == 1, status 0, the edited graph's
   gradient is the oracle's (NaN positions equal), every other graph keeps the bits of the clean run.
D. Padded sizes of the contraction gradient: user_k3 at X = 65, 97, 201 with a heavy last state and labels on it.

E. A normaliser Z that is itself tiny (1e-225) with every table entry, message and marginal in range
   (test_gradient_range_cpu.tiny_normaliser_inputs), and every pairwise table times 2^-700 under the standalone pairwise kernels:
   `Z > 0` is the only test a kernel may make on Z.

Do the tests notice?  Six breaks, one edited arithmetic line each, built into a library apart from the tree and run under this
module and under the modules that held the gradient before it (LAB_NOTES R37.5).  Tests of this module that fail:
1. shared_gradient_epilogue, `Z > 0.0` -> `Z > 1e-200`: test_tiny_normaliser_in_the_shared_epilogue_and_the_x64_pairwise_kernels
   (the older modules: none).
2. shared_gradient_epilogue, the bias-plane shortcut returns 1.0 with the plane flag 0: the two `random` cases of
   test_scaling_shared_table_epilogue_feature_planes, the tiny-normaliser test, all ten test_wide_range_shared_gradient (older: 25).
3. pair_gradient_x64, `Z > 0.0` -> `Z > 1e-200`: test_scaling_deep_pairwise_tables[own_x64], the tiny-normaliser test (older: none).
4. pair_gradient_combine_kernel, the same edit: test_scaling_deep_pairwise_tables[shared_x128] (older: none).
5. shared_prepare_kernel, the k == 3 weighted fragment as T * 0x1p-300: all four test_scaling_shared_table_epilogue_feature_planes,
   the tiny-normaliser test, all ten test_wide_range_shared_gradient (older: 31).
6. gradient_flagged_only with skip_pairs = 1: test_hand_over_shared_gradient[user_k4-negative], [user_k4-nan] (older: 8).
"""
import numpy as np
import pytest

import cases as C
import kernel_inventory as K
import test_gpu_exponent_range as E
import test_gpu_gradient as GG
import test_gpu_instances as TI
import test_gpu_kernels as GK
import test_gpu_shared as TS
import test_gradient_range_cpu as G
import test_range_cpu as R
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

GRAD_RTOL, GRAD_ATOL = TI.GRAD_RTOL, 1e-11
RTOL = 1e-10
EXACT, SHARED_MFMA, WIDE, GENERIC, SHARED_GEMM, LEAN = E.EXACT, E.SHARED_MFMA, E.WIDE, E.GENERIC, E.SHARED_GEMM, E.LEAN
KEYS = ('msgs', 'marg', 'g_ee', 'g_ed')
COMBINE, PAIRS64, WFRAG64 = ('pair_gradient_combine_kernel', ()), ('gradient_shared_pairs_kernel', ()), ('pair_weight_fragments_kernel', ())


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _ffi():
    from macaronicusermodeling_amd import _ffi
    return _ffi


def _replace(new):
    """(a shallow copy per graph: the cached references keep their own dicts)"""
    def mutate(inputs):
        inputs[:] = [dict(i) for i in new]
    return mutate


def _group(spec, X, B, layout, seed, mutate=None, **w):
    return TI._Group(dict(spec=spec, X=X, B=B, layout=layout, kind='sweep', grad=True, **w), seed, mutate=mutate)


def _run(fb, roots, F=(3, 6), **kw):
    """test_gpu_exponent_range._sweep with the gradient, plus what the call launched."""
    K.reset()
    out = E._sweep(fb, roots, grad_shape=F, **kw)
    out['fused'] = _ffi().lib.mlbp_last_sweep_fused_gradient()
    out['launched'], out['all'] = K.launched(), K.all_launched()
    return out


def _standalone(fb, roots, F=(3, 6), variant=1):
    """Sweeps without the gradient, then fb.gradient() from the messages in memory."""
    out = E._sweep(fb, roots, variant=variant)
    out['g_ee'] = torch.full((fb.B, F[0]), float('nan'), dtype=torch.float64, device=fb.device)
    out['g_ed'] = torch.full((fb.B, F[1]), float('nan'), dtype=torch.float64, device=fb.device)
    K.reset()
    fb.gradient(out['g_ee'], out['g_ed'])
    out['launched'], out['all'] = K.launched(), K.all_launched()
    torch.cuda.synchronize()
    assert _ffi().lib.mlbp_gradient_status() == 0
    return out


def _no_nan(run, keys=KEYS):
    for k in keys:
        assert not bool(torch.isnan(run[k]).any()), k


def _scaled_twice(name, fb, runner, kernel, want=(), absent=(), fused=None, keys=KEYS):
    """runner() on the tables as they are and on the scaled tables: the same kernels, the same bits."""
    a = runner()
    E._scale_(fb)
    b = runner()
    for r in (a, b):
        assert kernel is None or r['kernel'] == kernel, (name, r['kernel'])
        for k in want:
            assert k in r['all'], '%s did not launch %s (launched: %s)' % (name, k, r['all'])
        for k in absent:
            assert k not in r['all'], '%s launched %s' % (name, k)
        if fused is not None:
            assert r['fused'] == fused, (name, r['fused'])
    _no_nan(a, keys)
    E._same_bits(name, a, b, keys)
    return a, b


def _worst(got, want):
    got = got.cpu().numpy() if hasattr(got, 'cpu') else got
    return float(np.max(np.abs(got - want)))


def _assert_gradient(name, run, refs, graphs=None):
    """Every graph's g_ee / g_ed against the oracle's at the gradient bar; returns the worst absolute distance."""
    gee, ged = run['g_ee'].cpu().numpy(), run['g_ed'].cpu().numpy()
    worst = 0.0
    for b in (range(len(refs)) if graphs is None else graphs):
        worst = max(worst, _worst(gee[b], refs[b]['g_ee']), _worst(ged[b], refs[b]['g_ed']))
    print('%s: worst |gradient - oracle| %.3g over %d graphs' % (name, worst, len(refs)))
    for b in (range(len(refs)) if graphs is None else graphs):
        np.testing.assert_allclose(gee[b], refs[b]['g_ee'], rtol=GRAD_RTOL, atol=GRAD_ATOL, err_msg='%s: en_en gradient of graph %d' % (name, b))
        np.testing.assert_allclose(ged[b], refs[b]['g_ed'], rtol=GRAD_RTOL, atol=GRAD_ATOL, err_msg='%s: en_de gradient of graph %d' % (name, b))
    return worst


def _assert_same_gradient(name, a, b):
    for k in ('g_ee', 'g_ed'):
        np.testing.assert_allclose(a[k].cpu().numpy(), b[k].cpu().numpy(), rtol=GRAD_RTOL, atol=GRAD_ATOL, err_msg='%s: %s' % (name, k))


def _assert_messages(name, run, refs):
    msgs, marg = run['msgs'].cpu().numpy(), run['marg'].cpu().numpy()
    wm, wg = np.stack([p['messages'] for p in refs]), np.stack([p['marginals'] for p in refs])
    print('%s: worst relative error against the oracle: messages %.3g marginals %.3g' % (name, E._worst(msgs, wm), E._worst(marg, wg)))
    for b in range(len(refs)):
        np.testing.assert_allclose(msgs[b], wm[b], rtol=RTOL, atol=1e-300, err_msg='%s: messages of graph %d' % (name, b))
        np.testing.assert_allclose(marg[b], wg[b], rtol=RTOL, atol=1e-300, err_msg='%s: marginals of graph %d' % (name, b))


def _features(fb, topo, spec, inputs, labels=None):
    """set_features / set_observations on a test_gpu_shared._shared_batch: graph 0's feature tensors, the spec's labels."""
    pair_phi, kinds, obs, lab = GG._meta(spec, topo)
    fb.set_features(inputs[0]['phi_en_en'], inputs[0]['phi_en_en_w1'], inputs[0]['phi_en_de'], pair_phi, kinds)
    fb.set_observations(np.tile(lab, (fb.B, 1)) if labels is None else labels, np.tile(obs, (fb.B, 1)))


def _relabel(gr, labels):
    _, _, obs, _ = GG._meta(gr.spec, gr.topo)
    gr.fb.set_observations(labels, np.tile(obs, (gr.B, 1)))


# ---- A: the gradient as a sweep kernel's epilogue ------------------------------------------------------------------------
@pytest.mark.parametrize('name,nt', [('user_k2', 1), ('user_p2', 2)])
def test_scaling_lean_fused_gradient(name, nt):
    """The lean GRAD instances NT = 1, 2 (user_k3, NT = 3: test_gpu_exponent_range.test_scaling_lean_fused_gradient)."""
    gr = _group(name, 64, 9, 'unique', 6101 + nt)
    _scaled_twice('lean fused gradient %s' % name, gr.fb, lambda: _run(gr.fb, gr.roots), LEAN,
                  want=[('sweep_x64_lean_kernel', (nt, False, False, 0, True))], fused=1)


@pytest.mark.parametrize('name,nt', [('user_k1', 0), ('user_k2', 1), ('user_p2', 2), ('user_k3', 3)])
def test_scaling_exact_kernel_epilogue(name, nt):
    gr = _group(name, 64, 5, 'unique', 6110 + nt)
    _scaled_twice('exact kernel epilogue %s' % name, gr.fb, lambda: _run(gr.fb, gr.roots, variant=3), EXACT,
                  want=[('sweep_x64_fused_kernel', (True, nt, True))], fused=1)


# name -> (sweep_x64_shared_kernel instance, plan: product-fused, gradient from the tiles (DIRECT), three-source)
SHARED_FORMS = {
    'user_k2': ((1, False, False, False, True, True, False), (1, 0, 0)),          # product-fused; one pairwise factor: the epilogue reads memory
    'user_k3': ((2, False, False, False, True, True, False), (1, 1, 0)),          # DIRECT: the LDS tiles the sweeps left
    'user_k2_nou1': ((1, False, False, False, True, False, False), (0, 0, 0)),    # memory form
    'user_k3_nou4': ((2, False, False, False, True, False, False), (0, 0, 0)),
    'user_k4': ((2, False, False, False, True, True, True), (0, 0, 1)),           # three-source: sqrt(c) (.) message
    'user_k5': ((2, True, True, False, True, False, False), (0, 0, 0)),           # spilled and wide
}


def _plan_of(gr):
    p = gr.topo.plan(gr.roots)
    return p['shared_product_fused'], p['shared_gradient_from_tiles'], p['shared_product_fused3']


@pytest.mark.parametrize('name', list(SHARED_FORMS))
def test_scaling_shared_table_epilogue(name):
    """B = 37: ragged 16-graph workgroups.  The comment in shared_gradient_epilogue -- 'any positive per-graph scale cancels in
    S / Z' -- as a test."""
    inst, plan = SHARED_FORMS[name]
    gr = _group(name, 64, 37, 'shared', 6120)
    assert _plan_of(gr) == plan
    a, _ = _scaled_twice('shared epilogue %s' % name, gr.fb, lambda: _run(gr.fb, gr.roots), SHARED_MFMA,
                         want=[('sweep_x64_shared_kernel', inst)], fused=1)
    assert a['exact'] == 0


def _reference_planes(inputs):
    ref = C.reference_planes(inputs[0])
    for i in inputs:
        for k in ('phi_en_en', 'phi_en_en_w1', 'pot_en_en', 'pot_en_en_w1'):
            i[k] = ref[k]


@pytest.mark.parametrize('planes', ['reference', 'random'])
@pytest.mark.parametrize('name', ['user_k3', 'user_k4'])
def test_scaling_shared_table_epilogue_feature_planes(name, planes):
    """phi_en_en = [pmi, 0, 1], phi_en_en_w1 = [pmi, pmi_w1, 1] as train_mp.py stacks them: plane_flags marks the zero plane
    and the bias planes, and the epilogue returns 0 or 1 for them without contracting (user_k4 reads both tensors).  Random
    tensors: no plane is constant, neither shortcut is taken.  Either way the same bits under scaling -- and the oracle's values,
    so a shortcut taken for the wrong plane shows."""
    gr = _group(name, 64, 37, 'shared', 6130, mutate=_reference_planes if planes == 'reference' else None)
    phi, w1 = gr.inputs[0]['phi_en_en'], gr.inputs[0]['phi_en_en_w1']
    const = [bool((p[:, :, k] == p[0, 0, k]).all()) for p in (phi, w1) for k in range(3)]
    assert const == ([False, True, True, False, False, True] if planes == 'reference' else [False] * 6)
    a, _ = _scaled_twice('shared epilogue %s, %s planes' % (name, planes), gr.fb, lambda: _run(gr.fb, gr.roots), SHARED_MFMA,
                         want=[('sweep_x64_shared_kernel', SHARED_FORMS[name][0])], fused=1)
    assert a['exact'] == 0
    gr.g_ee, gr.g_ed, gr.marg = a['g_ee'], a['g_ed'], a['marg']
    gr.fb.msgs.copy_(a['msgs'])
    gr.check(sample=range(0, 37, 6))


def test_scaling_shared_grouped_call():
    from macaronicusermodeling_amd import batch as batch_mod
    grs = [_group('user_k2', 64, 17, 'shared', 6140), _group('user_k4', 64, 19, 'shared', 6141)]
    runs = []
    for scaled in (False, True):
        if scaled:
            for gr in grs:
                E._scale_(gr.fb)
        nan = float('nan')
        margs = [torch.full((gr.B, gr.topo.n_vars, 64), nan, dtype=torch.float64, device=gr.fb.device) for gr in grs]
        grads = [(torch.full((gr.B, 3), nan, dtype=torch.float64, device=gr.fb.device),
                  torch.full((gr.B, 6), nan, dtype=torch.float64, device=gr.fb.device)) for gr in grs]
        for gr in grs:
            gr.fb.msgs.fill_(nan)
        K.reset()
        progs = batch_mod.sweep_groups([gr.fb for gr in grs], [gr.roots for gr in grs], init=True, marginals=margs, gradients=grads)
        log = K.launched()
        torch.cuda.synchronize()
        assert _ffi().lib.mlbp_last_sweep_kernel() == SHARED_MFMA and _ffi().lib.mlbp_last_sweep_fused_gradient() == 1
        forms = [i[1] for i in log if i[0] == 'sweep_x64_shared_kernel']
        assert forms and all(f[3] and f[4] for f in forms), forms                       # grouped instances with the gradient
        assert sorted((f[5], f[6]) for f in forms) == [(True, False), (True, True)], forms
        runs.append([dict(msgs=gr.fb.msgs.clone(), marg=m, g_ee=g[0], g_ed=g[1], status=p.status(), exact=p.exact_count(gr.B))
                     for gr, m, g, p in zip(grs, margs, grads, progs)])
    for k in range(2):
        _no_nan(runs[0][k])
        assert runs[0][k]['exact'] == 0
        E._same_bits('shared grouped call with gradients, group %d' % k, runs[0][k], runs[1][k], KEYS)


DEEP_K = -700          # 2^-700 = 1.9e-211: a normal number, and far below any threshold a kernel might hold Z against


@pytest.mark.parametrize('what', ['own_x64', 'shared_x64', 'shared_x128'])
def test_scaling_deep_pairwise_tables(what):
    """Every pairwise table times 2^-700 (PAIR_K and the shared pots stop at 2^-400, where Z is still near 1e-121): the
    normaliser Z of a belief is itself near 1e-211, and `Z > 0` must stay the only test made on it -- in gradient_x64_kernel, in
    gradient_shared_pairs_kernel and in pair_gradient_combine_kernel.  The messages come from the per-graph kernels (variant 3),
    which normalise every message: at this depth the shared-table sweep kernel hands every graph over (measured: exact_count 37
    of 37), as its contract allows, so its epilogue never sees such a Z."""
    gr = _group('user_k3', 128 if what == 'shared_x128' else 64, 5 if what == 'own_x64' else 19, 'unique' if what == 'own_x64' else 'shared', 6146)
    kernel, want = {'own_x64': (EXACT, ('gradient_x64_kernel', (3, 6))), 'shared_x64': (EXACT, PAIRS64), 'shared_x128': (WIDE, COMBINE)}[what]
    a = _standalone(gr.fb, gr.roots, variant=3)
    E._ldexp_(gr.fb.pair_tables, np.full(gr.fb.pair_tables.shape[0], DEEP_K, dtype=np.int32))
    b = _standalone(gr.fb, gr.roots, variant=3)
    for r in (a, b):
        assert r['kernel'] == kernel and want in r['all'], (what, r['kernel'], r['all'])
    _no_nan(a)
    E._same_bits('pairwise tables times 2^%d, %s' % (DEEP_K, what), a, b, KEYS)


def test_tiny_normaliser_in_the_shared_epilogue_and_the_x64_pairwise_kernels():
    """tests/test_gradient_range_cpu.py: tiny_normaliser_inputs -- shared user_k2 whose pairwise belief has Z near 1e-225 with every
    table entry, message and marginal in range.  The sweep kernel keeps every graph (exact_count 0 is asserted: the epilogue itself
    met that Z), and the gradient is the oracle's in the epilogue, in gradient_shared_pairs_kernel and in gradient_x64_kernel."""
    case, refs = G.tiny_normaliser_reference()
    spec, B = case['spec'], len(refs)
    fb, topo, inputs = TS._shared_batch(spec, B, mutate=_replace(case['inputs']))
    _features(fb, topo, spec, inputs)
    got = _run(fb, case['roots'])
    print('tiny normaliser: exact_count %d of %d' % (got['exact'], B))
    assert got['kernel'] == SHARED_MFMA and got['fused'] == 1 and got['status'] == 0
    assert any(i[0] == 'sweep_x64_shared_kernel' and i[1][4] for i in got['launched']), got['launched']
    assert got['exact'] == 0
    _assert_messages('tiny normaliser', got, refs)
    _assert_gradient('tiny normaliser (shared epilogue)', got, refs)
    alone = _standalone(fb, case['roots'])
    assert PAIRS64 in alone['all'] and alone['exact'] == 0
    _assert_gradient('tiny normaliser (gradient_shared_pairs_kernel)', alone, refs)
    fb.use_shared_gradient = False
    per_graph = _standalone(fb, case['roots'])
    assert ('gradient_x64_kernel', (3, 6)) in per_graph['launched'] and PAIRS64 not in per_graph['all']
    _assert_gradient('tiny normaliser (gradient_x64_kernel)', per_graph, refs)


# ---- A: the standalone gradient, beliefs, expectations --------------------------------------------------------------------
@pytest.mark.parametrize('F,planar', [((1, 1), True), ((2, 2), True), ((3, 6), True), ((3, 6), False)])
def test_scaling_standalone_gradient_x64_own_tables(F, planar):
    gr = _group('user_k3', 64, 5, 'unique', 6150, F=F)
    gr.fb.use_planar = planar
    _scaled_twice('gradient_x64_kernel F=%s planar=%s' % (F, planar), gr.fb, lambda: _standalone(gr.fb, gr.roots, F), LEAN,
                  want=[('gradient_x64_kernel', F)], absent=[PAIRS64])


@pytest.mark.parametrize('gather', [True, False])
def test_scaling_standalone_gradient_x64_shared(gather):
    """gather: the unary part from mlbp_unary_expectations_f64 rows inside the pair kernel; without (_row_kind = False) the
    per-graph kernel takes the unary factors and the matrix-core kernel adds the pairwise ones."""
    gr = _group('user_k3', 64, 19, 'shared', 6160)
    if not gather:
        gr.fb._row_kind = False
    per_graph = ('gradient_x64_kernel', (3, 6))
    _scaled_twice('standalone shared gradient x64 gather=%s' % gather, gr.fb, lambda: _standalone(gr.fb, gr.roots), SHARED_MFMA,
                  want=[PAIRS64, WFRAG64] + ([('unary_expectations_kernel', ())] if gather else [per_graph]),
                  absent=[per_graph] if gather else [('unary_expectations_kernel', ())])


@pytest.mark.parametrize('approx', [False, True])
def test_scaling_standalone_gradient_x128_own_tables(approx):
    gr = _group('user_k3', 128, 5, 'unique', 6170)
    gr.fb.use_approx_beliefs = approx
    _scaled_twice('gradient_kernel x128 approx=%s' % approx, gr.fb, lambda: _standalone(gr.fb, gr.roots), WIDE,
                  want=[('gradient_kernel', (3, 6))], absent=[COMBINE])


@pytest.mark.parametrize('X', [128, 97])
def test_scaling_standalone_gradient_contraction_path(X):
    gr = _group('user_k3', X, 19, 'shared', 6180)
    a, _ = _scaled_twice('contraction gradient x%d' % X, gr.fb, lambda: _standalone(gr.fb, gr.roots), SHARED_GEMM,
                         want=[COMBINE, ('gradient_kernel', (3, 6))])
    assert any(i[0] == 'contract_kernel' and i[1][-1] == (X == 97) for i in a['launched']), a['launched']      # (the padded instance at 97)
    assert any(i[0] == 'table_frag_kernel' for i in a['launched']), a['launched']


@pytest.mark.parametrize('X', [64, 20])
def test_scaling_pair_beliefs(X):
    gr = _group('user_k3', X, 5, 'unique', 6190)

    def runner():
        out = E._sweep(gr.fb, gr.roots)
        K.reset()
        out['beliefs'] = gr.fb.pair_beliefs()
        out['all'] = K.all_launched()
        torch.cuda.synchronize()
        return out
    a, _ = _scaled_twice('pair_beliefs x%d' % X, gr.fb, runner, LEAN if X == 64 else None, want=[('pair_beliefs_kernel', ())], keys=('msgs', 'marg', 'beliefs'))
    assert float((a['beliefs'].sum((-1, -2)) - 1).abs().max()) < 1e-12


def test_scaling_unary_expectations():
    rs = np.random.RandomState(6200)
    n_rows, Vde = 23, 30
    tables = rs.rand(n_rows, 64) + 0.01
    kind = np.array([0, 1, 2] * 8, np.int32)[:n_rows]
    obs = np.where(kind == 2, rs.randint(0, Vde, n_rows), rs.randint(0, 64, n_rows)).astype(np.int32)
    t_ee, t_w1, t_ed = GK._up(rs.rand(64, 64, 3)), GK._up(rs.rand(64, 64, 3)), GK._up(rs.rand(Vde, 64, 6))
    k = np.array([E.UNARY_K[i % len(E.UNARY_K)] for i in range(n_rows)])
    outs = []
    for t in (tables, np.ldexp(tables, k[:, None])):
        out = GK._full((n_rows * 8,), GK.NAN)
        GK._status()
        with GK._Launches('unary_expectations_kernel'):
            GK._call('mlbp_unary_expectations_f64', GK._up(t), n_rows, 64, GK._up(kind), GK._up(obs), t_ee, t_w1, t_ed, 3, 6, Vde, out)
        assert GK._status() == 0
        outs.append(out.cpu().numpy().reshape(n_rows, 8))
    F = np.where(kind == 2, 6, 3)
    live = np.arange(8)[None, :] < F[:, None]
    assert not np.isnan(outs[0][live]).any() and np.isnan(outs[0][~live]).all()
    print('unary expectations: %d of %d entries differ under scaling' % (int((outs[0][live] != outs[1][live]).sum()), int(live.sum())))
    assert np.array_equal(outs[0][live], outs[1][live])


def test_potentials_expect_is_unary_expectations_of_the_produced_table():
    """mlbp_potentials_multi_f64's `expect` at thetas times 64 (a theta shift that multiplies a column by an exact power of two is
    not available): bit for bit what mlbp_unary_expectations_f64 gives on the pot_t the same launch produced."""
    rs = np.random.RandomState(6210)
    cols, F = 40, 6
    phi = rs.rand(64, cols, F)
    theta = (rs.randn(1, F) * 0.5) * 64
    pot_t, ex = GK._full((1, cols * 64), GK.NAN), GK._full((1, cols * 8), GK.NAN)
    tphi, ttheta = GK._up(phi), GK._up(theta)
    with GK._Launches('potentials_multi_kernel'):
        GK._multi([GK._job(tphi, ttheta, None, pot_t, ex, (F, 0, cols * 64, cols * 8), F)], 1)
    tables = pot_t.cpu().numpy().reshape(cols, 64)
    assert np.isfinite(tables).all() and tables.min() > 0 and tables.max() / tables.min() > 1e30
    out = GK._full((cols * 8,), GK.NAN)
    t_ed = GK._up(np.ascontiguousarray(phi.transpose(1, 0, 2)))
    z = GK._up(np.zeros((64, 64, 3)))
    GK._status()
    with GK._Launches('unary_expectations_kernel'):
        GK._call('mlbp_unary_expectations_f64', pot_t, cols, 64, GK._up(np.full(cols, 2, np.int32)), GK._up(np.arange(cols, dtype=np.int32)),
                 z, z, t_ed, 3, F, cols, out)
    assert GK._status() == 0
    a, b = ex.cpu().numpy().reshape(cols, 8)[:, :F], out.cpu().numpy().reshape(cols, 8)[:, :F]
    differ = int((a != b).sum())
    print('potentials expect against unary expectations: %d of %d entries differ, largest relative difference %.3g'
          % (differ, a.size, float(np.max(np.abs(a - b) / np.abs(b)))))
    want = (tables[:, :, None] * phi.transpose(1, 0, 2)).sum(1) / tables.sum(1)[:, None]
    np.testing.assert_allclose(b, want, rtol=1e-11)
    assert np.array_equal(a, b)


# ---- B: wide-range tables against the oracle, every graph -------------------------------------------------------------------
@pytest.mark.parametrize('name,width', G.SHARED_CASES)
def test_wide_range_shared_gradient(name, width):
    case, refs = G.shared_reference(name, width)
    spec, B = case['spec'], len(refs)
    fb, topo, inputs = TS._shared_batch(spec, B, seed=R.SHARED_SEED, mutate=lambda i: (R.scale_thetas(i, width), G._batch_features(i)))
    assert all(np.array_equal(inputs[b]['pot_en_de'], case['inputs'][b]['pot_en_de']) for b in (0, 5, B - 1))
    _features(fb, topo, spec, inputs)
    roots = case['roots']
    for b, pre in enumerate(refs):
        R.assert_normal('%s thetas x %d graph %d' % (name, width, b), pre)
    got = _run(fb, roots)
    fb.use_shared_gradient = False                           # (larger cliques: the per-graph gradient kernel behind the exact sweeps)
    ex = _run(fb, roots, variant=3)
    assert PAIRS64 not in ex['all'] and (('gradient_x64_kernel', (3, 6)) in ex['launched'] or
                                         ('sweep_x64_fused_kernel', (True, topo.P, True)) in ex['launched']), ex['launched']
    tag = 'wide range shared gradient %s thetas x %d' % (name, width)
    print('%s: exact_count %d of %d' % (tag, got['exact'], B))
    assert got['kernel'] == SHARED_MFMA and got['fused'] == 1 and ex['kernel'] != SHARED_MFMA
    assert any(i[0] == 'sweep_x64_shared_kernel' and i[1][4] for i in got['launched']), got['launched']
    assert got['status'] == 0 and ex['status'] == 0
    _assert_gradient(tag, got, refs)
    _assert_gradient(tag + ' (per-graph kernels)', ex, refs)
    _assert_same_gradient(tag + ' against the per-graph kernels', got, ex)


@pytest.mark.parametrize('name,width', G.OWN_CASES)
def test_wide_range_own_table_gradient(name, width):
    case, refs = G.own_reference(name, width)
    gr = _group(name, 64, G.OWN_B, 'unique', 6300, mutate=_replace(case['inputs']))
    for b, pre in enumerate(refs):
        R.assert_normal('own tables %s thetas x %d graph %d' % (name, width, b), pre)
    got = _run(gr.fb, gr.roots)
    ex = _run(gr.fb, gr.roots, variant=3)
    tag = 'wide range own-table gradient %s thetas x %d' % (name, width)
    print('%s: exact_count %d of %d' % (tag, got['exact'], gr.B))
    assert got['kernel'] == LEAN and got['fused'] == 1 and ex['kernel'] == EXACT and ex['fused'] == 1
    assert got['status'] == 0 and ex['status'] == 0
    _assert_gradient(tag, got, refs)
    _assert_gradient(tag + ' (exact kernel)', ex, refs)
    _assert_same_gradient(tag + ' against the exact kernel', got, ex)
    alone = _standalone(gr.fb, gr.roots)                     # gradient_x64_kernel from the messages in memory
    assert ('gradient_x64_kernel', (3, 6)) in alone['launched']
    _assert_gradient(tag + ' (standalone)', alone, refs)


def test_wide_range_standalone_shared_gradient_x128():
    case, refs = G.standalone_x128_reference()
    gr = _group('user_k3', 128, len(refs), 'shared', 6310, mutate=_replace(case['inputs']))
    for b, pre in enumerate(refs):
        R.assert_normal('user_k3 x128 thetas x 8 graph %d' % b, pre)
    got = _standalone(gr.fb, gr.roots)
    assert got['kernel'] == SHARED_GEMM and got['status'] == 0 and COMBINE in got['all']
    _assert_messages('wide range x128', got, refs)
    _assert_gradient('wide range standalone shared gradient x128 thetas x 8', got, refs)


# ---- C: hand-over with a gradient behind it -----------------------------------------------------------------------------------
def _assert_hand_over(tag, got, clean, ref, b_edit, B):
    print('hand-over %s: exact_count %d, status %d' % (tag, got['exact'], got['status']))
    assert got['status'] == 0 and clean['status'] == 0 and clean['exact'] == 0
    assert got['exact'] == 1
    gee, ged = got['g_ee'][b_edit].cpu().numpy(), got['g_ed'][b_edit].cpu().numpy()
    print('hand-over %s: edited graph, worst |gradient - oracle| %.3g' % (tag, max(_worst(gee, ref['g_ee']), _worst(ged, ref['g_ed']))))
    assert np.array_equal(np.isnan(gee), np.isnan(ref['g_ee'])) and np.array_equal(np.isnan(ged), np.isnan(ref['g_ed']))
    np.testing.assert_allclose(gee, ref['g_ee'], rtol=GRAD_RTOL, atol=GRAD_ATOL)
    np.testing.assert_allclose(ged, ref['g_ed'], rtol=GRAD_RTOL, atol=GRAD_ATOL)
    others = [b for b in range(B) if b != b_edit]
    for k in KEYS:
        assert torch.equal(got[k][others], clean[k][others]), '%s: %s of an untouched graph changed' % (tag, k)
    assert not torch.equal(got['g_ee'][b_edit], clean['g_ee'][b_edit]) or not torch.equal(got['g_ed'][b_edit], clean['g_ed'][b_edit])


@pytest.mark.parametrize('init', [True, False])
@pytest.mark.parametrize('what', list(G.HAND_OVER))
def test_hand_over_lean_gradient(what, init):
    h = G.hand_over_inputs('lean_user_k3', what)
    B, b = len(h['inputs']), h['b_edit']
    start = None if init else R.start_messages(h['spec'], B, 6401)
    runs = {}
    for key in ('clean', 'inputs'):
        gr = _group('user_k3', 64, B, 'unique', 6400, mutate=_replace(h[key]))
        runs[key] = _run(gr.fb, gr.roots, init=init, start=start)
        assert runs[key]['kernel'] == LEAN and runs[key]['fused'] == 1
        assert ('sweep_x64_lean_kernel', (3, False, False, 0, True)) in runs[key]['launched']
    assert ('sweep_x64_fused_kernel', (True, 3, True)) in runs['inputs']['launched']          # the exact kernel's own epilogue
    ref = G.graph_reference(h['spec'], h['inputs'][b], h['roots'], None if init else start[b])
    _assert_hand_over('lean %s init=%s' % (what, init), runs['inputs'], runs['clean'], ref, b, B)


@pytest.mark.parametrize('what', list(G.HAND_OVER))
@pytest.mark.parametrize('name', ['user_k3_gaps_3_6', 'user_k4'])
def test_hand_over_shared_gradient(name, what):
    """user_k3_gaps_3_6: the fix-up pass of the exact kernel carries the gradient.  user_k4 (six pairwise factors, the exact kernel
    streams its tables and has no epilogue): gradient_flagged_only, the per-graph kernel on the flagged graph alone."""
    h = G.hand_over_inputs('shared_' + name, what)
    B, b, spec = len(h['inputs']), h['b_edit'], h['spec']
    runs = {}
    for key in ('clean', 'inputs'):
        fb, topo, inputs = TS._shared_batch(spec, B, mutate=_replace(h[key]))
        _features(fb, topo, spec, inputs)
        runs[key] = _run(fb, h['roots'])
        assert runs[key]['kernel'] == SHARED_MFMA and runs[key]['fused'] == 1
    fix = ('gradient_x64_kernel', (3, 6)) if name == 'user_k4' else ('sweep_x64_fused_kernel', (True, 3, True))
    assert fix in runs['inputs']['launched'], runs['inputs']['launched']
    with np.errstate(all='ignore'):
        ref = G.graph_reference(spec, h['inputs'][b], h['roots'])
    _assert_hand_over('shared %s %s' % (name, what), runs['inputs'], runs['clean'], ref, b, B)


@pytest.mark.parametrize('what', list(G.HAND_OVER))
def test_hand_over_grouped_shared_gradient(what):
    """The edited graph sits in the second group of one grouped call: gradient_x64_groups_kernel."""
    from macaronicusermodeling_amd import batch as batch_mod
    first = G.shared_inputs('user_k2', 1, B=17)
    h = G.hand_over_inputs('shared_user_k3_gaps_3_6', what, B=19, b_edit=11)
    b = h['b_edit']
    runs = {}
    for key in ('clean', 'inputs'):
        built = []
        for case, inp in ((first, first['inputs']), (h, h[key])):
            fb, topo, inputs = TS._shared_batch(case['spec'], len(inp), mutate=_replace([dict(i) for i in inp]))
            _features(fb, topo, case['spec'], inputs)
            built.append((fb, topo, case['roots']))
        nan = float('nan')
        margs = [torch.full((fb.B, topo.n_vars, 64), nan, dtype=torch.float64, device=fb.device) for fb, topo, _ in built]
        grads = [(torch.full((fb.B, 3), nan, dtype=torch.float64, device=fb.device),
                  torch.full((fb.B, 6), nan, dtype=torch.float64, device=fb.device)) for fb, _, _ in built]
        for fb, _, _ in built:
            fb.msgs.fill_(nan)
        K.reset()
        progs = batch_mod.sweep_groups([fb for fb, _, _ in built], [r for _, _, r in built], init=True, marginals=margs, gradients=grads)
        log = K.all_launched()
        torch.cuda.synchronize()
        assert _ffi().lib.mlbp_last_sweep_kernel() == SHARED_MFMA and _ffi().lib.mlbp_last_sweep_fused_gradient() == 1
        assert ('gradient_x64_groups_kernel', ()) in log, log
        runs[key] = [dict(msgs=fb.msgs.clone(), marg=m, g_ee=g[0], g_ed=g[1], status=p.status(), exact=p.exact_count(fb.B))
                     for (fb, _, _), m, g, p in zip(built, margs, grads, progs)]
    for k in KEYS:                                           # the first group: untouched as a whole
        assert torch.equal(runs['inputs'][0][k], runs['clean'][0][k]), k
    assert runs['inputs'][0]['exact'] == 0 and runs['inputs'][0]['status'] == 0
    with np.errstate(all='ignore'):
        ref = G.graph_reference(h['spec'], h['inputs'][b], h['roots'])
    _assert_hand_over('grouped shared %s' % what, runs['inputs'][1], runs['clean'][1], ref, b, 19)


# ---- D: padded sizes of the contraction gradient ---------------------------------------------------------------------------------
def _padded_group(X, B, layout):
    case, refs = G.padded_reference(X, B)
    gr = _group('user_k3', X, B, layout, 6500, mutate=_replace(case['inputs']))
    _relabel(gr, case['labels'])
    for b, pre in enumerate(refs):
        R.assert_normal('padded user_k3 x%d graph %d' % (X, b), pre)
    return gr, refs


@pytest.mark.parametrize('X,B', [(65, 19), (97, 19), (201, 19), (97, 1)])
def test_padded_contraction_gradient(X, B):
    gr, refs = _padded_group(X, B, 'shared')
    tag = 'padded contraction gradient x%d B=%d' % (X, B)
    got = _run(gr.fb, gr.roots)                              # the gradient behind the sweeps of the call
    assert got['kernel'] == SHARED_GEMM and got['status'] == 0
    assert any(i[0] == 'contract_kernel' and i[1][-1] is True for i in got['launched']), got['launched']      # the padded instances
    assert COMBINE in got['all'] and ('gradient_kernel', (3, 6)) in got['launched']
    _assert_messages(tag, got, refs)
    _assert_gradient(tag + ' (behind the sweeps)', got, refs)
    alone = _standalone(gr.fb, gr.roots)
    assert alone['kernel'] == SHARED_GEMM and COMBINE in alone['all']
    _assert_gradient(tag + ' (standalone)', alone, refs)


def test_padded_per_graph_gradient_and_beliefs_x65():
    """The same tables in the own-table layout: gradient_kernel and pair_beliefs_kernel at X = 65."""
    gr, refs = _padded_group(65, 3, 'unique')
    got = _standalone(gr.fb, gr.roots)
    assert got['kernel'] == WIDE and got['status'] == 0
    assert ('gradient_kernel', (3, 6)) in got['launched'] and COMBINE not in got['all']
    _assert_messages('padded x65 own tables', got, refs)
    _assert_gradient('padded gradient_kernel x65', got, refs)
    K.reset()
    bel = gr.fb.pair_beliefs().cpu().numpy()
    assert ('pair_beliefs_kernel', ()) in K.all_launched()
    worst = 0.0
    for b, pre in enumerate(refs):
        for p, j in enumerate(gr.topo.pair_factors):
            want = O.factor_beliefs(pre['g'], gr.inputs[b], pre['msgs'], gr.topo.factor_ids[j])
            worst = max(worst, E._worst(bel[b, p], want))
            np.testing.assert_allclose(bel[b, p], want, rtol=RTOL, atol=1e-300, err_msg='beliefs of graph %d factor %d' % (b, p))
    print('padded pair_beliefs x65: worst relative error against the oracle %.3g' % worst)
