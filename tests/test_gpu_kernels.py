"""GPU parity per kernel outside the sweep and contraction families: the statistics reductions, potentials and expectations,
the per-instance patched tables, marginals, beliefs, log-posteriors, top-k and every `au.*` primitive.  Each case calls the
kernel's C entry (or its Python wrapper), checks in the launch log (mlbp_launch_log) that the kernel ran, and compares the
output with a float64 NumPy statement of the operation or with oracle/array_oracle.py, at the shapes where the kernel
branches: register paths against loops, column chunks, workgroup and grid limits, LDS limits, empty selections and gaps.

Tolerances: integers and index sets exact; sums 1e-11 relative (inputs of one sign, so that a relative error means
something); exp and log 1e-13.  Kernels that promise a fixed summation order are called twice and give the same bits.
Outputs are prefilled with NaN or a sentinel, so that a slot the kernel should not write -- or should, and did not -- shows.

CASES (kernel -> the tests here that reach it) is checked against the built library by tests/test_kernel_inventory.py,
together with test_gpu_instances.COVERED and COMPOUND (the kernels that run only inside a sweep or gradient call).
"""
import ctypes as C

import numpy as np
import pytest

import kernel_inventory as K
from oracle import array_oracle as AO

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-11
EXP_RTOL = 1e-13
NAN = float('nan')
DBL_MAX = np.finfo(np.float64).max
EINVAL, EUNSUPPORTED = -1, -5

# kernel -> the tests of this module that launch it and check its output
CASES = {
    ('sum_rows_kernel', ()): ['test_select_sum_rows', 'test_select_sum_rows_column_limit',
                              'test_select_sum_rows_in_a_replayed_graph', 'test_step_statistics_other_feature_counts'],
    ('step_statistics_kernel', (3, 6)): ['test_step_statistics'],
    ('segment_sum_rows_kernel', ()): ['test_segment_sum_rows'],
    ('potentials_kernel', ()): ['test_potentials'],
    ('potentials_multi_kernel', ()): ['test_potentials_multi_with_expectations', 'test_potentials_multi_general_path'],
    ('unary_expectations_kernel', ()): ['test_unary_expectations'],
    ('patch_tables_kernel', ()): ['test_patch_tables'],
    ('patch_gradient_kernel', ()): ['test_patch_gradient'],
    ('log_posterior_kernel', ()): ['test_log_posterior', 'test_log_posterior_batch_limit_and_alternating_counters'],
    ('log_posterior_groups_kernel', ()): ['test_log_posterior_groups'],
    ('topk_kernel', ()): ['test_topk', 'test_topk_strided', 'test_topk_limits', 'test_topk_rows', 'test_topk_nan',
                          'test_topk_rows_nan', 'test_sparse_products_with_nan_entries'],
    ('fill_kernel', ()): ['test_init_messages'],
    ('marginals_kernel', ()): ['test_marginals'],
    ('pair_beliefs_kernel', ()): ['test_pair_beliefs'],
    ('dense_dot_kernel', ()): ['test_dense_dot'],
    ('dense_dot_thin_kernel', ()): ['test_dense_dot'],
    ('pointwise_multiply_kernel', ()): ['test_pointwise_multiply'],
    ('normalize_kernel', ()): ['test_normalize'],
    ('gather_dot_kernel', ()): ['test_sparse_vec_mat_dot', 'test_sparse_products_with_nan_entries'],
    ('block_op_kernel', ()): ['test_sparse_block_ops'],
    ('block_sum_kernel', ()): ['test_sparse_block_ops'],
    ('zero_kernel', ()): ['test_sparse_block_ops'],
    ('log_kernel', ()): ['test_log'],
    ('observed_minus_kernel', ()): ['test_observed_minus'],
}


# ---- helpers ---------------------------------------------------------------------------------------------------------
def _lib():
    from macaronicusermodeling_amd import _ffi
    return _ffi


def _dev():
    return torch.device('cuda:0')


def _stream():
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _full(shape, v, dtype=torch.float64):
    return torch.full(shape, v, dtype=dtype, device=_dev())


def _call(name, *args):
    """The C entry `name` on the current stream (tensors passed by their device address); MlbpError on a failure code."""
    f = _lib()
    args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    return f.check(getattr(f.lib, name)(*args, _stream()))


def _refused(code, name, *args):
    with pytest.raises(_lib().MlbpError) as e:
        _call(name, *args)
    assert e.value.code == code, e.value


class _Launches:
    """`with _Launches(kernel, ...):` -- the calls inside launch every named kernel, and none of `absent`.  A kernel is named
    by its identifier (a plain kernel) or as (identifier, template arguments)."""

    def __init__(self, *kernels, absent=()):
        key = lambda k: k if isinstance(k, tuple) else (k, ())          # noqa: E731
        self.kernels, self.absent = [key(k) for k in kernels], [key(k) for k in absent]

    def __enter__(self):
        K.reset()
        return self

    def __exit__(self, typ, *_):
        if typ is None:
            torch.cuda.synchronize()
            self.log = K.all_launched()
            for k in self.kernels:
                assert k in self.log, '%s did not launch (launched: %s)' % (k, self.log)
            for k in self.absent:
                assert k not in self.log, '%s launched' % (k,)
        return False


def _status():
    """mlbp_gradient_status: synchronising read-and-reset of the status word of the statistics and gradient kernels."""
    torch.cuda.synchronize()
    return _lib().lib.mlbp_gradient_status()


def _lp_reference(marg, labels, X):
    """LBP.py:247-259 per graph: sum_v log marg[b][v][labels[b][v]] with log 0 -> -99.99; a label out of [0, X) is skipped."""
    B, nv = labels.shape
    out = np.zeros(B)
    for v in range(nv):
        lab = labels[:, v]
        ok = (lab >= 0) & (lab < X)
        with np.errstate(divide='ignore'):
            lp = np.log(marg[np.arange(B), v, np.where(ok, lab, 0)])
        out += np.where(ok, np.where(np.isneginf(lp), -99.99, lp), 0.0)
    return out


def _lexsort_topk(v, K):
    """The K largest of v: numbers by value, NaN below every number, ties (NaNs among themselves too) to the lower index."""
    return np.lexsort((np.arange(v.size), -v))[:K]


# ---- fixed-order row sums --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [1, 63, 64 * 5 + 1, 3000])
@pytest.mark.parametrize('cols', [(5, 0, 0), (3, 6, 1), (30, 20, 13)])
def test_select_sum_rows(rows, cols):
    """mlbp_select_sum_rows_cat_f64: the columns of up to three arrays summed over the rows whose key equals *key_value, the
    count of those rows appended (63 columns and the count: all 64 of the kernel).  A key no row has gives zeros and a count
    of 0; a key every row has, or no key, gives every row and B.  Fewer rows than the 64 slices leave slices empty.  Two calls: the same bits."""
    rs = np.random.RandomState(rows * 7 + sum(cols))
    arrs = [(rs.rand(rows, c) + 0.5) * (1 + np.arange(c)) for c in cols]
    key = rs.randint(0, 3, size=rows).astype(np.int32)
    key[0] = 1
    t = [_up(a) if c else None for a, c in zip(arrs, cols)]
    tkey, tsame = _up(key), _up(np.full(rows, 4, np.int32))
    n = sum(cols)
    for tk, kv, sel in ((tkey, 1, key == 1), (tkey, 7, np.zeros(rows, bool)), (tsame, 4, np.ones(rows, bool)),
                        (None, None, np.ones(rows, bool))):
        got = []
        for _ in range(2):
            out = _full((n + 2,), NAN)
            with _Launches('sum_rows_kernel'):
                _call('mlbp_select_sum_rows_cat_f64', t[0], cols[0], t[1], cols[1], t[2], cols[2], rows,
                      tk, _up(np.array([kv], np.int32)) if kv is not None else None, 1, out)
            got.append(out.cpu().numpy())
        assert got[0].tobytes() == got[1].tobytes(), 'not the same bits on a second call'
        assert got[0][n] == sel.sum(), 'count'
        assert np.isnan(got[0][n + 1]), 'written past the count'
        if sel.any():
            want = np.concatenate([a[sel].sum(0) for a, c in zip(arrs, cols) if c])
            np.testing.assert_allclose(got[0][:n], want, rtol=SUM_RTOL, atol=0)
        else:
            assert (got[0][:n] == 0).all()


def test_select_sum_rows_column_limit():
    """64 columns without the count are accepted; 64 with it, or 65, are refused (EUNSUPPORTED)."""
    rs = np.random.RandomState(5)
    rows = 257
    a, b, c = rs.rand(rows, 30) + 0.5, rs.rand(rows, 20) + 0.5, rs.rand(rows, 14) + 0.5
    ta, tb, tc = _up(a), _up(b), _up(c)
    out = _full((66,), NAN)
    with _Launches('sum_rows_kernel'):
        _call('mlbp_select_sum_rows_cat_f64', ta, 30, tb, 20, tc, 14, rows, None, None, 0, out)
    got = out.cpu().numpy()
    np.testing.assert_allclose(got[:64], np.concatenate([a.sum(0), b.sum(0), c.sum(0)]), rtol=SUM_RTOL, atol=0)
    assert np.isnan(got[64:]).all()
    _refused(EUNSUPPORTED, 'mlbp_select_sum_rows_cat_f64', ta, 30, tb, 20, tc, 14, rows, None, None, 1, out)
    _refused(EUNSUPPORTED, 'mlbp_select_sum_rows_cat_f64', ta, 30, tb, 20, tc, 15, rows, None, None, 0, out)


def test_select_sum_rows_in_a_replayed_graph():
    """The trainer's minibatch selection: one captured torch.cuda.graph (one stream), *key_value changed on the device between
    replays, each replay sums the rows of the new key."""
    rs = np.random.RandomState(6)
    rows, cols = 1000, 9
    a = rs.rand(rows, cols) + 0.5
    key = rs.randint(0, 4, size=rows).astype(np.int32)
    ta, tkey, tkv = _up(a), _up(key), _up(np.array([0], np.int32))
    out = _full((cols + 1,), NAN)
    g = torch.cuda.CUDAGraph()
    with _Launches('sum_rows_kernel'):
        with torch.cuda.graph(g):
            _call('mlbp_select_sum_rows_cat_f64', ta, cols, None, 0, None, 0, rows, tkey, tkv, 1, out)
    for kv in (2, 0, 3, 9, 2):
        tkv.fill_(kv)
        out.fill_(NAN)
        g.replay()
        torch.cuda.synchronize()
        got, sel = out.cpu().numpy(), key == kv
        assert got[cols] == sel.sum()
        if sel.any():
            np.testing.assert_allclose(got[:cols], a[sel].sum(0), rtol=SUM_RTOL, atol=0)
        else:
            assert (got[:cols] == 0).all()


def _statistics_inputs(seed, B, n_vars, X, F):
    rs = np.random.RandomState(seed)
    marg = rs.rand(B, n_vars, X) * 0.9 + 0.05
    labels = rs.randint(0, X, size=(B, n_vars)).astype(np.int32)
    marg[5, n_vars - 1, labels[5, n_vars - 1]] = 0.0                  # log 0 -> -99.99
    marg[6, 0, labels[6, 0]] = 0.0
    return marg, labels, rs.rand(B, F[0]) + 0.5, rs.rand(B, F[1]) + 0.5


@pytest.mark.parametrize('n_vars', [8, 9])
@pytest.mark.parametrize('bad_label', [False, True])
@pytest.mark.parametrize('lp_out', [False, True])
def test_step_statistics(n_vars, bad_label, lp_out):
    """mlbp_step_statistics_f64 at F = (3, 6): [sum g_ee | sum g_ed | sum log-posterior | B] with the per-graph log-posteriors
    (LBP.py:247-259, log 0 -> -99.99) -- n_vars <= 8 in registers, 9 by the loop.  A label out of range is skipped and sets
    mlbp_gradient_status, in either path.  Two calls: the same bits."""
    B, X = 1000, 7
    marg, labels, gee, ged = _statistics_inputs(n_vars + 10 * bad_label, B, n_vars, X, (3, 6))
    if bad_label:
        labels[9, n_vars - 1] = X
        labels[10, 0] = -1
    tm, tl, ta, tb = _up(marg), _up(labels), _up(gee), _up(ged)
    lp_want = _lp_reference(marg, labels, X)
    want = np.concatenate([gee.sum(0), ged.sum(0), [lp_want.sum(), B]])
    _status()
    got = []
    for _ in range(2):
        out, lp = _full((12,), NAN), (_full((B + 1,), NAN) if lp_out else None)
        with _Launches(('step_statistics_kernel', (3, 6)), absent=['sum_rows_kernel']):
            _call('mlbp_step_statistics_f64', ta, 3, tb, 6, tm, tl, n_vars, X, B, lp, out)
        assert _status() == (1 if bad_label else 0)
        got.append(out.cpu().numpy())
        if lp_out:
            lpg = lp.cpu().numpy()
            np.testing.assert_allclose(lpg[:B], lp_want, rtol=EXP_RTOL, atol=0)
            assert np.isnan(lpg[B])
    assert got[0].tobytes() == got[1].tobytes()
    np.testing.assert_allclose(got[0][:11], want, rtol=SUM_RTOL, atol=0)
    assert np.isnan(got[0][11])


@pytest.mark.parametrize('F', [(2, 2), (1, 1), (5, 7)])
def test_step_statistics_other_feature_counts(F):
    """Feature counts other than (3, 6) take sum_rows_kernel with the log-posterior column: the same statistics vector."""
    B, X, n_vars = 700, 5, 4
    marg, labels, gee, ged = _statistics_inputs(20 + F[1], B, n_vars, X, F)
    lp_want = _lp_reference(marg, labels, X)
    want = np.concatenate([gee.sum(0), ged.sum(0), [lp_want.sum(), B]])
    n = F[0] + F[1] + 2
    out, lp = _full((n + 1,), NAN), _full((B,), NAN)
    _status()
    with _Launches('sum_rows_kernel', absent=[('step_statistics_kernel', (3, 6))]):
        _call('mlbp_step_statistics_f64', _up(gee), F[0], _up(ged), F[1], _up(marg), _up(labels), n_vars, X, B, lp, out)
    assert _status() == 0
    got = out.cpu().numpy()
    np.testing.assert_allclose(got[:n], want, rtol=SUM_RTOL, atol=0)
    assert np.isnan(got[n])
    np.testing.assert_allclose(lp.cpu().numpy(), lp_want, rtol=EXP_RTOL, atol=0)


@pytest.mark.parametrize('cols', [1, 16, 17, 33])
@pytest.mark.parametrize('rows', [1, 1000])
def test_segment_sum_rows(cols, rows):
    """mlbp_segment_sum_rows_f64: out[s] = sum of the rows with seg_id == s, in 16-column chunks; a segment no row names is
    zero; ids >= n_seg are ignored; rows not a multiple of the workgroup.  Two calls: the same bits."""
    rs = np.random.RandomState(cols + rows)
    n_seg = 5
    a = (rs.rand(rows, cols) + 0.5) * (1 + np.arange(cols))
    seg = rs.randint(0, n_seg + 3, size=rows).astype(np.int32)
    seg[seg == 3] = n_seg + 1                                          # segment 3: empty
    seg[0] = 1
    ta, ts = _up(a), _up(seg)
    got = []
    for _ in range(2):
        out = _full((n_seg * cols + 1,), NAN)
        with _Launches('segment_sum_rows_kernel'):
            _call('mlbp_segment_sum_rows_f64', ta, rows, cols, ts, n_seg, out)
        got.append(out.cpu().numpy())
    assert got[0].tobytes() == got[1].tobytes()
    assert np.isnan(got[0][-1])
    o = got[0][:-1].reshape(n_seg, cols)
    for s in range(n_seg):
        sel = seg == s
        if sel.any():
            np.testing.assert_allclose(o[s], a[sel].sum(0), rtol=SUM_RTOL, atol=0, err_msg='segment %d' % s)
        else:
            assert (o[s] == 0).all(), 'segment %d' % s


# ---- potentials and expectations -------------------------------------------------------------------------------------
def _exp_dot(phi, theta):
    """exp(sum_k phi[..., k] theta[k]), the sum in k order."""
    acc = np.zeros(phi.shape[:-1])
    for k in range(phi.shape[-1]):
        acc = acc + phi[..., k] * theta[k]
    with np.errstate(over='ignore'):
        return np.exp(acc)


def test_potentials():
    """mlbp_potentials_f64: pot = exp(phi . theta) row-major and transposed; exp past the range is inf, as NumPy's."""
    rs = np.random.RandomState(7)
    rows, cols, F = 37, 50, 3
    phi, theta = rs.rand(rows, cols, F) * 2, np.array([1.0, -0.5, 0.75])
    phi[4, 7] = [500.0, 0.0, 400.0]                                    # exp(800) = inf
    want = _exp_dot(phi, theta)
    assert np.isinf(want[4, 7])
    pot, pot_t = _full((rows * cols + 1,), NAN), _full((rows * cols + 1,), NAN)
    with _Launches('potentials_kernel'):
        _call('mlbp_potentials_f64', _up(phi), _up(theta), rows, cols, F, pot, pot_t)
    p, pt = pot.cpu().numpy(), pot_t.cpu().numpy()
    np.testing.assert_allclose(p[:-1].reshape(rows, cols), want, rtol=EXP_RTOL, atol=0)
    np.testing.assert_allclose(pt[:-1].reshape(cols, rows), want.T, rtol=EXP_RTOL, atol=0)
    assert np.isnan(p[-1]) and np.isnan(pt[-1])


def _job(phi, theta, pot, pot_t, ex, strides, F):
    j = _lib().PotentialsJob()
    j.phi, j.theta = phi.data_ptr(), theta.data_ptr()
    j.pot = pot.data_ptr() if pot is not None else None
    j.pot_t = pot_t.data_ptr() if pot_t is not None else None
    j.expect = ex.data_ptr() if ex is not None else None
    j.theta_stride, j.pot_stride, j.pot_t_stride, j.expect_stride = strides
    j.rows, j.cols, j.F = phi.shape[0], phi.shape[1], F
    return j


def _multi(jobs, n_rep):
    arr = (_lib().PotentialsJob * len(jobs))(*jobs)
    _call('mlbp_potentials_multi_f64', arr, len(jobs), n_rep)


def test_potentials_multi_with_expectations():
    """mlbp_potentials_multi_f64, rows == 64 with expectations: F = 8 over 16 390 columns (the grid stops at 4096 blocks of
    four waves, so a wave takes a second column) and F = 1; two repetitions at their strides.  expect[j][k] =
    sum_i normalize(pot[:, j])[i] phi[i][j][k]; a column whose potentials are all 0 gives expectations of 0; slots k >= F are
    left alone."""
    rs = np.random.RandomState(8)
    n_rep = 2
    specs = [(16390, 8), (40, 1)]
    jobs, keep, want = [], [], []
    for cols, F in specs:
        phi = rs.rand(64, cols, F)
        theta = rs.rand(n_rep, F) * 2 - 0.5
        theta[:, 0] = [-1.0, -0.8]
        phi[:, 5, 0] = 1000.0                                           # column 5: exp(< -745) = 0 in every row
        tphi, ttheta = _up(phi), _up(theta)
        pot, pot_t = _full((n_rep, 64 * cols + 3), NAN), _full((n_rep, cols * 64 + 1), NAN)
        ex = _full((n_rep, cols * 8 + 2), NAN)
        jobs.append(_job(tphi, ttheta, pot if F == 8 else None, pot_t, ex, (F, 64 * cols + 3, cols * 64 + 1, cols * 8 + 2), F))
        keep.append((tphi, ttheta, pot, pot_t, ex))
        want.append((phi, theta))
    with _Launches('potentials_multi_kernel'):
        _multi(jobs, n_rep)
    for (cols, F), (phi, theta), (_, _, pot, pot_t, ex) in zip(specs, want, keep):
        for r in range(n_rep):
            v = _exp_dot(phi, theta[r])
            assert (v[:, 5] == 0).all()
            Z = v.sum(0)
            e = np.zeros((cols, 8))
            for k in range(F):
                e[:, k] = np.where(Z > 0, (v * phi[:, :, k]).sum(0) / np.where(Z > 0, Z, 1), 0.0)
            got = ex[r].cpu().numpy()
            g = got[:cols * 8].reshape(cols, 8)
            np.testing.assert_allclose(g[:, :F], e[:, :F], rtol=SUM_RTOL, atol=0, err_msg='F=%d rep %d' % (F, r))
            assert np.isnan(g[:, F:]).all() and np.isnan(got[cols * 8:]).all()
            pt = pot_t[r].cpu().numpy()
            np.testing.assert_allclose(pt[:-1].reshape(cols, 64), v.T, rtol=EXP_RTOL, atol=0)
            assert np.isnan(pt[-1])
            if F == 8:
                p = pot[r].cpu().numpy()
                np.testing.assert_allclose(p[:64 * cols].reshape(64, cols), v, rtol=EXP_RTOL, atol=0)
                assert np.isnan(p[64 * cols:]).all()
    bad = _job(keep[1][0], keep[1][1], None, keep[1][3], keep[1][4], (1, 0, 64 * 40 + 1, 8 * 40 + 2), 1)
    bad.rows = 63
    with pytest.raises(_lib().MlbpError):
        _multi([bad], 1)


def test_potentials_multi_general_path():
    """mlbp_potentials_multi_f64 without expectations: jobs of 37 and 64 rows, three repetitions at padded strides (the
    padding is left alone), exp overflow to inf as NumPy's; at most 8 features with expectations."""
    rs = np.random.RandomState(9)
    n_rep = 3
    specs = [(37, 50, 3), (64, 21, 6), (64, 3, 9)]
    jobs, keep = [], []
    for rows, cols, F in specs:
        phi = rs.rand(rows, cols, F)
        phi[1, 2, 0] = 900.0
        theta = rs.rand(n_rep, F + 2) - 0.25
        theta[:, 0] = 1.0
        n = rows * cols
        tphi, ttheta = _up(phi), _up(theta)
        pot, pot_t = _full((n_rep, n + 5), NAN), _full((n_rep, n + 2), NAN)
        jobs.append(_job(tphi, ttheta, pot, pot_t, None, (F + 2, n + 5, n + 2, 0), F))
        keep.append((phi, theta, tphi, ttheta, pot, pot_t))
    with _Launches('potentials_multi_kernel'):
        _multi(jobs, n_rep)
    for (rows, cols, F), (phi, theta, _, _, pot, pot_t) in zip(specs, keep):
        n = rows * cols
        for r in range(n_rep):
            v = _exp_dot(phi, theta[r, :F])
            assert np.isinf(v[1, 2])
            p, pt = pot[r].cpu().numpy(), pot_t[r].cpu().numpy()
            np.testing.assert_allclose(p[:n].reshape(rows, cols), v, rtol=EXP_RTOL, atol=0)
            np.testing.assert_allclose(pt[:n].reshape(cols, rows), v.T, rtol=EXP_RTOL, atol=0)
            assert np.isnan(p[n:]).all() and np.isnan(pt[n:]).all()
    ex = _full((3 * 8,), NAN)
    j = jobs[2]
    j.expect, j.expect_stride = ex.data_ptr(), 0
    with pytest.raises(_lib().MlbpError):
        _multi([j], 1)


def test_unary_expectations():
    """mlbp_unary_expectations_f64: E[row][f] = sum_x normalize(tables[row])[x] phi_t[obs][x][f] for the three row kinds
    (0: phi_en_en, 1: phi_en_en_w1, 2: phi_en_de); an all-zero row gives 0; slots f >= F are left alone."""
    rs = np.random.RandomState(10)
    n_rows, Vde, F_ee, F_ed = 11, 30, 3, 6
    tables = rs.rand(n_rows, 64)
    tables[4] = 0.0
    kind = np.array([0, 1, 2] * 4, np.int32)[:n_rows]
    obs = np.where(kind == 2, rs.randint(0, Vde, n_rows), rs.randint(0, 64, n_rows)).astype(np.int32)
    obs[2] = Vde - 1
    t_ee, t_w1, t_ed = rs.rand(64, 64, F_ee), rs.rand(64, 64, F_ee), rs.rand(Vde, 64, F_ed)
    out = _full((n_rows * 8 + 1,), NAN)
    _status()
    with _Launches('unary_expectations_kernel'):
        _call('mlbp_unary_expectations_f64', _up(tables), n_rows, 64, _up(kind), _up(obs), _up(t_ee), _up(t_w1), _up(t_ed),
              F_ee, F_ed, Vde, out)
    assert _status() == 0
    got = out.cpu().numpy()
    assert np.isnan(got[-1])
    got = got[:-1].reshape(n_rows, 8)
    for r in range(n_rows):
        ph = (t_ee, t_w1, t_ed)[kind[r]][obs[r]]
        F = F_ed if kind[r] == 2 else F_ee
        Z = tables[r].sum()
        want = (tables[r][:, None] * ph).sum(0) / Z if Z > 0 else np.zeros(F)
        np.testing.assert_allclose(got[r, :F], want, rtol=SUM_RTOL, atol=0, err_msg='row %d' % r)
        assert np.isnan(got[r, F:]).all()


def _patch_items(rs, n_rows, X, F):
    """CSR items (x, k, val) per row: row 1 has none, row 2 names one cell twice, cells 0 and X - 1 appear."""
    counts = [3, 0, 4, 1, 2, 5, 2, 3][:n_rows]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    n = int(off[-1])
    x = rs.randint(0, X, n).astype(np.int32)
    x[off[2]], x[off[2] + 1] = 7, 7
    x[0], x[-1] = 0, X - 1
    return off, x, rs.randint(0, F, n).astype(np.int32), rs.rand(n) * 2 - 0.5


@pytest.mark.parametrize('X', [64, 100])
def test_patch_tables(X):
    """mlbp_patch_unary_tables_f64: out[r][x] = base[base_row[r]][x] exp(sum of theta[k] val over the row's items at x); a row
    without items is its base row."""
    rs = np.random.RandomState(X)
    n_rows, F = 8, 5
    base = rs.rand(4, X)
    base_row = rs.randint(0, 4, n_rows).astype(np.int32)
    off, ix, ik, iv = _patch_items(rs, n_rows, X, F)
    theta = rs.randn(F)
    out = _full((n_rows * X + 1,), NAN)
    with _Launches('patch_tables_kernel'):
        _call('mlbp_patch_unary_tables_f64', _up(base), _up(base_row), _up(off), _up(ix), _up(ik), _up(iv), _up(theta),
              n_rows, X, out)
    got = out.cpu().numpy()
    assert np.isnan(got[-1])
    for r in range(n_rows):
        e = np.zeros(X)
        for q in range(off[r], off[r + 1]):
            e[ix[q]] += theta[ik[q]] * iv[q]
        np.testing.assert_allclose(got[r * X:(r + 1) * X], base[base_row[r]] * np.exp(e), rtol=EXP_RTOL, atol=0, err_msg='row %d' % r)
    np.testing.assert_array_equal(got[X:2 * X], base[base_row[1]])


@pytest.mark.parametrize('X', [64, 100])
def test_patch_gradient(X):
    """mlbp_patch_gradient_f64: grad[graph][k] += val ([x == label] - t[x] / sum t) over the items of every row; graph 0's rows
    form two separate runs (the atomic path), an all-zero row has beliefs 0, a row without items adds nothing.  The graphs
    whose rows are one run are added to in row order: the same bits on every call."""
    rs = np.random.RandomState(X + 1)
    n_rows, F = 8, 6
    row_graph = np.array([0, 0, 1, 1, 0, 2, 2, 2], np.int32)
    priv = rs.rand(n_rows, X)
    priv[3] = 0.0
    off, ix, ik, iv = _patch_items(rs, n_rows, X, F)
    label = rs.randint(0, X, n_rows).astype(np.int32)
    label[0] = ix[0]
    g0 = rs.rand(3, F) + 10.0
    want = g0.copy()
    for r in range(n_rows):
        Z = priv[r].sum()
        for q in range(off[r], off[r + 1]):
            belief = priv[r, ix[q]] / Z if Z > 0 else 0.0
            want[row_graph[r], ik[q]] += iv[q] * ((1.0 if ix[q] == label[r] else 0.0) - belief)
    args = [_up(priv), _up(off), _up(ix), _up(ik), _up(iv), _up(row_graph), _up(label), n_rows, X, F]
    got = []
    for _ in range(2):
        grad = _up(np.concatenate([g0.reshape(-1), [NAN]]))
        with _Launches('patch_gradient_kernel'):
            _call('mlbp_patch_gradient_f64', *args, grad)
        got.append(grad.cpu().numpy())
    assert np.isnan(got[0][-1])
    np.testing.assert_allclose(got[0][:-1].reshape(3, F), want, rtol=SUM_RTOL, atol=0)
    assert got[0][F:3 * F].tobytes() == got[1][F:3 * F].tobytes()


# ---- log-posteriors --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 333])
def test_log_posterior(B):
    """mlbp_log_posterior_sum_f64 / mlbp_log_posterior_f64: per graph sum_v log marg[b][v][label] (log 0 -> -99.99) and the
    batch sum; out[B] is left alone."""
    rs = np.random.RandomState(B)
    n_vars, X = 3, 7
    marg = rs.rand(B, n_vars, X) * 0.9 + 0.05
    labels = rs.randint(0, X, size=(B, n_vars)).astype(np.int32)
    marg[B - 1, 1, labels[B - 1, 1]] = 0.0
    want = _lp_reference(marg, labels, X)
    tm, tl = _up(marg), _up(labels)
    out, s = _full((B + 1,), NAN), _full((2,), NAN)
    with _Launches('log_posterior_kernel'):
        _call('mlbp_log_posterior_sum_f64', tm, tl, B, n_vars, X, out, s)
    got = out.cpu().numpy()
    np.testing.assert_allclose(got[:B], want, rtol=EXP_RTOL, atol=0)
    assert np.isnan(got[B]) and np.isnan(s[1].item())
    np.testing.assert_allclose(s[0].item(), want.sum(), rtol=SUM_RTOL)
    out2 = _full((B + 1,), NAN)
    with _Launches('log_posterior_kernel'):
        _call('mlbp_log_posterior_f64', tm, tl, B, n_vars, X, out2)
    assert torch.equal(out2[:B], out[:B])


def test_log_posterior_batch_limit_and_alternating_counters():
    """B = 4096 * 256, the most graphs with sum_out: calls with and without sum_out alternated (the launches with it take the two
    arrival counters in turn) give correct sums, the same bits every time.  One graph more is refused with sum_out and
    computed without it."""
    B = 4096 * 256
    n_vars, X = 2, 2
    rs = np.random.RandomState(12)
    marg = rs.rand(B + 1, n_vars, X) * 0.9 + 0.05
    labels = rs.randint(0, X, size=(B + 1, n_vars)).astype(np.int32)
    marg[B // 2, 0, labels[B // 2, 0]] = 0.0
    want = _lp_reference(marg, labels, X)
    tm, tl = _up(marg), _up(labels)
    sums = []
    for with_sum in (True, False, True, True, False, True):
        out, s = _full((B,), NAN), _full((1,), NAN)
        with _Launches('log_posterior_kernel'):
            _call('mlbp_log_posterior_sum_f64', tm, tl, B, n_vars, X, out, s if with_sum else None)
        if with_sum:
            sums.append(s.item())
        else:
            assert np.isnan(s.item())
        np.testing.assert_allclose(out.cpu().numpy(), want[:B], rtol=EXP_RTOL, atol=0)
    assert all(np.float64(s).tobytes() == np.float64(sums[0]).tobytes() for s in sums), sums
    np.testing.assert_allclose(sums[0], want[:B].sum(), rtol=SUM_RTOL)
    s = _full((1,), NAN)
    _refused(EUNSUPPORTED, 'mlbp_log_posterior_sum_f64', tm, tl, B + 1, n_vars, X, _full((B + 1,), NAN), s)
    out = _full((B + 1,), NAN)
    with _Launches('log_posterior_kernel'):
        _call('mlbp_log_posterior_sum_f64', tm, tl, B + 1, n_vars, X, out, None)
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=EXP_RTOL, atol=0)


_GROUP = np.dtype([('marginals', '<u8'), ('labels', '<u8'), ('n_vars', '<i4'), ('B', '<i4'), ('start', '<i8')])


@pytest.mark.parametrize('n_groups', [1, 2, 41])
def test_log_posterior_groups(n_groups):
    """mlbp_log_posterior_groups_f64: each group's log-posteriors at out[start ..]; groups of different variable counts,
    gaps between them and after the last (prefilled with a sentinel: left alone), enough groups that the search for a
    thread's group ends at both ends of the table."""
    rs = np.random.RandomState(n_groups)
    X = 6
    table = np.zeros(n_groups, _GROUP)
    keep, want = [], {}
    start = 0
    for k in range(n_groups):
        B = int(rs.randint(1, 70)) if n_groups > 1 else 300
        nv = int(rs.randint(1, 10))
        marg = rs.rand(B, nv, X) * 0.9 + 0.05
        labels = rs.randint(0, X, size=(B, nv)).astype(np.int32)
        marg[B - 1, nv - 1, labels[B - 1, nv - 1]] = 0.0
        tm, tl = _up(marg), _up(labels)
        keep += [tm, tl]
        table[k] = (tm.data_ptr(), tl.data_ptr(), nv, B, start)
        want[start] = _lp_reference(marg, labels, X)
        start += B + (int(rs.randint(0, 4)) if k % 3 else 0)
    n_total = start + 5
    sentinel = 12345.5
    out = _full((n_total + 1,), sentinel)
    tg = _up(np.frombuffer(table.tobytes(), np.uint8).copy())
    with _Launches('log_posterior_groups_kernel'):
        _call('mlbp_log_posterior_groups_f64', tg, n_groups, n_total, X, out)
    got = out.cpu().numpy()
    written = np.zeros(n_total + 1, bool)
    for s, w in want.items():
        np.testing.assert_allclose(got[s:s + len(w)], w, rtol=EXP_RTOL, atol=0, err_msg='group at %d' % s)
        written[s:s + len(w)] = True
    assert (got[~written] == sentinel).all(), 'a gap row was written'
    assert (~written).sum() >= 6


# ---- top-k -----------------------------------------------------------------------------------------------------------
def _topk(v, K, stride=1):
    """mlbp_topk_f64 on the device tensor v (elements `stride` apart) into a sentinel-prefilled index array."""
    idx = _full((K + 1,), -7, torch.int32)
    n = (v.numel() + stride - 1) // stride
    with _Launches('topk_kernel'):
        _call('mlbp_topk_f64', v, stride, n, K, idx)
    got = idx.cpu().numpy()
    assert got[K] == -7, 'written past K'
    return got[:K]


@pytest.mark.parametrize('n,K', [(1, 1), (300, 1), (300, 300), (8192, 100), (8193, 100), (16384, 100), (16384, 16384)])
def test_topk(n, K):
    """mlbp_topk_f64: the indices of the K largest in descending order, ties to the lower index -- exactly
    np.lexsort((arange, -v))[:K] -- on values with many ties; n = 8192 fits the default 64 KiB of LDS, larger n is granted
    more, 16384 is the limit.  An all-equal vector gives 0 .. K-1."""
    rs = np.random.RandomState(n + K)
    v = rs.randint(0, 50, n).astype(np.float64) + rs.choice([0.0, 0.5], n)
    np.testing.assert_array_equal(_topk(_up(v), K), _lexsort_topk(v, K))
    np.testing.assert_array_equal(_topk(_up(np.full(n, 0.25)), K), np.arange(K))


def test_topk_strided():
    """A strided vector (every third element of a larger one)."""
    rs = np.random.RandomState(13)
    big = rs.randn(3 * 1000)
    v = big[::3]
    np.testing.assert_array_equal(_topk(_up(big), 100, stride=3), _lexsort_topk(v, 100))
    assert set(_topk(_up(big), 100, stride=3)) == set(AO._topk_desc(v))


def test_topk_limits():
    """n = 16385 is refused (EUNSUPPORTED) by both entries, K > n with NumPy's error (EINVAL); nothing is written."""
    v = _up(np.zeros(16385))
    idx = _full((101,), -7, torch.int32)
    _refused(EUNSUPPORTED, 'mlbp_topk_f64', v, 1, 16385, 100, idx)
    _refused(EUNSUPPORTED, 'mlbp_topk_rows_f64', v, 1, 16385, 100, idx)
    _refused(EINVAL, 'mlbp_topk_f64', v, 1, 50, 51, idx)
    _refused(EINVAL, 'mlbp_topk_rows_f64', v, 1, 50, 51, idx)
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == -7).all()
    np.testing.assert_array_equal(_topk(_up(np.arange(16384.0)), 3), [16383, 16382, 16381])


@pytest.mark.parametrize('n', [300, 8193])
def test_topk_rows(n):
    """mlbp_topk_rows_f64: one selection per row of a [rows][n] matrix, row 2 all equal."""
    rs = np.random.RandomState(n)
    rows, K = 5, 100
    v = rs.randint(0, 40, (rows, n)).astype(np.float64)
    v[2] = 3.0
    idx = _full((rows * K + 1,), -7, torch.int32)
    with _Launches('topk_kernel'):
        _call('mlbp_topk_rows_f64', _up(v), rows, n, K, idx)
    got = idx.cpu().numpy()
    assert got[-1] == -7
    for r in range(rows):
        np.testing.assert_array_equal(got[r * K:(r + 1) * K], _lexsort_topk(v[r], K), err_msg='row %d' % r)


def _nan_vectors():
    """name -> (vector, K).  With one NaN and K = 100 the old rank rule gave the NaN rank 0 beside the largest number (which of
    the two landed in idx[0] was a race); with fewer numbers than K it left the last slots unwritten."""
    rs = np.random.RandomState(14)
    one = rs.randn(200)
    one[17] = NAN                                                      # one NaN, 199 numbers >= K
    many = rs.randn(200)
    many[rs.choice(200, 150, replace=False)] = NAN                     # 50 numbers < K = 100
    return {'one_nan': (one, 100), 'one_nan_k_is_n': (one, 200), 'fewer_numbers_than_k': (many, 100),
            'all_nan': (np.full(200, NAN), 100)}


def _check_nan_selection(name, v, got, K):
    assert ((got >= 0) & (got < v.size)).all(), '%s: index out of range (or never written): %s' % (name, got)
    assert len(set(got)) == K, '%s: repeated indices' % name
    np.testing.assert_array_equal(got, _lexsort_topk(v, K), err_msg=name)
    numbers = np.flatnonzero(~np.isnan(v))
    if numbers.size >= K == AO.TOP_K:
        assert set(got) == set(AO._topk_desc(v)), name               # the reference's selection: NaN last
    elif numbers.size >= K:
        assert set(got) <= set(numbers), name
    else:
        assert set(numbers) <= set(got), name


@pytest.mark.parametrize('name', ['one_nan', 'one_nan_k_is_n', 'fewer_numbers_than_k', 'all_nan'])
def test_topk_nan(name):
    """NaN ranks below every number and NaNs tie among themselves: the K indices are distinct, in range, the numbers first
    (the reference's np.argpartition(-v) selection), then NaNs by index."""
    v, K = _nan_vectors()[name]
    _check_nan_selection(name, v, _topk(_up(v), K), K)


def test_topk_rows_nan():
    """The same NaN rule for every row of mlbp_topk_rows_f64."""
    vs = _nan_vectors()
    names = ['all_nan', 'fewer_numbers_than_k', 'one_nan']
    v = np.stack([vs[k][0] for k in names])
    K = 100
    idx = _full((len(names) * K + 1,), -7, torch.int32)
    with _Launches('topk_kernel'):
        _call('mlbp_topk_rows_f64', _up(v), len(names), v.shape[1], K, idx)
    got = idx.cpu().numpy()
    assert got[-1] == -7
    for r, name in enumerate(names):
        _check_nan_selection(name, v[r], got[r * K:(r + 1) * K], K)


@pytest.fixture(scope='module')
def au():
    from macaronicusermodeling_amd.array_utils import c_array_utils
    return c_array_utils


def test_sparse_products_with_nan_entries(au):
    """au.sparse_vec_mat_dot and au.sparse_dot on vectors with a few NaNs (and at least K numbers) select the K largest numbers,
    as oracle/array_oracle.py: the NaNs do not enter the products."""
    rs = np.random.RandomState(15)
    X = 200
    vec = rs.rand(X) + 0.1
    vec[[3, 50, 199]] = NAN
    mat = rs.rand(X, X) + 0.1
    with _Launches('topk_kernel', 'gather_dot_kernel'):
        row = np.asarray(au.sparse_vec_mat_dot(vec.reshape(1, X), mat))
        col = np.asarray(au.sparse_vec_mat_dot(vec.reshape(X, 1), mat))
    np.testing.assert_allclose(row, AO.sparse_vec_mat_dot(vec.reshape(1, X), mat), rtol=SUM_RTOL, atol=0)
    np.testing.assert_allclose(col, AO.sparse_vec_mat_dot(vec.reshape(X, 1), mat), rtol=SUM_RTOL, atol=0)
    r = rs.rand(X) + 0.1
    r[[0, 120]] = NAN
    with _Launches('topk_kernel', 'block_op_kernel'):
        out, i1, i2 = au.sparse_dot(vec.reshape(X, 1), r.reshape(1, X))
    want, w1, w2 = AO.sparse_dot(vec.reshape(X, 1), r.reshape(1, X))
    assert set(np.asarray(i1).tolist()) == set(w1.tolist()) and set(np.asarray(i2).tolist()) == set(w2.tolist())
    np.testing.assert_array_equal(np.asarray(out), want)


# ---- messages, marginals, beliefs ------------------------------------------------------------------------------------
def test_init_messages():
    """mlbp_init_messages_f64: every message 1/X, X = 4096 (more than a workgroup); nothing past the rows."""
    rows, X = 3, 4096
    m = _full((rows * X + 1,), NAN)
    with _Launches('fill_kernel'):
        _call('mlbp_init_messages_f64', m, rows, X)
    got = m.cpu().numpy()
    assert (got[:-1] == 1.0 / X).all() and np.isnan(got[-1])


@pytest.mark.parametrize('X', [4096, 100])
@pytest.mark.parametrize('normalize', [0, 1])
def test_marginals(X, normalize):
    """mlbp_marginals_f64 (LBP.py:392-400): marginal = (1/X) times the incoming messages in order (nan_to_num after every
    product), normalised (a zero total -> uniform) or not.  Variable 1 has no incoming message (uniform), variable 2's product
    is all zero."""
    rs = np.random.RandomState(X + normalize)
    B, n_msgs, n_vars = 3, 5, 4
    msgs = rs.rand(B, n_msgs, X) + 0.05
    msgs[:, 4] = 0.0
    in_off = np.array([0, 2, 2, 5, 6], np.int32)
    in_slots = np.array([0, 3, 1, 4, 2, 3], np.int32)
    out = _full((B * n_vars * X + 1,), NAN)
    with _Launches('marginals_kernel'):
        _call('mlbp_marginals_f64', _up(msgs), B, n_msgs, X, n_vars, _up(in_off), _up(in_slots), normalize, out)
    got = out.cpu().numpy()
    assert np.isnan(got[-1])
    got = got[:-1].reshape(B, n_vars, X)
    for b in range(B):
        for v in range(n_vars):
            acc = np.full(X, 1.0 / X)
            for q in range(in_off[v], in_off[v + 1]):
                acc = np.nan_to_num(msgs[b, in_slots[q]] * acc)
            if normalize:
                t = acc.sum()
                acc = acc / t if t > 0 else np.full(X, 1.0 / X)
            np.testing.assert_allclose(got[b, v], acc, rtol=SUM_RTOL if normalize else EXP_RTOL, atol=0,
                                       err_msg='graph %d variable %d' % (b, v))
    np.testing.assert_allclose(got[:, 1], 1.0 / X, rtol=EXP_RTOL, atol=0)       # no message: uniform
    assert (got[:, 2] == (1.0 / X if normalize else 0.0)).all()                 # zero product: uniform, or zeros


@pytest.mark.parametrize('X', [64, 100])
def test_pair_beliefs(X):
    """mlbp_pair_beliefs_f64 (LBP.py:543-569): out[b][p] = normalise((c r^T) * T); an all-zero table gives zero beliefs."""
    rs = np.random.RandomState(X + 2)
    B, n_msgs, P, n_tab = 3, 4, 2, 3
    msgs = rs.rand(B, n_msgs, X) + 0.05
    tables = rs.rand(n_tab, X, X)
    tables[2] = 0.0
    pair_tab = np.array([[0, 1], [2, 0], [1, 1]], np.int32)
    c_slot, r_slot = np.array([0, 2], np.int32), np.array([1, 3], np.int32)
    out = _full((B * P * X * X + 1,), NAN)
    _status()
    with _Launches('pair_beliefs_kernel'):
        _call('mlbp_pair_beliefs_f64', _up(msgs), B, n_msgs, X, P, _up(tables), _up(pair_tab), n_tab, _up(c_slot), _up(r_slot), out)
    assert _status() == 0
    got = out.cpu().numpy()
    assert np.isnan(got[-1])
    got = got[:-1].reshape(B, P, X, X)
    for b in range(B):
        for p in range(P):
            w = np.outer(msgs[b, c_slot[p]], msgs[b, r_slot[p]]) * tables[pair_tab[b, p]]
            Z = w.sum()
            want = w / Z if Z > 0 else np.zeros_like(w)
            np.testing.assert_allclose(got[b, p], want, rtol=SUM_RTOL, atol=0, err_msg='graph %d factor %d' % (b, p))
    assert (got[1, 0] == 0).all()


# ---- au.* primitives -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,Kd,N', [(5, 1, 7), (4, 31, 3), (3, 32, 9), (6, 65, 5)])
def test_dense_dot(M, Kd, N):
    """mlbp_dense_dot_f64: C[b] = A[b] B[b] with A transposed (column stride 1 along the rows), B every other column, C with
    padded rows; K < 32 takes the thin kernel, K >= 32 the wave-per-output one."""
    rs = np.random.RandomState(M * Kd * N)
    batch = 2
    At = rs.rand(batch, Kd, M)                  # A[b] = At[b].T: row stride 1, column stride M
    Bw = rs.rand(batch, Kd, 2 * N)              # B[b] = Bw[b][:, ::2]: row stride 2N, column stride 2
    cr = N + 3
    out = _full((batch * M * cr + 1,), NAN)
    kern = 'dense_dot_thin_kernel' if Kd < 32 else 'dense_dot_kernel'
    other = 'dense_dot_kernel' if Kd < 32 else 'dense_dot_thin_kernel'
    with _Launches(kern, absent=[other]):
        _call('mlbp_dense_dot_f64', batch, M, Kd, N, _up(At), Kd * M, 1, M, _up(Bw), Kd * 2 * N, 2 * N, 2, out, M * cr, cr)
    got = out.cpu().numpy()
    assert np.isnan(got[-1])
    got = got[:-1].reshape(batch, M, cr)
    for b in range(batch):
        np.testing.assert_allclose(got[b, :, :N], At[b].T.dot(Bw[b][:, ::2]), rtol=SUM_RTOL, atol=0)
        assert np.isnan(got[b, :, N:]).all()


def test_pointwise_multiply():
    """mlbp_pointwise_multiply_f64: a * b exactly; with nan_to_num NaN -> 0, +inf -> DBL_MAX, -inf -> -DBL_MAX."""
    rs = np.random.RandomState(16)
    a, b = rs.randn(1000), rs.randn(1000)
    a[:6] = [NAN, np.inf, -np.inf, 1e300, -1e300, 0.0]
    b[:6] = [1.0, 2.0, 3.0, 1e10, 1e10, np.inf]
    ta, tb = _up(a), _up(b)
    with np.errstate(invalid='ignore', over='ignore'):
        raw = a * b
    for flag, want in ((0, raw), (1, np.nan_to_num(raw))):
        out = _full((1001,), 7.0)
        with _Launches('pointwise_multiply_kernel'):
            _call('mlbp_pointwise_multiply_f64', ta, tb, out, 1000, flag)
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[:-1], want)
        assert got[-1] == 7.0
    assert np.nan_to_num(raw)[1] == DBL_MAX and np.nan_to_num(raw)[2] == -DBL_MAX


@pytest.mark.parametrize('mode', [0, 1])
def test_normalize(mode):
    """mlbp_normalize_f64: x / total where the total is > 0; otherwise zeros (mode 0) or 1/n (mode 1), positive[b] saying
    which; vectors with a positive, zero, negative and mixed-sign positive total; in place as well."""
    rs = np.random.RandomState(17)
    n = 300
    v = np.stack([rs.rand(n) + 0.1, np.zeros(n), -(rs.rand(n) + 0.1), rs.rand(n) + 0.1])
    v[3, :5] = -0.05
    v[1, 7] = 0.0
    want_pos = np.array([1, 0, 0, 1], np.int32)
    fill = 0.0 if mode == 0 else 1.0 / n
    want = np.stack([v[b] / v[b].sum() if want_pos[b] else np.full(n, fill) for b in range(4)])
    tv = _up(v)
    out, pos = _full((4 * n + 1,), NAN), _full((5,), -3, torch.int32)
    with _Launches('normalize_kernel'):
        _call('mlbp_normalize_f64', tv, out, 4, n, mode, pos)
    got = out.cpu().numpy()
    np.testing.assert_allclose(got[:-1].reshape(4, n), want, rtol=SUM_RTOL, atol=0)
    assert np.isnan(got[-1])
    np.testing.assert_array_equal(pos.cpu().numpy(), list(want_pos) + [-3])
    with _Launches('normalize_kernel'):
        _call('mlbp_normalize_f64', tv, tv, 4, n, mode, None)
    assert torch.equal(tv, out[:-1].view(4, n))


@pytest.mark.parametrize('vec_is_row', [0, 1])
def test_sparse_vec_mat_dot(vec_is_row):
    """mlbp_sparse_vec_mat_dot_f64 on given indices: out_i = sum_q mat[i][idx_q] vec[idx_q] (column vector) or out_j =
    sum_q vec[idx_q] mat[idx_q][j] (row vector), a strided vector and a transposed matrix."""
    rs = np.random.RandomState(18 + vec_is_row)
    n, n_out, Kq = 150, 70, 37
    vbig = rs.rand(2 * n) + 0.1
    vec = vbig[::2]
    idx = rs.choice(n, Kq, replace=False).astype(np.int32)
    idx[0], idx[1] = 0, n - 1
    if vec_is_row:           # mat [n][n_out] = mt.T: element (k, j) at j * n + k
        mt = rs.rand(n_out, n) + 0.1
        strides, want = (1, n), sum(vec[k] * mt.T[k] for k in idx)
    else:                    # mat [n_out][n] = mt.T: element (i, k) at k * n_out + i
        mt = rs.rand(n, n_out) + 0.1
        strides, want = (1, n_out), sum(mt.T[:, k] * vec[k] for k in idx)
    out = _full((n_out + 1,), NAN)
    with _Launches('gather_dot_kernel'):
        _call('mlbp_sparse_vec_mat_dot_f64', _up(vbig), 2, _up(mt), strides[0], strides[1], n_out, _up(idx), Kq, vec_is_row, out)
    got = out.cpu().numpy()
    np.testing.assert_allclose(got[:-1], want, rtol=SUM_RTOL, atol=0)
    assert np.isnan(got[-1])


def test_sparse_block_ops():
    """mlbp_sparse_dot_f64 (zeros, block c[i] r[j]), mlbp_sparse_pointwise_multiply_f64 (zeros, block a * b) on a
    non-square matrix with Kc != Kr, and mlbp_sparse_normalize_f64 (block / its sum in place, the rest untouched)."""
    rs = np.random.RandomState(19)
    n = 12
    c, r = rs.rand(n), rs.rand(n)
    ci = np.array([0, 5, 11, 3], np.int32)
    ri = np.array([11, 2, 0, 7], np.int32)
    out = _full((n * n,), NAN)
    with _Launches('zero_kernel', 'block_op_kernel'):
        _call('mlbp_sparse_dot_f64', _up(c), _up(r), n, _up(ci), _up(ri), 4, out)
    want = np.zeros((n, n))
    want[np.ix_(ci, ri)] = np.outer(c[ci], r[ri])
    np.testing.assert_array_equal(out.cpu().numpy().reshape(n, n), want)

    rows, cols = 7, 11
    a, b = rs.rand(rows, cols), rs.rand(rows, cols)
    ci, ri = np.array([6, 0, 3], np.int32), np.array([10, 0, 4, 5, 9], np.int32)
    out = _full((rows * cols,), NAN)
    with _Launches('zero_kernel', 'block_op_kernel'):
        _call('mlbp_sparse_pointwise_multiply_f64', _up(a), _up(b), rows, cols, _up(ci), 3, _up(ri), 5, out)
    want = np.zeros((rows, cols))
    want[np.ix_(ci, ri)] = a[np.ix_(ci, ri)] * b[np.ix_(ci, ri)]
    np.testing.assert_array_equal(out.cpu().numpy().reshape(rows, cols), want)

    m = _up(a)
    scratch = _full((2,), NAN)
    with _Launches('block_sum_kernel', 'block_op_kernel'):
        _call('mlbp_sparse_normalize_f64', m, cols, _up(ci), 3, _up(ri), 5, scratch)
    want = a.copy()
    want[np.ix_(ci, ri)] /= a[np.ix_(ci, ri)].sum()
    np.testing.assert_allclose(m.cpu().numpy(), want, rtol=SUM_RTOL, atol=0)
    got = m.cpu().numpy()
    mask = np.ones((rows, cols), bool)
    mask[np.ix_(ci, ri)] = False
    np.testing.assert_array_equal(got[mask], a[mask])
    np.testing.assert_allclose(scratch[0].item(), a[np.ix_(ci, ri)].sum(), rtol=SUM_RTOL)


def test_log():
    """mlbp_log_f64 == np.log, log 0 = -inf, on values over many magnitudes."""
    rs = np.random.RandomState(20)
    x = np.exp(rs.uniform(-700, 700, 1003))
    x[:4] = [0.0, 1.0, 5e-324, DBL_MAX]
    out = _full((1004,), NAN)
    with _Launches('log_kernel'):
        _call('mlbp_log_f64', _up(x), out, 1003)
    got = out.cpu().numpy()
    with np.errstate(divide='ignore'):
        np.testing.assert_allclose(got[:-1], np.log(x), rtol=EXP_RTOL, atol=0)
    assert got[0] == -np.inf and got[1] == 0.0 and np.isnan(got[-1])


@pytest.mark.parametrize('cell', [0, 49])
def test_observed_minus(cell):
    """mlbp_observed_minus_f64 (LBP.py:615-619): onehot(cell) - beliefs, the cell first or last; a cell out of range is refused."""
    rs = np.random.RandomState(21 + cell)
    b = rs.rand(50)
    want = -b
    want[cell] = 1.0 - b[cell]
    out = _full((51,), NAN)
    tb = _up(b)
    with _Launches('observed_minus_kernel'):
        _call('mlbp_observed_minus_f64', tb, 50, cell, out)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:-1], want)
    assert np.isnan(got[-1])
    _refused(EINVAL, 'mlbp_observed_minus_f64', tb, 50, 50, out)
