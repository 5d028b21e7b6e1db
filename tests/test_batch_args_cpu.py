"""The argument helpers of batch.py and the per-shape loop of train.py, without a GPU: CPU tensors stand in for device tensors,
torch.device('meta') for "another device", plain objects for the per-shape trainers.

The messages are spelled out as the methods raised them before the helpers existed: a caller that matches on them must not
notice the fold.  tests/test_gpu_batch_args.py checks that every public method hands its own words to the helper."""
import collections

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from macaronicusermodeling_amd import _ffi                                     # noqa: E402
from macaronicusermodeling_amd import batch as BT                              # noqa: E402
from macaronicusermodeling_amd import train as TR                              # noqa: E402

CPU = torch.device('cpu')
F64, I32 = torch.float64, torch.int32
B, NV, X, S, N, NCUT, P, FEE, FED = 2, 3, 4, 5, 6, 1, 3, 3, 6

# (call site, what, shape, dtype, shape_text, message=, the full text the site raised before the fold)
SITES = [
    ('map_sweep', 'max_marginals', (B, NV, X), F64, None, 'max_marginals must be float64 [B][n_vars][X]',
     'max_marginals must be float64 [B][n_vars][X]'),
    ('log_partition', 'score', B, F64, None, 'score must be a float64 device tensor of B elements',
     'score must be a float64 device tensor of B elements'),
    ('log_partition', 'sum_out', 2, F64, None, 'sum_out must be a float64 device tensor of two elements',
     'sum_out must be a float64 device tensor of two elements'),
    ('sample', 'uniforms', (S, B, NV), F64, '[n_samples][B][n_vars]', None,
     'uniforms must be a contiguous float64 device tensor [n_samples][B][n_vars]'),
    ('sample', 'cond_marginals', (S, B, NV, X), F64, '[n_samples][B][n_vars][X]', None,
     'cond_marginals must be a contiguous float64 device tensor [n_samples][B][n_vars][X]'),
    ('converge', 'marginals', (B, NV, X), F64, '[B][n_vars][X]', None,
     'marginals must be a contiguous float64 device tensor [B][n_vars][X]'),
    ('exact_inference', 'marginals', (B, NV, X), F64, '[B][n_vars][X]', None,
     'marginals must be a contiguous float64 device tensor [B][n_vars][X]'),
    ('cutset_proposal', 'uniforms', (N, B, NV), F64, '[n_samples][B][n_vars]', None,
     'uniforms must be a contiguous float64 device tensor [n_samples][B][n_vars]'),
    ('cutset_draw', 'uniforms', (B, N, NCUT), F64, '[B][n_samples][n_cut]', None,
     'uniforms must be a contiguous float64 device tensor [B][n_samples][n_cut]'),
    ('cutset_logq', 'configs', (B, N, NCUT), I32, '[B][N][n_cut]', None,
     'configs must be a contiguous int32 device tensor [B][N][n_cut]'),
    ('cutset_estimate', 'log_q', (B, None), F64, '[B][N]', None,
     'log_q must be a contiguous float64 device tensor [B][N]'),
    ('cutset_estimate', 'configs', (B, N, NCUT), I32, '[B][N][n_cut]', None,
     'configs must be a contiguous int32 device tensor [B][N][n_cut]'),
    ('cutset_estimate', 'marginals', (B, NV, X), F64, '[B][n_vars][X]', None,
     'marginals must be a contiguous float64 device tensor [B][n_vars][X]'),
    ('exact_map', 'max_marginals', (B, NV, X), F64, None, 'max_marginals must be True or a contiguous float64 device tensor [B][n_vars][X]',
     'max_marginals must be True or a contiguous float64 device tensor [B][n_vars][X]'),
    ('cutset_map', 'configs', (B, None, NCUT), I32, '[B][N][n_cut]', None,
     'configs must be a contiguous int32 device tensor [B][N][n_cut]'),
    ('exact_sample', 'uniforms', (S, B, NV), F64, '[n_samples][B][n_vars]', None,
     'uniforms must be a contiguous float64 device tensor [n_samples][B][n_vars]'),
    # _exactgrad prints the sizes themselves
    ('exact_gradient', 'marginals', (B, NV, X), F64, [B, NV, X], None, 'marginals must be a contiguous float64 device tensor [2, 3, 4]'),
    ('exact_gradient', 'pair_marginals', (B, P, X, X), F64, [B, P, X, X], None,
     'pair_marginals must be a contiguous float64 device tensor [2, 3, 4, 4]'),
    ('exact_gradient', 'out_ee', (B, FEE), F64, [B, FEE], None, 'out_ee must be a contiguous float64 device tensor [2, 3]'),
    ('exact_gradient', 'out_ed', (B, FED), F64, [B, FED], None, 'out_ed must be a contiguous float64 device tensor [2, 6]'),
]


def _concrete(shape):
    """A shape the site accepts: N for an open axis, the least count for an element count."""
    return (shape,) if isinstance(shape, int) else tuple(N if s is None else s for s in shape)


def _bad(shape, dtype):
    """name -> argument the site must refuse.  The exact shapes take the four tensors of the issue; an element count is a lower
    bound in any shape, so its wrong shapes are one element short and a strided view."""
    good = _concrete(shape)
    other = torch.int64 if dtype == F64 else torch.float64
    bad = {'numpy': np.zeros(good), 'dtype': torch.zeros(good, dtype=other), 'device': torch.zeros(good, dtype=dtype, device='meta')}
    if isinstance(shape, int):
        bad['short'] = torch.zeros(shape - 1, dtype=dtype)
        bad['strided'] = torch.zeros(2 * shape, dtype=dtype)[::2]
    else:
        bad['row_too_many'] = torch.zeros((good[0] + 1,) + good[1:], dtype=dtype)
        bad['permuted'] = torch.zeros(good[::-1], dtype=dtype).permute(*range(len(good))[::-1])
        assert tuple(bad['permuted'].shape) == good and not bad['permuted'].is_contiguous()
    return bad


@pytest.mark.parametrize('site', SITES, ids=['%s-%s' % s[:2] for s in SITES])
def test_device_tensor_accepts_the_good_and_words_every_refusal_as_before(site):
    _, what, shape, dtype, shape_text, message, text = site
    good = torch.zeros(_concrete(shape), dtype=dtype)
    assert BT._device_tensor(good, shape, dtype, CPU, what, shape_text, message=message) == good.data_ptr()
    for name, t in _bad(shape, dtype).items():
        with pytest.raises(ValueError) as e:
            BT._device_tensor(t, shape, dtype, CPU, what, shape_text, message=message)
        assert str(e.value) == text, (name, str(e.value))


def test_device_tensor_open_axis_and_element_count():
    """None admits any size on its axis and nothing else; an int is a least element count in any shape."""
    for n in (1, 7):
        BT._device_tensor(torch.zeros(B, n, dtype=F64), (B, None), F64, CPU, 'log_q', '[B][N]')
    for shape in ((B,), (B, 1, 1), (B + 1, N)):
        with pytest.raises(ValueError):
            BT._device_tensor(torch.zeros(shape, dtype=F64), (B, None), F64, CPU, 'log_q', '[B][N]')
    BT._device_tensor(torch.zeros(3, 2, dtype=F64), 5, F64, CPU, 'score', message='m')
    with pytest.raises(ValueError, match='^m$'):
        BT._device_tensor(torch.zeros(2, 2, dtype=F64), 5, F64, CPU, 'score', message='m')


def test_rows_i32():
    want = np.arange(B * NV).reshape(B, NV)
    for rows in (want.tolist(), want.astype(np.int64), torch.from_numpy(want.astype(np.int64)),
                 torch.from_numpy(want.astype(np.int64)).t().contiguous().t()):
        out = BT._rows_i32(rows, (B, NV), CPU, 'labels')
        assert out.dtype == I32 and out.device == CPU and out.is_contiguous() and (out.numpy() == want).all()
    same = torch.from_numpy(want.astype(np.int32))
    assert BT._rows_i32(same, (B, NV), CPU, 'labels') is same
    for what in ('labels', 'given'):
        with pytest.raises(ValueError) as e:
            BT._rows_i32(np.zeros((B, NV + 1), dtype=np.int64), (B, NV), CPU, what)
        assert str(e.value) == '%s must be [B][n_vars]' % what
    with pytest.raises(ValueError):
        BT._rows_i32(torch.zeros(B + 1, NV, dtype=I32), (B, NV), CPU, 'labels')


def test_listed_count():
    K = collections.namedtuple('K', 'MAX_LISTED')(65536)
    assert BT._listed_count(1, K) == 1 and BT._listed_count(K.MAX_LISTED, K, 'N') == K.MAX_LISTED
    for n, word in ((0, 'n_samples'), (K.MAX_LISTED + 1, 'n_samples'), (0, 'N'), (K.MAX_LISTED + 1, 'N')):
        with pytest.raises(ValueError) as e:
            BT._listed_count(n, K, word)
        assert str(e.value) == '%s must be in [1, 65536]' % word
    from macaronicusermodeling_amd import cutdraw, cutsetis, exactmap
    assert cutdraw.MAX_LISTED == cutsetis.MAX_LISTED == exactmap.MAX_LISTED == 65536


def test_exactly_one_of_seed_and_uniforms():
    BT._exactly_one(0, None)
    BT._exactly_one(None, object())
    for seed, uniforms in ((None, None), (0, object())):
        with pytest.raises(ValueError) as e:
            BT._exactly_one(seed, uniforms)
        assert str(e.value) == 'give exactly one of seed and uniforms'


# ---- the per-shape loop of TiDirTrainer ------------------------------------------------------------------------------------
class _Refusal(RuntimeError):
    def __init__(self, code):
        RuntimeError.__init__(self, 'stub error %d' % code)
        self.code = code


class _Stub:
    """What _per_shape needs of a UserGraphTrainer: a topo and a method."""

    def __init__(self, n_rows, P=1, code=None):
        self.topo = collections.namedtuple('Topo', 'P')(P)
        self.n_rows, self.code, self.calls = n_rows, code, []

    def report(self, i):
        self.calls.append(i)
        if self.code is not None:
            raise _Refusal(self.code)
        return np.arange(self.n_rows) + 100.0 * i


def _shapes(with_einval):
    """Four shapes in order, their instances interleaved in the shard (instance j of shape k sits at 4 j + k): the second is
    refused as unsupported, the third fails with MLBP_EINVAL if asked to."""
    codes = [None, _ffi.MLBP_EUNSUPPORTED, _ffi.MLBP_EINVAL if with_einval else None, None]
    sizes = [2, 3, 1, 2]
    trainers, buckets = collections.OrderedDict(), {}
    for k in range(4):
        key = ('shape%d' % k, (k, k + 1))
        trainers[key] = _Stub(sizes[k], code=codes[k])
        buckets[key] = dict(rows=[dict(index=4 * j + k) for j in range(sizes[k])])
    return trainers, buckets


def test_per_shape_skips_the_unsupported_and_counts_every_shape():
    trainers, buckets = _shapes(with_einval=False)
    out, skipped = [((), 'empty')] * 16, []
    got = TR._per_shape(trainers, buckets, lambda i, tr: tr.report(i), out=out, row=lambda r, b: (float(r[b]),),
                        placeholder=(None,), refused=_Refusal, skipped=skipped)
    keys = list(trainers)
    assert [tr.calls for tr in trainers.values()] == [[0], [1], [2], [3]]                   # i == 3 for the fourth
    assert [(k, [r['index'] for r in rows]) for k, rows, _ in got] == [(keys[0], [0, 4]), (keys[2], [2]), (keys[3], [3, 7])]
    assert skipped == [((1, 2), 3, 'stub error %d' % _ffi.MLBP_EUNSUPPORTED)]
    want = [((), 'empty')] * 16
    want[0], want[4] = ((0, 1), 0.0), ((0, 1), 1.0)
    want[1] = want[5] = want[9] = ((1, 2), None)
    want[2] = ((2, 3), 200.0)
    want[3], want[7] = ((3, 4), 300.0), ((3, 4), 301.0)
    assert out == want


def test_per_shape_lets_every_other_error_through():
    trainers, buckets = _shapes(with_einval=True)
    skipped = []
    with pytest.raises(_Refusal) as e:
        TR._per_shape(trainers, buckets, lambda i, tr: tr.report(i), out=[None] * 16, row=lambda r, b: (r[b],), placeholder=(None,),
                      refused=_Refusal, skipped=skipped)
    assert e.value.code == _ffi.MLBP_EINVAL and len(skipped) == 1
    assert list(trainers.values())[3].calls == []                                           # the walk stopped at the third
    # and with no refusal class named, the unsupported shape is an error too
    trainers, buckets = _shapes(with_einval=False)
    with pytest.raises(_Refusal) as e:
        TR._per_shape(trainers, buckets, lambda i, tr: tr.report(i))
    assert e.value.code == _ffi.MLBP_EUNSUPPORTED


def test_per_shape_passes_over_a_shape_that_answers_none_and_tells_on_refused():
    trainers, buckets = _shapes(with_einval=False)
    list(trainers.values())[0].topo = collections.namedtuple('Topo', 'P')(0)
    out, skipped, told = [None] * 16, [], []
    got = TR._per_shape(trainers, buckets, lambda i, tr: tr.report(i) if tr.topo.P else None, out=out, row=lambda r, b: (r[b],),
                        placeholder=('-',), refused=_Refusal, skipped=skipped, on_refused=lambda tr, rows: told.append((tr, len(rows))))
    assert out[0] == out[4] == ((0, 1), '-') and len(skipped) == 1 and len(got) == 2
    assert told == [(list(trainers.values())[1], 3)]
    assert list(trainers.values())[3].calls == [3]


def test_reduced_in_one_process():
    assert not torch.distributed.is_available() or not torch.distributed.is_initialized()
    sums, maxima = TR._reduced(CPU, [3, 0.1, np.int64(7), -2.5], [1e-300, 4.0])
    assert sums.dtype == np.float64 and list(sums) == [3.0, 0.1, 7.0, -2.5] and list(maxima) == [1e-300, 4.0]
    sums, maxima = TR._reduced(CPU, np.array([1, 2], dtype=np.int64))
    assert list(sums) == [1.0, 2.0] and len(maxima) == 0
