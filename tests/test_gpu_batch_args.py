"""What FactorGraphBatch refuses before it launches anything, on the one shape that has tables of both kinds and a cutset: K3
at X = 4, B = 2 -- three variables, three pairwise and three unary factors, a cutset of one variable, four configurations.

Every refused tensor holds at least as many bytes as the one the call wants (a strided view of the same elements, int64 in
the place of float64 / int32, one more leading row), so a check that went missing could not make a kernel leave an
allocation; tensors on another device are left to tests/test_batch_args_cpu.py.  "No launch" is read off the bindings'
last_kernel() records, all of them, before and after the call."""
import re

import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_gpu_exactgrad as EG

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

F64, I32 = torch.float64, torch.int32
B, NV, X, P, NCUT = 2, 3, 4, 3, 1
S, N = 2, 3                                     # samples / listed entries per graph in the calls below
ROOTS = [0, 1, 2]


def _bindings():
    from macaronicusermodeling_amd import (converge, cutdraw, cutset, cutsetis, exactgrad, exactmap, exactmbest, exactsample, logz,
                                           mapdecode, sample)
    return (mapdecode, logz, sample, converge, cutset, cutsetis, cutdraw, exactmap, exactmbest, exactsample, exactgrad)


def _launched():
    return tuple(K.last_kernel() for K in _bindings())


@pytest.fixture(scope='module')
def fb():
    spec = R.kn_spec(3, X)
    fb = EG._batch(spec, [C.make_inputs(spec, s, 'uniform') for s in (1, 2)])
    assert (fb.B, fb.topo.n_vars, fb.topo.P, fb.topo.U) == (B, NV, P, 3)
    from macaronicusermodeling_amd import cutset
    assert cutset.plan(fb.topo, None, X, fb.device).n_cut == NCUT
    fb.sweep(ROOTS, init=True)                   # cutset_draw / cutset_logq read the messages as they stand
    torch.cuda.synchronize()
    return fb


def _good(fb, shape, dtype):
    return torch.zeros(shape, dtype=dtype, device=fb.device) if dtype == I32 else torch.full(shape, 0.5, dtype=dtype, device=fb.device)


def _bad(fb, shape, dtype):
    """The three refused tensors of a wanted (shape, dtype): never fewer bytes than the good one."""
    rev = tuple(reversed(range(len(shape))))
    permuted = torch.zeros(shape[::-1], dtype=dtype, device=fb.device).permute(*rev)
    assert tuple(permuted.shape) == tuple(shape) and not permuted.is_contiguous()
    return dict(permuted=permuted, int64=torch.zeros(shape, dtype=torch.int64, device=fb.device),
                extra_row=torch.zeros((shape[0] + 1,) + tuple(shape[1:]), dtype=dtype, device=fb.device))


M3, FEE, FED = (B, NV, X), 3, 6
UNI = 'uniforms must be a contiguous float64 device tensor [n_samples][B][n_vars]'
UNI_CUT = 'uniforms must be a contiguous float64 device tensor [B][n_samples][n_cut]'
MARG = 'marginals must be a contiguous float64 device tensor [B][n_vars][X]'
CONFIGS = 'configs must be a contiguous int32 device tensor [B][N][n_cut]'


def _configs(fb):
    return torch.zeros(B, N, NCUT, dtype=I32, device=fb.device)


def _log_q(fb):
    return torch.full((B, N), -1.0, dtype=F64, device=fb.device)


# (id, wanted shape, dtype, the words of the refusal, call(fb, tensor))
PARAMETERS = [
    ('map_sweep-max_marginals', M3, F64, 'max_marginals must be float64 [B][n_vars][X]', lambda fb, t: fb.map_sweep(ROOTS, max_marginals=t)),
    ('sample-uniforms', (S, B, NV), F64, UNI, lambda fb, t: fb.sample(ROOTS, S, uniforms=t)),
    ('sample-cond_marginals', (S, B, NV, X), F64, 'cond_marginals must be a contiguous float64 device tensor [n_samples][B][n_vars][X]',
     lambda fb, t: fb.sample(ROOTS, S, seed=0, cond_marginals=t)),
    ('converge-marginals', M3, F64, MARG, lambda fb, t: fb.converge(marginals=t)),
    ('exact_inference-marginals', M3, F64, MARG, lambda fb, t: fb.exact_inference(marginals=t)),
    ('cutset_proposal-uniforms', (N, B, NV), F64, UNI, lambda fb, t: fb.cutset_proposal(ROOTS, N, uniforms=t)),
    ('cutset_draw-uniforms', (B, N, NCUT), F64, UNI_CUT, lambda fb, t: fb.cutset_draw(N, uniforms=t)),
    ('cutset_logq-configs', (B, N, NCUT), I32, CONFIGS, lambda fb, t: fb.cutset_logq(t)),
    ('cutset_estimate-uniforms', (N, B, NV), F64, UNI, lambda fb, t: fb.cutset_estimate(ROOTS, N, uniforms=t)),
    ('cutset_estimate-messages-uniforms', (B, N, NCUT), F64, UNI_CUT,
     lambda fb, t: fb.cutset_estimate(n_samples=N, uniforms=t, proposal='messages')),
    ('cutset_estimate-configs', (B, N, NCUT), I32, CONFIGS, lambda fb, t: fb.cutset_estimate(configs=t, log_q=_log_q(fb))),
    ('cutset_estimate-log_q', (B, N), F64, 'log_q must be a contiguous float64 device tensor [B][N]',
     lambda fb, t: fb.cutset_estimate(configs=_configs(fb), log_q=t)),
    ('cutset_estimate-marginals', M3, F64, MARG, lambda fb, t: fb.cutset_estimate(configs=_configs(fb), log_q=_log_q(fb), marginals=t)),
    ('exact_map-max_marginals', M3, F64, 'max_marginals must be True or a contiguous float64 device tensor [B][n_vars][X]',
     lambda fb, t: fb.exact_map(max_marginals=t)),
    ('cutset_map-configs', (B, N, NCUT), I32, CONFIGS, lambda fb, t: fb.cutset_map(t)),
    ('exact_sample-uniforms', (S, B, NV), F64, UNI, lambda fb, t: fb.exact_sample(S, uniforms=t)),
    ('exact_pair_marginals-out', (B, P, X, X), F64, 'pair_marginals must be a contiguous float64 device tensor [2, 3, 4, 4]',
     lambda fb, t: fb.exact_pair_marginals(out=t)),
    ('exact_gradient-out_ee', (B, FEE), F64, 'out_ee must be a contiguous float64 device tensor [2, 3]', lambda fb, t: fb.exact_gradient(out_ee=t)),
    ('exact_gradient-out_ed', (B, FED), F64, 'out_ed must be a contiguous float64 device tensor [2, 6]', lambda fb, t: fb.exact_gradient(out_ed=t)),
    ('exact_gradient-pair_marginals', (B, P, X, X), F64, 'pair_marginals must be a contiguous float64 device tensor [2, 3, 4, 4]',
     lambda fb, t: fb.exact_gradient(pair_marginals=t)),
    ('exact_gradient-marginals', M3, F64, 'marginals must be a contiguous float64 device tensor [2, 3, 4]',
     lambda fb, t: fb.exact_gradient(marginals=t)),
    ('exact_gradient-expect_only-out_ee', (B, FEE), F64, 'out_ee must be a contiguous float64 device tensor [2, 3]',
     lambda fb, t: fb.exact_gradient(out_ee=t, expect_only=True)),
]


@pytest.mark.parametrize('name,shape,dtype,words,call', PARAMETERS, ids=[p[0] for p in PARAMETERS])
def test_a_wrong_tensor_is_refused_before_any_launch(fb, name, shape, dtype, words, call):
    assert (int(fb.phi_en_en.shape[2]), int(fb.phi_en_de.shape[2])) == (FEE, FED)
    before = _launched()
    for kind, t in _bad(fb, shape, dtype).items():
        assert t.numel() * t.element_size() >= int(np.prod(shape)) * (4 if dtype == I32 else 8)
        with pytest.raises(ValueError, match='^' + re.escape(words)):
            call(fb, t)
        assert _launched() == before, (name, kind)
    torch.cuda.synchronize()


def test_search_map_refuses_wrong_uniforms_before_the_draw(fb):
    """search_map's uniforms belong to its cutset_draw, which runs behind map_sweep and sweep: those two have launched, the draw
    and the listed walk have not."""
    from macaronicusermodeling_amd import cutdraw, exactmap
    for kind, t in _bad(fb, (B, N - 1, NCUT), F64).items():
        before = cutdraw.last_kernel(), exactmap.last_kernel()
        with pytest.raises(ValueError, match='^' + re.escape(UNI_CUT)):
            fb.search_map(ROOTS, n_samples=N, uniforms=t)
        assert (cutdraw.last_kernel(), exactmap.last_kernel()) == before, kind
    fb.sweep(ROOTS, init=True)                   # the messages the other tests expect
    torch.cuda.synchronize()


def _calls(fb):
    """name -> a valid call of each method that reads the tables."""
    configs, log_q = _configs(fb), _log_q(fb)
    return {
        'map_sweep': lambda: fb.map_sweep(ROOTS),
        'log_partition': lambda: fb.log_partition(),
        'sample': lambda: fb.sample(ROOTS, S, seed=0),
        'converge': lambda: fb.converge(max_rounds=2),
        'exact_inference': lambda: fb.exact_inference(),
        'cutset_proposal': lambda: fb.cutset_proposal(ROOTS, N, seed=0),
        'cutset_draw': lambda: fb.cutset_draw(N, seed=0),
        'cutset_logq': lambda: fb.cutset_logq(configs),
        'cutset_estimate': lambda: fb.cutset_estimate(configs=configs, log_q=log_q),
        'exact_map': lambda: fb.exact_map(),
        'cutset_map': lambda: fb.cutset_map(configs),
        'search_map': lambda: fb.search_map(ROOTS, n_samples=N),
        'exact_mbest': lambda: fb.exact_mbest(2),
        'exact_sample': lambda: fb.exact_sample(S, seed=0),
        'exact_pair_marginals': lambda: fb.exact_pair_marginals(),
        'exact_gradient': lambda: fb.exact_gradient(),
    }


TWELVE = ['map_sweep', 'log_partition', 'sample', 'converge', 'exact_inference', 'cutset_estimate', 'cutset_draw', 'exact_map',
          'cutset_map', 'exact_mbest', 'exact_sample', 'exact_gradient']


def test_tables_first():
    """A batch without tables: every call says which setter is missing, and launches nothing."""
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    spec = R.kn_spec(3, X)
    topo = GraphTopology.from_spec(spec)
    bare = FactorGraphBatch(topo, X, B)
    feat = EG.G.make_features(EG.O.Graph(spec), 77, kinds=[0, 1, 2])
    bare.set_features(feat['phi_en_en'], feat['phi_en_en_w1'], feat['phi_en_de'], [0] * P, [0] * 3)   # exact_gradient asks for them first
    calls = _calls(bare)
    before = _launched()
    for name in TWELVE + ['cutset_proposal', 'cutset_logq', 'exact_pair_marginals']:
        with pytest.raises(RuntimeError, match=r'^set_pair_tables\(\) first$'):
            calls[name]()
        assert _launched() == before, name
    bare.set_pair_tables(np.ones((B * P, X, X)))
    for name in TWELVE:
        if name == 'cutset_draw':                # reads pairwise tables and messages only
            continue
        with pytest.raises(RuntimeError, match=r'^set_unary_tables\(\) first$'):
            calls[name]()
        assert _launched() == before, name
    torch.cuda.synchronize()


def test_float32_pair_tables_are_refused(fb):
    """Every side-library call needs float64 pairwise tables.  (set_pair_tables admits float32 at X = 256 and 512 only; the
    refusal looks at the dtype alone, so the K3's tables are swapped for a float32 copy here.)"""
    calls = _calls(fb)
    kept = fb.pair_tables
    before = _launched()
    try:
        fb.pair_tables = kept.to(torch.float32)
        for name in sorted(calls):
            with pytest.raises(NotImplementedError, match='float64'):
                calls[name]()
            assert _launched() == before, name
    finally:
        fb.pair_tables = kept
    torch.cuda.synchronize()


def _nan(fb, *shape):
    return torch.full(shape, float('nan'), dtype=F64, device=fb.device)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.uint8) == b.contiguous().view(torch.uint8)).all())


def test_a_callers_tensor_is_returned_and_holds_the_bits_of_an_own_allocation(fb):
    configs, log_q = _configs(fb), _log_q(fb)
    for name, supplied, own in [
        ('exact_inference', lambda t: fb.exact_inference(marginals=t)[1], lambda: fb.exact_inference()[1]),
        ('cutset_estimate', lambda t: fb.cutset_estimate(configs=configs, log_q=log_q, marginals=t)[1],
         lambda: fb.cutset_estimate(configs=configs, log_q=log_q)[1]),
        ('exact_map', lambda t: fb.exact_map(max_marginals=t)[2], lambda: fb.exact_map(max_marginals=True)[2]),
    ]:
        t = _nan(fb, *M3)
        assert supplied(t) is t, name
        assert _same_bits(t, own()) and not bool(torch.isnan(t).any()), name
    t = _nan(fb, B, P, X, X)
    assert fb.exact_pair_marginals(out=t) is t and _same_bits(t, fb.exact_pair_marginals()) and not bool(torch.isnan(t).any())
    ee, ed = _nan(fb, B, FEE), _nan(fb, B, FED)
    got, own = fb.exact_gradient(out_ee=ee, out_ed=ed), fb.exact_gradient()
    assert got[0] is ee and got[1] is ed and all(_same_bits(a, b) for a, b in zip(got, own)) and not bool(torch.isnan(ee).any() | torch.isnan(ed).any())
    # outputs that are written but not returned: filled, and the call's own results are the bits of a call without them
    for name, with_t, without, shape in [
        ('map_sweep', lambda t: fb.map_sweep(ROOTS, max_marginals=t), lambda: fb.map_sweep(ROOTS), M3),
        ('converge', lambda t: fb.converge(max_rounds=3, marginals=t), lambda: fb.converge(max_rounds=3), M3),
        ('sample', lambda t: fb.sample(ROOTS, S, seed=3, cond_marginals=t), lambda: fb.sample(ROOTS, S, seed=3), (S, B, NV, X)),
    ]:
        t = _nan(fb, *shape)
        got, want = with_t(t), without()
        assert all(_same_bits(a, b) for a, b in zip(got, want)), name
        assert not bool(torch.isnan(t).any()), name
    fb.sweep(ROOTS, init=True)
    torch.cuda.synchronize()
