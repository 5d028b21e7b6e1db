"""The gradient beyond the exact limit on the GPU: the listed mode of libmlbp_exactgrad.so (FactorGraphBatch.cutset_gradient,
cutset_pair_marginals, estimate_gradient and the trainers' estimated_gradient / estimated_step) against the NumPy statement of
tests/test_estgrad_cpu.py, against exact_gradient() / exact_pair_marginals() where the list is the full one, and against
cutset_estimate() on the same list.

Bars, those of tests/test_gpu_exactgrad.py.  pair_marginals and marginals within 1e-10 absolute of the statement, log_z_hat
within 1e-10 * max(1, |log_z_hat|) of the statement and of cutset_estimate(); expect_* and grad_* within (P + U) * max(1e-12,
X^2 * 2^-51) of the NumPy contraction of the tensors the same call returned; rows and columns of every M_p sum to the marginals
of the same call at X * 2^-50.  Bit-for-bit claims: the full list in index order with log_q = 0 is the exact call in every output
but log_z; a graph's bits do not depend on B or on its position in the batch AT AN EQUAL NUMBER OF CHUNKS; a table times 2^+-300
moves no bit of a normalised output; a refused graph leaves every other graph its bits; exact_gradient() and
exact_pair_marginals() compute what they computed before the listed mode existed (tests/golden/exactgrad_exact_bits.json,
recorded on the library as it was).
Across chunk counts the walkers group the entries differently -- the header prescribes which entries a walker adds up, and a
floating-point sum regrouped is another sum -- so there the outputs are held to the statement's bars, not to bits; the test
prints how far apart they are.
No test asserts a statistical accuracy."""
import hashlib
import json
import os

import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_cutsetis_cpu as IS
import test_estgrad_cpu as L
import test_gpu_exactgrad as E
from helpers import batch_tables, tidir_gold, write_tidir
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

X64, GENERIC = 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'exactgrad_exact_bits.json')
KEYS = E.KEYS
NORMALISED = KEYS[1:]


def _M():
    from macaronicusermodeling_amd import exactgrad
    return exactgrad


def _dev(fb, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to(fb.device)


def _run(fb, configs, log_q, kernel=None, labels=None, cutset=None, fill=float('nan')):
    """One full listed call (every output), then the lean calls, which must repeat its bits.  configs [B][N][n_cut], log_q
    [B][N] (numpy)."""
    M, topo = _M(), fb.topo
    c, q = _dev(fb, configs, np.int32), _dev(fb, log_q, np.float64)
    pm = torch.full((fb.B, topo.P, fb.X, fb.X), fill, dtype=torch.float64, device=fb.device)
    mg = torch.full((fb.B, topo.n_vars, fb.X), fill, dtype=torch.float64, device=fb.device)
    msgs_before = fb.msgs.clone()
    g_ee, g_ed, log_z = fb.cutset_gradient(c, q, labels=labels, pair_marginals=pm, marginals=mg, cutset=cutset)
    ran = M.last_kernel()
    e_ee, e_ed, log_z2 = fb.cutset_gradient(c, q, expect_only=True, cutset=cutset)
    l_ee, l_ed, _ = fb.cutset_gradient(c, q, labels=labels, cutset=cutset)
    pm2 = torch.full_like(pm, fill)
    fb.cutset_pair_marginals(c, q, out=pm2, cutset=cutset)
    torch.cuda.synchronize()
    assert torch.equal(fb.msgs.view(torch.int64), msgs_before.view(torch.int64))          # self.msgs is left untouched (bits)
    if kernel is not None:
        assert ran == kernel, ran
    got = dict(log_z=log_z.cpu().numpy(), marg=mg.cpu().numpy(), pm=pm.cpu().numpy(), grad_ee=g_ee.cpu().numpy(), grad_ed=g_ed.cpu().numpy(),
               exp_ee=e_ee.cpu().numpy(), exp_ed=e_ed.cpu().numpy(), kernel=ran)
    assert np.array_equal(got['log_z'], log_z2.cpu().numpy(), equal_nan=True) and np.array_equal(got['pm'], pm2.cpu().numpy(), equal_nan=True)
    assert np.array_equal(got['grad_ee'], l_ee.cpu().numpy(), equal_nan=True) and np.array_equal(got['grad_ed'], l_ed.cpu().numpy(), equal_nan=True)
    return got


def _lists(spec, inputs, N, seed=50):
    """Per-graph lists from the statement's proposal: (cut ids, configs [B][N][n_cut], log_q [B][N])."""
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    drawn = [IS.make_list(g, inp, cut, N, seed + b) for b, inp in enumerate(inputs)]
    return cut, np.stack([d[0] for d in drawn]).reshape(len(inputs), N, len(cut)), np.stack([d[1] for d in drawn])


def _against_statement(name, fb, inputs, cut, configs, log_q, got, graphs=None):
    g = fb.ref['g']
    wz = wm = wp = 0.0
    for b in range(fb.B) if graphs is None else graphs:
        want = L.listed_pairs(g, inputs[b], cut, configs[b], log_q[b])
        wz = max(wz, abs(got['log_z'][b] - want['log_z_hat']) / max(1.0, abs(want['log_z_hat'])))
        wm = max(wm, float(np.abs(got['marg'][b] - want['marg']).max()))
        for p, fid in enumerate(fb.ref['pair_ids']):
            wp = max(wp, float(np.abs(got['pm'][b, p] - want['pairs'][fid]).max()))
    print('%s: log_z_hat within %.1e, marginals within %.1e, pair marginals within %.1e of the statement' % (name, wz, wm, wp))
    assert wz <= 1e-10 and wm <= 1e-10 and wp <= 1e-10, name
    E._check_consistency(name, fb, got, graphs)
    E._check_features(name, fb, got, graphs)


def _against_estimate(fb, configs, log_q, got, cutset=None):
    log_z_hat, marg, _ = fb.cutset_estimate(configs=_dev(fb, configs, np.int32), log_q=_dev(fb, log_q, np.float64), cutset=cutset)
    ref = log_z_hat.cpu().numpy()
    assert (np.abs(got['log_z'] - ref) <= 1e-10 * np.maximum(1.0, np.abs(ref))).all()
    assert np.abs(got['marg'] - marg.cpu().numpy()).max() <= 1e-10


def _case(name, spec, seeds, N, kernel, kind='uniform'):
    inputs = [C.make_inputs(spec, s, kind) for s in seeds]
    fb = E._batch(spec, inputs, seed=seeds[0])
    cut, configs, log_q = _lists(spec, inputs, N)
    got = _run(fb, configs, log_q, kernel=kernel)
    _against_statement(name, fb, inputs, cut, configs, log_q, got)
    _against_estimate(fb, configs, log_q, got)
    return fb, inputs, (cut, configs, log_q), got


def _full(spec, B):
    n_cut = len(R.chosen_ids(spec))
    full = IS.full_list(spec['X'], n_cut)
    return np.tile(full[None], (B, 1, 1)), np.zeros((B, len(full)))


def _full_list_is_exact(spec, seeds, kernel, kind='uniform'):
    inputs = [C.make_inputs(spec, s, kind) for s in seeds]
    fb = E._batch(spec, inputs, seed=seeds[0])
    exact = E._run(fb)
    configs, log_q = _full(spec, fb.B)
    got = _run(fb, configs, log_q, kernel=kernel)
    for key in NORMALISED:
        assert np.array_equal(got[key], exact[key]), key
    want = exact['log_z'] - np.log(configs.shape[1])
    assert (np.abs(got['log_z'] - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all()


# ---- against the statement, and the full list against the exact call ----------------------------------------
def test_k3_x64_full_list_is_the_exact_call_and_a_short_list_the_statement():
    M = _M()
    spec = R.kn_spec(3, 64)
    assert M.chunks(3, 64, M.KERNEL_X64) == 16 and M.chunks(3, 7, M.KERNEL_X64) == 2
    _full_list_is_exact(spec, (1, 2, 3), X64)
    _case('k3_x64_n7', spec, (1, 2, 3), 7, X64)


@pytest.mark.parametrize('N', [5, 37])
def test_k5_x64_beyond_the_exact_limit(N):
    """Three cutset variables, 64^3 configurations: the exact call refuses, the listed one answers.  N = 5 on 8 waves, N = 37 on
    40: ragged against the 4 C waves, so some waves hold no entry and write an empty partial."""
    M = _M()
    assert M.chunks(3, N, M.KERNEL_X64) == -(-N // 4) and N % 4
    fb, _, _, _ = _case('k5_x64_n%d' % N, R.kn_spec(5, 64), (1, 2, 3), N, X64, kind='lognormal' if N == 5 else 'uniform')
    with pytest.raises(M.ExactGradError, match='configurations'):
        fb.exact_gradient()


def test_k5_x64_one_chunk_and_idle_waves():
    """B = 600 with N = 3: C = 1, so the fourth wave of every workgroup has no entry; three sets of tables shared by the 600
    graphs, every graph a list of its own.  Every 41st graph against the statement; the graphs that share tables AND a list share
    their bits."""
    M = _M()
    B, N = 600, 3
    assert M.chunks(B, N, M.KERNEL_X64) == 1
    spec = R.kn_spec(5, 64)
    base = [C.make_inputs(spec, 70 + s) for s in range(3)]
    inputs = [base[b % 3] for b in range(B)]
    topo = E._batch(spec, base).topo
    index = np.arange(B) % 3
    ptab = np.arange(3 * topo.P).reshape(-1, topo.P)[index]
    utab = np.arange(3 * topo.U).reshape(-1, topo.U)[index]
    fb = E._batch(spec, inputs, batch_tables(spec, topo, base), ptab, utab, seed=3)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    lists = [IS.make_list(g, inputs[b], cut, N, 900 + b % 50) for b in range(B)]            # graphs b and b + 150 share tables and list
    configs, log_q = np.stack([l[0] for l in lists]), np.stack([l[1] for l in lists])
    got = _run(fb, configs, log_q, kernel=X64)
    _against_statement('k5_x64_b600', fb, inputs, cut, configs, log_q, got, graphs=range(0, B, 41))
    for key in ('log_z', 'marg', 'pm'):                          # (expect_* and grad_* read the graph's own columns and labels)
        assert np.array_equal(got[key][:150], got[key][150:300]), key
    assert np.isfinite(got['grad_ee']).all() and np.isfinite(got['log_z']).all()


def test_cycle4_x64_two_forest_factors():
    """A 4-cycle at X = 64: one cutset variable, the remainder a chain of three: both accumulators of the <2> instance."""
    M = _M()
    spec = C.ring_spec(4, 64)
    assert len(R.chosen_ids(spec)) == 1 and M.pick_kernel(64, 4, 4, 4, 2) == M.KERNEL_X64
    _full_list_is_exact(spec, (4, 5), X64)
    _case('cycle4_x64_n9', spec, (4, 5), 9, X64, kind='lognormal')


def test_chain4_x64_on_the_generic_kernel():
    """Three forest factors: past the X = 64 kernel's registers.  No cutset variable: every entry is the empty configuration."""
    M = _M()
    spec = C.chain_spec(4, 64)
    assert M.pick_kernel(64, 4, 3, 4, 3) == M.KERNEL_GENERIC and not R.chosen_ids(spec)
    _full_list_is_exact(spec, (1, 2), GENERIC)
    _case('chain4_x64_n3', spec, (1, 2), 3, GENERIC)


def test_k4_x5_full_list_and_a_long_list():
    M = _M()
    spec = R.kn_spec(4, 5)
    assert M.chunks(3, 25, M.KERNEL_GENERIC) == 25 and M.chunks(3, 300, M.KERNEL_GENERIC) == 86
    _full_list_is_exact(spec, (3, 4, 5), GENERIC, kind='lognormal')
    _case('k4_x5_n300', spec, (3, 4, 5), 300, GENERIC)           # 86 workgroups per graph: three or four entries each


def test_k6_x3_and_a_star_on_the_generic_kernel():
    _case('k6_x3_n50', R.kn_spec(6, 3), (6, 7), 50, GENERIC, kind='lognormal')
    spec = C.star_spec(4, 6)
    assert not R.chosen_ids(spec)
    _full_list_is_exact(spec, (8, 9), GENERIC)
    fb, inputs, (cut, configs, log_q), got = _case('star_x6_n4', spec, (8, 9), 4, GENERIC)
    log_q[:] = np.array([[-0.5, 0.25, 0.0, -1.0], [0.0, 0.0, 3.0, 0.1]])                     # weights of its own making: the same conditional
    moved = _run(fb, configs, log_q, kernel=GENERIC)
    _against_statement('star_x6_weights', fb, inputs, cut, configs, log_q, moved)
    assert np.abs(moved['pm'] - got['pm']).max() <= 1e-12        # one configuration: the normalised outputs do not see the weights


# ---- invariance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,make,kernel,N', [('k5_x64', lambda: R.kn_spec(5, 64), X64, 37), ('k6_x3', lambda: R.kn_spec(6, 3), GENERIC, 50)],
                         ids=['x64', 'generic'])
def test_bits_do_not_depend_on_batch_size_or_position(name, make, kernel, N):
    """At an equal number of chunks a graph's bits are its own: alone, in a batch, at another position, among graphs naming the
    same tables.  At another number of chunks the walkers group the entries differently: the statement's bars (see the module's
    docstring)."""
    M = _M()
    spec = make()
    inputs = [C.make_inputs(spec, s) for s in (1, 2, 3, 4)]
    fb = E._batch(spec, inputs)
    cut, configs, log_q = _lists(spec, inputs, N)
    full = _run(fb, configs, log_q, kernel=kernel)
    assert M.chunks(1, N, kernel) == M.chunks(4, N, kernel)
    alone = _run(E._batch(spec, inputs[1:2], labels=fb.ref['labels'][1:2], obs=fb.ref['obs'][1:2]), configs[1:2], log_q[1:2], kernel=kernel)
    for key in KEYS:
        assert np.array_equal(alone[key][0], full[key][1]), key
    order = [2, 1, 0, 3]
    moved = _run(E._batch(spec, [inputs[i] for i in order], labels=fb.ref['labels'][order], obs=fb.ref['obs'][order]), configs[order], log_q[order])
    for key in KEYS:
        assert np.array_equal(moved[key], full[key][order]), key
    # another number of chunks: B = 300 copies of graph 1 walk their lists on one chunk each
    B = 300
    assert M.chunks(B, N, kernel) == 1 and M.chunks(4, N, kernel) > 1
    pair, unary = batch_tables(spec, fb.topo, inputs[1:2])
    many = E._batch(spec, inputs[1:2] * B, (pair, unary), np.tile(np.arange(fb.topo.P), (B, 1)), np.tile(np.arange(fb.topo.U), (B, 1)),
                    labels=np.tile(fb.ref['labels'][1:2], (B, 1)), obs=np.tile(fb.ref['obs'][1:2], (B, 1)))
    wide = _run(many, np.tile(configs[1:2], (B, 1, 1)), np.tile(log_q[1:2], (B, 1)), kernel=kernel)
    for key in KEYS:
        assert np.array_equal(wide[key], np.tile(wide[key][:1], (B,) + (1,) * (wide[key].ndim - 1))), key       # every copy the same bits
        gap = float(np.abs(wide[key][0] - full[key][1]).max())
        print('%s %s: one chunk against %d: %.1e apart' % (name, key, M.chunks(4, N, kernel), gap))
        assert gap <= 1e-10 * max(1.0, float(np.abs(full[key][1]).max())), key


@pytest.mark.parametrize('name,make,kernel,N', [('k5_x64', lambda: R.kn_spec(5, 64), X64, 9), ('cycle4_x64', lambda: C.ring_spec(4, 64), X64, 6),
                                                ('k4_x5', lambda: R.kn_spec(4, 5), GENERIC, 30)], ids=['x64_1', 'x64_2', 'generic'])
def test_power_of_two_scaling(name, make, kernel, N):
    """Any table times 2^k, k = +-300: no bit of a normalised output moves, log_z_hat moves by k ln 2."""
    spec = make()
    inputs = [C.make_inputs(spec, s, 'lognormal') for s in (1, 2)]
    fb = E._batch(spec, inputs)
    cut, configs, log_q = _lists(spec, inputs, N)
    base = _run(fb, configs, log_q, kernel=kernel)
    pair, unary = batch_tables(spec, fb.topo, inputs)
    P, U, B = fb.topo.P, fb.topo.U, len(inputs)
    for pk, uk in (({0: 300}, {}), ({P - 1: -300}, {}), ({}, {0: 300}), ({1: -300, P - 1: 300}, {U - 1: -300, 0: 7})):
        p2, u2 = pair.copy(), unary.copy()
        for b in range(B):
            for p, k in pk.items():
                p2[b * P + p] = np.ldexp(p2[b * P + p], k)
            for u, k in uk.items():
                u2[b * U + u] = np.ldexp(u2[b * U + u], k)
        got = _run(E._batch(spec, inputs, (p2, u2)), configs, log_q, kernel=kernel)
        for key in NORMALISED:
            assert np.array_equal(got[key], base[key]), (name, key, pk, uk)
        want = base['log_z'] + (sum(pk.values()) + sum(uk.values())) * np.log(2.0)
        assert (np.abs(got['log_z'] - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), (pk, uk)


# ---- refusals --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,make,kernel,N', [('k5_x64', lambda: R.kn_spec(5, 64), X64, 6), ('k4_x5', lambda: R.kn_spec(4, 5), GENERIC, 30)],
                         ids=['x64', 'generic'])
def test_one_refused_graph_of_each_kind_leaves_the_others_their_bits(name, make, kernel, N):
    """A state above and a state below [0, X), a NaN, an infinite and an out-of-range log_q, a list whose every weight is zero --
    each in a graph of its own, the bad entry first, last or in the middle of its walker's share; every other graph keeps the bits
    of the clean batch, and a refused graph keeps what its tensors held."""
    spec = make()
    X = spec['X']
    inputs = [C.make_inputs(spec, s) for s in range(1, 10)]
    fb = E._batch(spec, inputs)
    cut, configs, log_q = _lists(spec, inputs, N)
    base = _run(fb, configs, log_q, kernel=kernel)
    c2, q2 = configs.copy(), log_q.copy()
    c2[0, 0, 0] = X                                              # graph 0: a state above the range, in the first entry
    c2[1, N - 1, len(cut) - 1] = -1                              # graph 1: a state below it, in the last entry
    c2[2, N // 2, 1] = 1 << 30                                   # graph 2: far outside: an address formed from it would leave the workspace
    q2[3, 1] = np.nan
    q2[4, N - 1] = np.inf
    q2[5, 0] = -np.inf
    q2[6, 2] = 2.0e6                                             # beyond MLBP_CUTSETIS_MAX_ABS_LOG_Q
    pair, unary = batch_tables(spec, fb.topo, inputs)
    U = fb.topo.U
    u2 = unary.copy()
    u2[7 * U:8 * U] = 0.0                                        # graph 7: every Z_c is zero
    bad = E._batch(spec, inputs, (pair, u2), labels=fb.ref['labels'], obs=fb.ref['obs'])
    got = _run(bad, c2, q2, kernel=kernel, fill=-7.0)
    for b in range(7):
        assert np.isnan(got['log_z'][b]) and (got['marg'][b] == -7.0).all() and (got['pm'][b] == -7.0).all(), b
        for key in KEYS[3:]:
            assert np.isnan(got[key][b]).all(), (key, b)
    assert got['log_z'][7] == -np.inf and np.array_equal(got['marg'][7], np.full_like(got['marg'][7], 1.0 / X))
    assert np.array_equal(got['pm'][7], np.full_like(got['pm'][7], (1.0 / X) * (1.0 / X))) and np.isfinite(got['grad_ee'][7]).all()
    for key in KEYS:
        assert np.array_equal(got[key][8], base[key][8]), key


def test_arguments_are_checked():
    from macaronicusermodeling_amd import cutsetis
    spec = R.kn_spec(5, 64)
    inputs = [C.make_inputs(spec, s) for s in (1, 2)]
    fb = E._batch(spec, inputs)
    cut, configs, log_q = _lists(spec, inputs, 4)
    c, q = _dev(fb, configs, np.int32), _dev(fb, log_q)
    for bad_c, bad_q in ((c.long(), q), (c[:, :3], q), (c, q.float()), (c[:1], q[:1]), (c.cpu(), q), (c[:, :, :2].contiguous(), q)):
        with pytest.raises(ValueError):
            fb.cutset_gradient(bad_c, bad_q)
    with pytest.raises(ValueError):
        fb.cutset_pair_marginals(c, q, out=torch.empty(2, 10, 64, 63, dtype=torch.float64, device=fb.device))
    with pytest.raises(ValueError, match='proposal'):
        fb.estimate_gradient([0], proposal='bp')
    with pytest.raises(ValueError, match='roots'):
        fb.estimate_gradient(None, proposal='sample')
    with pytest.raises(cutsetis.CutsetisError, match='cycle'):
        fb.cutset_gradient(c, q, cutset=[0])


# ---- capture ---------------------------------------------------------------------------------------------------
def test_capture_and_replay():
    """After one eager call cutset_gradient is captured and replayed on a changed list: the bits of the eager calls."""
    spec = R.kn_spec(5, 64)
    inputs = [C.make_inputs(spec, s) for s in (1, 2, 3)]
    fb = E._batch(spec, inputs)
    cut, configs, log_q = _lists(spec, inputs, 9)
    _, configs2, log_q2 = _lists(spec, inputs, 9, seed=77)
    eager, eager2 = _run(fb, configs, log_q, kernel=X64), _run(fb, configs2, log_q2, kernel=X64)
    c, q = _dev(fb, configs, np.int32), _dev(fb, log_q)
    pm = torch.empty(fb.B, fb.topo.P, fb.X, fb.X, dtype=torch.float64, device=fb.device)
    mg = torch.empty(fb.B, fb.topo.n_vars, fb.X, dtype=torch.float64, device=fb.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_ee, g_ed, log_z = fb.cutset_gradient(c, q, pair_marginals=pm, marginals=mg)
    for want in (eager, eager2, eager):
        for t in (g_ee, g_ed, log_z, pm, mg):
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for key, t in (('grad_ee', g_ee), ('grad_ed', g_ed), ('log_z', log_z), ('pm', pm), ('marg', mg)):
            assert np.array_equal(t.cpu().numpy(), want[key]), key
        c.copy_(torch.from_numpy(configs2 if want is eager else configs))
        q.copy_(torch.from_numpy(log_q2 if want is eager else log_q))


# ---- the exact path is what it was -------------------------------------------------------------------------------
def golden_batches():
    """The K3 and K4 batches of tests/test_gpu_exactgrad.py (test_k3_x64_against_enumeration, test_k4_x64_against_elimination)."""
    k3, k4 = R.kn_spec(3, 64), R.kn_spec(4, 64)
    return {'k3_x64': E._batch(k3, [C.make_inputs(k3, s, 'uniform') for s in (1, 2, 3)], seed=1),
            'k4_x64': E._batch(k4, [C.make_inputs(k4, s, 'lognormal') for s in (1, 2)], seed=1)}


def golden_record(fb, kernel=None):
    """Every output of the exact calls on `fb`: the small ones as hex floats, the tensors as the SHA-256 of their bytes."""
    got = E._run(fb, kernel=kernel)
    out = {key: [float(v).hex() for v in got[key].reshape(-1)] for key in ('log_z', 'grad_ee', 'grad_ed', 'exp_ee', 'exp_ed')}
    out.update({key + '_sha256': hashlib.sha256(np.ascontiguousarray(got[key]).tobytes()).hexdigest() for key in ('marg', 'pm')})
    return out


@pytest.mark.parametrize('name', ['k3_x64', 'k4_x64'])
def test_the_exact_calls_compute_the_bits_they_computed_before(name):
    """exact_gradient() and exact_pair_marginals() on the K3 and K4 inputs of tests/test_gpu_exactgrad.py: every bit is the one
    recorded on the library before it had a listed mode."""
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    assert golden_record(golden_batches()[name], kernel=E.X64_1) == want


# ---- estimate_gradient and the trainers ----------------------------------------------------------------------
@pytest.mark.parametrize('proposal', ['messages', 'sample'])
def test_estimate_gradient_is_the_list_then_the_gradient(proposal):
    spec = R.kn_spec(5, 64)
    inputs = [C.make_inputs(spec, 60 + s) for s in range(3)]
    roots = list(O.Graph(spec).var_order)
    fb = E._batch(spec, inputs)
    fb.initialize()
    g_ee, g_ed, log_z_hat = fb.estimate_gradient(roots, n_list=16, seed=7, proposal=proposal)
    assert _M().last_kernel() == X64
    fb2 = E._batch(spec, inputs)
    fb2.initialize()
    if proposal == 'messages':
        fb2.sweep(roots, init=True)
        configs, log_q = fb2.cutset_draw(16, seed=7)
    else:
        configs, log_q = fb2.cutset_proposal(roots, 16, seed=7)
    h_ee, h_ed, lz2 = fb2.cutset_gradient(configs, log_q)
    assert torch.equal(g_ee, h_ee) and torch.equal(g_ed, h_ed) and torch.equal(log_z_hat, lz2)
    assert torch.isfinite(g_ee).all() and torch.isfinite(g_ed).all() and torch.isfinite(log_z_hat).all()
    ref = fb2.cutset_estimate(configs=configs, log_q=log_q)[0]
    assert ((log_z_hat - ref).abs() <= 1e-10 * ref.abs().clamp(min=1.0)).all()
    if proposal == 'messages':                                  # roots=None: the messages as they stand
        k_ee, _, _ = fb.estimate_gradient(None, n_list=16, seed=7)
        assert torch.equal(g_ee, k_ee)


def test_trainers_estimate_every_shape_of_the_clique_fixture(tmp_path):
    """K1 to K12 at X = 64: UserGraphTrainer.estimated_gradient() answers for every shape and is the batch's cutset_gradient() on
    the documented list; estimated_step() takes the exact gradient where the exact call exists and the estimate elsewhere, skips
    nothing and falls back to nothing; the report's totals are the sums."""
    from test_gpu_cliques import _trainer
    from macaronicusermodeling_amd import exactgrad as K
    from macaronicusermodeling_amd.train import apply_update
    gold = tidir_gold('tidir_cliques_reference')
    paths = write_tidir(gold, str(tmp_path))
    tt = _trainer(paths, gold)
    N, seed = 8, 21
    F_ee, F_ed = tt.theta_en_en.numel(), tt.theta_en_de.numel()
    grad, est_all, loglik, n_est, seen, sizes = np.zeros(F_ee + F_ed), np.zeros(F_ee + F_ed), 0.0, 0, 0, set()
    for i, (key, tr) in enumerate(tt.trainers.items()):
        g_ee, g_ed, joint_hat, log_z_hat = tr.estimated_gradient(n_list=N, seed=seed + i)
        B = tr.batch.B
        assert g_ee.shape == (B, F_ee) and g_ed.shape == (B, F_ed) and joint_hat.shape == log_z_hat.shape == (B,)
        assert np.isfinite(g_ee).all() and np.isfinite(g_ed).all() and np.isfinite(joint_hat).all()
        tr.build_potentials()
        roots = tr.roots[:tr.n_sweeps_run]
        _, joint_bp = tr.batch.log_partition(roots, init=True, labels=tr.batch._labels)
        configs, log_q = tr.batch.cutset_draw(N, seed=seed + i)
        b_ee, _, b_lz = tr.batch.cutset_gradient(configs, log_q)
        assert np.array_equal(b_ee.cpu().numpy(), g_ee) and np.array_equal(b_lz.cpu().numpy(), log_z_hat)
        est_all += np.concatenate([g_ee.sum(axis=0), g_ed.sum(axis=0)])
        sizes.add(len(key[1]))
        seen += B
        try:
            x_ee, x_ed, joint, _, _ = tr.exact_gradient()
            assert len(key[1]) <= 4
            if len(key[1]) == 1:                                # a tree: one configuration, and the estimate is the exact gradient
                assert np.abs(g_ee - x_ee).max() <= 1e-10 and np.abs(g_ed - x_ed).max() <= 1e-10 and np.abs(joint_hat - joint).max() <= 1e-9
        except K.ExactGradError:
            assert len(key[1]) >= 5
            x_ee, x_ed, joint = g_ee, g_ed, joint_hat
            n_est += B
        grad += np.concatenate([x_ee.sum(axis=0), x_ed.sum(axis=0)])
        loglik += float(joint.sum())
    assert max(sizes) >= 12 and {5, 8} <= sizes and min(sizes) <= 4 and n_est
    report = tt.estimated_gradient_report(n_list=N, seed=seed)
    assert np.abs(report[0] - est_all).max() <= 1e-12 * max(1.0, np.abs(est_all).max()) and report[6] == seen and report[7] == seen - n_est
    print('estimate against exact on %d instances: cosine %.6f, relative distance %.3e (recorded, not asserted)' % (report[7], report[3], report[4]))
    before_ee, before_ed = tt.theta_en_en.clone(), tt.theta_en_de.clone()
    mean_ll, n_estimated = tt.estimated_step(0.01, 0.1, n_list=N, seed=seed)
    want = torch.from_numpy(np.concatenate([grad, [loglik, float(seen)]])).to(tt.device)
    apply_update(before_ee, before_ed, want, F_ee, F_ed, 0.01, 0.1)
    assert n_estimated == n_est and abs(mean_ll - loglik / seen) <= 1e-12 * abs(mean_ll)
    assert (tt.theta_en_en - before_ee).abs().max().item() <= 1e-13 and (tt.theta_en_de - before_ed).abs().max().item() <= 1e-13
    with pytest.raises(K.ExactGradError, match='configurations'):
        tt.exact_step(0.01, 0.1)                                # (what exact_step() refuses it still refuses)


def test_estimated_step_on_exact_shapes_is_exact_step_bit_for_bit(tmp_path):
    """A file of K3 and K4 shapes only: estimated_step() gives exact_step()'s thetas, every bit."""
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    a, _, _, _ = E._trainer(tmp_path / 'a', n_instances=12, X=16, Vde=16, sent_len=(5, 7), n_predicted=(3, 4), seed=5)
    b, _, _, _ = E._trainer(tmp_path / 'b', n_instances=12, X=16, Vde=16, sent_len=(5, 7), n_predicted=(3, 4), seed=5)
    assert sorted({tr.topo.n_vars for tr in a.trainers.values()}) == [3, 4]
    ll_a, fell = a.exact_step(0.025, 0.1)
    ll_b, n_estimated = b.estimated_step(0.025, 0.1, n_list=8, seed=3)
    assert fell == 0 and n_estimated == 0 and ll_a == ll_b
    assert torch.equal(a.theta_en_en.view(torch.int64), b.theta_en_en.view(torch.int64))
    assert torch.equal(a.theta_en_de.view(torch.int64), b.theta_en_de.view(torch.int64))
