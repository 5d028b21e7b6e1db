"""Exact inference by cutset conditioning on the GPU (libmlbp_cutset.so) against the float64 references of
tests/test_cutset_cpu.py: exhaustive enumeration in the log domain where X^n allows it, NumPy elimination (einsum / matmul) and
the forward algorithm beyond -- each pinned on enumeration there.

Bars: marginals within 1e-10 absolute, log_z within 1e-10 * max(1, |log_z|) -- the project's; the references' own distance
from enumeration is below 1e-12 (asserted in the CPU module), and loopy BP is more than 1e-6 away on the user-shaped graphs
(asserted there too), so the bar tells exact from BP.  Bit-for-bit claims compare graphs at an equal number of chunks: the
header makes a graph's bits a function of the graph and of C = mlbp_cutset_chunks(B, n_configs)."""
import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_logz_cpu as LZ
import test_map_cpu as W
from helpers import batch_tables, tidir_oracle_graph
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

X64 = ('cutset_x64_kernel', ())
GENERIC = ('cutset_generic_kernel', ())
COMBINE = ('cutset_combine_kernel', ())
# kernel -> the tests that launch it (tests/test_cutset_cpu.py holds this against the library's symbol table)
CASES = {
    X64: ['test_k3_x64_against_enumeration', 'test_k4_x64_against_elimination', 'test_both_sides_of_the_x64_lds_budget',
          'test_cutset_override_and_redundant_cutset', 'test_shared_tables_and_batch_position_give_the_same_bits',
          'test_power_of_two_scaling', 'test_wide_range_tables', 'test_zero_nan_inf_tables_bad_index_and_bad_label',
          'test_capture_and_replay', 'test_trees_equal_the_shipped_kernels', 'test_tidir_exactness_report'],
    GENERIC: ['test_small_loopy_graphs', 'test_generic_sizes_on_ring3', 'test_k3_x1024_vectors_in_the_workspace', 'test_chain260_x2',
              'test_both_sides_of_the_x64_lds_budget', 'test_trees_equal_the_shipped_kernels',
              'test_shared_tables_and_batch_position_give_the_same_bits', 'test_zero_nan_inf_tables_bad_index_and_bad_label'],
    COMBINE: ['test_k3_x64_against_enumeration', 'test_k4_x64_against_elimination', 'test_small_loopy_graphs'],
}
KERNEL_OF = {X64: 1, GENERIC: 2}


def _S():
    from macaronicusermodeling_amd import cutset
    return cutset


def _batch(spec, inputs_list, tables=None, pair_tab=None, unary_tab=None, B=None):
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(spec)
    assert topo.var_ids == O.Graph(spec).var_order
    fb = FactorGraphBatch(topo, spec['X'], len(inputs_list) if B is None else B)
    pair, unary = batch_tables(spec, topo, inputs_list) if tables is None else tables
    if topo.P:
        fb.set_pair_tables(pair, pair_tab)
    if topo.U:
        fb.set_unary_tables(unary, unary_tab)
    return fb


def _labels(fb, seed=0):
    return np.random.RandomState(seed).randint(0, fb.X, size=(fb.B, fb.topo.n_vars)).astype(np.int32)


def _run(fb, labels=None, cutset=None, kernel=None):
    marg = torch.full((fb.B, fb.topo.n_vars, fb.X), float('nan'), dtype=torch.float64, device=fb.device)
    out = fb.exact_inference(labels=labels, marginals=marg, cutset=cutset)
    ran = _S().last_kernel()
    torch.cuda.synchronize()
    assert out[1] is marg and out[0].dtype == torch.float64 and tuple(out[0].shape) == (fb.B,)
    if kernel is not None:
        assert ran == KERNEL_OF[kernel], ran
    got = dict(log_z=out[0].cpu().numpy(), marg=marg.cpu().numpy(), kernel=ran)
    if labels is not None:
        got['joint'] = out[2].cpu().numpy()
    return got


def _compare(name, got, refs, labels=None, specs=None):
    """refs: [(log_z, marginals)] per graph; with labels, specs = (g, inputs list) for score - log_z of the reference."""
    worst_z = worst_m = worst_j = 0.0
    for b, (z, m) in enumerate(refs):
        ez = abs(got['log_z'][b] - z) / max(1.0, abs(z))
        em = float(np.abs(got['marg'][b] - m).max())
        worst_z, worst_m = max(worst_z, ez), max(worst_m, em)
        if labels is not None:
            g, inputs = specs
            want = W.score_of(g, inputs[b], dict(zip(g.var_order, (int(x) for x in labels[b])))) - z
            worst_j = max(worst_j, abs(got['joint'][b] - want) / max(1.0, abs(want)))
    print('%s: log_z within %.1e (relative to max(1, |log_z|)), marginals within %.1e, joint_logp within %.1e' % (name, worst_z, worst_m, worst_j))
    assert worst_z <= 1e-10 and worst_m <= 1e-10 and worst_j <= 1e-10, name
    assert np.abs(got['marg'].sum(axis=2) - 1).max() <= 1e-12


def _case(name, spec, seeds, how, kernel, kind='uniform', cutset=None, inputs=None):
    g = O.Graph(spec)
    inputs = [C.make_inputs(spec, s, kind) for s in seeds] if inputs is None else inputs
    refs = [how(g, i)[:2] for i in inputs]
    fb = _batch(spec, inputs)
    labels = _labels(fb, seeds[0])
    got = _run(fb, labels=labels, cutset=cutset, kernel=kernel)
    _compare(name, got, refs, labels, (g, inputs))
    return fb, inputs, refs, got


# ---- against enumeration / elimination ------------------------------------------------------------------
def test_k3_x64_against_enumeration():
    """The X = 64 kernel with one cutset variable: 64 configurations of one forest edge."""
    fb, _, _, _ = _case('k3_x64', R.kn_spec(3, 64), (1, 2, 3), R.enumerate_exact, X64)
    assert _S().chunks(3, 64) == 64
    _case('user_k3_x64', C.user_spec(10, [1, 4, 7], 64, 64, seed=1), (5, 6), R.enumerate_exact, X64)


def test_k4_x64_against_elimination():
    """4096 configurations: 256 chunks per graph and the combine launch."""
    S = _S()
    assert S.chunks(2, 4096) == 256
    _case('k4_x64', R.kn_spec(4, 64), (1, 2), R.eliminate, X64, kind='lognormal')


SMALL = [('ring5_x7', lambda: C.ring_spec(5, 7)),                  # a remainder of four edges
         ('k5_x4', lambda: R.kn_spec(5, 4)),                       # three cutset variables, three internal constants
         ('shuffled_x5', lambda: C.shuffled_ids_spec(5)),
         ('double_pair_x6', lambda: R.double_pair_spec(6)),        # two factors over one pair
         ('forest_x9', lambda: R.forest_spec(9)),                  # two trees and a variable with unary factors only: no cutset
         ('user_p3_x16', lambda: C.user_spec(6, [0, 2, 5], 16, 16))]


@pytest.mark.parametrize('name,make', SMALL, ids=[s[0] for s in SMALL])
def test_small_loopy_graphs(name, make):
    spec = make()
    for kind in ('uniform',) if spec['style'] == 'trainmp' else ('uniform', 'lognormal'):
        _case(name + '/' + kind, spec, (3, 4, 5), R.enumerate_exact, GENERIC, kind=kind)


@pytest.mark.parametrize('X', [2, 257, 301])
def test_generic_sizes_on_ring3(X):
    """X = 2 and the odd sizes past a workgroup's 256 threads (masked tails), vectors in LDS."""
    _case('ring3_x%d' % X, C.ring_spec(3, X), (7, 8), R.enumerate_exact if X == 2 else R.eliminate, GENERIC)


def test_k3_x1024_vectors_in_the_workspace():
    S = _S()
    spec = R.kn_spec(3, 1024)
    assert S.workspace_bytes(1, 1024, 3, 3, 3, 1, 1) == 512 * (3 * 1024 + 2 + 17 * 1024) * 8      # the vectors are in the workspace
    _case('k3_x1024', spec, (9,), R.eliminate, GENERIC)


def test_chain260_x2():
    """259 forest edges at X = 2 against the forward algorithm; the empty cutset, one configuration."""
    spec = C.chain_spec(260, 2)
    assert _S().choose(_batch(spec, [C.make_inputs(spec, 1)]).topo) == []
    _case('chain260_x2', spec, (1, 2), R.chain_forward_backward, GENERIC)


def test_both_sides_of_the_x64_lds_budget():
    """A chain of three at X = 64 keeps its two tables on chip; a chain of four (three tables) streams them."""
    S = _S()
    assert S.pick_kernel(64, 3, 2, 3, 2) == S.KERNEL_X64 and S.pick_kernel(64, 4, 3, 4, 3) == S.KERNEL_GENERIC
    _case('chain3_x64', C.chain_spec(3, 64), (1, 2), R.enumerate_exact, X64)
    _case('chain4_x64', C.chain_spec(4, 64), (1,), R.eliminate, GENERIC)


def test_trees_equal_the_shipped_kernels():
    """On a tree log_partition and sweep are exact: the two libraries agree to 1e-10."""
    for spec, kernel in ((C.chain_spec(3, 64), X64), (C.star_spec(4, 8), GENERIC), (C.chain_spec(5, 8), GENERIC)):
        inputs = [C.make_inputs(spec, s) for s in (1, 2, 3)]
        fb = _batch(spec, inputs)
        got = _run(fb, kernel=kernel)
        fb.initialize()
        log_z = fb.log_partition([fb.topo.var_ids[0]], init=True).cpu().numpy()
        marg = fb.marginals().cpu().numpy()
        assert np.abs(got['log_z'] - log_z).max() <= 1e-10 * max(1.0, np.abs(log_z).max()), spec['name']
        assert np.abs(got['marg'] - marg).max() <= 1e-10, spec['name']


# ---- the cutset is a choice, not a result -----------------------------------------------------------------
def test_cutset_override_and_redundant_cutset():
    spec = R.kn_spec(3, 64)
    inputs = [C.make_inputs(spec, s) for s in (1, 2)]
    fb = _batch(spec, inputs)
    base = _run(fb, kernel=X64)
    other = _run(fb, cutset=[1], kernel=X64)
    assert np.abs(base['log_z'] - other['log_z']).max() <= 1e-12 * max(1.0, np.abs(base['log_z']).max())
    assert np.abs(base['marg'] - other['marg']).max() <= 1e-12
    S = _S()
    with pytest.raises(ValueError):
        fb.exact_inference(cutset=[9])
    with pytest.raises(S.CutsetError, match='cycle'):
        fb.exact_inference(cutset=[])
    spec = C.chain_spec(5, 8)
    fb = _batch(spec, [C.make_inputs(spec, s) for s in (1, 2)])
    base, redundant = _run(fb), _run(fb, cutset=[2, 0])
    assert np.abs(base['log_z'] - redundant['log_z']).max() <= 1e-12 * max(1.0, np.abs(base['log_z']).max())
    assert np.abs(base['marg'] - redundant['marg']).max() <= 1e-12


def test_shared_tables_and_batch_position_give_the_same_bits():
    S = _S()
    for spec, kernel in ((R.kn_spec(3, 64), X64), (C.ring_spec(5, 7), GENERIC)):
        n_configs = spec['X']
        inputs = [C.make_inputs(spec, s) for s in (1, 2, 3, 4)]
        fb = _batch(spec, inputs)
        labels = _labels(fb)
        full = _run(fb, labels=labels, kernel=kernel)
        pair, unary = batch_tables(spec, fb.topo, inputs)
        P, U = fb.topo.P, fb.topo.U
        # two graphs naming one table: graphs 0 and 2 of the shared batch both read the tables of graph 2
        ptab = np.arange(4 * P).reshape(4, P)
        utab = np.arange(4 * U).reshape(4, U)
        ptab[0], utab[0] = ptab[2], utab[2]
        shared = _run(_batch(spec, inputs, (pair, unary), ptab, utab), labels=np.stack([labels[2], labels[1], labels[2], labels[3]]))
        for key in ('log_z', 'marg', 'joint'):
            assert np.array_equal(shared[key][0], full[key][2]) and np.array_equal(shared[key][1:], full[key][1:]), key
        # B = 1 equals the graph inside the batch, at an equal number of chunks
        assert S.chunks(1, n_configs) == S.chunks(4, n_configs) == n_configs
        alone = _run(_batch(spec, inputs[1:2]), labels=labels[1:2], kernel=kernel)
        for key in ('log_z', 'marg', 'joint'):
            assert np.array_equal(alone[key][0], full[key][1]), key


# ---- range ----------------------------------------------------------------------------------------------
def test_power_of_two_scaling():
    """Any table times 2^k, |k| <= 400: no bit of the marginals moves, log_z moves by k ln 2."""
    spec = R.kn_spec(3, 64)
    inputs = [C.make_inputs(spec, s, 'lognormal') for s in (1, 2)]
    fb = _batch(spec, inputs)
    base = _run(fb, kernel=X64)
    pair, unary = batch_tables(spec, fb.topo, inputs)
    P = fb.topo.P
    moves = [({p: k}, {}) for p in range(P) for k in (400, -400)] + [({}, {0: 400}), ({}, {2: -400}), ({0: 37, 1: -5, 2: 400}, {0: -300, 1: 3, 2: 11})]
    for pk, uk in moves:
        p2, u2 = pair.copy(), unary.copy()
        for b in range(2):
            for p, k in pk.items():
                p2[b * P + p] = np.ldexp(p2[b * P + p], k)
            for u, k in uk.items():
                u2[b * fb.topo.U + u] = np.ldexp(u2[b * fb.topo.U + u], k)
        got = _run(_batch(spec, inputs, (p2, u2)), kernel=X64)
        total = sum(pk.values()) + sum(uk.values())
        assert np.array_equal(got['marg'], base['marg']), (pk, uk)
        want = base['log_z'] + total * np.log(2.0)
        assert (np.abs(got['log_z'] - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), (pk, uk, got['log_z'], want)
    spec = C.ring_spec(5, 7)
    inputs = [C.make_inputs(spec, 3)]
    fb = _batch(spec, inputs)
    base = _run(fb, kernel=GENERIC)
    pair, unary = batch_tables(spec, fb.topo, inputs)
    for p in range(fb.topo.P):
        for k in (400, -400):
            p2 = pair.copy()
            p2[p] = np.ldexp(p2[p], k)
            got = _run(_batch(spec, inputs, (p2, unary)), kernel=GENERIC)
            assert np.array_equal(got['marg'], base['marg']), (p, k)
            want = base['log_z'] + k * np.log(2.0)
            assert (np.abs(got['log_z'] - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), (p, k)


def test_wide_range_tables():
    """K3 at X = 64 on exp(20 N(0, 1)) tables -- 170 decades each -- against the log-domain grid."""
    spec = R.kn_spec(3, 64)
    _case('k3_x64_wide', spec, (21, 22), R.enumerate_exact, X64, inputs=[R.wide_inputs(spec, s) for s in (21, 22)])


# ---- edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,make,kernel', [('k3_x64', lambda: R.kn_spec(3, 64), X64), ('ring5_x7', lambda: C.ring_spec(5, 7), GENERIC)],
                         ids=['x64', 'generic'])
def test_zero_nan_inf_tables_bad_index_and_bad_label(name, make, kernel):
    spec = make()
    X = spec['X']
    inputs = [C.make_inputs(spec, s) for s in range(1, 7)]
    fb = _batch(spec, inputs)
    labels = _labels(fb)
    base = _run(fb, labels=labels, kernel=kernel)
    pair, unary = batch_tables(spec, fb.topo, inputs)
    P = fb.topo.P
    p2 = pair.copy()
    p2[0 * P + 1][:] = 0.0                                       # graph 0: an all-zero table
    p2[1 * P + 0][3 % X, 1] = np.nan                             # graph 1: a NaN entry
    p2[2 * P + 2][0, 2 % X] = np.inf                             # graph 2: +inf
    lab = labels.copy()
    lab[4, 1] = X                                                # graph 4: a label outside [0, X)
    fb2 = _batch(spec, inputs, (p2, unary))
    fb2.pair_tab[3, 1] = fb2.pair_tables.shape[0]                # graph 3: a table index outside the array
    marg = torch.full((fb2.B, fb2.topo.n_vars, X), -7.0, dtype=torch.float64, device=fb2.device)
    log_z, _, joint = fb2.exact_inference(labels=lab, marginals=marg)
    torch.cuda.synchronize()
    log_z, joint, marg = log_z.cpu().numpy(), joint.cpu().numpy(), marg.cpu().numpy()
    assert log_z[0] == -np.inf and np.array_equal(marg[0], np.full_like(marg[0], 1.0 / X))
    assert not np.isfinite(log_z[1]) and not np.isfinite(log_z[2])
    assert np.isnan(log_z[3]) and np.isnan(joint[3]) and (marg[3] == -7.0).all()
    assert np.isnan(joint[4]) and log_z[4] == base['log_z'][4] and np.array_equal(marg[4], base['marg'][4])
    assert log_z[5] == base['log_z'][5] and joint[5] == base['joint'][5] and np.array_equal(marg[5], base['marg'][5])


def test_float32_tables_are_refused():
    spec = C.user_spec(10, [1, 4, 7], 256, 64, seed=1)
    fb = _batch(spec, [C.make_inputs(spec, 1)])
    fb.set_pair_tables(fb.pair_tables, dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        fb.exact_inference()


def test_capture_and_replay():
    """After one eager call the call is captured and replayed twice: the bits of the eager call."""
    spec = R.kn_spec(3, 64)
    fb = _batch(spec, [C.make_inputs(spec, s) for s in (1, 2, 3)])
    labels = torch.from_numpy(_labels(fb)).to(fb.device)
    eager = _run(fb, labels=labels, kernel=X64)
    marg = torch.empty(fb.B, fb.topo.n_vars, fb.X, dtype=torch.float64, device=fb.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        log_z, _, joint = fb.exact_inference(labels=labels, marginals=marg)
    for _ in range(2):
        for t in (log_z, joint, marg):
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(log_z.cpu().numpy(), eager['log_z']) and np.array_equal(joint.cpu().numpy(), eager['joint'])
        assert np.array_equal(marg.cpu().numpy(), eager['marg'])


# ---- trainer --------------------------------------------------------------------------------------------
def test_tidir_exactness_report(tmp_path):
    """TiDirTrainer.exactness_report() on the synthetic file of the convergence report's test, with up to five predicted words:
    every instance against its own graph as tidir_oracle_graph builds it -- enumeration up to three predicted words, the
    elimination (pinned on enumeration in the CPU module) at four; K5 at X = 64 needs 64^3 configurations and is listed as
    skipped."""
    from macaronicusermodeling_amd import tidir
    from macaronicusermodeling_amd.train import TiDirTrainer
    paths = tidir.synthesize(str(tmp_path), n_instances=24, X=64, Vde=64, sent_len=(4, 7), n_predicted=(1, 5), seed=9)
    tt = TiDirTrainer(paths['ti'], paths['end'], paths['ded'], paths['phi_pmi'], paths['phi_pmi_w1'], paths['phi_ed'], paths['phi_ped'], sweeps=3)
    phi_ee, phi_w1, phi_ed = tidir.load_features(paths['phi_pmi'], paths['phi_pmi_w1'], paths['phi_ed'], paths['phi_ped'])
    rs = np.random.RandomState(1)
    th_ee, th_ed = rs.randn(1, 3) * 0.6, rs.randn(1, 6) * 0.6
    tt.theta_en_en.copy_(torch.from_numpy(th_ee.reshape(-1)))
    tt.theta_en_de.copy_(torch.from_numpy(th_ed.reshape(-1)))
    want, too_large = {}, {}
    for key, b in tt.buckets.items():
        topo = tt.trainers[key].topo
        for r, row in enumerate(b['rows']):
            if topo.n_vars >= 5:
                too_large[row['index']] = tuple(key[1])
                continue
            g, inputs, roots, _ = tidir_oracle_graph(key, b, r, phi_ee, phi_w1, phi_ed, th_ee, th_ed)
            assert list(g.var_order) == list(topo.var_ids)
            z, m = (R.enumerate_exact if topo.n_vars <= 3 else R.eliminate)(g, inputs)[:2]
            n = tt.trainers[key].n_sweeps_run
            _, msgs, _ = O.run(g.spec, inputs, roots[:n], n, force_loopy=True)
            bp = np.stack([O.marginal(g, msgs, v) for v in g.var_order])
            want[row['index']] = (tuple(key[1]), z, LZ.log_partition(g, inputs, msgs) - z, float(np.abs(bp - m).max()),
                                  bool((bp.argmax(axis=1) == m.argmax(axis=1)).all()))
    assert want and too_large
    per_instance, totals, skipped = tt.exactness_report()
    assert len(per_instance) == 24
    for i, p in enumerate(per_instance):
        if i in too_large:
            assert p == (too_large[i], None, None, None, None)
        elif i not in want:
            assert p == ((), 0.0, 0.0, 0.0, True)
        else:
            positions, z, gap, worst, agrees = want[i]
            assert p[0] == positions and abs(p[1] - z) <= 1e-10 * max(1.0, abs(z)), (i, p, want[i])
            assert abs(p[2] - gap) <= 2e-10 * max(1.0, abs(z)) and abs(p[3] - worst) <= 2e-10 and p[4] == agrees, (i, p, want[i])
    assert totals[0] == len(want) and totals[1] == len(too_large)
    assert abs(totals[2] - sum(abs(w[2]) for w in want.values())) <= 1e-9 * len(want)
    assert abs(totals[3] - max(w[3] for w in want.values())) <= 2e-10 and totals[4] == sum(w[4] for w in want.values())
    assert sorted(s[0] for s in skipped) == sorted(set(too_large.values())) and sum(s[1] for s in skipped) == len(too_large)
    assert all('configurations' in s[2] for s in skipped)
    assert max(w[3] for w in want.values()) > 1e-6             # the three sweeps are visibly not the model's marginals
