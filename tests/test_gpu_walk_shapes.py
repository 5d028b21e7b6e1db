"""The six cutset-conditioning libraries on every forest shape the shared walk (csrc/mlbp_cutset_walk.h) branches on, on the
GPU, against the float64 references of tests/test_walk_shapes_cpu.py: cutset, exactmap, exactgrad, exactsample, exactmbest and
cutsetis on each family at X = 64 (the wave-per-configuration kernels; unary13 falls to the generic kernel by the LDS rule, the
caterpillar is never on it) and once more at a small odd X on the generic kernel.

The walk path each family reaches (tests/test_walk_shapes_cpu.py asserts the plan that leads there):

  star2, diamond         a parent with two children: the loop "the parent's other children" of x64_down_step (X = 64) and of
                         generic_down (small X) multiplies the sibling's `up` into a child's downward message; in the max and
                         list forms the second child is folded into a parent that holds the first.
  bowtie                 two roots at X = 64 and small X: mul(z, Alg::root(x)) twice in x64_up, the block sum twice in generic_up,
                         parent == {-1, -1} in the middle of `order`.
  two_edges_and_a_loner  three roots, one without a forest factor; one configuration: waves 1 to 3 of the X = 64 workgroup walk
                         nothing and their partials are empty.
  star2 (variable 0)     a free variable with an empty item range: base == 1.
  pair2                  n_forest == 0 under [0] (no table in LDS, a cutset variable without a unary factor); n_free == 0 under
                         [0, 1]: both walk loops empty, Z_c the product of the constants alone.
  k3_two_cut             one free variable, no forest, 4096 configurations.
  unary12 / unary13      P == 0: pair_tables NULL, every variable a root; 12 variables are the X = 64 kernel's last, 13 the
                         generic kernel's by the table-free term of the LDS rule.
  caterpillar (cut 5)    a hub below a root on the generic kernel: dn[par] and the siblings' up in one product.
  ragged chunks          diamond at X = 64 with B = 100: 24 walkers for 64 configurations -- some take three, some two.

Breaking a line of the walk on a scratch copy makes these fail (run once each, LAB_NOTES R26.3): the sibling product of
x64_down_step -- test_cutset, test_exactmap, test_exactgrad, test_cutsetis [star2-x64] and [diamond-x64] and both
test_ragged_chunks_*; the sibling product of generic_down -- the same four at [star2-x5], [diamond-x5], [caterpillar_cut5-x5];
every Alg::root of x64_up but the last -- those four and test_exactsample at [bowtie-x64], [two_edges_and_a_loner-x64],
[unary12-x64]; the same in generic_up -- the five at the small sizes of bowtie, two_edges_and_a_loner, caterpillar, unary12,
unary13 and at [unary13-x64]; the sibling product below a grandparent in generic_down -- the four at [caterpillar_cut5-x5].
exactsample has no pass down and exactmbest folds lists in passes of its own: their sibling handling is held by the states and
rows of the same families.

Bars: each library's own GPU module's, through that module's own comparison (its _compare), none new -- cutset, exactgrad and
cutsetis 1e-10 (log Z relative to max(1, |log Z|), marginals and pair marginals absolute); exactmap and exactmbest rows equal,
scores at rtol 1e-12, max-marginals at 1e-10; exactsample states equal, logp and log Z at rtol 1e-10.  Rows, lists and draws
are compared exactly because tests/test_walk_shapes_cpu.py asserts the gap and the margin on the reference for every input used
here: no graph is exempted.  No header refuses any of these shapes; none is expected to be refused here."""
import numpy as np
import pytest

import test_gpu_cutset as GC
import test_gpu_cutsetis as GI
import test_gpu_exactgrad as GG
import test_gpu_exactmap as GM
import test_gpu_exactmbest as GB
import test_gpu_exactsample as GS
import test_walk_shapes_cpu as T
from helpers import batch_tables
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

RUNS = T.runs()
X64, GENERIC = 1, 2


def _kernel(case, X):
    """The walk kernel the run must take: KERNEL_X64 at X = 64 for all but unary13 (and the caterpillar, which is not run there)."""
    return X64 if X == 64 and case != 'unary13' else GENERIC


def _given(case):
    """The cutset argument of the call: None (cutset.choose) or the case's variable ids."""
    return T.CASES[case][1]


def _name(case, X):
    return '%s X = %d' % (case, X)


# ---- cutset ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', RUNS, ids=T.run_id)
def test_cutset(run):
    """exact_inference(labels, marginals): log_z, marginals, joint_logp, rows summing to 1 (GC._compare)."""
    case, X = run
    spec, inputs = T.inputs_of(case, X)
    fb = GC._batch(spec, inputs)
    labels = GC._labels(fb, 3)
    got = GC._run(fb, labels=labels, cutset=_given(case), kernel=GC.X64 if _kernel(case, X) == X64 else GC.GENERIC)
    GC._compare(_name(case, X), got, T.refs_cutset(case, X), labels, (O.Graph(spec), inputs))


# ---- exactmap -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', RUNS, ids=T.run_id)
def test_exactmap(run):
    """exact_map with and without max-marginals: assignment, score, max-marginals (GM._compare)."""
    case, X = run
    spec, inputs = T.inputs_of(case, X)
    got = GM._both(GM._batch(spec, inputs), cutset=_given(case), kernel=GM.X64 if _kernel(case, X) == X64 else GM.GENERIC)
    GM._compare(_name(case, X), got, O.Graph(spec), T.refs_map(case, X))


# ---- exactgrad ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', RUNS, ids=T.run_id)
def test_exactgrad(run):
    """exact_pair_marginals() and the node marginals and log Z of the same walk, every pairwise factor -- forest edges,
    cutset-incident ones, the constants of pair2 under [0, 1] -- and the expected features of the returned tensors
    (GG._run, GG._compare)."""
    case, X = run
    spec, inputs = T.inputs_of(case, X)
    fb = GG._batch(spec, inputs, seed=5)
    got = GG._run(fb, cutset=_given(case), kernel=GG.X64_1 if _kernel(case, X) == X64 else GG.GENERIC)
    assert got['pm'].shape == (len(inputs), fb.topo.P, X, X)
    GG._compare(_name(case, X), fb, got, T.refs_pairs(case, X))


# ---- exactsample ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', RUNS, ids=T.run_id)
def test_exactsample(run):
    """exact_sample(uniforms=...): the statement's states, logp, log_z and score; logp is exact_inference's joint_logp
    (GS._compare, GS._identity); log_z also against the sums' reference."""
    case, X = run
    spec, inputs = T.inputs_of(case, X)
    uniforms, walks, stmts = T.refs_sample(case, X)
    T.SS.check_margin(_name(case, X), walks)                    # asserted in the CPU module too: before the device is looked at
    fb = GS._batch(spec, inputs)
    got = GS._run(fb, uniforms, cutset=_given(case), kernel=_kernel(case, X))
    GS._compare(_name(case, X), spec, inputs, got, walks, stmts)
    GS._identity(_name(case, X), fb, got, cutset=_given(case))
    np.testing.assert_allclose(got['log_z'], [z for z, _ in T.refs_cutset(case, X)], rtol=1e-10)


# ---- exactmbest -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', RUNS, ids=T.run_id)
def test_exactmbest(run):
    """exact_mbest(m) for m = 1 and 5: rows, scores, n_found (GB._compare); row 0 is exact_map's assignment and score."""
    case, X = run
    spec, inputs = T.inputs_of(case, X)
    g = O.Graph(spec)
    fb = GB._batch(spec, inputs)
    x, score = fb.exact_map(cutset=_given(case))
    x, score = x.cpu().numpy(), score.cpu().numpy()
    for m in (1, T.MBEST_M):
        got = GB._run(fb, m, cutset=_given(case), values=_kernel(case, X))
        GB._compare('%s m = %d' % (_name(case, X), m), got, g, inputs, T.refs_mbest(case, X), m)
        assert (got['n'] == m).all()
        assert np.array_equal(got['x'][:, 0], x) and np.array_equal(got['score'][:, 0], score), (case, X, m)


# ---- cutsetis -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', RUNS, ids=T.run_id)
def test_cutsetis(run):
    """cutset_estimate(configs=the full list, log_q=-ln X^|C|): every configuration once, so log_z_hat and the marginals are the
    exact values and ess = (sum Z_c)^2 / sum Z_c^2, the statement's (GI._compare); the empty cutset's list is (1, 0)."""
    case, X = run
    spec, inputs = T.inputs_of(case, X)
    configs, log_q, stated = T.refs_listed(case, X)
    assert configs.shape[1:] == (X ** len(T.cut_of(case)), len(T.cut_of(case)))
    fb = GI._batch(spec, inputs)
    labels = GI._labels(fb, 1)
    got = GI._run(fb, configs, log_q, labels=labels, cutset=_given(case), kernel=GI.X64 if _kernel(case, X) == X64 else GI.GENERIC)
    GI._compare(_name(case, X), got, stated, labels, (O.Graph(spec), inputs))
    worst_z = worst_m = 0.0
    for b, (z, m) in enumerate(T.refs_cutset(case, X)):
        worst_z = max(worst_z, GI._close(got['log_z_hat'][b], z))
        worst_m = max(worst_m, float(np.abs(got['marg'][b] - m).max()))
    print('%s: log_z_hat within %.1e of log Z, marginals within %.1e of the exact ones' % (_name(case, X), worst_z, worst_m))
    assert worst_z <= 1e-10 and worst_m <= 1e-10
    if not T.cut_of(case):
        assert (np.abs(got['ess'] - 1.0) <= 1e-12).all()


# ---- ragged chunks --------------------------------------------------------------------------------------
def _ragged_tables(B):
    """(spec, inputs per batch position, the three graphs' tables, pair_tab, unary_tab, references per batch position)."""
    from macaronicusermodeling_amd.topology import GraphTopology
    spec, inputs, refs = T.ragged()
    topo = GraphTopology.from_spec(spec)
    index = np.arange(B) % len(inputs)
    ptab = np.arange(len(inputs) * topo.P).reshape(-1, topo.P)[index]
    utab = np.arange(len(inputs) * topo.U).reshape(-1, topo.U)[index]
    return spec, [inputs[i] for i in index], batch_tables(spec, topo, inputs), ptab, utab, [refs[i] for i in index], index


def test_ragged_chunks_cutset():
    """B = 100 on diamond at X = 64: C = 6, 24 wave-walkers for 64 configurations, so 16 of them walk three and 8 walk two."""
    from macaronicusermodeling_amd import cutset as S
    B = T.RAGGED_B
    walkers = 4 * S.chunks(B, 64)
    assert S.chunks(B, 64) == 6 and 1 < walkers < 64 and 64 % walkers != 0
    spec, inputs, tables, ptab, utab, refs, index = _ragged_tables(B)
    fb = GC._batch(spec, inputs, tables, ptab, utab, B=B)
    labels = GC._labels(fb, 2)
    got = GC._run(fb, labels=labels, kernel=GC.X64)
    GC._compare('diamond X = 64 B = %d' % B, got, [r[:2] for r in refs], labels, (O.Graph(spec), inputs))
    for key in ('log_z', 'marg'):
        for b in range(3, B):
            assert np.array_equal(got[key][b], got[key][index[b]]), (key, b)


def test_ragged_chunks_exactgrad():
    """The same launch shape in libmlbp_exactgrad.so, whose walkers also hold the forest factors' accumulators."""
    from macaronicusermodeling_amd import exactgrad as M
    B = T.RAGGED_B
    walkers = 4 * M.chunks(B, 64, M.KERNEL_X64)
    assert 1 < walkers < 64 and 64 % walkers != 0
    spec, inputs, tables, ptab, utab, refs, index = _ragged_tables(B)
    fb = GG._batch(spec, inputs, tables, ptab, utab, seed=6)
    got = GG._run(fb, kernel=GG.X64_2)
    GG._compare('diamond X = 64 B = %d' % B, fb, got, refs)
    for key in ('log_z', 'marg', 'pm'):
        for b in range(3, B):
            assert np.array_equal(got[key][b], got[key][index[b]]), (key, b)
