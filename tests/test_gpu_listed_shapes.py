"""The listed modes of the four exact cutset libraries on every forest shape the shared walk (csrc/mlbp_cutset_walk.h) branches
on, on the GPU: cutset_map (exactmap), cutset_mbest (exactmbest), cutset_resample (exactsample) and cutset_gradient /
cutset_pair_marginals (exactgrad) on each family of tests/test_walk_shapes_cpu.py at X = 64 (the wave-per-entry kernels with
their listed loops of their own; unary13 falls to the generic kernel by the LDS rule, the caterpillar is never on it) and once
more at a small odd X on the generic kernel, over the three lists of tests/test_listed_shapes_cpu.py: the full list in index
order with log_q = 0, a short one of seven entries with two repeats in arbitrary order under a proposal that is no distribution,
and its first entry alone.  tests/test_gpu_walk_shapes.py holds the exact calls on the same shapes; before this module the listed
loops had run on K_n, one ring, a chain and a star.

What a listed loop meets here that K_n never shows it (tests/test_walk_shapes_cpu.py asserts the plans):

  star2, diamond         a parent with two children: the sibling product of x64_down_step / generic_down reached from the listed
                         loop, ROW and COL cutset-incident items on siblings (diamond), and -- star2, diamond, bowtie,
                         two_edges_and_a_loner at X = 64 -- the second R[f] slot of exactgrad_x64_kernel<2>, under 64 listed
                         configurations on diamond and bowtie.
  bowtie                 two roots: Alg::root twice per entry; two_edges_and_a_loner three, one without a forest factor.
  star2, two_edges..,    n_cut == 0 with N = 7 and N = 1: exactmap and exactmbest select the listed loop by configs != NULL, which
  unary12 / unary13      is NULL here, so the exact loop walks N entries of the one empty configuration; exactgrad and exactsample
                         select by `listed`.  Entry 0 is reported, no uniform is spent on an entry.
  pair2                  n_forest == 0 with a cutset: no table in LDS, every item cutset-incident.
  pair2 under [0, 1]     n_free == 0: both walk loops empty, the constants alone; the ranked list is as long as the distinct rows
                         (five, four and one: shorter than m on `one` and on short at X = 5).
  k3_two_cut             two cutset variables: X64Packed's second lane, a constant inside the cutset.
  unary12 / unary13      P == 0: pair_tables NULL, pm of shape (B, 0, X, X).
  caterpillar (cut 5)    the hub below a root on the generic kernel, from EntryStates / ListedStates / DrawnStates.
  ragged lists           diamond at X = 64, B = 100, N = 29: 24 walkers (12 in exactgrad) with unequal shares.
  a refused list         diamond: a state of X in the last row of graph 0's short list is refused before it selects a row or a
                         cell; graph 1 keeps its bits.

Breaking one arithmetic line of a listed loop on a scratch copy (no index or address touched) makes these fail, run once each
(LAB_NOTES R36.3; every test named is [<case>-x64], none at the small X fails: the breaks are in the X = 64 kernels):
  exactgrad_x64_kernel, listed loop: the rank-1 update's v0 / v1 swapped -- test_estgrad at star2, diamond, bowtie,
      two_edges_and_a_loner (the four two-slot cases) and test_ragged_estgrad;
  the same loop: `+= wm` of the cutset-incident rows dropped -- test_estgrad at diamond, bowtie, pair2, k3_two_cut and
      test_ragged_estgrad;
  the same loop: `+= w` of the factors inside the cutset dropped -- test_estgrad at pair2_cut01 and k3_two_cut;
  the same loop: weighted(z, pf) skipped -- test_estgrad at every X = 64 case on that kernel (star2, diamond, bowtie,
      two_edges_and_a_loner, pair2, pair2_cut01, k3_two_cut, unary12) and test_ragged_estgrad;
  exactmap_x64_kernel, listed loop: X64Packed{0} for the entry's states -- test_searchmap and test_searchmbest (its row 0 is
      cutset_map's) at diamond, bowtie, pair2, pair2_cut01, k3_two_cut and test_ragged_searchmap_and_searchmbest;
  exactmbest_values_x64_kernel, listed loop: X64Packed{0} -- test_searchmbest at the same five cases and the ragged test;
  exactsample's X = 64 weights kernel, listed loop: X64Packed{0} -- test_resample at the same five cases and test_ragged_resample.

Bars: each library's own listed GPU module's, through that module's own _run and comparison, none new -- assignments, entries,
rows and draws equal, scores at rtol 1e-12, logp / log_z_hat / ess at rtol 1e-10, log_z_hat, marginals and pair marginals of the
gradient within 1e-10 of the statement and of cutset_estimate().  The discrete outputs are compared exactly because
tests/test_listed_shapes_cpu.py asserts the 1e-6 nat leads and gaps and the 1e-8 margin on the reference for every (case, X, list)
used here: none is exempted.  On the full list the listed call is held to the exact call's bits on the same device."""
import numpy as np
import pytest

import test_exactmbest_cpu as SB
import test_gpu_estgrad as LEG
import test_gpu_exactgrad as GG
import test_gpu_exactmap as GM
import test_gpu_exactmbest as GB
import test_gpu_resample as LRG
import test_gpu_searchmap as LSM
import test_gpu_searchmbest as LSB
import test_listed_shapes_cpu as L
import test_resample_cpu as LR
import test_walk_shapes_cpu as T
from oracle import lbp_oracle as O
from test_gpu_walk_shapes import _ragged_tables

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

RUNS = T.runs()
X64, GENERIC = 1, 2
TWO_SLOTS = ('star2', 'diamond', 'bowtie', 'two_edges_and_a_loner')


def _kernel(case, X):
    """The walk kernel the run must take: KERNEL_X64 at X = 64 for all but unary13 (and the caterpillar, which is not run there)."""
    return X64 if X == 64 and case != 'unary13' else GENERIC


def _given(case):
    """The cutset argument of the call: None (cutset.choose) or the case's variable ids."""
    return T.CASES[case][1]


def _name(case, X, name):
    return '%s X = %d %s' % (case, X, name)


def _numbers(x, cut_pos, X):
    """The configuration number of every row of x [...][n_vars]: digit q is the state of cut position q."""
    return sum((x[..., p].astype(np.int64) * X ** q for q, p in enumerate(cut_pos)), np.zeros(x.shape[:-1], dtype=np.int64))


def _cut_pos(spec, case):
    order = list(O.Graph(spec).var_order)
    return [order.index(v) for v in T.cut_of(case)]


# ---- exactmap -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', RUNS, ids=T.run_id)
def test_searchmap(run):
    """cutset_map(entry=True): the full list is exact_map()'s bits with the configuration number as entry; the short list and
    the single entry are the statement's assignment and entry, the score at rtol 1e-12 (LSM._compare)."""
    case, X = run
    spec, inputs = T.inputs_of(case, X)
    g, kernel = O.Graph(spec), LSM.X64 if _kernel(case, X) == X64 else LSM.GENERIC
    fb = GM._batch(spec, inputs)
    for name in L.LISTS:
        configs = L.lists_of(case, X)[name][0]
        got = LSM._run(fb, list(configs), kernel=kernel, cutset=_given(case))
        if name == 'full':
            x, score = fb.exact_map(cutset=_given(case))
            assert np.array_equal(got['x'], x.cpu().numpy()) and np.array_equal(got['score'], score.cpu().numpy()), (case, X)
            assert np.array_equal(got['entry'], _numbers(got['x'], _cut_pos(spec, case), X))
        LSM._compare(_name(case, X, name), got, g, L.refs_map(case, X, name))
        if not T.cut_of(case):
            assert (got['entry'] == 0).all()


# ---- exactmbest -----------------------------------------------------------------------------------------
def _mbest_kernels(case, X, m):
    """(values, lists): the values kernel of the run and the lists kernel by the header's rule (test_exactmbest_cpu.lists_rule)."""
    return _kernel(case, X), SB.lists_rule(*L.shape_of(case, X), m)


@pytest.mark.parametrize('run', RUNS, ids=T.run_id)
def test_searchmbest(run):
    """cutset_mbest(entries=True) for m = 1 and 5: the full list is exact_mbest(m)'s bits in rows, scores and n_found with the
    configuration numbers as entries; the other lists are the statement's rows and entries, scores at rtol 1e-12, -1 / -inf behind
    n_found (LSB._compare); row 0 is cutset_map()'s bits on the same list."""
    case, X = run
    spec, inputs = T.inputs_of(case, X)
    fb = GB._batch(spec, inputs)
    for name in L.LISTS:
        configs = L.lists_of(case, X)[name][0]
        x0, score0, entry0 = (t.cpu().numpy() for t in fb.cutset_map(LSB._configs(fb, list(configs)), cutset=_given(case), entry=True))
        for m in L.M_VALUES:
            got = LSB._run(fb, list(configs), m, kernels=_mbest_kernels(case, X, m), cutset=_given(case))
            LSB._compare('%s m = %d' % (_name(case, X, name), m), got, L.refs_mbest(case, X, name), m)
            assert np.array_equal(got['x'][:, 0], x0) and np.array_equal(got['score'][:, 0], score0) and np.array_equal(got['entries'][:, 0], entry0)
            if name == 'full':
                x, score, n = (t.cpu().numpy() for t in fb.exact_mbest(m, cutset=_given(case)))
                assert np.array_equal(got['x'], x) and np.array_equal(got['score'], score) and np.array_equal(got['n'], n), (case, X, m)
                assert (n == m).all() and np.array_equal(got['entries'], _numbers(got['x'], _cut_pos(spec, case), X))
            if case == 'pair2_cut01' and name == 'one':
                assert (got['n'] == 1).all() and ((got['x'][:, 1:] == -1).all() and (got['score'][:, 1:] == -np.inf).all())


def test_both_lists_kernels_were_asked_for():
    """(values, lists) over the X = 64 runs and m = 1, 5: the X = 64 pair, the generic lists pass behind the X = 64 values pass,
    and the generic pair (unary13)."""
    seen = {_mbest_kernels(case, X, m) for case, X in RUNS if X == 64 for m in L.M_VALUES}
    assert seen == {(X64, X64), (X64, GENERIC), (GENERIC, GENERIC)}


# ---- exactsample ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', RUNS, ids=T.run_id)
def test_resample(run):
    """cutset_resample(uniforms=..., log_z, score, entry, ess): the full list with log_q = 0 is exact_sample()'s bits in samples
    and logp; the other lists are the statement's samples and entries, logp, log_z_hat, score and ess at that module's bars
    (LRG._compare, LRG._identity).  Without cutset variables: entry 0, exact_sample()'s draws on the same uniforms -- none is
    spent on an entry -- and log_z_hat = log Z + ln mean exp(-log_q)."""
    case, X = run
    spec, inputs = T.inputs_of(case, X)
    cut = T.cut_of(case)
    u = L.uniforms_of(case, X)
    fb = LRG._batch(spec, inputs)
    ex, elogp, elog_z, escore = (t.cpu().numpy() for t in fb.exact_sample(n_samples=u.shape[0], uniforms=LRG._dev(fb, u), cutset=_given(case),
                                                                          log_z=True, score=True))
    for name in L.LISTS:
        configs, log_q = L.lists_of(case, X)[name]
        runs = L.refs_resample(case, X, name)
        LR.check_margin(_name(case, X, name), runs)             # the CPU module asserts it too: before the device is looked at
        got = LRG._run(fb, configs, log_q, u, kernel=_kernel(case, X), cutset=_given(case))
        LRG._compare(_name(case, X, name), got, runs)
        LRG._identity(got, log_q, len(cut))
        if name == 'full' or not cut:
            assert np.array_equal(got['x'], ex) and np.array_equal(got['logp'], elogp) and np.array_equal(got['score'], escore), (case, X, name)
        if name == 'full':
            assert np.array_equal(got['entry'], _numbers(got['x'], _cut_pos(spec, case), X))
            np.testing.assert_allclose(got['log_z_hat'], elog_z - np.log(configs.shape[1]), rtol=1e-12)
        if not cut:
            assert (got['entry'] == 0).all()
            np.testing.assert_allclose(got['log_z_hat'], elog_z + np.log(np.exp(-log_q).mean(axis=1)), rtol=1e-10)


# ---- exactgrad ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', RUNS, ids=T.run_id)
def test_estgrad(run):
    """cutset_gradient / cutset_pair_marginals (LEG._run: the full call, then the lean ones, which must repeat its bits).  The
    full list: every normalised output has the exact calls' bits (GG._run), log_z_hat = log_z - ln N at 1e-12.  The other lists:
    the statement and cutset_estimate() at 1e-10, rows and columns of every M_p and the contraction with the features (LEG
    ._against_statement, LEG._against_estimate)."""
    case, X = run
    spec, inputs = T.inputs_of(case, X)
    cut = T.cut_of(case)
    fb = GG._batch(spec, inputs, seed=5)
    for name in L.LISTS:
        configs, log_q = L.lists_of(case, X)[name]
        got = LEG._run(fb, configs, log_q, kernel=_kernel(case, X), cutset=_given(case))
        assert got['pm'].shape == (len(inputs), fb.topo.P, X, X) and got['kernel'] == _kernel(case, X)
        if X == 64 and _kernel(case, X) == X64:                 # exactgrad_x64_kernel<max(n_forest, 1)>
            assert (T.CASES[case][4] == 2) == (case in TWO_SLOTS) and T.CASES[case][4] <= 2
        if name == 'full':
            exact = GG._run(fb, cutset=_given(case), kernel=GG.X64_1 if _kernel(case, X) == X64 else GG.GENERIC)
            for key in LEG.NORMALISED:
                assert np.array_equal(got[key], exact[key]), (case, X, key)
            want = exact['log_z'] - np.log(configs.shape[1])
            assert (np.abs(got['log_z'] - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all()
        LEG._against_statement(_name(case, X, name), fb, inputs, cut, configs, log_q, got)
        LEG._against_estimate(fb, configs, log_q, got, cutset=_given(case))


# ---- ragged listed walkers --------------------------------------------------------------------------------
def _ragged():
    """diamond at X = 64, B = T.RAGGED_B, three graphs' tables and lists at positions b % 3."""
    B = T.RAGGED_B
    spec, inputs, tables, ptab, utab, _, index = _ragged_tables(B)
    configs, log_q, u = L.ragged_lists()
    walkers = L.ragged_walkers(B, L.RAGGED_N)
    assert all(1 < w < L.RAGGED_N and L.RAGGED_N % w != 0 for w in walkers.values()), walkers
    return B, spec, inputs, (tables, ptab, utab), index, configs[index], log_q[index], np.ascontiguousarray(u[:, index])


def _repeats(got, keys, index, axis=0):
    for key in keys:
        a = np.moveaxis(got[key], axis, 0) if got[key].ndim > axis else got[key]
        for b in range(3, len(index)):
            assert np.array_equal(a[b], a[index[b]], equal_nan=False), (key, b)


def _first(got, n=3, axis=0):
    return {k: (np.take(v, range(n), axis=axis) if isinstance(v, np.ndarray) and v.ndim > axis else v) for k, v in got.items()}


def test_ragged_searchmap_and_searchmbest():
    """24 wave-walkers for 29 entries: five walk two, nineteen one.  Positions b >= 3 repeat the bits of b % 3; positions 0 to 2
    against the statement."""
    B, spec, inputs, (tables, ptab, utab), index, configs, _, _ = _ragged()
    g = O.Graph(spec)
    tops, ranked, _ = L.ragged_refs()
    fb = GM._batch(spec, inputs, tables, ptab, utab, B=B)
    got = LSM._run(fb, list(configs), kernel=LSM.X64)
    LSM._compare('diamond X = 64 B = %d' % B, _first(got), g, tops)
    _repeats(got, ('x', 'score', 'entry'), index)
    for m in L.M_VALUES:
        lists = LSB._run(fb, list(configs), m, kernels=_mbest_kernels('diamond', 64, m))
        LSB._compare('diamond X = 64 B = %d m = %d' % (B, m), _first(lists), ranked, m)
        _repeats(lists, LSB.KEYS, index)
        assert np.array_equal(lists['x'][:, 0], got['x']) and np.array_equal(lists['score'][:, 0], got['score'])


def test_ragged_resample():
    B, spec, inputs, (tables, ptab, utab), index, configs, log_q, u = _ragged()
    _, _, runs = L.ragged_refs()
    LR.check_margin('diamond X = 64 ragged', runs)
    fb = LRG._batch(spec, inputs, tables, ptab, utab, B=B)
    got = LRG._run(fb, configs, log_q, u, kernel=X64)
    LRG._compare('diamond X = 64 B = %d' % B, got, [runs[i] for i in index])
    LRG._identity(got, log_q, 1)
    _repeats(got, ('x', 'logp', 'score', 'entry'), index, axis=1)
    _repeats(got, ('log_z_hat', 'ess'), index)


def test_ragged_estgrad():
    """12 wave-walkers for 29 entries in libmlbp_exactgrad.so, whose walkers also hold the two forest factors' accumulators."""
    B, spec, inputs, (tables, ptab, utab), index, configs, log_q, _ = _ragged()
    fb = GG._batch(spec, inputs, tables, ptab, utab, seed=6)
    got = LEG._run(fb, configs, log_q, kernel=X64)
    LEG._against_statement('diamond X = 64 B = %d' % B, fb, inputs, T.cut_of('diamond'), configs, log_q, got, graphs=range(3))
    LEG._against_estimate(fb, configs, log_q, got)
    _repeats(got, ('log_z', 'marg', 'pm'), index)               # (expect_* and grad_* read the position's own columns and labels)


# ---- one refused graph on a forest with siblings -----------------------------------------------------------
@pytest.mark.parametrize('X', [64, 5])
def test_one_refused_graph(X):
    """diamond: a state of X in the last row of graph 0's short list.  Graph 0 is refused as each header says -- assignment -1,
    score NaN, entry -1; n_found -1, rows -1, scores NaN, entries -1; samples -1, entry -1 and NaN; log_z_hat and the features NaN
    with the tensors left as they were --, graph 1 keeps the bits of the clean call."""
    case = 'diamond'
    spec, inputs = T.inputs_of(case, X)
    kernel = _kernel(case, X)
    clean, log_q = L.lists_of(case, X)['short']
    bad, _ = L.refused_lists(X)
    assert (bad[0] >= X).sum() == 1 and (bad[1] < X).all() and (bad >= 0).all()
    u = L.uniforms_of(case, X)
    # exactmap
    fb = GM._batch(spec, inputs)
    base = LSM._run(fb, list(clean), kernel=LSM.X64 if kernel == X64 else LSM.GENERIC)
    got = LSM._run(fb, list(bad), kernel=LSM.X64 if kernel == X64 else LSM.GENERIC)
    assert (got['x'][0] == -1).all() and np.isnan(got['score'][0]) and got['entry'][0] == -1
    assert np.array_equal(got['x'][1], base['x'][1]) and got['score'][1] == base['score'][1] and got['entry'][1] == base['entry'][1]
    # exactmbest
    for m in L.M_VALUES:
        base = LSB._run(fb, list(clean), m, kernels=_mbest_kernels(case, X, m))
        got = LSB._run(fb, list(bad), m, kernels=_mbest_kernels(case, X, m))
        assert got['n'][0] == -1 and (got['x'][0] == -1).all() and np.isnan(got['score'][0]).all() and (got['entries'][0] == -1).all()
        LSB._same_bits(got, base, rows=(1, 1))
    # exactsample
    base = LRG._run(fb, clean, log_q, u, kernel=kernel)
    got = LRG._run(fb, bad, log_q, u, kernel=kernel)
    assert (got['x'][:, 0] == -1).all() and (got['entry'][:, 0] == -1).all() and np.isnan(got['logp'][:, 0]).all() and np.isnan(got['score'][:, 0]).all()
    assert np.isnan(got['log_z_hat'][0]) and np.isnan(got['ess'][0])
    for key in ('x', 'logp', 'score', 'entry'):
        assert np.array_equal(got[key][:, 1], base[key][:, 1]), key
    assert got['log_z_hat'][1] == base['log_z_hat'][1] and got['ess'][1] == base['ess'][1]
    # exactgrad
    fg = GG._batch(spec, inputs, seed=5)
    base = LEG._run(fg, clean, log_q, kernel=kernel)
    got = LEG._run(fg, bad, log_q, kernel=kernel, fill=-7.0)
    assert np.isnan(got['log_z'][0]) and (got['marg'][0] == -7.0).all() and (got['pm'][0] == -7.0).all()
    for key in LEG.KEYS[3:]:
        assert np.isnan(got[key][0]).all(), key
    for key in LEG.KEYS:
        assert np.array_equal(got[key][1], base[key][1]), key
