"""The three sampling kernel instances of libmlbp_sample.so at their edges: exponent range, size edges of the generic kernel,
the X = 64 kernel's LDS budget, more than 256 variables, bad table entries.  Inputs, references and preconditions are those of
tests/test_sample_edges_cpu.py (parts A to F there); every case calls its `precondition` -- the walk's smallest margin, its
finiteness, for wide tables the floor under its marginal entries -- before the device is looked at.

The rules are test_gpu_sample's: conditional marginals and log q at rtol 1e-10 (atol 1e-300), samples exact, MARGIN 1e-8 and a
cap of 0 on left-out (graph, sample) pairs; drawn states and margins are the walk's.

Mutations these cases are built to catch:
  the scale of a table dropped, or a threshold compared with unscaled data   test_scaling_keeps_every_bit (same bits under 2^k)
  a normalisation that flushes or overflows away from unit magnitude         test_wide_range_tables
  the second pass of a 256-stride loop missing, block_sum with two terms
  per thread, the padding of raw at odd X                                    test_generic_size_edges (X = 301, 257; 2 and 1024)
  LDS beyond 64 KiB addressed wrongly (message slots, partial sums, the
  cached marginal, the clamp states)                                         test_x64_kernel_above_64k_of_lds (real potentials)
  the budget rule handing a graph to the wrong kernel                        test_k8_past_the_lds_budget
  clamp[] filled or read for the first 256 variables only                    test_260_variables
  nan_to_num skipped after a product in one kernel                           test_empty_marginal (with normalised messages a
                                                                             NaN product and a zeroed one both end as the
                                                                             uniform message: test_non_finite_entry pins that)
  "total not positive gives uniform" dropped, for a zero or a NaN total      test_all_zero_table, test_non_finite_entry
  a table read before graph_in_range has refused the graph                   test_table_index_outside_the_table_array"""
import numpy as np
import pytest

import test_gpu_sample as G
import test_sample_edges_cpu as EC

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

# kernel instance -> the tests here that launch it (tests/test_sample_cpu.py holds this against the library's symbol table)
CASES = {
    G.X64_RESIDENT: ['test_scaling_keeps_every_bit', 'test_wide_range_tables', 'test_non_finite_entry', 'test_all_zero_table',
                     'test_empty_marginal', 'test_table_index_outside_the_table_array'],
    G.X64_STREAMED: ['test_scaling_keeps_every_bit', 'test_wide_range_tables', 'test_x64_kernel_above_64k_of_lds',
                     'test_table_index_outside_the_table_array'],
    G.GENERIC: ['test_scaling_keeps_every_bit', 'test_wide_range_tables', 'test_generic_size_edges', 'test_k8_past_the_lds_budget',
                'test_260_variables', 'test_non_finite_entry', 'test_all_zero_table', 'test_empty_marginal',
                'test_table_index_outside_the_table_array'],
}
KEYS = ('x', 'logq', 'cm')


def _launch(name, fb=None):
    """One eager call on the case's batch -> (case, batch, outputs); the kernel is the one the case names."""
    c = EC.case(name)
    if fb is None:
        fb = G._batch(c['spec'], c['inputs'], normalize=c['normalize'])
    got = G._run(fb, c['roots'], c['uniforms'], order=c['order'], given=c['given'])
    assert got['kernel'] == G.KERNEL_OF[c['instance']] == G._S().pick_kernel(c['spec']['X'], fb.topo.n_msgs, fb.topo.n_vars), name
    assert c['instance'] == G.GENERIC or (fb.topo.P <= 3) == (c['instance'] == G.X64_RESIDENT), name
    return c, fb, got


def _against_the_walk(name):
    walks = EC.precondition(name)                              # before the device is looked at
    c, fb, got = _launch(name)
    G._compare(name, fb.topo, got, walks)
    return c, fb, got, walks


def _same_bits(name, a, b, graphs=None):
    """Prints how many entries of the two runs differ before it asserts that none does (floats by their bit patterns)."""
    pairs = {}
    for k in KEYS:
        x, y = (a[k], b[k]) if graphs is None else (a[k][:, graphs], b[k][:, graphs])
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        pairs[k] = (x, y) if k == 'x' else (x.view(np.int64), y.view(np.int64))
        print('%s %s: %d of %d entries differ' % (name, k, int((pairs[k][0] != pairs[k][1]).sum()), x.size))
    for k in KEYS:
        assert np.array_equal(*pairs[k]), (name, k)


# ---- A: power-of-two scaling ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n in EC.CASES if n.startswith('scale_')])
def test_scaling_keeps_every_bit(name):
    """Tables as they are, then times 2^k on the device (test_gpu_exponent_range._scale_: PAIR_K / UNARY_K by graph and slot;
    the unnormalised cases: test_sample_edges_cpu.UNNORM_K): the same samples, log q and conditional marginals bit for bit,
    from the same kernel.  Every marginal is normalised, so log q needs no ln 2 correction."""
    import test_gpu_exponent_range as XR
    c, fb, a, _ = _against_the_walk(name)
    _, kp, ku = EC.exponents(name)
    if c.get('exponents'):
        XR._ldexp_(fb.pair_tables, kp)
        XR._ldexp_(fb.unary_tables, ku)
    else:
        kp_dev, ku_dev = XR._exponents(fb)
        assert np.array_equal(kp_dev, kp) and np.array_equal(ku_dev, ku)          # the CPU twin scaled by the same exponents
        XR._scale_(fb)
    _, _, b = _launch(name, fb)
    assert a['kernel'] == b['kernel']
    _same_bits(name, a, b)


# ---- B: wide-range tables --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n in EC.CASES if n.startswith('wide_')])
def test_wide_range_tables(name):
    """exp(sigma N(0,1)) tables, every graph compared with the walk."""
    c, _, got, _ = _against_the_walk(name)
    assert np.isfinite(got['cm']).all() and np.isfinite(got['logq']).all()
    assert (got['x'] >= 0).all() and (got['x'] < c['spec']['X']).all()


# ---- C: size edges of the generic kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ring3_x301', 'chain3_x257', 'chain3_x2', 'chain2_x1024'])
def test_generic_size_edges(name):
    """X = 301: odd, two passes of every 256-stride loop, raw padded to 302; X = 257: one element in the second pass; X = 2 and
    X = 1024: the ends of the supported range (X = 1025 is refused on the host: tests/test_sample_cpu.py)."""
    c, _, got, _ = _against_the_walk(name)
    assert (got['x'] >= 0).all() and (got['x'] < c['spec']['X']).all()


# ---- D: the X = 64 kernel's LDS budget ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['k7_lds', 'chain28_lds'])
def test_x64_kernel_above_64k_of_lds(name):
    """Random potentials, so LDS addressed wrongly changes the answer.  K7: 126 message slots, 69 664 bytes of dynamic LDS -- the
    partial sums from their third row on, the raw vector, the cached marginal and the clamp states lie beyond 64 KiB.
    chain_spec(28, 64): 136 slots, 74 864 bytes -- the message slots from 128 on lie beyond it as well."""
    _, fb, got, _ = _against_the_walk(name)
    slots, lds, P = {'k7_lds': (126, 69664, 21), 'chain28_lds': (136, 74864, 27)}[name]
    assert got['kernel'] == 1 and (fb.topo.n_msgs, fb.topo.P) == (slots, P)
    assert EC.x64_lds_bytes(fb.topo.n_msgs, fb.topo.n_vars) == lds > 65536
    assert (fb.topo.n_msgs * 512 > 65536) == (name == 'chain28_lds')


def test_k8_past_the_lds_budget():
    """K8 at X = 64: 152 slots, 82 976 bytes > MLBP_SAMPLE_X64_LDS_BYTES, so the generic kernel, with random potentials."""
    _, fb, got, _ = _against_the_walk('k8_generic')
    assert EC.x64_lds_bytes(fb.topo.n_msgs, fb.topo.n_vars) == 82976 > G._S().X64_LDS_BYTES
    assert got['kernel'] == 2 == G._S().pick_kernel(64, fb.topo.n_msgs, fb.topo.n_vars)


# ---- E: more than 256 variables ----------------------------------------------------------------------------------------------
def test_260_variables():
    """chain_spec(260, 2): clamp[] is filled and read beyond the first 256 variables; the reference is the chain recursion of
    tests/test_sample_edges_cpu.py."""
    c, fb, got, _ = _against_the_walk('chain260_x2')
    assert c['reference'] == 'chain' and fb.topo.n_vars == 260 and fb.topo.n_msgs == 1296
    assert (got['x'] >= 0).all() and (got['x'] < 2).all()


# ---- F: bad entries ------------------------------------------------------------------------------------------------------------
def _edit_leaves_the_others_alone(name, clean_name):
    c, _, got, _ = _against_the_walk(name)
    _, _, clean = _launch(clean_name)
    assert np.array_equal(EC.case(clean_name)['uniforms'], c['uniforms'])
    others = [b for b in range(len(c['inputs'])) if b != c['edited']]
    _same_bits('%s, untouched graphs' % name, got, clean, graphs=others)
    assert not np.array_equal(got['cm'][:, c['edited']], clean['cm'][:, c['edited']])
    return c, got


@pytest.mark.parametrize('name', ['nan_k3', 'inf_k3', 'nan_x128', 'inf_x128'])
def test_non_finite_entry(name):
    """NaN or +inf at entry (3, 9) of one pairwise table of graph 2, normalised messages: the graph follows the walk (the emptied
    message becomes uniform, nan_to_num after every product), the other graphs keep the bits of a run without the edit."""
    _, got = _edit_leaves_the_others_alone(name, 'clean_' + name.split('_')[1])
    assert np.isfinite(got['cm']).all() and np.isfinite(got['logq']).all()


@pytest.mark.parametrize('name', ['zero_k3', 'zero_k3_unnormalised', 'zero_x128', 'zero_x128_unnormalised'])
def test_all_zero_table(name):
    """One pairwise table of graph 1 all zero.  Normalised: its messages have no positive total and become uniform.
    Unnormalised: every marginal of the graph is exactly uniform."""
    c, got = _edit_leaves_the_others_alone(name, 'clean_' + name[len('zero_'):])
    if not c['normalize']:
        X = c['spec']['X']
        assert np.array_equal(got['cm'][:, c['edited']], np.full((c['uniforms'].shape[0], 3, X), 1.0 / X))


@pytest.mark.parametrize('name', ['empty_k3', 'empty_x128'])
def test_empty_marginal(name):
    """+inf at entry (3, 9) with unnormalised messages: the marginal's total overflows, every m_i is 0, and include/mlbp_sample.h
    step 4 gives x_v = 0 and log q = -inf; the later variables are drawn as the walk draws them."""
    c, got = _edit_leaves_the_others_alone(name, 'clean_%s_unnormalised' % name.split('_')[1])
    walks = EC.reference(name)[0]
    for s in range(c['uniforms'].shape[0]):
        w = walks[s, c['edited']]
        emptied = [i for i, v in enumerate(sorted(w['cm'])) if not (w['cm'][v] > 0).any()]
        assert emptied and np.isneginf(got['logq'][s, c['edited']])
        assert (got['x'][s, c['edited'], emptied] == 0).all() and (got['cm'][s, c['edited'], emptied] == 0).all()


@pytest.mark.parametrize('name', ['clean_k3', 'clean_k4', 'clean_x128'])
def test_table_index_outside_the_table_array(name):
    """A table index outside the table array, written behind Python's check (one too large in pair_tab, -1 in unary_tab): those
    graphs return -1, NaN and untouched cond_marginals -- graph_in_range refuses them before any table is read -- and every other
    graph keeps its bits."""
    c, fb, clean, _ = _against_the_walk(name)
    B = fb.B
    fb.pair_tab[B - 1, 1] = fb.pair_tables.shape[0]
    fb.unary_tab[1, 0] = -1
    _, _, got = _launch(name, fb)
    for b in (1, B - 1):
        assert (got['x'][:, b] == -1).all() and np.isnan(got['logq'][:, b]).all() and np.isnan(got['cm'][:, b]).all(), b
    _same_bits('%s, graphs that name their own tables' % name, got, clean, graphs=[b for b in range(B) if b not in (1, B - 1)])
