"""The three max-product kernel instances of libmlbp_map.so at their edges: size edges of the generic kernel, the X = 64
kernel's LDS budget, more than 256 variables and factors, ties across passes and waves, the device-side refusal of a bad
table index, bad table entries.  Inputs, references and preconditions are those of tests/test_map_logz_edges_cpu.py (parts A
to G there); every case calls its `precondition` -- the kernel choice, the walk's smallest gap, its finiteness -- before
the device is looked at.

The rules are test_gpu_map._compare's, with nothing new: messages and max-marginals at rtol 1e-10, assignments exact, the score
at rtol 1e-10 at the device's own assignment, no variable left out.  (A graph that the CPU module lists as `tied` holds
max-marginals without a positive total: exactly uniform in the walk and in every correct kernel.  _compare counts such a
graph as left out; the case then compares its assignment with the walk's here, every variable of it, exactly.)

Mutations these cases are built to catch:
  the second pass of a 256-stride loop missing, the padding of raw at odd X      test_generic_size_edges (X = 301, 257; 2, 1024)
  `mm > best` turned into `>=`, the min over lanes or waves into a max           test_tie_rule_across_passes_and_waves
  the assignment copy, xs[] or a score loop for the first 256 entries only       test_260_variables
  LDS above 64 KiB addressed wrongly (message slots 128 and up)                  test_x64_kernel_at_the_top_of_its_lds_budget
  the X = 64 score's unary loop stopped after 64 factors                         test_x64_kernel_at_the_top_of_its_lds_budget[k3_len44]
  the budget rule handing a graph to the wrong kernel                            test_x64_graphs_past_the_lds_budget
  refuse_graph writing something else, or a table read before the refusal        test_table_index_outside_the_table_array
  a maximum that lets a NaN through, or turns +inf into something finite         test_non_finite_entry, test_nan_row
  "total not positive gives uniform" dropped                                     test_all_zero_table, test_nan_row"""
import numpy as np
import pytest

import test_gpu_map as G
import test_map_logz_edges_cpu as EC

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

# kernel instance -> the tests here that launch it (tests/test_map_cpu.py holds this against the library's symbol table)
CASES = {
    G.X64_RESIDENT: ['test_x64_kernel_at_the_top_of_its_lds_budget', 'test_table_index_outside_the_table_array', 'test_non_finite_entry',
                     'test_nan_row'],
    G.X64_STREAMED: ['test_x64_kernel_at_the_top_of_its_lds_budget', 'test_table_index_outside_the_table_array', 'test_non_finite_entry',
                     'test_nan_row', 'test_all_zero_table'],
    G.GENERIC: ['test_generic_size_edges', 'test_x64_graphs_past_the_lds_budget', 'test_260_variables', 'test_tie_rule_across_passes_and_waves',
                'test_all_ones_tie_everywhere',
                'test_table_index_outside_the_table_array', 'test_non_finite_entry', 'test_nan_row', 'test_all_zero_table'],
}
KEYS = ('x', 'score', 'mm', 'msgs')


def _launch(name, fb=None, **kw):
    """One eager call on the case's batch -> (case, batch, outputs); the kernel is the one the case names."""
    c = EC.case('map/' + name)
    if fb is None:
        fb = G._batch(c['spec'], c['inputs'], normalize=c['normalize'])
    got = G._run(fb, c['roots'], **kw)
    assert got['kernel'] == G.KERNEL_OF[c['instance']] == G._M().pick_kernel(c['spec']['X'], fb.topo.n_msgs, fb.topo.n_vars), name
    assert c['instance'] == G.GENERIC or (fb.topo.P <= 3) == (c['instance'] == G.X64_RESIDENT), name
    return c, fb, got


def _against_the_walk(name):
    ref = EC.precondition('map/' + name)                         # before the device is looked at
    c, fb, got = _launch(name)
    G._compare(name, c['spec'], fb.topo, c['inputs'], c['roots'], got, may_omit=len(c['tied']), normalize=c['normalize'], ref=ref)
    for b in c['tied']:                                          # nothing is left out: exact ties go to state 0, as in the walk
        want = [ref[b]['x'][v] for v in fb.topo.var_ids]
        print('%s graph %d: device assignment %s, the walk\'s %s' % (name, b, got['x'][b].tolist(), want))
        assert got['x'][b].tolist() == want, (name, b)
    return c, fb, got, ref


def _same_bits(name, a, b, graphs=None, keys=KEYS):
    """Prints how many entries of the two runs differ before it asserts that none does (floats by their bit patterns)."""
    pairs = {}
    for k in keys:
        x, y = (a[k], b[k]) if graphs is None else (a[k][graphs], b[k][graphs])
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        pairs[k] = (x, y) if k == 'x' else (x.view(np.int64), y.view(np.int64))
        print('%s %s: %d of %d entries differ' % (name, k, int((pairs[k][0] != pairs[k][1]).sum()), x.size))
    for k in keys:
        assert np.array_equal(*pairs[k]), (name, k)


# ---- A: size edges of the generic kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ring3_x301', 'chain3_x257', 'chain3_x2', 'chain2_x1024'])
def test_generic_size_edges(name):
    """X = 301: odd, two passes of every 256-stride loop, raw padded to 302 with scratch behind it; X = 257: one element in the
    second pass; X = 2 and X = 1024: the ends of the supported range (X = 1025 is refused on the host: tests/test_map_cpu.py)."""
    c, _, got, _ = _against_the_walk(name)
    assert (got['x'] >= 0).all() and (got['x'] < c['spec']['X']).all()


@pytest.mark.parametrize('name', ['chain31_x64', 'k8_x64'])
def test_x64_graphs_past_the_lds_budget(name):
    """X = 64 with 151 (a chain) and 152 (K8, loopy) message slots: past MLBP_MAP_X64_LDS_BYTES, so the generic kernel."""
    c, fb, got, _ = _against_the_walk(name)
    assert got['kernel'] == 2 and EC.map_lds_bytes(fb.topo.n_msgs, fb.topo.n_vars) == c['lds'] > G._M().X64_LDS_BYTES


# ---- B: more than 256 variables and factors ----------------------------------------------------------------------------------
def test_260_variables():
    """chain_spec(260, 4): xs[], the assignment copy and both score loops go beyond their first 256 entries.  A chain is a tree:
    the assignment is Viterbi's."""
    c, fb, got, _ = _against_the_walk('chain260_x4')
    assert (fb.topo.n_vars, fb.topo.P, fb.topo.U) == (260, 259, 260)
    for b, inp in enumerate(c['inputs']):
        assert got['x'][b].tolist() == G._viterbi(c['spec'], inp), b


# ---- C: the X = 64 kernel's LDS budget -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['chain30_x64', 'k3_len44'])
def test_x64_kernel_at_the_top_of_its_lds_budget(name):
    """Random potentials, so LDS addressed wrongly changes the answer.  chain_spec(30, 64): 146 slots, 79 488 bytes, streamed
    tables -- slots 128 to 145 lie above 64 KiB.  K3 under 41 given words: 138 slots, 75 280 bytes, tables in registers; 126
    unary factors, so the score's unary loop runs twice, and a variable update has 43 sources."""
    c, fb, got, _ = _against_the_walk(name)
    assert got['kernel'] == 1 and fb.topo.n_msgs == c['slots'] and fb.topo.n_msgs * 512 > 65536
    assert EC.map_lds_bytes(fb.topo.n_msgs, fb.topo.n_vars) == c['lds'] <= G._M().X64_LDS_BYTES
    assert (fb.topo.U > 64) == (name == 'k3_len44')


# ---- F: ties -------------------------------------------------------------------------------------------------------------------
def _ones(spec, B=2):
    inputs = [EC.C.make_inputs(spec, 1)] * B
    fb = G._batch(spec, inputs)
    if fb.topo.P:
        fb.pair_tables.fill_(1.0)
    fb.unary_tables.fill_(1.0)
    return fb


@pytest.mark.parametrize('lo,hi', EC.TIE_PAIRS)
def test_tie_rule_across_passes_and_waves(lo, hi):
    """All-ones tables with one larger, bit-equal value at states lo and hi of every unary row (X = 301: one variable without a
    pairwise factor, and a chain of three): two maxima held by one thread in two passes (40, 296), by waves 2 and 0 (140, 290),
    by waves 3 and 0 (200, 300).  The assignment is the lower index."""
    for name, spec, roots in EC.tie_specs():
        fb = _ones(spec)
        fb.unary_tables[:, lo] = EC.TIE_VALUE
        fb.unary_tables[:, hi] = EC.TIE_VALUE
        got = G._run(fb, roots)
        assert got['kernel'] == G.KERNEL_OF[G.GENERIC]
        top = got['mm'].max(-1)
        print('%s (%d, %d): assignments %s, maxima at lo and hi equal in %d of %d max-marginals'
              % (name, lo, hi, sorted(set(got['x'].reshape(-1).tolist())), int((got['mm'][..., lo] == got['mm'][..., hi]).sum()), top.size))
        assert np.array_equal(got['mm'][..., lo], top) and np.array_equal(got['mm'][..., hi], top)
        assert int((got['mm'] == top[..., None]).sum()) == 2 * top.size
        assert (got['x'] == lo).all(), (name, got['x'])


@pytest.mark.parametrize('spec,roots', [(EC.C.chain_spec(3, 301), [0, 0]), (EC.C.chain_spec(2, 1024), [0, 0])], ids=['x301', 'x1024'])
def test_all_ones_tie_everywhere(spec, roots):
    """Every state ties in every pass and wave: assignment 0."""
    fb = _ones(spec)
    got = G._run(fb, roots)
    assert got['kernel'] == G.KERNEL_OF[G.GENERIC]
    assert (got['x'] == 0).all() and np.allclose(got['mm'], 1.0 / spec['X'], rtol=1e-12) and np.array_equal(got['score'], np.zeros(fb.B))


# ---- the device-side refusal -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['clean_k3', 'clean_k4', 'clean_x128'])
def test_table_index_outside_the_table_array(name):
    """A table index outside the table array, written behind Python's check (one too large in pair_tab, -1 in unary_tab): those
    graphs return assignment -1 and score NaN, their max-marginals keep _run's NaN fill and their messages a sentinel
    written beforehand -- include/mlbp_map.h -- and every other graph keeps the bits of the clean run."""
    c, fb, clean, _ = _against_the_walk(name)
    B = fb.B
    fb.pair_tab[B - 1, 1] = fb.pair_tables.shape[0]
    fb.unary_tab[1, 0] = -1
    fb.msgs.fill_(-7.0)
    _, _, got = _launch(name, fb, keep_messages=True)
    for b in (1, B - 1):
        print('%s graph %d: assignment %s, score %r' % (name, b, sorted(set(got['x'][b].tolist())), got['score'][b]))
        assert (got['x'][b] == -1).all() and np.isnan(got['score'][b]), b
        assert np.isnan(got['mm'][b]).all() and (got['msgs'][b] == -7.0).all(), b
    _same_bits('%s, graphs that name their own tables' % name, got, clean, graphs=[b for b in range(B) if b not in (1, B - 1)])


# ---- G: bad entries ------------------------------------------------------------------------------------------------------------------
def _edit_leaves_the_others_alone(name, clean_name):
    c, _, got, ref = _against_the_walk(name)
    _, _, clean = _launch(clean_name)
    others = [b for b in range(len(c['inputs'])) if b != c['edited']]
    _same_bits('%s, untouched graphs' % name, got, clean, graphs=others)
    return c, got, clean, ref


@pytest.mark.parametrize('name', ['nan_k3', 'nan_k4', 'nan_x128', 'inf_k3', 'inf_k4', 'inf_x128'])
def test_non_finite_entry(name):
    """NaN or +inf at entry (3, 9) of one pairwise table of graph 2, normalised messages.  The graph follows the walk, whose
    maximum ignores a NaN (np.fmax); +inf gives the messages [0, ..., NaN, ..., 0] (compared as they are, NaN with NaN), which
    the next product zeroes.  The other graphs keep the bits of a run without the edit."""
    c, got, clean, _ = _edit_leaves_the_others_alone(name, 'clean_' + name.split('_')[1])
    e = c['edited']
    assert np.isfinite(got['mm']).all() and (got['x'] >= 0).all()
    if name.startswith('nan'):
        assert np.isfinite(got['msgs']).all() and np.isfinite(got['score']).all()
    else:
        assert int(np.isnan(got['msgs'][e]).sum()) == 2 and not np.array_equal(got['mm'][e], clean['mm'][e])


@pytest.mark.parametrize('name', ['nanrow_k3', 'nanrow_k4', 'nanrow_x128'])
def test_nan_row(name):
    """Row 3 of one pairwise table of graph 2 all NaN, normalised messages: the maximum over that row has no number to return,
    the message has no positive total and is uniform (include/mlbp_map.h leaves the maximum itself unspecified)."""
    c, got, clean, ref = _edit_leaves_the_others_alone(name, 'clean_' + name.split('_')[1])
    e, X = c['edited'], c['spec']['X']
    keys = EC.C.msg_keys(c['spec'])
    f = [f for f in c['spec']['factors'] if len(f['vars']) == 2][1]
    slot = keys.index(('F_%d' % f['id'], 'X_%d' % dict(zip(f['dims'], f['vars']))[0]))
    assert np.array_equal(got['msgs'][e, slot], np.full(X, 1.0 / X)) and not np.array_equal(clean['msgs'][e, slot], np.full(X, 1.0 / X))
    assert np.isfinite(got['msgs']).all() and np.isfinite(got['mm']).all()


@pytest.mark.parametrize('name', ['zero_k4', 'zero_k4_unnormalised', 'zero_x128', 'zero_x128_unnormalised'])
def test_all_zero_table(name):
    """One pairwise table of graph 1 all zero, on the streamed and the generic instance (the resident one:
    test_gpu_map.test_tie_rule_and_zero_table).  Normalised: the factor's messages have no positive total and are uniform.
    Unnormalised: they are zero, and so is every product they enter -- every max-marginal of the graph is exactly uniform and
    the assignment state 0.  The score is -inf."""
    c, got, _, _ = _edit_leaves_the_others_alone(name, 'clean_' + name[len('zero_'):])
    e, X = c['edited'], c['spec']['X']
    keys = EC.C.msg_keys(c['spec'])
    f = [f for f in c['spec']['factors'] if len(f['vars']) == 2][0]
    for v in f['vars']:
        m = got['msgs'][e, keys.index(('F_%d' % f['id'], 'X_%d' % v))]
        assert np.array_equal(m, np.full(X, 1.0 / X) if c['normalize'] else np.zeros(X)), (name, v)
    assert np.isneginf(got['score'][e]) and np.isfinite(np.delete(got['score'], e)).all()
    if not c['normalize']:
        assert np.array_equal(got['mm'][e], np.full_like(got['mm'][e], 1.0 / X)) and (got['x'][e] == 0).all()
