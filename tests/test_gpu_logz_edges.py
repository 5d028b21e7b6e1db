"""The four kernels of libmlbp_logz.so at their edges: size edges of the generic kernel, the X = 64 kernel's LDS budget from
both sides, more than 256 (and more than 64) variables and factors, the shared-table kernel on a large graph, the batch sums
beyond one pass, bad table entries.  Inputs, references and preconditions are those of tests/test_map_logz_edges_cpu.py (parts
A to G there); every case calls its `precondition` -- the kernel choice, the LDS byte count, a finite statement -- before
the device is looked at.

The rules are test_gpu_logz._compare's, with nothing new: kernel_atol(topo, X) plus rtol 1e-12 against the statement on the
device's own messages, plus 1e-10 per message factor against the statement on the oracle's sweeps; the batch sums at
B * kernel_atol.

These cases pin the log-partition kernels, not the sweep library.  Where the sweep kernels have no case of their own -- 260
variables, chains of 40, 41 and 70 at X = 64 -- the messages are the CPU statement's (S.sweeps), uploaded into fb.msgs, and
log_partition(roots=None) reads them; elsewhere the sweeps run on the device as in test_gpu_logz._case.

Mutations these cases are built to catch:
  the second pass of a 256-stride (or, per wave, 64-stride) loop missing, the
  padding of na / nb at odd X                                                    test_generic_size_edges (X = 301, 257; 2, 1024)
  wave_score's label, pairwise or unary loop stopped after one pass              test_260_variables, test_shared_kernel_on_70_variables,
                                                                                 test_x64_kernel_at_the_top_of_its_lds_budget[k3_len38]
  the budget rule handing a graph to the wrong kernel; LDS rows near 64 KiB      test_x64_kernel_at_the_top_of_its_lds_budget,
                                                                                 test_x64_chain_past_the_lds_budget
  the shared kernel's group bookkeeping beyond 64 factors or in a ragged group   test_shared_kernel_on_70_variables
  logz_sum_kernel stopped after one pass                                         test_batch_sums_beyond_one_pass
  a clamp, or a NaN or zero swallowed on the way to the logarithm                test_non_finite_and_zero_tables"""
import math

import numpy as np
import pytest

import cases as C
import test_gpu_logz as G
import test_map_logz_edges_cpu as EC

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

# kernel -> the tests here that launch it (tests/test_logz_cpu.py holds this against the library's symbol table)
CASES = {
    G.X64: ['test_x64_kernel_at_the_top_of_its_lds_budget', 'test_batch_sums_beyond_one_pass', 'test_non_finite_and_zero_tables'],
    G.X64_SHARED: ['test_shared_kernel_on_70_variables', 'test_non_finite_and_zero_tables'],
    G.GENERIC: ['test_generic_size_edges', 'test_x64_chain_past_the_lds_budget', 'test_260_variables', 'test_batch_sums_beyond_one_pass',
                'test_non_finite_and_zero_tables'],
    G.SUM: ['test_batch_sums_beyond_one_pass', 'test_generic_size_edges', 'test_shared_kernel_on_70_variables'],
}


def _batch_of(c):
    spec, inputs = c['spec'], c['inputs']
    if not c['shared']:
        return G._batch(spec, inputs)
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(spec)                         # one set of pairwise tables (graph 0's) behind every graph
    pair, unary = G.batch_tables(spec, topo, inputs)
    assert all(np.array_equal(pair[b * topo.P:(b + 1) * topo.P], pair[:topo.P]) for b in range(len(inputs)))
    return G._batch(spec, inputs, tables=(pair[:topo.P], unary), pair_tab=np.tile(np.arange(topo.P), (len(inputs), 1)))


def _launch(name):
    """The case's batch, its messages (uploaded or swept on the device) and one log_partition call -> (case, batch, outputs,
    reference); the kernel is the one the case names."""
    ref = EC.precondition('logz/' + name)                        # before the device is looked at
    c = EC.case('logz/' + name)
    fb = _batch_of(c)
    if c['upload']:
        keys = C.msg_keys(c['spec'])
        host = np.stack([np.stack([ref[b][k] for k in keys]) for b in range(fb.B)])
        assert host.shape == tuple(fb.msgs.shape)
        fb.msgs.copy_(torch.from_numpy(host))
    got = G._run(fb, None if c['upload'] else c['roots'], c['labels'])
    L = G._L()
    flags = L.SHARED_PAIR_TABLES if getattr(fb, 'pair_tables_shared', False) else 0
    assert bool(flags) == c['shared'], name
    assert got['kernel'] == G.KERNEL_OF[c['instance']] == L.pick_kernel(c['spec']['X'], int(fb.topo.in_off[-1]), fb.topo.n_vars, flags), name
    return c, fb, got, ref


def _against_the_statement(name, graphs=None):
    c, fb, got, ref = _launch(name)
    G._compare(name, c['spec'], fb.topo, c['inputs'], c['roots'], c['labels'], got, graphs=graphs, ref=ref)
    assert np.isfinite(got['log_z']).all() and np.isfinite(got['score']).all() and np.isfinite(got['joint']).all()
    return c, fb, got, ref


# ---- A: size edges of the generic kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ring3_x301', 'chain3_x257', 'chain3_x2', 'chain2_x1024'])
def test_generic_size_edges(name):
    """X = 301: odd, na and nb padded to 302 with nb and scratch behind the padding, two passes of every strided loop; X = 257:
    one element in the second pass; X = 2 and X = 1024: the ends of the supported range (kernel_atol at X = 1024: 1.2e-9)."""
    c, fb, _, _ = _against_the_statement(name)
    if name == 'chain2_x1024':
        assert abs(G.kernel_atol(fb.topo, 1024) - 1.2e-9) < 5e-11


def test_x64_chain_past_the_lds_budget():
    """chain_spec(41, 64): 121 in-slots, 66 112 bytes > MLBP_LOGZ_X64_LDS_BYTES, so the generic kernel at X = 64."""
    c, fb, got, _ = _against_the_statement('chain41_x64')
    assert got['kernel'] == 3 and EC.logz_lds_bytes(int(fb.topo.in_off[-1])) == 66112 > G._L().X64_LDS_BYTES


# ---- B: more than 256 variables and factors ----------------------------------------------------------------------------------
def test_260_variables():
    """chain_spec(260, 4): wave_score makes five passes over labels, pairwise and unary factors.  A chain is a tree: log_z is the
    forward algorithm's."""
    c, fb, got, _ = _against_the_statement('chain260_x4')
    assert (fb.topo.n_vars, fb.topo.P, fb.topo.U) == (260, 259, 260)
    bound = G.kernel_atol(fb.topo, 4) + 1e-10 * G.message_factors(fb.topo)
    for b, inp in enumerate(c['inputs']):
        G._close(got['log_z'][b], G._forward_log_z(c['spec'], inp), bound, 'chain260 graph %d' % b)


# ---- C: the X = 64 kernel's LDS budget -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['chain40_x64', 'k3_len38'])
def test_x64_kernel_at_the_top_of_its_lds_budget(name):
    """chain_spec(40, 64): 118 in-slots, 64 576 bytes of dynamic LDS, the last chain inside the budget.  K3 under 35 given words:
    114 in-slots, 108 unary factors -- wave_score's unary loop runs twice -- and leave-one-out products of 37 messages."""
    c, fb, got, _ = _against_the_statement(name)
    n_in = int(fb.topo.in_off[-1])
    assert got['kernel'] == 1 and n_in == c['in_slots'] and EC.logz_lds_bytes(n_in) == c['lds'] <= G._L().X64_LDS_BYTES
    assert (fb.topo.U > 64) == (name == 'k3_len38')


# ---- D: the shared-table kernel ------------------------------------------------------------------------------------------------
def test_shared_kernel_on_70_variables():
    """chain_spec(70, 64), B = 20, one set of 69 pairwise tables behind every graph and unary tables per graph: P, U and n_vars
    above 64 in the 16-graph kernel, with a ragged second group.  Compared with the statement graph by graph."""
    c, fb, got, _ = _against_the_statement('chain70_x64_shared')
    assert fb.pair_tables_shared and fb.pair_tables.shape[0] == 69 and (fb.B, fb.topo.n_vars, fb.topo.U) == (20, 70, 70)
    assert len(set(got['log_z'].tolist())) == 20


# ---- E: the batch sums -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['sum_B600_x4', 'sum_B300_k3'])
def test_batch_sums_beyond_one_pass(name):
    """logz_sum_kernel adds 256 graphs per pass: B = 600 behind the generic kernel (a third, partial pass) and B = 300 behind the
    X = 64 kernel (inputs repeating every 64 graphs).  Both sums against math.fsum of the device's own per-graph values."""
    c = EC.case('logz/' + name)
    B = len(c['inputs'])
    graphs = list(range(c['distinct'])) if c['distinct'] else sorted(set(range(0, B, 37)) | {255, 256, 511, 512, B - 1})
    c, fb, got, _ = _against_the_statement(name, graphs=graphs)
    if c['distinct']:                                            # every graph: equal inputs give equal bits
        for k in ('log_z', 'score', 'joint'):
            assert np.array_equal(got[k], got[k][np.arange(B) % c['distinct']]), k
    bound = B * G.kernel_atol(fb.topo, c['spec']['X'])
    for i, k in enumerate(('log_z', 'joint')):
        want = math.fsum(got[k].tolist())
        print('%s: sum of %s %.12f, fsum of the %d device values %.12f, |diff| %.2e (bound %.2e)'
              % (name, k, got['sums'][i], B, want, abs(got['sums'][i] - want), bound))
        G._close(got['sums'][i], want, bound, '%s sum of %s' % (name, k))
    assert abs(math.fsum(got['log_z'][:256].tolist()) - got['sums'][0]) > 1e3 * bound          # one pass alone is far off


# ---- G: bad entries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['bad_k3', 'bad_k3_shared', 'bad_x128'])
def test_non_finite_and_zero_tables(name):
    """Behind the sweeps: NaN at entry (3, 9) of one pairwise table of graph 2, and one pairwise table of graph 1 all zero.  IEEE
    arithmetic, nothing is clamped (include/mlbp_logz.h): the statement on the device's messages gives NaN for graph 2's log_z
    and joint_logp, -inf for graph 1's log_z and score and NaN for its joint_logp; the device says the same, and every other
    graph keeps its bits.  (bad_k3_shared: the caller's claim on unique tables, so every group falls back factor by factor.)"""
    EC.precondition('logz/' + name)
    c = EC.case('logz/' + name)
    fb = G._batch(c['spec'], c['inputs'])
    topo, B = fb.topo, fb.B
    fb.sweep(c['roots'], init=True)
    fb.pair_tables_shared = c['shared']
    clean = G._run(fb, None, c['labels'])
    assert clean['kernel'] == G.KERNEL_OF[c['instance']] and np.isfinite(clean['joint']).all()
    fb.pair_tables[2 * topo.P + 1, EC.AT[0], EC.AT[1]] = float('nan')
    fb.pair_tables[1 * topo.P + 0].fill_(0.0)
    got = G._run(fb, None, c['labels'])
    assert got['kernel'] == clean['kernel'] and np.array_equal(got['msgs'], clean['msgs'])
    for b, k in ((2, 'log_z'), (2, 'joint'), (1, 'log_z'), (1, 'score'), (1, 'joint')):
        print('%s graph %d %s: %r' % (name, b, k, got[k][b]))
    assert np.isnan(got['log_z'][2]) and np.isnan(got['joint'][2])
    assert np.isneginf(got['log_z'][1]) and np.isneginf(got['score'][1]) and np.isnan(got['joint'][1])
    G._compare(name, c['spec'], topo, EC.bad_logz_inputs('logz/' + name), None, c['labels'], got, walk=False)
    for b in range(B):
        if b not in (1, 2):
            assert all(got[k][b].tobytes() == clean[k][b].tobytes() for k in ('log_z', 'score', 'joint')), b
