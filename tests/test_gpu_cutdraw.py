"""The cutset proposal drawn from held messages on the GPU (libmlbp_cutdraw.so) against the NumPy statement of
tests/test_cutdraw_cpu.py, fed the messages read back from fb.msgs and the same uniforms.

Bars.  States equal; log_q within 1e-10 absolute (the derived error is about 16 * (20 + log2 X) * 2^-53: at most 16 positions,
per position a handful of roundings in the products, log2 X in the prefix sums and one logarithm).  The CPU module asserts, for
every input family used here, that no draw of the statement comes within 1e-8 * total of a prefix sum, so the device's other
summation order cannot move a state.  No test asserts a statistical accuracy: every assertion is a deterministic function of
its inputs."""
import ctypes

import numpy as np
import pytest

import cases as C
import test_cutdraw_cpu as S
import test_cutset_cpu as R
from helpers import batch_tables, tidir_gold, write_tidir
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

X64 = ('cutdraw_x64_kernel', ())
GENERIC = ('cutdraw_generic_kernel', ())
# kernel -> the tests that launch it (tests/test_cutdraw_cpu.py holds this against the library's symbol table)
CASES = {
    X64: ['test_x64_shapes', 'test_second_mode', 'test_trees_end_to_end', 'test_the_messages_proposal_is_its_three_steps', 'test_position_zero_is_the_marginal',
          'test_batch_position_list_length_and_grid_keep_the_bits', 'test_power_of_two_scaling_keeps_every_bit', 'test_bad_entries_change_their_graph_or_entry_alone',
          'test_capture_and_replay', 'test_trainer'],
    GENERIC: ['test_generic_shapes', 'test_second_mode', 'test_trees_end_to_end', 'test_the_messages_proposal_is_its_three_steps',
              'test_batch_position_list_length_and_grid_keep_the_bits', 'test_power_of_two_scaling_keeps_every_bit',
              'test_bad_entries_change_their_graph_or_entry_alone'],
}
KERNEL_OF = {X64: 1, GENERIC: 2}
# every input family held against the statement here (tests/test_cutdraw_cpu.py asserts each clears its boundaries)
INPUTS_USED = {
    'k3_x64': 'test_x64_shapes', 'k4_x64_col': 'test_x64_shapes', 'k6_x64': 'test_x64_shapes', 'k9_x64': 'test_x64_shapes', 'k3_x64_n600': 'test_x64_shapes',
    'ring3_x2': 'test_generic_shapes', 'k5_x7': 'test_generic_shapes', 'k4_x33': 'test_generic_shapes', 'ring3_x65': 'test_generic_shapes',
    'ring3_x257': 'test_generic_shapes', 'k3_x1024': 'test_generic_shapes',
    'k4_x4': 'test_second_mode',
}


def _M():
    from macaronicusermodeling_amd import cutdraw
    return cutdraw


def _batch(spec, inputs_list, tables=None, pair_tab=None, unary_tab=None):
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(spec)
    assert topo.var_ids == O.Graph(spec).var_order
    fb = FactorGraphBatch(topo, spec['X'], len(inputs_list))
    pair, unary = batch_tables(spec, topo, inputs_list) if tables is None else tables
    if topo.P:
        fb.set_pair_tables(pair, pair_tab)
    if topo.U:
        fb.set_unary_tables(unary, unary_tab)
    return fb


def _t(fb, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(fb.device)


def _draw(fb, uniforms, cutset=None, kernel=None):
    """One cutset_draw(uniforms=...) on the messages fb holds: (configs, log_q) as host arrays."""
    M = _M()
    configs, log_q = fb.cutset_draw(uniforms.shape[1], uniforms=_t(fb, uniforms, np.float64), cutset=cutset)
    ran = M.last_kernel()
    torch.cuda.synchronize()
    assert ran == M.pick_kernel(fb.X) and (kernel is None or ran == KERNEL_OF[kernel]), ran
    assert configs.dtype == torch.int32 and tuple(configs.shape) == tuple(uniforms.shape) and tuple(log_q.shape) == tuple(uniforms.shape[:2])
    return configs.cpu().numpy(), log_q.cpu().numpy()


def _against_statement(name, spec, inputs, cut, uniforms, msgs, configs, log_q):
    worst = 0.0
    for b, i in enumerate(inputs):
        want = S.stated(spec, i, msgs[b], cut, uniforms=uniforms[b])
        assert np.array_equal(configs[b], want['configs']), (name, b)
        worst = max(worst, float(np.abs(log_q[b] - want['log_q']).max()))
    print('%s: states equal, log_q within %.1e' % (name, worst))
    assert worst <= 1e-10, (name, worst)


def _family(name, kernel):
    spec, inputs, cut, uniforms, _ = S.family(name)
    fb = _batch(spec, inputs)
    fb.sweep(list(fb.topo.var_ids), init=True)
    explicit = S.INPUTS[name][3] is not None
    configs, log_q = _draw(fb, uniforms, cutset=cut if explicit else None, kernel=kernel)
    _against_statement(name, spec, inputs, cut, uniforms, fb.msgs.cpu().numpy(), configs, log_q)
    return fb, configs, log_q


# ---- shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['k3_x64', 'k4_x64_col', 'k6_x64', 'k9_x64', 'k3_x64_n600'])
def test_x64_shapes(name):
    """K3: one position, the base alone.  K4 with cutset [1, 0]: the column read.  K6: four positions, N = 7 no multiple of 4.
    K9 at N = 3: walkers without an entry.  B = 1, N = 600: C = 512 and the stride 4 C wraps."""
    M = _M()
    spec, inputs, cut, uniforms, _ = S.family(name)
    B, N = uniforms.shape[:2]
    if name == 'k4_x64_col':
        assert M.plan_words(R._topo(spec), cut)[-3:].tolist() == [0, 0, 0]
    if name == 'k9_x64':
        assert len(cut) == 7 and 4 * M.chunks(B, N) > N
    if name == 'k3_x64_n600':
        assert M.chunks(B, N) == 512 and N > 512
    _family(name, X64)


@pytest.mark.parametrize('name', ['ring3_x2', 'k5_x7', 'k4_x33', 'ring3_x65', 'ring3_x257', 'k3_x1024'])
def test_generic_shapes(name):
    """Two states; odd sizes below a wave, around a wave and past a workgroup's 256 threads; X = 1024, four states a thread."""
    _family(name, GENERIC)


# ---- the second mode ------------------------------------------------------------------------------------
def test_second_mode():
    """K4 at X = 4 with all 16 configurations listed: exp(log_q) sums to 1 at 1e-12 and every log_q is the statement's.  On the
    X = 64 kernel (and at X = 7) cutset_logq() of a drawn list returns the drawn log_q bit for bit."""
    spec, inputs, cut, _, _ = S.family('k4_x4')
    fb = _batch(spec, inputs)
    fb.sweep(list(fb.topo.var_ids), init=True)
    every = S.every_config(4, len(cut))
    log_q = fb.cutset_logq(_t(fb, np.tile(every[None], (fb.B, 1, 1)), np.int32)).cpu().numpy()
    msgs = fb.msgs.cpu().numpy()
    for b, i in enumerate(inputs):
        assert abs(np.exp(log_q[b]).sum() - 1.0) <= 1e-12, b
        assert np.abs(log_q[b] - S.stated(spec, i, msgs[b], cut, configs_in=every)['log_q']).max() <= 1e-10
    for name, kernel in (('k6_x64', X64), ('k5_x7', GENERIC)):
        fb, configs, drawn = _family(name, kernel)
        again = fb.cutset_logq(_t(fb, configs, np.int32))
        assert _M().last_kernel() == KERNEL_OF[kernel]
        assert np.array_equal(again.cpu().numpy(), drawn), name


# ---- end to end, no statistics --------------------------------------------------------------------------
@pytest.mark.parametrize('X', [64, 5])
def test_trees_end_to_end(X):
    """A tree, BP's fixed point, a connected cutset: the proposal is Z_c / Z, so every weight is Z -- ess = N at 1e-9 relative
    and log_z_hat = exact_inference()'s log_z at 1e-10, for any seed."""
    for spec, cut in ((C.chain_spec(4, X), [1, 2, 0]), (C.star_spec(4, X), [0, 2])):
        inputs = [C.make_inputs(spec, s, 'lognormal') for s in (1, 2, 3)]
        fb = _batch(spec, inputs)
        log_z = fb.exact_inference()[0].cpu().numpy()
        fb.sweep(list(fb.topo.var_ids), init=True)
        held = fb.msgs.clone()
        for seed, N in ((0, 9), (7, 32)):
            log_z_hat, _, ess = fb.cutset_estimate(n_samples=N, seed=seed, cutset=cut, proposal='messages')
            log_z_hat, ess = log_z_hat.cpu().numpy(), ess.cpu().numpy()
            print('%s X = %d: |log_z_hat - log_z| <= %.1e, |ess / N - 1| <= %.1e' % (spec['name'], X, np.abs(log_z_hat - log_z).max(), np.abs(ess / N - 1).max()))
            assert (np.abs(ess - N) <= 1e-9 * N).all(), ess
            assert np.abs(log_z_hat - log_z).max() <= 1e-10
        assert torch.equal(fb.msgs, held)                       # roots=None: the messages are read as they stand


@pytest.mark.parametrize('name,make', [('k5_x64', lambda: R.kn_spec(5, 64)), ('ring5_x7', lambda: C.ring_spec(5, 7))], ids=['k5_x64', 'ring5_x7'])
def test_the_messages_proposal_is_its_three_steps(name, make):
    """cutset_estimate(roots, n_samples, seed, proposal='messages') = sweep(roots, init=True) + cutset_draw + cutset_estimate(configs,
    log_q), bit for bit; the default proposal is untouched by the new argument; any other value is refused."""
    spec = make()
    inputs = [C.make_inputs(spec, s, 'lognormal') for s in (1, 2, 3)]
    fb = _batch(spec, inputs)
    roots, N = list(fb.topo.var_ids), 16
    a = fb.cutset_estimate(roots, n_samples=N, seed=3, log_w=True, proposal='messages')
    fb.msgs.fill_(float('nan'))
    fb.sweep(roots, init=True)
    configs, log_q = fb.cutset_draw(N, seed=3)
    gen = torch.Generator(fb.device).manual_seed(3)
    uniforms = torch.rand((fb.B, N, configs.shape[2]), dtype=torch.float64, device=fb.device, generator=gen)
    same = fb.cutset_draw(N, uniforms=uniforms)
    assert torch.equal(same[0], configs) and torch.equal(same[1], log_q)
    b = fb.cutset_estimate(configs=configs, log_q=log_q, log_w=True)
    for x, y in zip(a, b):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    assert np.isfinite(a[0].cpu().numpy()).all() and (a[2].cpu().numpy() >= 1 - 1e-9).all()
    d0 = fb.cutset_estimate(roots, n_samples=N, seed=3)
    d1 = fb.cutset_estimate(roots, n_samples=N, seed=3, proposal='sample')
    for x, y in zip(d0, d1):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    with pytest.raises(ValueError):
        fb.cutset_estimate(roots, n_samples=N, seed=3, proposal='bp')
    with pytest.raises(ValueError):
        fb.cutset_draw(N)
    with pytest.raises(ValueError):
        fb.cutset_draw(N, seed=1, uniforms=uniforms)


def test_position_zero_is_the_marginal():
    """K3: the one position is drawn from the loopy-BP marginal of its variable."""
    fb, configs, log_q = _family('k3_x64', X64)
    cut = S.family('k3_x64')[2]
    marg = fb.marginals().cpu().numpy()
    v = fb.topo.var_index[cut[0]]
    for b in range(fb.B):
        want = marg[b, v, configs[b, :, 0]]
        assert np.abs(np.exp(log_q[b]) / want - 1.0).max() <= 1e-12, b


# ---- bits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel', [('k6_x64', X64), ('k5_x7', GENERIC)])
def test_batch_position_list_length_and_grid_keep_the_bits(name, kernel):
    """The same graph at another batch position with shared tables, under a longer list, and alone in a batch whose C differs:
    every entry keeps its bits."""
    M = _M()
    spec, inputs, cut, _, _ = S.family(name)
    inputs = list(inputs[:2])
    n_cut, N = len(cut), 300
    uniforms = np.random.RandomState(5).rand(2, N, n_cut)
    fb = _batch(spec, inputs)
    fb.sweep(list(fb.topo.var_ids), init=True)
    base_c, base_q = _draw(fb, uniforms, kernel=kernel)
    pair, unary = batch_tables(spec, fb.topo, inputs)
    P, U = fb.topo.P, fb.topo.U
    ptab, utab = np.array([np.arange(P) + P, np.arange(P), np.arange(P) + P]), np.array([np.arange(U) + U, np.arange(U), np.arange(U) + U])
    fb3 = _batch(spec, inputs + inputs[:1], (pair, unary), ptab, utab)         # graphs 0 and 2 are graph 1 of the base
    fb3.msgs.copy_(fb.msgs[[1, 0, 1]])
    longer = np.random.RandomState(6).rand(3, N + 37, n_cut)
    longer[:, :N] = uniforms[[1, 0, 1]]
    c3, q3 = _draw(fb3, longer, kernel=kernel)
    assert M.chunks(3, N + 37) != M.chunks(2, N)
    for g3, g in ((0, 1), (1, 0), (2, 1)):
        assert np.array_equal(c3[g3, :N], base_c[g]) and np.array_equal(q3[g3, :N], base_q[g]), (g3, g)
    fb1 = _batch(spec, inputs[1:2])
    fb1.msgs.copy_(fb.msgs[1:2])
    assert M.chunks(1, N) == N != M.chunks(2, N)
    c1, q1 = _draw(fb1, uniforms[1:2], kernel=kernel)
    assert np.array_equal(c1[0], base_c[1]) and np.array_equal(q1[0], base_q[1])


@pytest.mark.parametrize('name,kernel', [('k6_x64', X64), ('k5_x7', GENERIC)])
def test_power_of_two_scaling_keeps_every_bit(name, kernel):
    """Tables times 2^+-400 with the messages held fixed: no bit of configs or log_q moves.  The lognormal tables span far
    less than 2^100, so no entry of a product goes subnormal."""
    spec, inputs, cut, _, _ = S.family(name)
    uniforms = np.random.RandomState(8).rand(len(inputs), 24, len(cut))
    fb = _batch(spec, inputs)
    fb.sweep(list(fb.topo.var_ids), init=True)
    base_c, base_q = _draw(fb, uniforms, kernel=kernel)
    pair, unary = batch_tables(spec, fb.topo, inputs)
    assert pair.max() / pair.min() < 2.0 ** 100
    for k in (400, -400):
        p2 = pair.copy()
        for p in range(len(p2)):
            p2[p] = np.ldexp(p2[p], k if p % 2 else -k // 2)
        fb2 = _batch(spec, inputs, (p2, unary))
        fb2.msgs.copy_(fb.msgs)
        c2, q2 = _draw(fb2, uniforms, kernel=kernel)
        assert np.array_equal(c2, base_c) and np.array_equal(q2, base_q), (name, k)


# ---- bad entries ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel,make', [('k6_x64', X64, lambda: R.kn_spec(6, 64)), ('k5_x7', GENERIC, lambda: R.kn_spec(5, 7))], ids=['k6_x64', 'k5_x7'])
def test_bad_entries_change_their_graph_or_entry_alone(name, kernel, make):
    """Graph 0: a table index outside its array -- configs -1, log_q NaN.  Graph 1: a NaN table that every later position reads --
    log_q NaN, states in range.  Graph 2: a NaN message -- the same.  Graph 3: an all-zero table between the first two
    positions -- log_q -inf, states in range.  Graph 4: uniforms 1.0 and NaN in two entries -- the statement's states.  Graph 5
    and every other entry of graph 4 keep their bits.  Then a configs_in state of X: that entry NaN, every other its bits."""
    M = _M()
    spec = make()
    X = spec['X']
    inputs = [C.make_inputs(spec, s, 'lognormal') for s in (1, 2, 3, 4, 5, 6)]
    cut = R.chosen_ids(spec)
    N, n_cut = 10, len(cut)
    uniforms = np.random.RandomState(11).rand(6, N, n_cut)
    fb = _batch(spec, inputs)
    roots = list(fb.topo.var_ids)
    fb.sweep(roots, init=True)
    base_c, base_q = _draw(fb, uniforms, kernel=kernel)
    assert np.isfinite(base_q).all()
    topo = fb.topo
    items = S.items_of(topo, [topo.var_index[v] for v in cut])
    first_row = items[1][1][0][0]                               # the pair slot between positions 0 and 1
    pair, unary = batch_tables(spec, topo, inputs)
    p2 = pair.copy()
    p2[1 * topo.P + first_row][:] = np.nan
    p2[3 * topo.P + first_row][:] = 0.0
    fb2 = _batch(spec, inputs, (p2, unary))
    fb2.msgs.copy_(fb.msgs)
    fb2.msgs[2, items[0][0][0], 1] = float('nan')
    fb2.pair_tab[0, topo.P - 1] = fb2.pair_tables.shape[0]
    u2 = uniforms.copy()
    u2[4, 3, 0], u2[4, 6, n_cut - 1] = 1.0, np.nan
    c2, q2 = _draw(fb2, u2, kernel=kernel)
    assert (c2[0] == -1).all() and np.isnan(q2[0]).all()
    for b in (1, 2):
        assert np.isnan(q2[b]).all() and (c2[b] >= 0).all() and (c2[b] < X).all(), b
    assert np.isneginf(q2[3]).all() and (c2[3] >= 0).all() and (c2[3] < X).all() and (c2[3][:, 1] == 0).all()
    assert np.array_equal(c2[5], base_c[5]) and np.array_equal(q2[5], base_q[5])
    keep = [i for i in range(N) if i not in (3, 6)]
    assert np.array_equal(c2[4][keep], base_c[4][keep]) and np.array_equal(q2[4][keep], base_q[4][keep])
    want = S.stated(spec, inputs[4], fb.msgs[4].cpu().numpy(), cut, uniforms=u2[4])
    assert np.array_equal(c2[4], want['configs']) and np.abs(q2[4] - want['log_q']).max() <= 1e-10 and np.isfinite(q2[4]).all()
    assert c2[4, 6, n_cut - 1] == X - 1                         # a NaN uniform: the highest state of positive weight
    listed = base_c.copy()
    listed[1, 4, n_cut - 1], listed[5, 0, 0] = X, -1
    q3 = fb.cutset_logq(_t(fb, listed, np.int32)).cpu().numpy()
    assert M.last_kernel() == KERNEL_OF[kernel]
    assert np.isnan(q3[1, 4]) and np.isnan(q3[5, 0])
    q3[1, 4], q3[5, 0] = base_q[1, 4], base_q[5, 0]
    assert np.array_equal(q3, base_q)


# ---- capture --------------------------------------------------------------------------------------------
def test_capture_and_replay():
    """After one eager call a captured cutset_draw, replayed with changed messages and uniforms, gives the eager bits.  The call
    itself, captured on a stream of its own, is one kernel node and no edge."""
    M = _M()
    spec, inputs, cut, _, _ = S.family('k6_x64')
    fb = _batch(spec, inputs)
    roots = list(fb.topo.var_ids)
    fb.sweep(roots, init=True)
    N, n_cut = 13, len(cut)
    uniforms = _t(fb, np.random.RandomState(1).rand(fb.B, N, n_cut), np.float64)
    fb.cutset_draw(N, uniforms=uniforms)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fb.cutset_draw(N, uniforms=uniforms)
    for round_ in range(2):
        if round_:
            fb.sweep(roots[::-1], init=True)
            uniforms.copy_(_t(fb, np.random.RandomState(2).rand(fb.B, N, n_cut), np.float64))
        eager = fb.cutset_draw(N, uniforms=uniforms)
        out[0].fill_(-5)
        out[1].fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1]), round_
    # the call on its own: caller-owned buffers, nothing but the enqueue between begin and end of the capture
    pl = M.plan(fb.topo, None, fb.X, fb.device)
    configs, log_q = torch.empty_like(eager[0]), torch.empty_like(eager[1])
    a = M.CutdrawArgs()
    a.B, a.X, a.n_msgs, a.P, a.n_cut, a.N = fb.B, fb.X, fb.topo.n_msgs, fb.topo.P, pl.n_cut, N
    a.plan, a.plan_words, a.n_pair_tables = pl.dev.data_ptr(), len(pl.words), fb.pair_tables.shape[0]
    a.pair_tables, a.pair_tab, a.msgs = fb.pair_tables.data_ptr(), fb.pair_tab.data_ptr(), fb.msgs.data_ptr()
    a.uniforms, a.configs, a.log_q = uniforms.data_ptr(), configs.data_ptr(), log_q.data_ptr()
    hip = M.lib                                                 # the HIP runtime the library is linked against
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp, g = ctypes.c_void_p(stream.cuda_stream), ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(sp, 0) == 0
    rc = M.lib.mlbp_cutdraw_f64(ctypes.byref(a), sp)
    assert hip.hipStreamEndCapture(sp, ctypes.byref(g)) == 0
    assert rc == 0, M.last_error()
    n_nodes, n_edges = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n_nodes)) == 0 and n_nodes.value == 1
    node, kind = ctypes.c_void_p(), ctypes.c_int(-1)
    assert hip.hipGraphGetNodes(g, ctypes.byref(node), ctypes.byref(n_nodes)) == 0
    assert hip.hipGraphNodeGetType(node, ctypes.byref(kind)) == 0 and kind.value == 0          # hipGraphNodeTypeKernel
    assert hip.hipGraphGetEdges(g, None, None, ctypes.byref(n_edges)) == 0 and n_edges.value == 0
    assert hip.hipGraphDestroy(g) == 0


# ---- refusals and the tree ------------------------------------------------------------------------------
def test_float32_tables_and_the_approximate_mode_are_refused():
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    spec = C.user_spec(10, [1, 4, 7], 256, 64, seed=1)
    fb = _batch(spec, [C.make_inputs(spec, 1)])
    fb.set_pair_tables(fb.pair_tables, dtype=torch.float32)
    with pytest.raises(NotImplementedError, match='float64'):
        fb.cutset_draw(4, seed=0)
    with pytest.raises(NotImplementedError, match='float64'):
        fb.cutset_logq(torch.zeros(1, 4, 1, dtype=torch.int32, device=fb.device))
    with pytest.raises(NotImplementedError):
        fb.cutset_estimate(list(fb.topo.var_ids), n_samples=4, seed=0, proposal='messages')
    spec = R.kn_spec(3, 128)
    topo = R._topo(spec)
    fa = FactorGraphBatch(topo, 128, 1, use_approx_inference=True)
    pair, unary = batch_tables(spec, topo, [C.make_inputs(spec, 1)])
    fa.set_pair_tables(pair)
    fa.set_unary_tables(unary)
    with pytest.raises(NotImplementedError, match='approximate'):
        fa.cutset_draw(4, seed=0)


def test_a_tree_needs_no_launch():
    M = _M()
    spec = C.star_spec(4, 9)
    fb = _batch(spec, [C.make_inputs(spec, s) for s in (1, 2)])
    fb.sweep(list(fb.topo.var_ids), init=True)
    fb.cutset_draw(2, seed=1, cutset=[0])                       # (a launch, so that last_kernel is not NONE already)
    assert M.last_kernel() == M.KERNEL_GENERIC
    configs, log_q = fb.cutset_draw(4, seed=1)
    assert M.last_kernel() == M.KERNEL_GENERIC                  # the library was not called
    assert configs.dtype == torch.int32 and tuple(configs.shape) == (2, 4, 0) and tuple(log_q.shape) == (2, 4) and (log_q.cpu().numpy() == 0.0).all()
    assert (fb.cutset_logq(configs).cpu().numpy() == 0.0).all()
    log_z_hat, marg, ess = fb.cutset_estimate(n_samples=4, seed=1, proposal='messages')
    for b in range(2):
        z, m, _ = R.enumerate_exact(O.Graph(spec), C.make_inputs(spec, b + 1))
        assert abs(log_z_hat[b].item() - z) <= 1e-10 * max(1.0, abs(z)) and np.abs(marg[b].cpu().numpy() - m).max() <= 1e-10


# ---- trainer --------------------------------------------------------------------------------------------
def test_trainer(tmp_path):
    """estimated_inference and estimate_report with proposal='messages' on the clique fixture's sentences of 3, 4 and 6 predicted
    words: finite, shaped as documented, and what log_partition + cutset_draw + cutset_estimate give; the default proposal's
    results are the same bits before and after."""
    from macaronicusermodeling_amd import tidir
    from test_gpu_cliques import _trainer
    gold = dict(tidir_gold('tidir_cliques_reference'))
    keep, count = [], {3: 0, 4: 0, 6: 0}
    for line in gold['instances']:
        for key in tidir.bucket_instances([tidir.parse_instance(line)], gold['vocab_en'], gold['vocab_de']):
            if len(key[1]) in count and count[len(key[1])] < 2:
                count[len(key[1])] += 1
                keep.append(line)
    assert all(count.values())
    gold['instances'] = keep
    tt = _trainer(write_tidir(gold, str(tmp_path)), gold)
    n, seed = 16, 5
    before = tt.estimate_report(n_samples=n, seed=seed)
    per_instance, totals, skipped = tt.estimate_report(n_samples=n, seed=seed, proposal='messages')
    assert skipped == [] and len(per_instance) == len(keep) and totals[0] == len(keep) and totals[1] == count[3] + count[4]
    assert np.isfinite(totals[2:]).all() and 0 < totals[4] <= len(keep) * (1 + 1e-9)
    for i, (key, tr) in enumerate(tt.trainers.items()):
        fb = tr.batch
        log_z_hat, ess, gap, marg = tr.estimated_inference(n, seed + i, proposal='messages')
        assert log_z_hat.shape == ess.shape == gap.shape == (fb.B,) and marg.shape == (fb.B, fb.topo.n_vars, fb.X)
        assert np.isfinite(log_z_hat).all() and np.isfinite(gap).all() and np.isfinite(marg).all() and (ess >= 1 - 1e-9).all() and (ess <= n * (1 + 1e-9)).all()
        tr.build_potentials()
        bethe = fb.log_partition(tr.roots[:tr.n_sweeps_run], init=True)
        configs, log_q = fb.cutset_draw(n, seed=seed + i)
        z2, m2, e2 = fb.cutset_estimate(configs=configs, log_q=log_q)
        assert np.array_equal(z2.cpu().numpy(), log_z_hat) and np.array_equal(e2.cpu().numpy(), ess) and np.array_equal(m2.cpu().numpy(), marg)
        assert np.array_equal((bethe - z2).cpu().numpy(), gap)
        for r, row in enumerate(tt.buckets[key]['rows']):
            positions, z_hat, rse, g_, z = per_instance[row['index']]
            assert positions == tuple(key[1]) and z_hat == log_z_hat[r] and g_ == gap[r] and (z is None) == (len(key[1]) > 4)
            assert abs(rse - np.sqrt(max(1.0 / ess[r] - 1.0 / n, 0.0))) <= 1e-12
    after = tt.estimate_report(n_samples=n, seed=seed)
    assert repr(after) == repr(before)
    with pytest.raises(ValueError):
        next(iter(tt.trainers.values())).estimated_inference(n, seed, proposal='bp')
