"""Max-product / MAP decoding without a GPU: the float64 NumPy walk the GPU tests compare against, pinned on exhaustive
enumeration; and the host checks of libmlbp_map.so
(the contract it shares with the other side libraries is in tests/test_side_libraries_cpu.py).

The walk is FactorGraph.treelike_inference as oracle/lbp_oracle.py restates it, with ONE change: a pairwise
factor-to-variable update takes max_j T[i][j] m[j] in place of the sum.  Schedule, initial messages, the variable update,
renormalisation and the product of incoming messages are the oracle's own functions.  The reference has no max-product, so
the walk itself is pinned on brute force: log-potentials summed over the whole X^n grid and their argmax, which one sweep
must reproduce on every tree."""
import ctypes

import numpy as np
import pytest

import cases as C
import helpers
from oracle import lbp_oracle as O


# ------------------------------------------------------------------------------------------------
# the NumPy max-product walk
# ------------------------------------------------------------------------------------------------
def _finish(v, normalize):
    return O.renormalize(v) if normalize else v


def mp_factor_to_var(g, inputs, msgs, fid, v, normalize=True):
    """O.factor_to_var with max in place of the contraction's sum.  The maximum is the header's: it ignores NaN entries
    (np.fmax; on NaN-free input np.fmax.reduce and ndarray.max return the same bits)."""
    f = g.by_id[fid]
    T = O.factor_table(g, inputs, f)
    if len(f['vars']) == 1:
        out = np.copy(T).reshape(-1)
    else:
        other = [u for u in f['vars'] if u != v][0]
        m = msgs['X_%d' % other, 'F_%d' % fid]
        if g.dim_of(f, other) == 1:
            out = np.fmax.reduce(T * m[None, :], axis=1)
        else:
            out = np.fmax.reduce(m[:, None] * T, axis=0)
    msgs['F_%d' % fid, 'X_%d' % v] = _finish(out, normalize)


def _mp_send(g, inputs, msgs, frm, to, normalize):
    if to[0] == O.FAC and len(g.by_id[to[1]]['vars']) < 2:
        return
    if frm[0] == O.VAR:
        if normalize:
            O.var_to_factor(g, msgs, frm[1], to[1])
        else:
            msgs['X_%d' % frm[1], 'F_%d' % to[1]] = O._product_of_incoming(g, msgs, frm[1], skip=to[1])
    else:
        mp_factor_to_var(g, inputs, msgs, frm[1], to[1], normalize)


def mp_sweep(g, inputs, msgs, root, normalize=True):
    sched = O.message_schedule(g, root)
    for child, parent in reversed(sched):
        _mp_send(g, inputs, msgs, child, parent, normalize)
    for child, parent in sched:
        _mp_send(g, inputs, msgs, parent, child, normalize)


def max_marginal(g, msgs, v):
    return O.renormalize(O._product_of_incoming(g, msgs, v))


def score_of(g, inputs, x):
    """sum over factors of log(table entry at x); x: {variable id: state}."""
    total = 0.0
    for f in g.factors:
        T = O.factor_table(g, inputs, f)
        if len(f['vars']) == 1:
            entry = T.reshape(-1)[x[f['vars'][0]]]
        else:
            by_axis = {g.dim_of(f, v): v for v in f['vars']}
            entry = T[x[by_axis[0]], x[by_axis[1]]]
        with np.errstate(divide='ignore'):
            total += np.log(entry)
    return total


def walk(spec, inputs, roots, normalize=True, msgs=None):
    """-> dict(g, msgs, mm {v: max-marginal}, x {v: state}, score, gap {v: relative gap of the two largest entries})."""
    g = O.Graph(spec)
    msgs = O.init_messages(g) if msgs is None else msgs
    for r in roots:
        mp_sweep(g, inputs, msgs, r, normalize)
    mm = {v: max_marginal(g, msgs, v) for v in g.var_order}
    x = {v: int(np.argmax(mm[v])) for v in g.var_order}          # np.argmax: the first (lowest) index at the maximum
    gap = {}
    for v in g.var_order:
        top = np.sort(mm[v])[-2:]
        gap[v] = (top[1] - top[0]) / top[1] if top[1] > 0 else 0.0
    return dict(g=g, msgs=msgs, mm=mm, x=x, score=score_of(g, inputs, x), gap=gap)


def brute_force(g, inputs):
    """(argmax {v: state}, maximum, the grid of summed log-potentials) over all X^n assignments."""
    order = g.var_order
    n, X = len(order), g.X
    grid = np.zeros((X,) * n)
    for f in g.factors:
        T = O.factor_table(g, inputs, f)
        shape = [1] * n
        if len(f['vars']) == 1:
            shape[order.index(f['vars'][0])] = X
            grid = grid + np.log(T.reshape(-1)).reshape(shape)
        else:
            by_axis = {g.dim_of(f, v): v for v in f['vars']}
            a0, a1 = order.index(by_axis[0]), order.index(by_axis[1])
            shape[a0] = shape[a1] = X
            L = np.log(T)
            grid = grid + (L if a0 < a1 else L.T).reshape(shape)
    best = np.unravel_index(int(np.argmax(grid)), grid.shape)
    return {v: int(best[i]) for i, v in enumerate(order)}, float(grid.max()), grid


TREE_CASES = [('chain5_x8/root0/uniform', lambda: C.chain_spec(5, 8), [0], 'uniform'),
              ('chain5_x8/root2/lognormal', lambda: C.chain_spec(5, 8), [2], 'lognormal'),
              ('star4_x8/root0', lambda: C.star_spec(4, 8), [0], 'uniform'),
              ('star4_x8/root3', lambda: C.star_spec(4, 8), [3], 'uniform')]


def random_trees():
    """The loop-free graphs among 60 draws of helpers.random_spec(RandomState(7), ..., X=4)."""
    rs = np.random.RandomState(7)
    specs = [helpers.random_spec(rs, 'random%d' % i, X=4) for i in range(60)]
    return [s for s in specs if not O.has_loops(O.Graph(s), s['var_ids'][0])]


@pytest.mark.parametrize('name,make,roots,kind', TREE_CASES, ids=[c[0] for c in TREE_CASES])
def test_walk_equals_brute_force_on_trees(name, make, roots, kind):
    spec = make()
    hits = 0
    for seed in range(40):
        inputs = C.make_inputs(spec, seed, kind)
        w = walk(spec, inputs, roots)
        x, best, grid = brute_force(w['g'], inputs)
        assert w['x'] == x, (name, seed)
        np.testing.assert_allclose(w['score'], best, rtol=1e-12)
        hits += 1
    print('%s: %d/40 decoded assignments equal the brute-force MAP' % (name, hits))


def test_walk_equals_brute_force_on_random_trees():
    trees = random_trees()
    assert len(trees) >= 5
    for i, spec in enumerate(trees):
        inputs = C.make_inputs(spec, i)
        w = walk(spec, inputs, [spec['var_ids'][0]])
        x, best, _ = brute_force(w['g'], inputs)
        assert w['x'] == x, spec['name']
        np.testing.assert_allclose(w['score'], best, rtol=1e-12)
    print('random trees: %d/%d decoded assignments equal the brute-force MAP' % (len(trees), len(trees)))


@pytest.mark.parametrize('name,make,seeds,roots', [
    ('user_k3_x64', lambda: C.user_spec(10, [1, 4, 7], 64, 64, seed=1), range(500, 564), [1, 4, 7]),
    ('ring5_x8', lambda: C.ring_spec(5, 8), range(40), [0, 2, 4])], ids=['user_k3_x64', 'ring5_x8'])
def test_walk_never_beats_brute_force_on_loopy_graphs(name, make, seeds, roots):
    """Loopy max-product is an approximation: the decoded assignment's score can only be below or equal to the maximum
    (how often it is equal is printed, not asserted)."""
    spec = make()
    equal = 0
    for seed in seeds:
        inputs = C.make_inputs(spec, seed)
        w = walk(spec, inputs, roots)
        x, best, grid = brute_force(w['g'], inputs)
        at = grid[tuple(w['x'][v] for v in w['g'].var_order)]
        np.testing.assert_allclose(w['score'], at, rtol=1e-12)
        assert w['score'] <= best + 1e-9 * abs(best), (name, seed)
        equal += w['x'] == x
    print('%s: the decoded assignment is the brute-force MAP for %d of %d graphs' % (name, equal, len(seeds)))


# ------------------------------------------------------------------------------------------------
# C ABI of libmlbp_map.so
# ------------------------------------------------------------------------------------------------
def _map():
    from macaronicusermodeling_amd import mapdecode
    return mapdecode


def _valid_args(M, X=64, n_msgs=27, n_vars=3):
    """Arguments that pass every host-side check (the pointers are never dereferenced on the host)."""
    a = M.MapArgs()
    a.B, a.X, a.n_msgs, a.P, a.U, a.n_vars = 2, X, n_msgs, 3, 15, n_vars
    a.n_ops, a.n_srcs, a.n_sweeps, a.n_pair_tables, a.n_unary_tables = 10, 4, 1, 6, 30
    a.init_messages, a.normalize_messages, a.write_messages = 1, 1, 0
    for name, typ in M.MapArgs._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, name, 4096)
    return a


def test_library_identity_and_bad_arguments():
    M = _map()
    from macaronicusermodeling_amd import _ffi
    assert M.lib.mlbp_map_arch() == b'gfx950'
    assert M.lib.mlbp_map_last_kernel() in (M.KERNEL_NONE, M.KERNEL_X64, M.KERNEL_GENERIC)
    assert M.lib.mlbp_map_sweep_f64(None, None) == _ffi.MLBP_EINVAL and 'NULL' in M.last_error()
    for field, value, word in (('B', 0, 'sizes'), ('X', 1, 'two states'), ('ops', None, 'NULL'), ('in_off', None, 'NULL'),
                               ('pair_tab', None, 'pair_tab'), ('unary_var', None, 'unary_var'), ('n_pair_tables', 0, 'pair_tables')):
        a = _valid_args(M)
        setattr(a, field, value)
        assert M.lib.mlbp_map_sweep_f64(ctypes.byref(a), None) == _ffi.MLBP_EINVAL, field
        assert word in M.last_error(), (field, M.last_error())
        assert M.lib.mlbp_map_last_kernel() == M.KERNEL_NONE
    a = _valid_args(M)
    a.msgs, a.write_messages = None, 1                         # no buffer to write the messages to
    assert M.lib.mlbp_map_sweep_f64(ctypes.byref(a), None) == _ffi.MLBP_EINVAL and 'msgs' in M.last_error()
    a = _valid_args(M, X=128)
    a.msgs = None                                              # the generic kernel keeps its messages there
    assert M.lib.mlbp_map_sweep_f64(ctypes.byref(a), None) == _ffi.MLBP_EINVAL and 'msgs' in M.last_error()
    a = _valid_args(M, X=1025)
    assert M.lib.mlbp_map_sweep_f64(ctypes.byref(a), None) == _ffi.MLBP_EUNSUPPORTED and '1024' in M.last_error()
    with pytest.raises(M.MapError):
        M.check(_ffi.MLBP_EINVAL)


def test_compute_entry_fails_loudly_without_a_gpu():
    import torch
    M = _map()
    from macaronicusermodeling_amd import _ffi
    if torch.cuda.is_available():
        return                                                  # (the GPU module runs the entry for real)
    a = _valid_args(M)
    assert M.lib.mlbp_map_sweep_f64(ctypes.byref(a), None) == _ffi.MLBP_ENODEVICE
    assert 'no CPU fallback' in M.last_error() and M.lib.mlbp_map_last_kernel() == M.KERNEL_NONE


def test_kernel_choice_is_the_rule_of_the_header():
    M = _map()
    from macaronicusermodeling_amd import _ffi

    def rule(X, n_msgs, n_vars):
        fits = n_msgs * 512 + 4608 + 4 * ((n_vars + 3) // 4 * 4) <= M.X64_LDS_BYTES
        return M.KERNEL_X64 if X == 64 and fits else M.KERNEL_GENERIC
    for X, n_msgs, n_vars in ((64, 27, 3), (64, 126, 7), (64, 150, 4), (64, 151, 4), (64, 152, 4), (64, 288, 12), (63, 27, 3), (128, 27, 3),
                              (2, 1, 1), (1024, 5, 2), (8, 13, 5)):
        assert M.pick_kernel(X, n_msgs, n_vars) == rule(X, n_msgs, n_vars), (X, n_msgs, n_vars)
    assert M.pick_kernel(64, 126, 7) == M.KERNEL_X64 and M.pick_kernel(64, 288, 12) == M.KERNEL_GENERIC      # K7, K12
    assert M.pick_kernel(64, 150, 4) == M.KERNEL_X64 and M.pick_kernel(64, 151, 4) == M.KERNEL_GENERIC       # 151 slots + the assignment: 81 936 B
    assert M.lib.mlbp_map_pick_kernel(1025, 5, 2) == _ffi.MLBP_EUNSUPPORTED
    assert M.lib.mlbp_map_pick_kernel(1, 5, 2) == _ffi.MLBP_EINVAL


def test_program_checks_refuse_what_would_index_outside_a_buffer():
    M = _map()
    from macaronicusermodeling_amd import _ffi
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(C.user_spec(10, [1, 4, 7], 64, 64, seed=1))
    ops, srcs, sweeps = topo.compile_program([1, 4, 7])
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)          # noqa: E731

    def check(ops, srcs, sweeps, n_msgs=topo.n_msgs, P=topo.P, U=topo.U):
        o, s, w = i32(ops), i32(srcs), i32(sweeps)
        return M.lib.mlbp_map_check_program(_ffi.i32ptr(o), len(o) // 4, _ffi.i32ptr(s), len(s), _ffi.i32ptr(w), len(w) // 2, n_msgs, P, U)
    assert check(ops, srcs, sweeps) == _ffi.MLBP_OK
    kinds = ops[:, 0]
    for row, col, value, word in ((0, 3, topo.n_msgs, 'destination'), (int(np.argmax(kinds == _ffi.OP_PAIR_TM)), 1, topo.P, 'pair slot'),
                                  (int(np.argmax(kinds == _ffi.OP_PAIR_MT)), 2, -1, 'source slot'),
                                  (int(np.argmax(kinds == _ffi.OP_UNARY)), 1, topo.U, 'unary slot'),
                                  (int(np.argmax(kinds == _ffi.OP_VAR)), 2, len(srcs) + 1, 'srcs range'), (0, 0, 7, 'unknown kind')):
        bad = ops.copy()
        bad[row, col] = value
        assert check(bad, srcs, sweeps) == _ffi.MLBP_EINVAL and word in M.last_error(), (word, M.last_error())
    bad = srcs.copy()
    bad[0] = topo.n_msgs
    assert check(ops, bad, sweeps) == _ffi.MLBP_EINVAL and 'source slot' in M.last_error()
    bad = sweeps.copy()
    bad[-1, 1] += 1
    assert check(ops, srcs, bad) == _ffi.MLBP_EINVAL and 'sweep' in M.last_error()
    assert M.lib.mlbp_map_check_program(None, 1, None, 0, None, 1, 1, 0, 0) == _ffi.MLBP_EINVAL and 'NULL' in M.last_error()
    # the read-out arrays
    pav, uv = M.readout_arrays(topo)

    def readout(in_off=topo.in_off, in_slots=topo.in_slots, pav=pav, uv=uv):
        return M.lib.mlbp_map_check_readout(topo.n_vars, _ffi.i32ptr(i32(in_off)), _ffi.i32ptr(i32(in_slots)), topo.n_msgs, topo.P,
                                            _ffi.i32ptr(i32(pav)), topo.U, _ffi.i32ptr(i32(uv)))
    assert readout() == _ffi.MLBP_OK
    bad = topo.in_slots.copy(); bad[-1] = topo.n_msgs
    assert readout(in_slots=bad) == _ffi.MLBP_EINVAL and 'slot' in M.last_error()
    bad = pav.copy(); bad[0, 1] = topo.n_vars
    assert readout(pav=bad) == _ffi.MLBP_EINVAL and 'pair factor' in M.last_error()
    bad = uv.copy(); bad[0] = -1
    assert readout(uv=bad) == _ffi.MLBP_EINVAL and 'unary factor' in M.last_error()
    bad = topo.in_off.copy(); bad[1] = bad[2] + 1
    assert readout(in_off=bad) == _ffi.MLBP_EINVAL and 'monotone' in M.last_error()


def test_readout_arrays_follow_the_table_axes():
    """pair_axis_var[p] = (variable on axis 0, variable on axis 1): star_spec puts the hub on axis 1 of odd factors and on axis 0
    of even ones, and lists it second in the varset either way."""
    M = _map()
    from macaronicusermodeling_amd.topology import GraphTopology
    spec = C.star_spec(4, 8)
    topo = GraphTopology.from_spec(spec)
    pav, uv = M.readout_arrays(topo)
    by_id = {f['id']: f for f in spec['factors']}
    for p, j in enumerate(topo.pair_factors):
        f = by_id[topo.factor_ids[j]]
        want = [topo.var_index[v] for _, v in sorted(zip(f['dims'], f['vars']))]
        assert list(pav[p]) == want
    hub = topo.var_index[0]
    assert sorted(int(r[0] == hub) for r in pav) == [0, 0, 1, 1] and all((r[0] == hub) != (r[1] == hub) for r in pav)
    assert list(uv) == [topo.var_index[by_id[topo.factor_ids[j]]['vars'][0]] for j in topo.unary_factors]
