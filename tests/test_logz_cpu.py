"""log Z and the joint log-likelihood without a GPU: the float64 NumPy statement of the formula the GPU tests compare against,
pinned on exhaustive enumeration (trees) and on the Bethe free energy of the beliefs (loopy graphs); the C ABI of
libmlbp_logz.so (the contract it shares with the other side libraries is in tests/test_side_libraries_cpu.py).

The statement reads factor->variable messages only (include/mlbp_logz.h):
    log Z = sum_f log Z_f - sum_v (d_v - 1) log Z_v,    Z_f = the factor's table contracted with the leave-one-out products of
its variables, Z_v = the sum of the product of all messages into v; products are pure products (no uniform 1/X, no nan_to_num).
A variable with one factor has weight 0 and is left out.  Messages come from the oracle's own sweeps."""
import ctypes

import numpy as np
import pytest

import cases as C
import test_map_cpu as W
from oracle import lbp_oracle as O


# ------------------------------------------------------------------------------------------------
# the NumPy statement
# ------------------------------------------------------------------------------------------------
def leave_one_out(g, msgs, v, skip=None):
    acc = np.ones(g.X)
    for fid in g.facset[v]:
        if fid != skip:
            acc = acc * msgs['F_%d' % fid, 'X_%d' % v]
    return acc


def log_partition(g, inputs, msgs):
    """log Z by the message form; msgs: the oracle's message dict."""
    total = 0.0
    with np.errstate(divide='ignore'):
        for f in g.factors:
            T = O.factor_table(g, inputs, f)
            if len(f['vars']) == 1:
                z = np.sum(T.reshape(-1) * leave_one_out(g, msgs, f['vars'][0], f['id']))
            else:
                by_axis = {g.dim_of(f, v): v for v in f['vars']}
                z = leave_one_out(g, msgs, by_axis[0], f['id']).dot(T).dot(leave_one_out(g, msgs, by_axis[1], f['id']))
            total += np.log(z)
        for v in g.var_order:
            d = len(g.facset[v])
            if d != 1:
                total -= (d - 1) * np.log(np.sum(leave_one_out(g, msgs, v)))
    return float(total)


def joint_logp(g, inputs, msgs, x):
    """(log Z, score(x), score(x) - log Z); x: {variable id: state}."""
    lz = log_partition(g, inputs, msgs)
    sc = W.score_of(g, inputs, x)
    return lz, sc, sc - lz


def sweeps(spec, inputs, roots, normalize=True):
    """(graph, messages) after the oracle's sum-product sweeps; normalize=False leaves every message unnormalised (the
    oracle's own schedule, product of incoming messages and contraction, without the renormalisation)."""
    g = O.Graph(spec)
    msgs = O.init_messages(g)
    for r in roots:
        if normalize:
            O.sweep(g, inputs, msgs, r)
        else:
            _raw_sweep(g, inputs, msgs, r)
    return g, msgs


def _raw_send(g, inputs, msgs, frm, to):
    if to[0] == O.FAC and len(g.by_id[to[1]]['vars']) < 2:
        return
    if frm[0] == O.VAR:
        msgs['X_%d' % frm[1], 'F_%d' % to[1]] = O._product_of_incoming(g, msgs, frm[1], skip=to[1])
        return
    f = g.by_id[frm[1]]
    T = O.factor_table(g, inputs, f)
    if len(f['vars']) == 1:
        out = np.copy(T).reshape(-1)
    else:
        other = [u for u in f['vars'] if u != to[1]][0]
        m = msgs['X_%d' % other, 'F_%d' % frm[1]]
        out = T.dot(m) if g.dim_of(f, other) == 1 else m.dot(T)
    msgs['F_%d' % frm[1], 'X_%d' % to[1]] = out


def _raw_sweep(g, inputs, msgs, root):
    sched = O.message_schedule(g, root)
    for child, parent in reversed(sched):
        _raw_send(g, inputs, msgs, child, parent)
    for child, parent in sched:
        _raw_send(g, inputs, msgs, parent, child)


def logsumexp(a):
    m = a.max()
    return float(m + np.log(np.sum(np.exp(a - m))))


def bethe_from_beliefs(g, inputs, msgs):
    """-F_Bethe of the beliefs: sum_f sum b_f log(T_f / b_f) + sum_v (d_v - 1) sum b_v log b_v.  A pairwise factor's belief is
    O.factor_beliefs; a unary factor's belief is its variable's marginal (O.marginal) -- O.factor_beliefs returns the
    normalised table alone for a unary factor, which is no belief."""
    def xlogy(b, y):
        out = np.zeros_like(b)
        nz = b > 0
        out[nz] = b[nz] * np.log(y[nz])
        return out
    total = 0.0
    for f in g.factors:
        T = O.factor_table(g, inputs, f)
        if len(f['vars']) == 1:
            b = O.marginal(g, msgs, f['vars'][0])
            total += np.sum(xlogy(b, T.reshape(-1)) - xlogy(b, b))
        else:
            b = np.asarray(O.factor_beliefs(g, inputs, msgs, f['id']))
            total += np.sum(xlogy(b, T) - xlogy(b, b))
    for v in g.var_order:
        b = O.marginal(g, msgs, v)
        total += (len(g.facset[v]) - 1) * np.sum(xlogy(b, b))
    return float(total)


# ------------------------------------------------------------------------------------------------
# trees: exact
# ------------------------------------------------------------------------------------------------
def _check_tree(name, spec, inputs, roots, rs):
    g, msgs = sweeps(spec, inputs, roots)
    _, _, grid = W.brute_force(g, inputs)
    lse = logsumexp(grid)
    lz = log_partition(g, inputs, msgs)
    np.testing.assert_allclose(lz, lse, rtol=1e-12, err_msg=name)
    x = {v: int(rs.randint(g.X)) for v in g.var_order}
    _, sc, jl = joint_logp(g, inputs, msgs, x)
    at = grid[tuple(x[v] for v in g.var_order)]
    np.testing.assert_allclose(sc, at, rtol=1e-12, err_msg=name)
    np.testing.assert_allclose(jl, at - lse, rtol=1e-12, atol=1e-12 * abs(lse), err_msg=name)
    # joint_logp is a log-probability: it sums to one over the whole grid
    assert abs(np.sum(np.exp(grid - lz)) - 1.0) <= 1e-12 * max(1.0, abs(lz)) + 1e-13, name
    # ... and does not depend on the scale of any message
    g2, raw = sweeps(spec, inputs, roots, normalize=False)
    np.testing.assert_allclose(log_partition(g2, inputs, raw), lz, rtol=1e-12, err_msg=name + ' unnormalised')
    return abs(lz - lse) / abs(lse)


@pytest.mark.parametrize('name,make,roots,kind', W.TREE_CASES, ids=[c[0] for c in W.TREE_CASES])
def test_log_z_is_exact_on_trees(name, make, roots, kind):
    spec = make()
    rs = np.random.RandomState(11)
    worst = max(_check_tree(name, spec, C.make_inputs(spec, seed, kind), roots, rs) for seed in range(40))
    print('%s: 40 seeds, log Z against logsumexp of the grid: worst relative difference %.2e' % (name, worst))


def test_log_z_is_exact_on_random_trees():
    trees = W.random_trees()
    assert len(trees) >= 5
    rs = np.random.RandomState(12)
    worst = 0.0
    for i, spec in enumerate(trees):
        for seed in range(40):
            worst = max(worst, _check_tree(spec['name'], spec, C.make_inputs(spec, 1000 * i + seed), [spec['var_ids'][0]], rs))
    print('random trees: %d graphs x 40 seeds, worst relative difference %.2e' % (len(trees), worst))


# ------------------------------------------------------------------------------------------------
# loopy graphs: the Bethe value
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,make,seeds,roots', [
    ('ring5_x8', lambda: C.ring_spec(5, 8), (500, 501, 502), [0, 2, 4]),
    ('user_k3_x64', lambda: C.user_spec(10, [1, 4, 7], 64, 64, seed=1), (500, 501, 502), [1, 4, 7])], ids=['ring5_x8', 'user_k3_x64'])
def test_message_form_is_the_bethe_value_on_loopy_graphs(name, make, seeds, roots):
    spec = make()
    for seed in seeds:
        inputs = C.make_inputs(spec, seed)
        g, m40 = sweeps(spec, inputs, [roots[i % len(roots)] for i in range(40)])
        lz40 = log_partition(g, inputs, m40)
        bethe = bethe_from_beliefs(g, inputs, m40)
        _, m3 = sweeps(spec, inputs, roots)
        lz3 = log_partition(g, inputs, m3)
        print('%s seed %d: log Z %.12f, -F_Bethe(beliefs, 40 sweeps) differs by %.2e, the 3-sweep value by %.2e, '
              '-F_Bethe(beliefs, 3 sweeps) by %.2e' % (name, seed, lz40, abs(lz40 - bethe), abs(lz3 - lz40),
                                                         abs(bethe_from_beliefs(g, inputs, m3) - lz40)))
        np.testing.assert_allclose(lz40, bethe, rtol=0, atol=1e-9, err_msg='%s seed %d' % (name, seed))
        _, raw = sweeps(spec, inputs, roots, normalize=False)
        np.testing.assert_allclose(log_partition(g, inputs, raw), lz3, rtol=1e-12)


# ------------------------------------------------------------------------------------------------
# C ABI of libmlbp_logz.so
# ------------------------------------------------------------------------------------------------
def _logz():
    from macaronicusermodeling_amd import logz
    return logz


def _valid_args(L, X=64):
    """Arguments that pass every host-side check (the pointers are never dereferenced on the host)."""
    a = L.LogzArgs()
    a.B, a.X, a.n_msgs, a.P, a.U, a.n_vars = 2, X, 27, 3, 15, 3
    a.n_pair_tables, a.n_unary_tables, a.flags = 6, 30, 0
    for name, typ in L.LogzArgs._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, name, 4096)
    return a


def test_library_identity_and_bad_arguments():
    L = _logz()
    from macaronicusermodeling_amd import _ffi
    assert L.lib.mlbp_logz_arch() == b'gfx950'
    assert L.lib.mlbp_logz_f64(None, None) == _ffi.MLBP_EINVAL and 'NULL' in L.last_error()
    for field, value, word in (('B', 0, 'sizes'), ('X', 1, 'two states'), ('msgs', None, 'msgs'), ('in_off', None, 'in_off'),
                               ('pair_tab', None, 'pair_tab'), ('pair_in_slot', None, 'pair_in_slot'),
                               ('unary_in_slot', None, 'unary_in_slot'), ('n_pair_tables', 0, 'pair_tables'),
                               ('labels', None, 'labels'), ('log_z', None, 'sum_out'), ('flags', 2, 'flags')):
        a = _valid_args(L)
        setattr(a, field, value)
        assert L.lib.mlbp_logz_f64(ctypes.byref(a), None) == _ffi.MLBP_EINVAL, field
        assert word in L.last_error(), (field, L.last_error())
        assert L.lib.mlbp_logz_last_kernel() == L.KERNEL_NONE
    a = _valid_args(L)
    a.log_z = a.score = a.joint_logp = a.sum_out = None
    assert L.lib.mlbp_logz_f64(ctypes.byref(a), None) == _ffi.MLBP_EINVAL and 'nothing to compute' in L.last_error()
    a = _valid_args(L, X=1025)
    assert L.lib.mlbp_logz_f64(ctypes.byref(a), None) == _ffi.MLBP_EUNSUPPORTED and '1024' in L.last_error()
    with pytest.raises(L.LogzError):
        L.check(_ffi.MLBP_EINVAL)


def test_compute_entry_fails_loudly_without_a_gpu():
    import torch
    L = _logz()
    from macaronicusermodeling_amd import _ffi
    if torch.cuda.is_available():
        return                                                  # (the GPU module runs the entry for real)
    for flags in (0, L.SHARED_PAIR_TABLES):
        a = _valid_args(L)
        a.flags = flags
        assert L.lib.mlbp_logz_f64(ctypes.byref(a), None) == _ffi.MLBP_ENODEVICE
        assert 'no CPU fallback' in L.last_error() and L.lib.mlbp_logz_last_kernel() == L.KERNEL_NONE


def test_kernel_choice_is_the_rule_of_the_header():
    L = _logz()
    from macaronicusermodeling_amd import _ffi

    def rule(X, n_in, n_vars, flags):
        if X == 64 and flags & L.SHARED_PAIR_TABLES:
            return L.KERNEL_X64_SHARED
        if X == 64 and n_in * 512 + 4096 + 64 <= L.X64_LDS_BYTES:
            return L.KERNEL_X64
        return L.KERNEL_GENERIC
    for X, n_in, n_vars in ((64, 21, 3), (64, 84, 7), (64, 119, 4), (64, 120, 4), (64, 300, 12), (63, 21, 3), (128, 21, 3), (2, 1, 1),
                            (1024, 5, 2), (8, 13, 5)):
        for flags in (0, 1):
            assert L.pick_kernel(X, n_in, n_vars, flags) == rule(X, n_in, n_vars, flags), (X, n_in, n_vars, flags)
    assert L.pick_kernel(64, 84, 7) == L.KERNEL_X64 and L.pick_kernel(64, 120, 4) == L.KERNEL_GENERIC
    assert L.pick_kernel(64, 300, 12, 1) == L.KERNEL_X64_SHARED and L.pick_kernel(128, 21, 3, 1) == L.KERNEL_GENERIC
    assert L.lib.mlbp_logz_pick_kernel(1025, 5, 2, 0) == _ffi.MLBP_EUNSUPPORTED
    assert L.lib.mlbp_logz_pick_kernel(1, 5, 2, 0) == _ffi.MLBP_EINVAL
    assert L.lib.mlbp_logz_pick_kernel(64, 5, 2, 4) == _ffi.MLBP_EINVAL and 'flags' in L.last_error()


def test_readout_check_refuses_what_would_index_outside_a_buffer():
    L = _logz()
    from macaronicusermodeling_amd import _ffi
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(C.user_spec(10, [1, 4, 7], 64, 64, seed=1))
    pav, uv, pis, uis = L.readout_arrays(topo)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)          # noqa: E731

    def readout(in_off=topo.in_off, in_slots=topo.in_slots, pav=pav, uv=uv, pis=pis, uis=uis, P=topo.P, U=topo.U):
        return L.lib.mlbp_logz_check_readout(topo.n_vars, _ffi.i32ptr(i32(in_off)), _ffi.i32ptr(i32(in_slots)), topo.n_msgs, P,
                                             _ffi.i32ptr(i32(pav)), _ffi.i32ptr(i32(pis)), U, _ffi.i32ptr(i32(uv)), _ffi.i32ptr(i32(uis)))
    assert readout() == _ffi.MLBP_OK
    assert int(topo.in_off[-1]) == 2 * topo.P + topo.U
    bad = topo.in_slots.copy(); bad[-1] = topo.n_msgs
    assert readout(in_slots=bad) == _ffi.MLBP_EINVAL and 'slot' in L.last_error()
    bad = topo.in_slots.copy(); bad[0] = -1
    assert readout(in_slots=bad) == _ffi.MLBP_EINVAL and 'slot' in L.last_error()
    bad = pav.copy(); bad[0, 1] = topo.n_vars
    assert readout(pav=bad) == _ffi.MLBP_EINVAL and 'pair factor' in L.last_error()
    bad = uv.copy(); bad[0] = -1
    assert readout(uv=bad) == _ffi.MLBP_EINVAL and 'unary factor' in L.last_error()
    bad = topo.in_off.copy(); bad[1] = bad[2] + 1
    assert readout(in_off=bad) == _ffi.MLBP_EINVAL and 'monotone' in L.last_error()
    bad = topo.in_off.copy(); bad[-1] += 1
    assert readout(in_off=bad) == _ffi.MLBP_EINVAL and '2 P + U' in L.last_error()
    assert readout(U=topo.U - 1) == _ffi.MLBP_EINVAL and '2 P + U' in L.last_error()
    # a slot that exists but belongs to the factor's OTHER variable, or to a variable->factor message
    bad = pis.copy(); bad[0] = bad[0, ::-1]
    assert readout(pis=bad) == _ffi.MLBP_EINVAL and 'no in-slot' in L.last_error() and 'pair factor 0' in L.last_error()
    v2f = [int(s) for s in topo.v2f if s >= 0]
    bad = pis.copy(); bad[1, 0] = v2f[0]
    assert readout(pis=bad) == _ffi.MLBP_EINVAL and 'no in-slot' in L.last_error()
    other = int(np.argmax(uv != uv[0]))
    bad = uis.copy(); bad[0] = uis[other]
    assert readout(uis=bad) == _ffi.MLBP_EINVAL and 'no in-slot' in L.last_error() and 'unary factor 0' in L.last_error()
    assert L.lib.mlbp_logz_check_readout(1, None, None, 1, 0, None, None, 1, None, None) == _ffi.MLBP_EINVAL and 'NULL' in L.last_error()


def test_readout_arrays_follow_the_table_axes_and_f2v():
    """pair_axis_var[p] / pair_in_slot[p] are ordered by TABLE AXIS: star_spec puts the hub on axis 1 of odd factors and on
    axis 0 of even ones.  Every slot is the factor->variable slot of that incidence by name."""
    L = _logz()
    from macaronicusermodeling_amd.topology import GraphTopology
    spec = C.star_spec(4, 8)
    topo = GraphTopology.from_spec(spec)
    pav, uv, pis, uis = L.readout_arrays(topo)
    keys = topo.slot_keys()
    by_id = {f['id']: f for f in spec['factors']}
    for p, j in enumerate(topo.pair_factors):
        f = by_id[topo.factor_ids[j]]
        want = [v for _, v in sorted(zip(f['dims'], f['vars']))]
        assert [topo.var_ids[v] for v in pav[p]] == want
        assert [keys[s] for s in pis[p]] == [('F_%d' % f['id'], 'X_%d' % v) for v in want]
    for u, j in enumerate(topo.unary_factors):
        f = by_id[topo.factor_ids[j]]
        assert topo.var_ids[uv[u]] == f['vars'][0] and keys[uis[u]] == ('F_%d' % f['id'], 'X_%d' % f['vars'][0])
    assert sorted(list(pis.reshape(-1)) + list(uis)) == sorted(int(s) for s in topo.in_slots)
