"""Posterior sampling without a GPU: the float64 NumPy walk the GPU tests compare against, pinned on exhaustive enumeration;
the draw rule on dyadic marginals; and the host checks of libmlbp_sample.so
(the contract it shares with the other side libraries is in tests/test_side_libraries_cpu.py).

The walk is the semantics of include/mlbp_sample.h written with the oracle's own functions: schedule, initial messages,
the product of incoming messages, the factor-to-variable update and renormalisation are oracle/lbp_oracle.py's;
O.var_to_factor is restated with ONE change -- the indicator of a clamped variable's state is folded into its outgoing
message, followed by np.nan_to_num.  The reference has no sampler, so the walk itself is pinned on brute force: on a tree
log q(x) must equal log p(x) = grid[x] - logsumexp(grid) for EVERY assignment x and every conditional marginal must equal the
exact conditional read off the grid; on a loopy graph q must still be a distribution (sum to one) while differing from p."""
import ctypes
import itertools

import numpy as np
import pytest

import cases as C
import helpers
import test_map_cpu as W
from oracle import lbp_oracle as O


# ------------------------------------------------------------------------------------------------
# the NumPy walk
# ------------------------------------------------------------------------------------------------
def sc_var_to_factor(g, msgs, v, fid, clamp, normalize=True):
    """O.var_to_factor with the indicator of a clamped variable's state folded in."""
    acc = O._product_of_incoming(g, msgs, v, skip=fid)
    if v in clamp:
        ind = np.zeros(g.X)
        ind[clamp[v]] = 1.0
        acc = np.nan_to_num(acc * ind)
    msgs['X_%d' % v, 'F_%d' % fid] = O.renormalize(acc) if normalize else acc


def _raw_factor_to_var(g, inputs, msgs, fid, v):
    """O.factor_to_var without the renormalisation (normalize_messages = 0 only)."""
    f = g.by_id[fid]
    T = O.factor_table(g, inputs, f)
    if len(f['vars']) == 1:
        out = np.copy(T).reshape(-1)
    else:
        other = [u for u in f['vars'] if u != v][0]
        m = msgs['X_%d' % other, 'F_%d' % fid]
        out = T.dot(m) if g.dim_of(f, other) == 1 else m.dot(T)
    msgs['F_%d' % fid, 'X_%d' % v] = out


def _sc_send(g, inputs, msgs, frm, to, clamp, normalize):
    if to[0] == O.FAC and len(g.by_id[to[1]]['vars']) < 2:
        return
    if frm[0] == O.VAR:
        sc_var_to_factor(g, msgs, frm[1], to[1], clamp, normalize)
    elif normalize:
        O.factor_to_var(g, inputs, msgs, frm[1], to[1])
    else:
        _raw_factor_to_var(g, inputs, msgs, frm[1], to[1])


def sc_sweep(g, inputs, msgs, root, clamp, normalize=True):
    sched = O.message_schedule(g, root)
    for child, parent in reversed(sched):
        _sc_send(g, inputs, msgs, child, parent, clamp, normalize)
    for child, parent in sched:
        _sc_send(g, inputs, msgs, parent, child, clamp, normalize)


def step_marginal(g, inputs, roots, clamp, v, normalize=True):
    """Steps 1 to 3: uniform messages, the sweeps on the clamped model, the marginal of v (always normalised)."""
    msgs = O.init_messages(g)
    for r in roots:
        sc_sweep(g, inputs, msgs, r, clamp, normalize)
    return O.renormalize(O._product_of_incoming(g, msgs, v))


def draw(m, u):
    """Step 4 -> (state, margin): the lowest i with cumsum(m)_i > u * cumsum(m)_{X-1}, else the highest i with m_i > 0;
    margin = min_i |c_i - t|.  The empty marginal (no m_i > 0) gives state 0 whatever u is: margin inf, as for a given
    variable."""
    c = np.cumsum(m)
    t = u * c[-1]
    above = np.nonzero(c > t)[0]
    positive = np.nonzero(m > 0)[0]
    if not len(above) and not len(positive):
        return 0, np.inf
    x = int(above[0]) if len(above) else int(positive[-1])
    return x, float(np.abs(c - t).min())


def walk(spec, inputs, roots, uniforms, order=None, given=None, normalize=True):
    """One sample of one graph.  uniforms: [n_vars] indexed by step; order: variable ids (default g.var_order); given:
    {variable id: state} (missing or -1: draw).  -> dict(g, x {v: state}, logq, cm {v: conditional marginal},
    margin {v: min_i |c_i - t|, inf for a given variable})."""
    g = O.Graph(spec)
    order = list(g.var_order) if order is None else list(order)
    assert sorted(order) == sorted(g.var_order)
    given = {} if given is None else given
    clamp, cm, margin, logq = {}, {}, {}, 0.0
    for k, v in enumerate(order):
        m = cm[v] = step_marginal(g, inputs, roots, clamp, v, normalize)
        if given.get(v, -1) >= 0:
            xv, margin[v] = int(given[v]), np.inf
        else:
            xv, margin[v] = draw(m, float(uniforms[k]))
        with np.errstate(divide='ignore'):
            logq += np.log(m[xv])
        clamp[v] = xv
    return dict(g=g, x=dict(clamp), logq=float(logq), cm=cm, margin=margin)


def enumerate_q(spec, inputs, roots, order=None):
    """walk() with `given` set to every one of the X^n assignments: -> (logq grid [X]*n in g.var_order axes, nodes), nodes =
    [(prefix {v: state}, v, conditional marginal)] for every clamped prefix.  The marginal of a step depends on the clamped
    prefix alone, so assignments that share a prefix share its steps (computed once, by step_marginal as walk() calls it)."""
    g = O.Graph(spec)
    order = list(g.var_order) if order is None else list(order)
    n, X = len(order), g.X
    axis = {v: g.var_order.index(v) for v in order}
    logq = np.zeros((X,) * n)
    nodes = []

    def descend(k, clamp, acc):
        if k == n:
            logq[tuple(clamp[v] for v in g.var_order)] = acc
            return
        v = order[k]
        m = step_marginal(g, inputs, roots, clamp, v)
        nodes.append((dict(clamp), v, m))
        with np.errstate(divide='ignore'):
            lm = np.log(m)
        for x in range(X):
            clamp[v] = x
            descend(k + 1, clamp, acc + lm[x])
        del clamp[v]
    descend(0, {}, 0.0)
    assert len(axis) == n
    return g, logq, nodes


def logsumexp(a):
    top = a.max()
    return float(top + np.log(np.exp(a - top).sum()))


def exact_conditional(g, grid, prefix, v):
    """p(x_v | prefix) from the grid of summed log-potentials."""
    index = tuple(prefix.get(u, slice(None)) for u in g.var_order)
    sub = grid[index]
    free = [u for u in g.var_order if u not in prefix]
    w = np.exp(sub - sub.max())
    w = w.sum(axis=tuple(i for i, u in enumerate(free) if u != v))
    return w / w.sum()


MAX_ENUM_VARS = 6        # X^n assignments with X = 4: 4096 leaves, 1365 clamped prefixes per order


def small_random_trees():
    """The loop-free graphs among test_map_cpu's 60 draws of helpers.random_spec(RandomState(7), ..., X=4) whose X^n
    assignments can be enumerated (at most MAX_ENUM_VARS variables)."""
    return [s for s in W.random_trees() if len(s['var_ids']) <= MAX_ENUM_VARS]


def _two_orders(spec):
    ids = list(O.Graph(spec).var_order)
    return [ids, ids[::-1][1:] + ids[::-1][:1]]          # var_ids order; reversed and rotated by one


TREES = [('chain4_x3', lambda: C.chain_spec(4, 3)), ('star4_x3', lambda: C.star_spec(4, 3)), ('chain5_x4', lambda: C.chain_spec(5, 4))]


def _check_tree(name, spec, inputs):
    worst_q = worst_m = 0.0
    for order in _two_orders(spec):
        root = [order[0]]                                   # one sweep; the root differs between the two orders
        g, logq, nodes = enumerate_q(spec, inputs, root, order)
        _, _, grid = W.brute_force(g, inputs)
        logp = grid - logsumexp(grid)
        np.testing.assert_allclose(logq, logp, rtol=1e-10, err_msg='%s order %r' % (name, order))
        worst_q = max(worst_q, float(np.abs(logq - logp).max()))
        for prefix, v, m in nodes:
            want = exact_conditional(g, grid, prefix, v)
            np.testing.assert_allclose(m, want, rtol=1e-10, err_msg='%s prefix %r variable %d' % (name, prefix, v))
            worst_m = max(worst_m, float(np.abs(m / want - 1).max()))
    return worst_q, worst_m


@pytest.mark.parametrize('name,make', TREES, ids=[t[0] for t in TREES])
def test_walk_is_exact_on_trees(name, make):
    spec = make()
    for seed, kind in ((3, 'uniform'), (4, 'lognormal')):
        wq, wm = _check_tree(name, spec, C.make_inputs(spec, seed, kind))
        print('%s seed %d: max |log q - log p| %.1e over all assignments, conditionals within %.1e relative' % (name, seed, wq, wm))


def test_walk_is_exact_on_random_trees():
    trees = small_random_trees()
    assert len(trees) >= 3, len(trees)
    for i, spec in enumerate(trees):
        wq, wm = _check_tree(spec['name'], spec, C.make_inputs(spec, i))
        print('%s (%d variables): max |log q - log p| %.1e, conditionals within %.1e relative' % (spec['name'], len(spec['var_ids']), wq, wm))


def test_walk_is_exact_on_the_larger_random_trees_at_sampled_assignments():
    """The loop-free draws with 7 to 9 variables have 4^7 to 4^9 assignments and as many clamped prefixes to sweep: too many to
    walk one by one.  Their grid is still summed exactly, and the walk is held to it on 24 seeded assignments each, for the
    same two orders: log q = log p and every conditional marginal along the way."""
    trees = [s for s in W.random_trees() if len(s['var_ids']) > MAX_ENUM_VARS]
    assert len(trees) + len(small_random_trees()) == len(W.random_trees()) and trees
    rs = np.random.RandomState(11)
    for i, spec in enumerate(trees):
        inputs = C.make_inputs(spec, 100 + i)
        g = O.Graph(spec)
        _, _, grid = W.brute_force(g, inputs)
        log_z = logsumexp(grid)
        worst = 0.0
        for order in _two_orders(spec):
            for _ in range(12):
                x = {v: int(rs.randint(g.X)) for v in g.var_order}
                w = walk(spec, inputs, [order[0]], None, order=order, given=x)
                want = grid[tuple(x[v] for v in g.var_order)] - log_z
                np.testing.assert_allclose(w['logq'], want, rtol=1e-10, err_msg=spec['name'])
                worst = max(worst, abs(w['logq'] - want))
                for k, v in enumerate(order):
                    prefix = {u: x[u] for u in order[:k]}
                    np.testing.assert_allclose(w['cm'][v], exact_conditional(g, grid, prefix, v), rtol=1e-10, err_msg=spec['name'])
        print('%s (%d variables): max |log q - log p| %.1e over 24 assignments' % (spec['name'], len(g.var_order), worst))


def test_enumeration_is_the_walk_with_given():
    """enumerate_q shares prefixes; walk() with `given` set to single assignments gives the same log q, conditional marginals
    and states -- and needs no uniforms."""
    spec = C.star_spec(4, 3)
    inputs = C.make_inputs(spec, 3)
    order = _two_orders(spec)[1]
    g, logq, _ = enumerate_q(spec, inputs, [order[0]], order)
    rs = np.random.RandomState(0)
    for _ in range(12):
        x = {v: int(rs.randint(3)) for v in g.var_order}
        w = walk(spec, inputs, [order[0]], None, order=order, given=x)
        assert w['x'] == x and w['logq'] == logq[tuple(x[v] for v in g.var_order)]
        assert all(np.isinf(w['margin'][v]) for v in g.var_order)


LOOPY = [('ring3_x3', lambda: C.ring_spec(3, 3), [0, 1, 2]),
         ('user_k3_x4', lambda: C.user_spec(10, [1, 4, 7], 4, 4, seed=1), [1, 4, 7])]


@pytest.mark.parametrize('name,make,roots', LOOPY, ids=[t[0] for t in LOOPY])
def test_walk_is_a_distribution_on_loopy_graphs(name, make, roots):
    """q sums to one over all assignments; it is NOT p (the approximation is stated, not bounded)."""
    spec = make()
    for seed in (3, 4):
        inputs = C.make_inputs(spec, seed)
        for order in _two_orders(spec):
            g, logq, _ = enumerate_q(spec, inputs, roots, order)
            assert O.has_loops(g, roots[0])
            total = float(np.exp(logq).sum())
            _, _, grid = W.brute_force(g, inputs)
            off = float(np.abs(logq - (grid - logsumexp(grid))).max())
            print('%s seed %d order %r: sum_x q(x) - 1 = %.1e, max |log q - log p| = %.3f' % (name, seed, order, total - 1.0, off))
            assert abs(total - 1.0) <= 1e-12
            assert off > 1e-6


def test_walk_draws_follow_q():
    """Sanity of draw() inside walk(): over a fine grid of uniforms for a two-variable chain the drawn pairs' frequencies are
    q's (exactly p's here) to the grid's resolution."""
    spec = C.chain_spec(2, 3)
    inputs = C.make_inputs(spec, 5)
    g, logq, _ = enumerate_q(spec, inputs, [0])
    n = 60
    us = (np.arange(n) + 0.5) / n
    counts = np.zeros((3, 3))
    for u0, u1 in itertools.product(us, us):
        w = walk(spec, inputs, [0], [u0, u1])
        counts[w['x'][0], w['x'][1]] += 1
        assert w['logq'] == logq[w['x'][0], w['x'][1]]
    np.testing.assert_allclose(counts / n ** 2, np.exp(logq), atol=2.5 / n)


# ------------------------------------------------------------------------------------------------
# the draw rule on dyadic marginals
# ------------------------------------------------------------------------------------------------
def dyadic_case(X=8):
    """A K1 graph (one variable, one unary factor) whose unary row makes m = [1/4, 0, 1/4, 1/2, 0, ...] exactly: the row sums to
    one, uniform = 1/X is a power of two, so renorm(uniform * renorm(row)) = row bit for bit."""
    spec = C.chain_spec(1, X)
    row = np.zeros(X)
    row[[0, 2, 3]] = [0.25, 0.25, 0.5]
    return spec, dict(tables=[row.reshape(X, 1)]), row


DYADIC_DRAWS = [(0.0, 0), (0.25, 2), (0.5, 3), (1.0 - 2.0 ** -53, 3), (0.2499999, 0), (0.4999999, 2)]


@pytest.mark.parametrize('X', [8, 64])
def test_draw_rule_on_dyadic_marginals(X):
    spec, inputs, row = dyadic_case(X)
    for u, state in DYADIC_DRAWS:
        w = walk(spec, inputs, [0], [u])
        assert np.array_equal(w['cm'][0], row)
        assert w['x'][0] == state, (u, w['x'])
        assert w['logq'] == np.log(row[state])
    # u = 0.25: t = 0.25 = c_0 = c_1 -- the comparison is strict, so states 0 and 1 (probability zero) are passed over
    assert draw(row, 0.25) == (2, 0.0)
    # no c_i above t (possible only by rounding): the highest state of positive probability, never a trailing empty one
    assert draw(row, 1.0)[0] == 3
    # a given state of probability zero: log q = -inf
    w = walk(spec, inputs, [0], [0.5], given={0: 1})
    assert w['x'][0] == 1 and np.isneginf(w['logq'])


# ------------------------------------------------------------------------------------------------
# C ABI of libmlbp_sample.so
# ------------------------------------------------------------------------------------------------
def _S():
    from macaronicusermodeling_amd import sample
    return sample


def _valid_args(S, X=64, n_msgs=27, n_vars=3, B=2, n_samples=2):
    """Arguments that pass every host-side check (the pointers are never dereferenced on the host)."""
    a = S.SampleArgs()
    a.B, a.X, a.n_msgs, a.P, a.U, a.n_vars = B, X, n_msgs, 3, 15, n_vars
    a.n_ops, a.n_srcs, a.n_sweeps, a.n_pair_tables, a.n_unary_tables = 10, 4, 1, 6, 30
    a.normalize_messages, a.S = 1, n_samples
    for name, typ in S.SampleArgs._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, name, 4096)
    a.workspace_bytes = 1 << 40
    return a


def test_library_identity_and_bad_arguments():
    S = _S()
    from macaronicusermodeling_amd import _ffi
    assert S.lib.mlbp_sample_arch() == b'gfx950'
    assert S.lib.mlbp_sample_last_kernel() in (S.KERNEL_NONE, S.KERNEL_X64, S.KERNEL_GENERIC)
    assert S.lib.mlbp_sample_f64(None, None) == _ffi.MLBP_EINVAL and 'NULL' in S.last_error()
    for field, value, word in (('B', 0, 'sizes'), ('X', 1, 'two states'), ('S', 0, 'sample'), ('uniforms', None, 'uniforms'),
                               ('ops', None, 'NULL'), ('in_off', None, 'NULL'), ('slot_var', None, 'slot_var'), ('order', None, 'order'),
                               ('samples', None, 'samples'), ('logq', None, 'logq'),
                               ('pair_tab', None, 'pair_tab'), ('n_unary_tables', 0, 'unary_tables')):
        a = _valid_args(S)
        setattr(a, field, value)
        assert S.lib.mlbp_sample_f64(ctypes.byref(a), None) == _ffi.MLBP_EINVAL, field
        assert word in S.last_error(), (field, S.last_error())
        assert S.lib.mlbp_sample_last_kernel() == S.KERNEL_NONE
    # the generic kernel keeps its messages in the workspace: none, or one too small
    a = _valid_args(S, X=128)
    a.workspace = None
    assert S.lib.mlbp_sample_f64(ctypes.byref(a), None) == _ffi.MLBP_EINVAL and 'workspace' in S.last_error()
    a = _valid_args(S, X=128)
    a.workspace_bytes = S.workspace_bytes(a.B, a.S, 128, a.n_msgs, a.n_vars) - 8
    assert S.lib.mlbp_sample_f64(ctypes.byref(a), None) == _ffi.MLBP_EINVAL and 'workspace' in S.last_error()
    a = _valid_args(S, X=1025)
    assert S.lib.mlbp_sample_f64(ctypes.byref(a), None) == _ffi.MLBP_EUNSUPPORTED and '1024' in S.last_error()
    with pytest.raises(S.SampleError):
        S.check(_ffi.MLBP_EINVAL)


def test_compute_entry_fails_loudly_without_a_gpu():
    import torch
    S = _S()
    from macaronicusermodeling_amd import _ffi
    if torch.cuda.is_available():
        return                                                  # (the GPU module runs the entry for real)
    for X in (64, 128):
        a = _valid_args(S, X=X)
        a.given = a.cond_marginals = None                       # both are optional
        if X == 64:
            a.workspace, a.workspace_bytes = None, 0            # the X = 64 kernel needs none
        assert S.lib.mlbp_sample_f64(ctypes.byref(a), None) == _ffi.MLBP_ENODEVICE
        assert 'no CPU fallback' in S.last_error() and S.lib.mlbp_sample_last_kernel() == S.KERNEL_NONE


def test_kernel_choice_chunks_and_workspace_are_the_rules_of_the_header():
    S = _S()
    from macaronicusermodeling_amd import _ffi

    def rule(X, n_msgs, n_vars):
        fits = n_msgs * 512 + 4608 + 512 + 4 * ((n_vars + 3) // 4 * 4) <= S.X64_LDS_BYTES
        return S.KERNEL_X64 if X == 64 and fits else S.KERNEL_GENERIC

    def chunks(B, n_samples):
        return min(n_samples, -(-S.MIN_WORKGROUPS // B))
    shapes = ((64, 27, 3), (64, 126, 7), (64, 149, 4), (64, 150, 4), (64, 149, 128), (64, 149, 129), (64, 288, 12), (63, 27, 3), (128, 27, 3),
              (2, 1, 1), (1024, 5, 2), (8, 13, 5))
    for X, n_msgs, n_vars in shapes:
        assert S.pick_kernel(X, n_msgs, n_vars) == rule(X, n_msgs, n_vars), (X, n_msgs, n_vars)
    # the largest n_msgs that fits and the first that does not; K7 fits, K12 does not
    assert S.pick_kernel(64, 149, 4) == S.KERNEL_X64 and S.pick_kernel(64, 150, 4) == S.KERNEL_GENERIC
    assert S.pick_kernel(64, 149, 128) == S.KERNEL_X64 and S.pick_kernel(64, 149, 129) == S.KERNEL_GENERIC      # 512 bytes of clamp states
    assert S.pick_kernel(64, 126, 7) == S.KERNEL_X64 and S.pick_kernel(64, 288, 12) == S.KERNEL_GENERIC
    assert S.lib.mlbp_sample_pick_kernel(1025, 5, 2) == _ffi.MLBP_EUNSUPPORTED
    assert S.lib.mlbp_sample_pick_kernel(1, 5, 2) == _ffi.MLBP_EINVAL
    for B, n_samples in ((1, 1000), (8192, 32), (1, 5), (3, 1), (257, 3), (600, 2), (256, 2), (256, 3), (511, 7), (512, 7), (513, 7), (2, 255), (2, 257)):
        assert S.chunks(B, n_samples) == chunks(B, n_samples), (B, n_samples)
        for X, n_msgs, n_vars in shapes:
            want = 0 if rule(X, n_msgs, n_vars) == S.KERNEL_X64 else B * chunks(B, n_samples) * n_msgs * X * 8
            assert S.workspace_bytes(B, n_samples, X, n_msgs, n_vars) == want, (B, n_samples, X, n_msgs, n_vars)
    assert (S.chunks(1, 1000), S.chunks(8192, 32), S.chunks(257, 3), S.chunks(600, 2)) == (512, 1, 2, 1)
    assert S.lib.mlbp_sample_chunks(0, 1) == _ffi.MLBP_EINVAL and S.lib.mlbp_sample_chunks(1, 0) == _ffi.MLBP_EINVAL
    assert S.lib.mlbp_sample_workspace_bytes(1, 1, 1025, 5, 2) == _ffi.MLBP_EUNSUPPORTED
    assert S.lib.mlbp_sample_workspace_bytes(0, 1, 64, 5, 2) == _ffi.MLBP_EINVAL
    assert S.workspace_bytes(8192, 32, 1024, 5, 2) == 8192 * 5 * 1024 * 8                      # past 2^31 bytes: 64-bit


def test_program_checks_refuse_what_would_index_outside_a_buffer():
    S = _S()
    from macaronicusermodeling_amd import _ffi
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(C.user_spec(10, [1, 4, 7], 64, 64, seed=1))
    ops, srcs, sweeps = topo.compile_program([1, 4, 7])
    slot_var = S.slot_var_array(topo)
    order = np.arange(topo.n_vars, dtype=np.int32)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)          # noqa: E731

    def check(ops=ops, srcs=srcs, sweeps=sweeps, slot_var=slot_var, order=order, n_vars=topo.n_vars):
        o, s, w, sv, od = i32(ops), i32(srcs), i32(sweeps), i32(slot_var), i32(order)
        return S.lib.mlbp_sample_check_program(_ffi.i32ptr(o), len(o) // 4, _ffi.i32ptr(s), len(s), _ffi.i32ptr(w), len(w) // 2,
                                               topo.n_msgs, topo.P, topo.U, n_vars, _ffi.i32ptr(sv), _ffi.i32ptr(od))
    assert check() == _ffi.MLBP_OK
    # slot_var by name: the source variable of every X -> F slot, -1 for every F -> X slot
    for slot, (frm, to) in enumerate(topo.slot_keys()):
        assert slot_var[slot] == (topo.var_index[int(frm[2:])] if frm[0] == 'X' else -1)
    kinds = ops[:, 0]
    for row, col, value, word in ((0, 3, topo.n_msgs, 'destination'), (int(np.argmax(kinds == _ffi.OP_PAIR_TM)), 1, topo.P, 'pair slot'),
                                  (int(np.argmax(kinds == _ffi.OP_PAIR_MT)), 2, -1, 'source slot'),
                                  (int(np.argmax(kinds == _ffi.OP_UNARY)), 1, topo.U, 'unary slot'),
                                  (int(np.argmax(kinds == _ffi.OP_VAR)), 2, len(srcs) + 1, 'srcs range'), (0, 0, 7, 'unknown kind')):
        bad = ops.copy()
        bad[row, col] = value
        assert check(ops=bad) == _ffi.MLBP_EINVAL and word in S.last_error(), (word, S.last_error())
    bad = sweeps.copy()
    bad[-1, 1] += 1
    assert check(sweeps=bad) == _ffi.MLBP_EINVAL and 'sweep' in S.last_error()
    # a VAR destination without a variable, or with one out of range; a factor's destination with one
    var_dst = int(ops[int(np.argmax(kinds == _ffi.OP_VAR)), 3])
    fac_dst = int(ops[int(np.argmax(kinds == _ffi.OP_PAIR_TM)), 3])
    for slot, value, word in ((var_dst, -1, 'no source variable'), (var_dst, topo.n_vars, 'no source variable'), (fac_dst, 0, 'not -1')):
        bad = slot_var.copy()
        bad[slot] = value
        assert check(slot_var=bad) == _ffi.MLBP_EINVAL and word in S.last_error(), (word, S.last_error())
    # order: a repeated variable, one out of range
    for bad in ([0, 1, 1], [0, 1, 3], [-1, 1, 2]):
        assert check(order=bad) == _ffi.MLBP_EINVAL and 'permutation' in S.last_error(), bad
    assert check(order=[2, 0, 1]) == _ffi.MLBP_OK
    assert S.lib.mlbp_sample_check_program(None, 1, None, 0, None, 1, 1, 0, 0, 1, None, None) == _ffi.MLBP_EINVAL and 'NULL' in S.last_error()
    # the read-out arrays

    def readout(in_off=topo.in_off, in_slots=topo.in_slots):
        return S.lib.mlbp_sample_check_readout(topo.n_vars, _ffi.i32ptr(i32(in_off)), _ffi.i32ptr(i32(in_slots)), topo.n_msgs)
    assert readout() == _ffi.MLBP_OK
    bad = topo.in_slots.copy(); bad[-1] = topo.n_msgs
    assert readout(in_slots=bad) == _ffi.MLBP_EINVAL and 'slot' in S.last_error()
    bad = topo.in_off.copy(); bad[1] = bad[2] + 1
    assert readout(in_off=bad) == _ffi.MLBP_EINVAL and 'monotone' in S.last_error()
    assert S.lib.mlbp_sample_check_readout(1, None, None, 1) == _ffi.MLBP_EINVAL and 'NULL' in S.last_error()
