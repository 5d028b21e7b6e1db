"""Max-product sweeps to convergence without a GPU: the float64 NumPy walk of the max-product mode of include/mlbp_converge.h
that tests/test_gpu_mapconverge.py compares against, pinned on things it does not define itself; the inputs of the GPU cases
and what their comparisons rely on; the host checks of the mode's new fields.

The walk is built from two walks that are pinned already: every update is tests/test_map_cpu.py's max-product send (W._mp_send,
pinned there on exhaustive enumeration), and the residual, the round and the stop rule are tests/test_converge_cpu.py's (the
delta of a slot before and after its update, NaN rule included; a round is O.sweep's two passes for every root in turn; a graph
stops after the first round with residual <= tol).  The decode is W's: the argmax of the max-marginal (np.argmax: the lowest
index) and the sum of the log table entries at it.

What the GPU cases rely on, asserted here on the walk alone, for every graph of every case, none left out:
  * rounds are compared exactly: every case runs at tol = 1e-6 and no residual of any round lies within MARGIN = 1e-3 * tol of
    tol (the argument of tests/test_converge_cpu.py: the bar of 1e-10 on messages bounds a residual's disagreement by 2e-4 tol);
  * assignments are compared exactly: the two largest entries of every variable's max-marginal lie at least LEAD = 1e-8 apart,
    a hundred times the bar of 1e-10 on max-marginals (entries in [0, 1]);
  * max-product need not settle, and a graph that oscillates amplifies rounding round after round: every case whose messages
    are compared either settles in the walk within its max_rounds -- every graph of it: SETTLES names those cases -- or runs
    with max_rounds <= 5."""
import ctypes
import functools

import numpy as np

import cases as C
import test_converge_cpu as CV
import test_map_cpu as W
from oracle import lbp_oracle as O

TOL = CV.TOL
MARGIN = CV.MARGIN
LEAD = 1e-8


# ------------------------------------------------------------------------------------------------
# the NumPy walk
# ------------------------------------------------------------------------------------------------
def _send(g, inputs, msgs, frm, to):
    """W._mp_send (normalised), and the delta of the slot it wrote (0.0 for the send the reference skips)."""
    if to[0] == O.FAC and len(g.by_id[to[1]]['vars']) < 2:
        return 0.0
    key = (O.name(frm), O.name(to))
    old = msgs[key].copy()
    with np.errstate(all='ignore'):
        W._mp_send(g, inputs, msgs, frm, to, True)
    return CV._delta(msgs[key], old)


def one_round(g, inputs, msgs, roots):
    res = 0.0
    for r in roots:
        sched = O.message_schedule(g, r)
        for child, parent in reversed(sched):
            res = max(res, _send(g, inputs, msgs, child, parent))
        for child, parent in sched:
            res = max(res, _send(g, inputs, msgs, parent, child))
    return res


def walk(spec, inputs, roots=None, tol=TOL, max_rounds=50, msgs=None, extra=0):
    """One graph.  -> dict(g, msgs, rounds, residual, history, mm {v: max-marginal}, x {v: state}, score, lead {v: distance of
    the two largest max-marginal entries}, after [the residuals of `extra` further rounds, run on a copy])."""
    g = O.Graph(spec)
    roots = list(g.var_order) if roots is None else list(roots)
    msgs = O.init_messages(g) if msgs is None else msgs
    history = []
    while True:
        history.append(one_round(g, inputs, msgs, roots))
        if history[-1] <= tol or len(history) >= max_rounds:
            break
    with np.errstate(all='ignore'):
        mm = {v: W.max_marginal(g, msgs, v) for v in g.var_order}
    x = {v: int(np.argmax(mm[v])) for v in g.var_order}
    lead = {}
    for v in g.var_order:
        top = np.sort(mm[v])[-2:]
        lead[v] = float(top[1] - top[0])
    more, after = {k: v.copy() for k, v in msgs.items()}, []
    for _ in range(extra):
        after.append(one_round(g, inputs, more, roots))
    return dict(g=g, msgs=msgs, rounds=len(history), residual=history[-1], history=history, mm=mm, x=x,
                score=W.score_of(g, inputs, x), lead=lead, after=after)


# ------------------------------------------------------------------------------------------------
# graphs and inputs of the GPU cases
# ------------------------------------------------------------------------------------------------
def two_chains_spec(X):
    """Two components, both trees: a chain over (0, 1, 2) and a chain over (10, 11), every variable with a unary factor."""
    s = C.chain_spec(3, X, name='two_chains_x%d' % X)
    base = len(s['factors'])
    s['var_ids'] += [10, 11]
    s['labels'] += [0, 1]
    s['factors'] += [dict(id=100, vars=[10], dims=[0], table=base), dict(id=101, vars=[11], dims=[0], table=base + 1),
                     dict(id=102, vars=[11, 10], dims=[1, 0], table=base + 2)]
    return s


# name -> (spec, [(s, seed) per graph: tables exp(s N(0,1))], max_rounds, roots (None: every variable once))
GPU_CASES = {
    'k3_x64': (lambda: CV.clique_spec(3, 64), [(0.5, 0), (0.5, 1), (1, 2), (1, 3), (2, 4), (2, 6), (4, 2)], 20, None),       # B = 7
    'k4_x64': (lambda: CV.clique_spec(4, 64), [(0.5, 0), (1, 2), (2, 3), (2, 6)], 20, None),
    'k4_x64_short': (lambda: CV.clique_spec(4, 64), [(1, 1), (2, 4), (4, 5)], 4, None),
    'star31_x64': (lambda: C.star_spec(31, 64), [(1, 0), (1, 1)], 4, [0]),
    'k3_x5': (lambda: CV.clique_spec(3, 5), [(0.5, 1), (1, 2), (2, 3), (2, 7)], 20, None),
    'k3_x65': (lambda: CV.clique_spec(3, 65), [(0.5, 1), (1, 2), (2, 5)], 20, None),
    'ring8_x4': (lambda: C.ring_spec(8, 4), [(0.5, 0), (1, 0), (2, 0)], 20, None),
    'k3_x64_one': (lambda: CV.clique_spec(3, 64), [(1, 3)], 20, None),                                                          # B = 1
}
# the cases every graph of which settles in the walk within max_rounds; the others run max_rounds <= 5
SETTLES = {'k3_x64', 'k4_x64', 'star31_x64', 'k3_x5', 'k3_x65', 'ring8_x4', 'k3_x64_one'}


@functools.lru_cache(maxsize=None)
def gpu_case(name):
    """(spec, [inputs per graph], [walk per graph (with one further round)], max_rounds, roots) -- computed once, shared, never
    changed."""
    make, graphs, max_rounds, roots = GPU_CASES[name]
    spec = make()
    inputs = [CV.scaled_inputs(spec, s, seed) for s, seed in graphs]
    walks = [walk(spec, inp, roots=roots, tol=TOL, max_rounds=max_rounds, extra=1) for inp in inputs]
    return spec, inputs, walks, max_rounds, roots


def check_walks(name, walks, max_rounds, settles):
    """The three conditions of the module's docstring on the walks of one case."""
    for b, w in enumerate(walks):
        for r in w['history']:
            assert np.isfinite(r) and abs(r - TOL) > MARGIN, (name, b, w['history'])
        assert 1 <= w['rounds'] <= max_rounds and (w['residual'] <= TOL or w['rounds'] == max_rounds)
        for v, d in w['lead'].items():
            assert d >= LEAD, (name, b, v, d)
        if settles:
            assert w['residual'] <= TOL, (name, b, w['history'])
    assert settles or max_rounds <= 5, name


# ------------------------------------------------------------------------------------------------
# the walk, pinned
# ------------------------------------------------------------------------------------------------
def _trees():
    return [make(X) for X in (2, 3, 4) for make in (lambda X: C.chain_spec(4, X), lambda X: C.star_spec(4, X), two_chains_spec)]


def test_trees_take_two_rounds_and_decode_the_enumerated_best():
    """On a tree the first round reaches the fixed point and the second recomputes every message from the same inputs: rounds
    == 2 and residual == 0.0 at tol = 0.  Assignment and score are those of exhaustive enumeration; that needs the best to be
    unique, and it leads the runner-up by 1e-6 nats for every input here (asserted, none left out)."""
    trees = _trees()
    assert len(trees) == 9
    for i, spec in enumerate(trees):
        for kind in ('uniform', 'lognormal'):
            inputs = C.make_inputs(spec, 20 + i, kind)
            w = walk(spec, inputs, tol=0.0, max_rounds=5)
            for root in w['g'].var_order:
                assert not O.has_loops(w['g'], root)
            assert w['rounds'] == 2 and w['residual'] == 0.0 and w['history'][0] > 0.0, (spec['name'], w['history'])
            x, best, grid = W.brute_force(w['g'], inputs)
            top = np.sort(grid.reshape(-1))[-2:]
            assert top[1] - top[0] >= 1e-6, (spec['name'], kind, top)
            assert w['x'] == x, (spec['name'], kind)
            np.testing.assert_allclose(w['score'], best, rtol=1e-12, atol=1e-12)


def test_one_round_is_the_max_product_walks_sweeps_bit_for_bit():
    shapes = [CV.clique_spec(3, 64), CV.clique_spec(4, 64), CV.clique_spec(4, 4), C.ring_spec(8, 4), C.ring_spec(4, 4)]
    for spec in shapes:
        inputs = CV.scaled_inputs(spec, 1.0, 1)
        for roots in (None, [spec['var_ids'][-1], spec['var_ids'][0]]):
            w = walk(spec, inputs, roots=roots, max_rounds=1)
            want = W.walk(spec, inputs, list(w['g'].var_order) if roots is None else roots)
            assert w['rounds'] == 1 and set(w['msgs']) == set(want['msgs'])
            for k in want['msgs']:
                assert np.array_equal(w['msgs'][k], want['msgs'][k]), (spec['name'], k)
            assert w['x'] == want['x'] and w['score'] == want['score']
            for v in want['mm']:
                assert np.array_equal(w['mm'][v], want['mm'][v])


def test_one_more_round_after_a_settled_call_moves_nothing_beyond_tol():
    settled = 0
    for name in sorted(SETTLES):
        _, _, walks, _, _ = gpu_case(name)
        for b, w in enumerate(walks):
            assert w['residual'] <= TOL and w['after'][0] <= TOL, (name, b, w['residual'], w['after'])
            settled += 1
    assert settled >= 20


def test_continuing_is_the_same_walk():
    spec, inputs, walks, max_rounds, _ = gpu_case('k3_x64')
    b = int(np.argmax([w['rounds'] for w in walks]))
    assert walks[b]['rounds'] > 3
    first = walk(spec, inputs[b], max_rounds=3)
    rest = walk(spec, inputs[b], max_rounds=max_rounds - 3, msgs=first['msgs'])
    assert first['history'] + rest['history'] == walks[b]['history']


def test_the_gpu_cases_meet_what_their_comparisons_rely_on():
    assert SETTLES <= set(GPU_CASES)
    for name in GPU_CASES:
        _, _, walks, max_rounds, _ = gpu_case(name)
        print('%s: rounds %r, last residuals %s, nearest residual to tol %.3e, least lead %.3e'
              % (name, [w['rounds'] for w in walks], ['%.2e' % w['residual'] for w in walks], CV.nearest_to_tol(walks),
                 min(min(w['lead'].values()) for w in walks)))
        check_walks(name, walks, max_rounds, name in SETTLES)
    # the mixed batch is mixed, and the short case is one that has not settled when it is cut off
    rounds = [w['rounds'] for w in gpu_case('k3_x64')[2]]
    assert len(set(rounds)) >= 3, rounds
    assert any(w['residual'] > TOL for w in gpu_case('k4_x64_short')[2])
    assert len(gpu_case('k3_x64')[1]) == 7 and len(gpu_case('k3_x64_one')[1]) == 1


# ------------------------------------------------------------------------------------------------
# host checks of the new fields, through the built library
# ------------------------------------------------------------------------------------------------
def _V():
    from macaronicusermodeling_amd import converge
    return converge


def _max_args(V, **fields):
    a = CV._valid_args(V)                                # every pointer set, max_product 0
    a.max_product = 1
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def test_every_new_refusal_names_its_argument():
    V = _V()
    from macaronicusermodeling_amd import _ffi
    for fields, word in ((dict(score=None), 'assignment without score'), (dict(assignment=None), 'score without assignment'),
                         (dict(pair_axis_var=None), 'pair_axis_var'), (dict(unary_var=None), 'unary_var')):
        a = _max_args(V, **fields)
        assert V.lib.mlbp_converge_f64(ctypes.byref(a), None) == _ffi.MLBP_EINVAL, fields
        assert word in V.last_error(), (fields, V.last_error())
        assert V.lib.mlbp_converge_last_kernel() == V.KERNEL_NONE
    # the earlier refusals come first in max mode too
    a = _max_args(V, tol=-1.0)
    assert V.lib.mlbp_converge_f64(ctypes.byref(a), None) == _ffi.MLBP_EINVAL and 'tol' in V.last_error()


def test_a_decode_without_max_product_is_refused_once_a_device_is_there():
    """`assignment` or `score` with max_product = 0 is MLBP_EINVAL.  The header puts this one check behind the device check (a
    call with every pointer set and no mode has always reached that one), so a machine without a device says MLBP_ENODEVICE."""
    import torch
    V = _V()
    from macaronicusermodeling_amd import _ffi
    for fields in (dict(), dict(score=None), dict(assignment=None)):
        a = _max_args(V, max_product=0, **fields)
        rc = V.lib.mlbp_converge_f64(ctypes.byref(a), None)
        if torch.cuda.is_available():
            assert rc == _ffi.MLBP_EINVAL and 'without max_product' in V.last_error(), (fields, V.last_error())
        else:
            assert rc == _ffi.MLBP_ENODEVICE
        assert V.lib.mlbp_converge_last_kernel() == V.KERNEL_NONE


def test_zero_and_null_in_the_new_fields_are_accepted():
    """What passes every host check reaches the device check: without a device that is MLBP_ENODEVICE.  (With one the pointers
    would be used: tests/test_gpu_mapconverge.py runs these calls for real.)"""
    import torch
    V = _V()
    from macaronicusermodeling_amd import _ffi
    if torch.cuda.is_available():
        return
    new = ('max_product', 'assignment', 'score', 'pair_axis_var', 'unary_var')
    assert [f[0] for f in V.ConvergeArgs._fields_[-5:]] == list(new)
    zero = {k: None for k in new[1:]}
    calls = [_max_args(V, max_product=0, **zero),                                  # today's call
             _max_args(V, **zero),                                                 # max rounds without a decode
             _max_args(V, pair_axis_var=None, unary_var=None, assignment=None, score=None),
             _max_args(V),                                                         # max rounds and the decode
             _max_args(V, P=0, pair_tables=None, pair_tab=None, pair_axis_var=None),       # no pairwise factor: no pair_axis_var
             _max_args(V, U=0, unary_tables=None, unary_tab=None, unary_var=None)]
    for a in calls:
        assert V.lib.mlbp_converge_f64(ctypes.byref(a), None) == _ffi.MLBP_ENODEVICE, V.last_error()
        assert 'no CPU fallback' in V.last_error()


def test_pick_kernel_is_unchanged():
    V = _V()
    for X, n_msgs, n_vars in ((64, 15, 3), (64, 27, 3), (64, 150, 31), (64, 151, 31), (64, 155, 32), (63, 27, 3), (65, 15, 3), (5, 15, 3),
                              (4, 32, 8), (1024, 5, 2)):
        want = V.KERNEL_X64 if X == 64 and n_msgs * 512 + 4608 + 8 <= V.X64_LDS_BYTES else V.KERNEL_GENERIC
        assert V.pick_kernel(X, n_msgs, n_vars) == want, (X, n_msgs)
    assert V.X64_LDS_BYTES == 81920


def test_decode_arrays_are_the_map_bindings():
    """The converge program builds pair_axis_var / unary_var from the topology on its own; they are the map program's arrays."""
    from macaronicusermodeling_amd import mapdecode
    from macaronicusermodeling_amd.topology import GraphTopology
    V = _V()
    for spec in (C.star_spec(4, 8), CV.clique_spec(4, 4), two_chains_spec(3), C.user_spec(10, [1, 4, 7], 64, 64, seed=1)):
        topo = GraphTopology.from_spec(spec)
        for mine, theirs in zip(V.decode_arrays(topo), mapdecode.readout_arrays(topo)):
            assert mine.dtype == np.int32 and np.array_equal(mine, theirs)
