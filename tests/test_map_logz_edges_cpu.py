"""The max-product and log-partition kernels at their edges, without a GPU: the inputs of tests/test_gpu_map_edges.py and
tests/test_gpu_logz_edges.py and the preconditions under which the float64 references (the max-product walk of
tests/test_map_cpu.py, the statement of tests/test_logz_cpu.py) are ground truth for them.

Every GPU case of the two modules is an entry of CASES here ('map/...' and 'logz/...') and has a twin below that asserts, on
the references alone, what the GPU test relies on before it looks at the device.  The GPU tests call `precondition(name)`
themselves, so a seed that leaves the regime fails here, on the CPU, and never reaches the device.
  MAP:  the walk's smallest relative gap over all variables and graphs is at least test_gpu_map.NEAR_TIE -- the cap on
        left-out variables is 0 in this file -- and every max-marginal is finite.  (A graph listed under `tied` is the one
        exception, stated where it is made: a bad table leaves some of its max-marginals without a positive total, so they are
        EXACTLY uniform, in the walk and in every correct kernel.  The tie rule decides those, exactly: state 0.  The device
        tests compare them too; only test_gpu_map._compare counts them as left out.)
  logz: the statement's log_z, score and joint_logp on the oracle's sweeps are finite (the non-finite cases say what they are
        instead).
  both: mlbp_*_pick_kernel (host only) returns the kernel the case names, and the LDS byte count of the case is the header's
        formula on the topology's own sizes.
Each twin prints the smallest gap (MAP), the kernel and the LDS bytes.

A. Size edges of the generic kernels: odd X above 256 (raw / na / nb padded to 302, two passes of every 256-stride loop),
   X = 257 (one element in the second pass), X = 2 and X = 1024, and X = 64 past the LDS budgets.
B. More than 256 variables and factors: chain_spec(260, 4).  A chain is a tree: test_gpu_map._viterbi and
   test_gpu_logz._forward_log_z are the independent references, pinned on the walk / the statement here.
C. The X = 64 kernels' LDS budgets with real potentials: the last chain inside each budget, the first one past it, and K3
   under 41 / 35 given words (U above 64: the score loops run twice).
D. The shared-table log-partition kernel on 70 variables, B = 20 (a ragged second group).
E. The batch sums beyond 256 and 512 graphs.
F. Ties: two bit-equal maxima held by one thread in two passes, by waves 2 and 0, by waves 3 and 0.
G. Bad entries: NaN and +inf in a pairwise table, a whole NaN row, an all-zero table."""
import functools

import numpy as np
import pytest

import cases as C
import test_gpu_logz as GL
import test_gpu_map as GM
import test_logz_cpu as S
import test_map_cpu as W
import test_range_cpu as R
from oracle import lbp_oracle as O

AT = (3, 9)                                  # the edited entry of part G
INF, NAN = float('inf'), float('nan')
TIE_PAIRS = [(40, 296), (140, 290), (200, 300)]          # part F: (thread 40, passes 0 and 1), (wave 2, wave 0), (wave 3, wave 0)
TIE_VALUE = 1.5


def _topo(spec):
    from macaronicusermodeling_amd.topology import GraphTopology
    return GraphTopology.from_spec(spec)


def _k3x():
    return R._explicit(C.user_spec(10, [1, 4, 7], 64, 64, seed=1))             # K3, X = 64, one table per factor


def _k4x():
    return R._explicit(C.user_spec(10, [0, 2, 5, 8], 64, 64, seed=4))


def _k3x128():
    return R._explicit(C.user_spec(10, [1, 4, 7], 128, 128, seed=1))


K8 = lambda: C.user_spec(12, [0, 1, 3, 5, 7, 8, 9, 11], 64, 64, seed=5)          # noqa: E731
K3_LEN44 = lambda: C.user_spec(44, [1, 4, 7], 64, 64, seed=1)                      # noqa: E731
K3_LEN38 = lambda: C.user_spec(38, [1, 4, 7], 64, 64, seed=1)                      # noqa: E731
K3_ROOTS = [1, 4, 7]


def _pair_table(spec, p):
    return [f for f in spec['factors'] if len(f['vars']) == 2][p]['table']


# ------------------------------------------------------------------------------------------------
# MAP cases
# ------------------------------------------------------------------------------------------------
def map_lds_bytes(n_msgs, n_vars):
    """include/mlbp_map.h: messages, partial maxima and one raw vector, the assignment."""
    return n_msgs * 512 + 4608 + 4 * ((n_vars + 3) // 4 * 4)


def _map(spec, seeds, roots, instance, normalize=True, slots=None, lds=None, tied=(), edited=None, inputs=None):
    inputs = [C.make_inputs(spec, s) for s in seeds] if inputs is None else inputs
    return dict(kind='map', spec=spec, inputs=inputs, roots=list(roots), instance=instance, normalize=normalize, slots=slots, lds=lds,
                tied=tuple(tied), edited=edited)


def _seeded(spec, B=4, seed=5600):
    return [C.make_inputs(spec, seed + 1000 * b) for b in range(B)]


def _map_edited(spec, roots, instance, value, graph, table, normalize=True, what='entry', tied=()):
    """_seeded(spec) with one pairwise table of one graph edited: one entry (AT), row AT[0], or the whole table."""
    inputs = _seeded(spec)
    if value is not None:
        t = _pair_table(spec, table)
        tabs = list(inputs[graph]['tables'])
        tabs[t] = tabs[t].copy()
        if what == 'entry':
            tabs[t][AT] = value
        elif what == 'row':
            tabs[t][AT[0], :] = value
        else:
            tabs[t][:] = value
        inputs[graph] = dict(tables=tabs)
    return _map(spec, None, roots, instance, normalize=normalize, tied=tied, edited=graph, inputs=inputs)


BAD_SHAPES = {'k3': (_k3x, K3_ROOTS, GM.X64_RESIDENT), 'k4': (_k4x, [0, 2, 5], GM.X64_STREAMED), 'x128': (_k3x128, K3_ROOTS, GM.GENERIC)}


def _bad(shape, value, graph=2, table=1, roots=None, **kw):
    make, shape_roots, instance = BAD_SHAPES[shape]
    return lambda: _map_edited(make(), roots or shape_roots, instance, value, graph, table, **kw)


MAP_CASES = {
    # A
    'ring3_x301': lambda: _map(C.ring_spec(3, 301), range(1, 5), [0, 1, 2], GM.GENERIC),
    'chain3_x257': lambda: _map(C.chain_spec(3, 257), range(1, 5), [0], GM.GENERIC),
    'chain3_x2': lambda: _map(C.chain_spec(3, 2), range(1, 9), [0], GM.GENERIC),
    'chain2_x1024': lambda: _map(C.chain_spec(2, 1024), range(1, 3), [0], GM.GENERIC),
    'chain31_x64': lambda: _map(C.chain_spec(31, 64), range(1, 5), [0], GM.GENERIC, slots=151, lds=82048),
    'k8_x64': lambda: _map(K8(), range(800, 804), [0, 1, 3], GM.GENERIC, slots=152, lds=82464),
    # B
    'chain260_x4': lambda: _map(C.chain_spec(260, 4), range(1, 5), [0], GM.GENERIC, slots=1296),
    # C
    'chain30_x64': lambda: _map(C.chain_spec(30, 64), range(1, 5), [0], GM.X64_STREAMED, slots=146, lds=79488),
    'k3_len44': lambda: _map(K3_LEN44(), range(500, 508), K3_ROOTS, GM.X64_RESIDENT, slots=138, lds=75280),
    # G: the batches without an edit (the graphs whose bits an edit must leave alone; the batches of the table-index case)
    'clean_k3': _bad('k3', None), 'clean_k4': _bad('k4', None), 'clean_x128': _bad('x128', None),
    'clean_k4_unnormalised': _bad('k4', None, normalize=False, roots=[0, 2]), 'clean_x128_unnormalised': _bad('x128', None, normalize=False),
    # G.1: one entry.  +inf: the factor's two messages are [0, ..., NaN, ..., 0]; the next product zeroes them, so its two
    # variables send uniform messages on and have exactly uniform max-marginals themselves: `tied`.
    'nan_k3': _bad('k3', NAN), 'nan_k4': _bad('k4', NAN), 'nan_x128': _bad('x128', NAN),
    'inf_k3': _bad('k3', INF, tied=(2,)), 'inf_k4': _bad('k4', INF, tied=(2,)), 'inf_x128': _bad('x128', INF, tied=(2,)),
    # G.2: a whole row
    'nanrow_k3': _bad('k3', NAN, what='row'), 'nanrow_k4': _bad('k4', NAN, what='row'), 'nanrow_x128': _bad('x128', NAN, what='row'),
    # G.3: a whole table of zeros (the resident instance: test_gpu_map.test_tie_rule_and_zero_table).  Without normalisation
    # every message of the graph becomes exactly zero, every max-marginal exactly uniform: `tied`.  (K4 without normalisation
    # takes two sweeps: every product of a variable update carries a factor 1/64, and a third sweep round the loops of K4
    # underflows float64 on clean tables.)
    'zero_k4': _bad('k4', 0.0, graph=1, table=0, what='table'), 'zero_x128': _bad('x128', 0.0, graph=1, table=0, what='table'),
    'zero_k4_unnormalised': _bad('k4', 0.0, graph=1, table=0, what='table', normalize=False, tied=(1,), roots=[0, 2]),
    'zero_x128_unnormalised': _bad('x128', 0.0, graph=1, table=0, what='table', normalize=False, tied=(1,)),
}


# ------------------------------------------------------------------------------------------------
# log-partition cases
# ------------------------------------------------------------------------------------------------
def logz_lds_bytes(n_in):
    """include/mlbp_logz.h: the in-slot messages, two leave-one-out vectors per wave, the per-wave partial sums."""
    return n_in * 512 + 4096 + 64


def _logz(spec, seeds, roots, instance, upload=False, in_slots=None, lds=None, shared=False, inputs=None, distinct=None, label_seed=3):
    """upload: the messages come from the CPU statement's sweeps (the sweep library has no case of its own at this shape);
    distinct: graph b repeats graph b % distinct."""
    inputs = [C.make_inputs(spec, s) for s in seeds] if inputs is None else inputs
    B, n = len(inputs), len(spec['var_ids'])
    labels = np.random.RandomState(label_seed).randint(0, spec['X'], size=(distinct or B, n)).astype(np.int32)
    if distinct:
        labels = labels[np.arange(B) % distinct]
    return dict(kind='logz', spec=spec, inputs=inputs, roots=list(roots), instance=instance, upload=upload, in_slots=in_slots, lds=lds,
                shared=shared, labels=labels, distinct=distinct)


def _chain70_shared(B=20):
    """One set of 69 pairwise tables (graph 0's) behind every graph, unary tables per graph."""
    spec = C.chain_spec(70, 64)
    own = [C.make_inputs(spec, 1 + b) for b in range(B)]
    inputs = [dict(tables=list(own[b]['tables'][:70]) + list(own[0]['tables'][70:])) for b in range(B)]
    return _logz(spec, None, [0], GL.X64_SHARED, upload=True, in_slots=208, shared=True, inputs=inputs)


def _repeating(spec, seeds, B):
    distinct = [C.make_inputs(spec, s) for s in seeds]
    return [distinct[b % len(distinct)] for b in range(B)]


LOGZ_CASES = {
    # A
    'ring3_x301': lambda: _logz(C.ring_spec(3, 301), range(1, 5), [0, 1, 2], GL.GENERIC),
    'chain3_x257': lambda: _logz(C.chain_spec(3, 257), range(1, 5), [0], GL.GENERIC),
    'chain3_x2': lambda: _logz(C.chain_spec(3, 2), range(1, 9), [0], GL.GENERIC),
    'chain2_x1024': lambda: _logz(C.chain_spec(2, 1024), range(1, 3), [0], GL.GENERIC),
    'chain41_x64': lambda: _logz(C.chain_spec(41, 64), range(1, 5), [0], GL.GENERIC, upload=True, in_slots=121, lds=66112),
    # B
    'chain260_x4': lambda: _logz(C.chain_spec(260, 4), range(1, 5), [0], GL.GENERIC, upload=True, in_slots=778),
    # C
    'chain40_x64': lambda: _logz(C.chain_spec(40, 64), range(1, 5), [0], GL.X64, upload=True, in_slots=118, lds=64576),
    'k3_len38': lambda: _logz(K3_LEN38(), range(500, 508), K3_ROOTS, GL.X64, in_slots=114, lds=62528),
    # D
    'chain70_x64_shared': _chain70_shared,
    # E
    'sum_B600_x4': lambda: _logz(C.chain_spec(3, 4), range(1, 601), [0], GL.GENERIC),
    'sum_B300_k3': lambda: _logz(GL.K3['spec'](), None, K3_ROOTS, GL.X64, inputs=_repeating(GL.K3['spec'](), GL.K3['seeds'], 300), distinct=64),
    # G: the batches of test_non_finite_and_zero_tables before the edit (the device test edits the tables behind the sweeps)
    'bad_k3': lambda: _logz(_k3x(), None, K3_ROOTS, GL.X64, inputs=_seeded(_k3x(), 6)),
    'bad_k3_shared': lambda: _logz(_k3x(), None, K3_ROOTS, GL.X64_SHARED, inputs=_seeded(_k3x(), 6), shared=True),
    'bad_x128': lambda: _logz(_k3x128(), None, K3_ROOTS, GL.GENERIC, inputs=_seeded(_k3x128(), 6)),
}

CASES = dict([('map/' + n, c) for n, c in MAP_CASES.items()] + [('logz/' + n, c) for n, c in LOGZ_CASES.items()])


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of one case (shared by the tests of a process: read, never written)."""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """{graph: walk} of a MAP case, {graph: messages of S.sweeps} of a log-partition case; once per process, read only.  A
    batch that repeats its inputs computes each distinct graph once."""
    c = case(name)
    out = {}
    with np.errstate(all='ignore'):
        for b, inp in enumerate(c['inputs']):
            first = b % c['distinct'] if c.get('distinct') else b
            if first != b:
                out[b] = out[first]
            elif c['kind'] == 'map':
                out[b] = W.walk(c['spec'], inp, c['roots'], normalize=c['normalize'])
            else:
                out[b] = S.sweeps(c['spec'], inp, c['roots'])[1]
    return out


def bad_logz_inputs(name):
    """The inputs of a 'logz/bad_*' case after the edit the device test makes behind the sweeps: NaN at AT of pairwise table 1
    of graph 2, pairwise table 0 of graph 1 all zero."""
    c = case(name)
    inputs = list(c['inputs'])
    for graph, table, value in ((2, 1, NAN), (1, 0, 0.0)):
        t = _pair_table(c['spec'], table)
        tabs = list(inputs[graph]['tables'])
        tabs[t] = tabs[t].copy()
        if value == 0.0:
            tabs[t][:] = 0.0
        else:
            tabs[t][AT] = value
        inputs[graph] = dict(tables=tabs)
    return inputs


def statement(name, inputs=None):
    """[(log_z, score, joint_logp)] of a log-partition case on the oracle's sweeps, graph by graph."""
    c = case(name)
    ref = reference(name)
    g = O.Graph(c['spec'])
    order = _topo(c['spec']).var_ids
    out = []
    with np.errstate(all='ignore'):
        for b, inp in enumerate(c['inputs'] if inputs is None else inputs):
            x = {v: int(c['labels'][b, i]) for i, v in enumerate(order)}
            out.append(S.joint_logp(g, inp, ref[b], x))
    return out


def check_kernel(name):
    """pick_kernel (host only) names the case's kernel; the case's slot and LDS byte counts are the header's formulas."""
    c = case(name)
    topo = _topo(c['spec'])
    X = c['spec']['X']
    if c['kind'] == 'map':
        from macaronicusermodeling_amd import mapdecode as M
        assert M.pick_kernel(X, topo.n_msgs, topo.n_vars) == GM.KERNEL_OF[c['instance']], name
        assert c['instance'] == GM.GENERIC or (topo.P <= 3) == (c['instance'] == GM.X64_RESIDENT), name
        n, lds, budget = topo.n_msgs, map_lds_bytes(topo.n_msgs, topo.n_vars), M.X64_LDS_BYTES
        fits = c['instance'] != GM.GENERIC
    else:
        from macaronicusermodeling_amd import logz as L
        n = int(topo.in_off[-1])
        assert n == 2 * topo.P + topo.U
        assert L.pick_kernel(X, n, topo.n_vars, L.SHARED_PAIR_TABLES if c['shared'] else 0) == GL.KERNEL_OF[c['instance']], name
        lds, budget = logz_lds_bytes(n), L.X64_LDS_BYTES
        fits = c['instance'] == GL.X64
    if c.get('slots' if c['kind'] == 'map' else 'in_slots') is not None:
        assert n == c['slots' if c['kind'] == 'map' else 'in_slots'], (name, n)
    if c['lds'] is not None:
        assert lds == c['lds'], (name, lds)
    if X == 64 and not c.get('shared'):
        assert (lds <= budget) == fits, (name, lds, budget)
    print('%s: kernel %s, %d slots, %d B of LDS by the header (X = 64 budget %d)' % (name, c['instance'][0], n, lds, budget))
    return topo


def precondition(name):
    """What a GPU case relies on, asserted on the references alone; returns reference(name)."""
    c = case(name)
    check_kernel(name)
    ref = reference(name)
    assert sorted(ref) == list(range(len(c['inputs'])))
    if c['kind'] == 'map':
        gaps = []
        for b, w in ref.items():
            mm = np.stack([w['mm'][v] for v in w['g'].var_order])
            assert np.isfinite(mm).all(), (name, b)
            flat = [v for i, v in enumerate(w['g'].var_order) if np.array_equal(mm[i], np.full(mm.shape[1], 1.0 / mm.shape[1]))]
            assert bool(flat) == (b in c['tied']), (name, b, flat)
            assert all(w['x'][v] == 0 for v in flat), (name, b)
            gaps += [w['gap'][v] for v in w['g'].var_order if v not in flat]
        print('%s: %d graphs, smallest gap of the walk %.2e (NEAR_TIE %.0e, cap on left-out variables 0)%s'
              % (name, len(ref), min(gaps), GM.NEAR_TIE, '; graphs %s hold exactly uniform max-marginals' % (c['tied'],) if c['tied'] else ''))
        assert min(gaps) >= GM.NEAR_TIE, (name, min(gaps))
    else:
        st = np.array(statement(name))
        print('%s: %d graphs, log_z of the statement %.6g .. %.6g' % (name, len(st), st[:, 0].min(), st[:, 0].max()))
        assert np.isfinite(st).all(), name
    return ref


@pytest.mark.parametrize('name', list(CASES))
def test_precondition(name):
    precondition(name)


# ------------------------------------------------------------------------------------------------
# the walk's maximum is the header's
# ------------------------------------------------------------------------------------------------
def _walk_with_plain_max(spec, inputs, roots):
    """The walk as it was before it learned the NaN rule: ndarray.max in both orientations."""
    def plain(g, inp, msgs, fid, v, normalize=True):
        f = g.by_id[fid]
        T = O.factor_table(g, inp, f)
        if len(f['vars']) == 1:
            out = np.copy(T).reshape(-1)
        else:
            other = [u for u in f['vars'] if u != v][0]
            m = msgs['X_%d' % other, 'F_%d' % fid]
            out = (T * m[None, :]).max(1) if g.dim_of(f, other) == 1 else (m[:, None] * T).max(0)
        msgs['F_%d' % fid, 'X_%d' % v] = W._finish(out, normalize)
    keep = W.mp_factor_to_var
    W.mp_factor_to_var = plain
    try:
        return W.walk(spec, inputs, roots)
    finally:
        W.mp_factor_to_var = keep


def test_fmax_changes_no_bit_of_the_walk_on_nan_free_tables():
    """np.fmax.reduce in place of ndarray.max: bit-identical messages, max-marginals and assignments on K3 (both table
    orientations occur), so no existing case moves."""
    spec = GM.K3['spec']()
    for seed in (500, 501, 502):
        inputs = C.make_inputs(spec, seed)
        new, old = W.walk(spec, inputs, K3_ROOTS), _walk_with_plain_max(spec, inputs, K3_ROOTS)
        assert new['x'] == old['x'] and new['score'] == old['score']
        assert sorted(new['msgs']) == sorted(old['msgs'])
        for k in new['msgs']:
            assert np.array_equal(new['msgs'][k].view(np.int64), old['msgs'][k].view(np.int64)), k
        for v in new['mm']:
            assert np.array_equal(new['mm'][v].view(np.int64), old['mm'][v].view(np.int64)), v
    a = np.array([[1.0, NAN, 3.0], [NAN, NAN, NAN]])
    with np.errstate(all='ignore'):
        assert np.fmax.reduce(a, axis=1)[0] == 3.0 and np.isnan(np.fmax.reduce(a, axis=1)[1]) and np.isnan(a.max(1)).all()


# ------------------------------------------------------------------------------------------------
# B: the chain of 260 variables against dynamic programming
# ------------------------------------------------------------------------------------------------
def test_chain260_walk_is_viterbi():
    c = case('map/chain260_x4')
    ref = precondition('map/chain260_x4')
    topo = _topo(c['spec'])
    assert (topo.n_vars, topo.P, topo.U, topo.n_msgs) == (260, 259, 260, 1296)
    for b, inp in enumerate(c['inputs']):
        assert [ref[b]['x'][v] for v in topo.var_ids] == GM._viterbi(c['spec'], inp), b


def test_chain260_statement_is_the_forward_algorithm():
    c = case('logz/chain260_x4')
    precondition('logz/chain260_x4')
    topo = _topo(c['spec'])
    bound = GL.kernel_atol(topo, 4) + 1e-10 * GL.message_factors(topo)
    worst = 0.0
    for b, (lz, _, _) in enumerate(statement('logz/chain260_x4')):
        worst = max(worst, GL._close(lz, GL._forward_log_z(c['spec'], c['inputs'][b]), bound, 'chain260 graph %d' % b))
    print('chain260_x4: statement against the forward algorithm, worst |diff| %.2e (bound %.2e)' % (worst, bound))


# ------------------------------------------------------------------------------------------------
# C, D: what the host says about the shapes
# ------------------------------------------------------------------------------------------------
def test_budget_cases_sit_on_both_sides_of_the_budgets():
    from macaronicusermodeling_amd import logz as L, mapdecode as M
    for n, slots, lds, kernel in ((30, 146, 79488, M.KERNEL_X64), (31, 151, 82048, M.KERNEL_GENERIC)):
        topo = _topo(C.chain_spec(n, 64))
        assert (topo.n_msgs, map_lds_bytes(topo.n_msgs, n)) == (slots, lds) and M.pick_kernel(64, slots, n) == kernel
    assert map_lds_bytes(150, 4) == 81424 <= M.X64_LDS_BYTES < map_lds_bytes(151, 1) == 81936          # at most 150 slots, whatever n_vars
    assert 128 * 512 == 65536 < 146 * 512                                  # chain30: slots 128 to 145 lie above 64 KiB
    for n, n_in, lds, kernel in ((40, 118, 64576, L.KERNEL_X64), (41, 121, 66112, L.KERNEL_GENERIC)):
        topo = _topo(C.chain_spec(n, 64))
        assert (int(topo.in_off[-1]), logz_lds_bytes(n_in)) == (n_in, lds) and L.pick_kernel(64, n_in, n) == kernel
    assert logz_lds_bytes(119) <= L.X64_LDS_BYTES < logz_lds_bytes(120)
    k44, k38, k8 = _topo(K3_LEN44()), _topo(K3_LEN38()), _topo(K8())
    assert (k44.P, k44.U, k44.n_msgs) == (3, 126, 138) and (k38.P, k38.U, int(k38.in_off[-1])) == (3, 108, 114)
    assert max(np.diff(k44.in_off)) == 44 and max(np.diff(k38.in_off)) == 38                 # 43 / 37 sources in a variable update
    assert (k8.n_msgs, k8.n_vars, k8.P) == (152, 8, 28)
    c70 = _topo(C.chain_spec(70, 64))
    assert (c70.n_vars, c70.P, c70.U) == (70, 69, 70) and L.pick_kernel(64, 208, 70, L.SHARED_PAIR_TABLES) == L.KERNEL_X64_SHARED


def test_chain70_shares_its_pairwise_tables_and_nothing_else():
    c = case('logz/chain70_x64_shared')
    assert len(c['inputs']) == 20 and 20 % 16 == 4                          # a ragged second group of the 16-graph kernel
    for b in range(1, 20):
        assert all(c['inputs'][b]['tables'][t] is c['inputs'][0]['tables'][t] for t in range(70, 139))
        assert not any(np.array_equal(c['inputs'][b]['tables'][t], c['inputs'][0]['tables'][t]) for t in range(70))
    lz = np.array(statement('logz/chain70_x64_shared'))[:, 0]
    assert len(set(lz.tolist())) == 20


# ------------------------------------------------------------------------------------------------
# F: ties
# ------------------------------------------------------------------------------------------------
def tie_specs():
    """(name, spec, roots): one variable without a pairwise factor, and a chain of three, at X = 301."""
    return [('k1_x301', C.user_spec(10, [4], 301, 301, seed=3), [4]), ('chain3_x301', C.chain_spec(3, 301), [0])]


@pytest.mark.parametrize('lo,hi', TIE_PAIRS)
def test_the_walk_breaks_a_tie_towards_the_lower_index(lo, hi):
    """All-ones tables with TIE_VALUE at states lo and hi of every unary row: pairwise messages are constant, so every
    max-marginal has exactly two bit-equal maxima, and np.argmax returns the lower one.  In the generic kernel thread t holds
    states t and t + 256; wave w holds threads 64 w to 64 w + 63."""
    assert 0 <= lo < hi < 301 and (lo % 256 == hi % 256 or (lo % 256) // 64 != (hi % 256) // 64)
    for name, spec, roots in tie_specs():
        ex = R._explicit(spec) if spec['style'] != 'explicit' else spec
        ntab = 1 + max(f['table'] for f in ex['factors'])
        tabs = [None] * ntab
        for f in ex['factors']:
            tabs[f['table']] = np.ones((301, 301)) if len(f['vars']) == 2 else np.ones((301, 1))
            if len(f['vars']) == 1:
                tabs[f['table']][[lo, hi], 0] = TIE_VALUE
        w = W.walk(ex, dict(tables=tabs), roots)
        for v, mm in w['mm'].items():
            assert mm[lo] == mm[hi] == mm.max() and int((mm == mm.max()).sum()) == 2, (name, v)
        assert set(w['x'].values()) == {lo}, (name, w['x'])


# ------------------------------------------------------------------------------------------------
# G: what the references do with bad entries
# ------------------------------------------------------------------------------------------------
def _stack(msgs):
    return np.stack([msgs[k] for k in sorted(msgs)])


@pytest.mark.parametrize('name', [n for n in MAP_CASES if n.split('_')[0] in ('nan', 'inf', 'nanrow')])
def test_a_non_finite_entry_changes_the_walk_of_its_graph_only(name):
    c = case('map/' + name)
    ref, clean = precondition('map/' + name), precondition('map/clean_' + name.split('_')[1])
    for b, w in ref.items():
        same = np.array_equal(_stack(w['msgs']), _stack(clean[b]['msgs']), equal_nan=True)
        if b != c['edited']:
            assert same, (name, b)
        elif name.startswith('nan_'):          # the maximum ignores the entry: the walk moves only if AT held a row or column maximum
            print('%s: the walk of graph %d %s' % (name, b, 'is the clean walk' if same else 'differs from the clean walk'))
        else:
            assert not same, (name, b)
    w = ref[c['edited']]
    f = [f for f in c['spec']['factors'] if len(f['vars']) == 2][1]
    by_axis = {d: v for d, v in zip(f['dims'], f['vars'])}
    to_axis0 = w['msgs']['F_%d' % f['id'], 'X_%d' % by_axis[0]]
    X = c['spec']['X']
    if name.startswith('inf'):
        # the message towards axis 0 is [0, ..., NaN at AT[0], ..., 0] (inf / inf), towards axis 1 the same at AT[1]; the next
        # product zeroes the NaN, so the variable's message on is uniform
        assert np.isnan(to_axis0[AT[0]]) and (np.delete(to_axis0, AT[0]) == 0).all()
    elif name.startswith('nanrow'):
        assert np.array_equal(to_axis0, np.full(X, 1.0 / X))                 # a NaN total is no positive total
    else:
        assert np.isfinite(_stack(w['msgs'])).all()                          # the maximum ignored the entry


@pytest.mark.parametrize('name', ['zero_k4', 'zero_x128', 'zero_k4_unnormalised', 'zero_x128_unnormalised'])
def test_an_all_zero_table_in_the_walk(name):
    """Normalised: both messages of the factor are uniform.  Unnormalised: every message that has passed the factor is zero,
    every max-marginal of the graph exactly uniform (precondition: `tied`).  The score is -inf either way."""
    c = case('map/' + name)
    ref = precondition('map/' + name)
    w = ref[c['edited']]
    f = [f for f in c['spec']['factors'] if len(f['vars']) == 2][0]
    X = c['spec']['X']
    for v in f['vars']:
        m = w['msgs']['F_%d' % f['id'], 'X_%d' % v]
        assert np.array_equal(m, np.full(X, 1.0 / X) if c['normalize'] else np.zeros(X))
    assert np.isneginf(w['score']) and all(np.isfinite(ref[b]['score']) for b in ref if b != c['edited'])


@pytest.mark.parametrize('name', ['bad_k3', 'bad_k3_shared', 'bad_x128'])
def test_the_statement_on_a_nan_entry_and_on_an_all_zero_table(name):
    """IEEE arithmetic, nothing clamped: a NaN entry makes Z_f, log_z and joint_logp NaN; an all-zero table makes Z_f = 0 and
    log_z = -inf, the score -inf and joint_logp = -inf - -inf = NaN.  The other graphs are untouched."""
    clean = np.array(statement('logz/' + name))
    bad = np.array(statement('logz/' + name, bad_logz_inputs('logz/' + name)))
    assert np.isnan(bad[2, 0]) and np.isnan(bad[2, 2])
    assert np.isneginf(bad[1, 0]) and np.isneginf(bad[1, 1]) and np.isnan(bad[1, 2])
    others = [b for b in range(len(clean)) if b not in (1, 2)]
    assert np.array_equal(bad[others], clean[others]) and np.isfinite(clean).all()
    print('%s: graph 2 (NaN entry) %s, graph 1 (zero table) %s' % (name, bad[2], bad[1]))
