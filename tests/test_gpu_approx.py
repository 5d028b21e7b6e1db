"""The batched top-100 approximate paths -- FactorGraphBatch(use_approx_inference=True, use_approx_beliefs=...) -- at real
vocabulary sizes, on ties, on messages the caller supplies and in the gradient, against the walk of tests/test_approx_cpu.py:
the oracle's approximate sweeps with the selection following the library's rule (by value, NaN below every number, ties to the
lower index).  The unpatched oracle is no reference for a loopy graph at X >= 300: see that module.

Every case is a row of CASES (graph shape, X, how its inputs are made); `graphs(name)` builds its per-graph specs and inputs,
`reference(name)` walks them once per process.  Every compared graph first passes test_approx_cpu.decided -- each selection is
a tie of bit-equal values or has a relative gap of at least 1e-8 at the 100th place -- and each case prints its smallest gap
before it asserts.  Tolerances are the project's: messages and marginals 1e-10 relative, gradients rtol 1e-8 / atol 1e-11.

  A  every normalised float64 instance of sweep_wide_kernel under selection (APPROX_CASES: instance -> cases; the inventory
     test requires an entry per compiled instance), ring3 with uniform and lognormal tables, one tree
  B  X = 100 keeps everything: the exact call's bits; X = 99 and 64 are refused with nothing launched
  C  ties: uniform first selections at X = 300, zero-padded selections of sparse messages, the object API on the same graph
  D  init=False: duplicates across the 100th place, NaNs, +inf, an all-zero message in the slots selected from first
  E  approximate beliefs in the gradient: sizes, feature counts, stand-alone and behind the sweeps, shared tables, NaN, a zero
     table, the on-chip bound of X
  F  the call around it: split calls, skip_unchanged, posterior, B = 1, one launch for four sweeps"""
import copy
import functools

import numpy as np
import pytest

import cases as C
import kernel_inventory as K
import test_approx_cpu as A
from helpers import batch_tables
from oracle import lbp_oracle as O

try:                                        # (the case table and reference() are read by CPU tests: no skip at import)
    import torch
except ImportError:
    torch = None
pytestmark = pytest.mark.gpu

RTOL = 1e-10
GRAD_TOL = dict(rtol=1e-8, atol=1e-11)
ROOTS = {'ring3': [0, 2, 1, 0], 'chain3': [0, 2, 1, 0], 'user_k3': [4, 1, 7, 4], 'user_k3w': [2, 1, 7, 2]}
SPECS = {'ring3': lambda X: C.ring_spec(3, X), 'chain3': lambda X: C.chain_spec(3, X),
         'user_k3': lambda X: C.user_spec(10, [1, 4, 7], X, 40, seed=1),
         'user_k3w': lambda X: C.user_spec(10, [1, 2, 7], X, 40, seed=1)}      # (1, 2) is the one factor on pot_en_en_w1

# X -> (Q, PAD) of the sweep_wide_kernel<true, Q, double, 2, PAD> that takes it (launch_wide_sweep)
WIDE_SIZES = {128: (1, 0), 102: (1, 1), 101: (1, 2), 256: (2, 0), 200: (2, 1), 201: (2, 2), 300: (3, 1), 301: (3, 2),
              512: (4, 0), 450: (4, 1), 451: (4, 2), 700: (6, 1), 701: (6, 2), 1024: (8, 1), 1001: (8, 2)}


def wide_instance(X):
    q, pad = WIDE_SIZES[X] if X in WIDE_SIZES else {100: (1, 1)}[X]           # (X = 100: part B, the even padded instance)
    return ('sweep_wide_kernel', (True, q, 'double', 2, pad))


# name -> dict(shape, X, B, kind, ...).  Inputs of graph s: cases.make_inputs(spec, 7000 + s, kind).
CASES = {}
for _X in WIDE_SIZES:
    for _kind in ('uniform', 'lognormal'):
        CASES['ring3_x%d_%s' % (_X, _kind)] = dict(shape='ring3', X=_X, B=3, kind=_kind)
CASES['chain3_x300_lognormal'] = dict(shape='chain3', X=300, B=3, kind='lognormal')
CASES['ring3_x100_uniform'] = dict(shape='ring3', X=100, B=3, kind='uniform')
CASES['ring3_x300_sparse'] = dict(shape='ring3', X=300, B=3, kind='uniform', sparse_unary=30)
CASES['ring3_x201_start'] = dict(shape='ring3', X=201, B=6, kind='uniform', sweeps=1, start='patterns')
CASES['ring3_x201_b1'] = dict(shape='ring3', X=201, B=1, kind='lognormal')
for _X in (101, 201, 300):
    CASES['user_k3_x%d' % _X] = dict(shape='user_k3', X=_X, B=3, beliefs=True)
CASES['user_k3_x201_f11'] = dict(shape='user_k3', X=201, B=3, beliefs=True, F=(1, 1))
CASES['user_k3_x201_f22'] = dict(shape='user_k3', X=201, B=3, beliefs=True, F=(2, 2))
CASES['user_k3_x100'] = dict(shape='user_k3', X=100, B=3, beliefs=True)
CASES['user_k3_x201_shared'] = dict(shape='user_k3', X=201, B=3, beliefs=True, shared=True)
CASES['user_k3_x201_nan'] = dict(shape='user_k3', X=201, B=3, beliefs=True, sweeps=0, start='nan')
CASES['user_k3w_x201_zero'] = dict(shape='user_k3w', X=201, B=3, beliefs=True, zero_w1=1)

# instance -> the cases of part A that run it with approx_k > 0 (tests/test_kernel_inventory.py: every compiled
# sweep_wide_kernel<true, Q, double, 2, PAD> has an entry, every entry a compiled instance, every case exists)
APPROX_CASES = {wide_instance(X): ['ring3_x%d_uniform' % X, 'ring3_x%d_lognormal' % X] for X in WIDE_SIZES}
APPROX_CASES[wide_instance(300)].append('chain3_x300_lognormal')

START_PATTERNS = ('duplicates', 'three_nans', 'mostly_nans', 'infs', 'zeros', 'untouched')


def _instance_spec(spec, rs):
    """A copy of a train_mp-style spec with its own labels and observed columns (what differs between instances of one shape)."""
    s = copy.deepcopy(spec)
    s['labels'] = [int(v) for v in rs.randint(0, s['X'], size=len(s['labels']))]
    for f in s['factors']:
        if f['observed_dim'] is not None:
            f['observed_dim'] = int(rs.randint(0, s['Vde'] if f['factor_type'] == 'en_de' else s['X']))
    return s


def _selected_first(spec, inputs, roots, start):
    """The slots the walk selects from while they still hold the caller's bits."""
    w = A.walk(spec, inputs, roots, start=start)
    return sorted({r['slot'] for r in w['records'] if r['supplied']})


def _apply_pattern(v, pattern):
    order = A.select(v, v.size)
    if pattern == 'duplicates':                 # five equal values around the 100th place: the lower indices are kept
        v[order[97:102]] = v[order[99]]
    elif pattern == 'three_nans':
        v[[5, 77, 150]] = np.nan
    elif pattern == 'mostly_nans':              # 150 NaNs of 201: 49 of them must be selected, lowest index first
        v[np.random.RandomState(5).choice(v.size, 150, replace=False)] = np.nan
    elif pattern == 'infs':
        v[[3, 120]] = np.inf
    elif pattern == 'zeros':
        v[:] = 0.0


@functools.lru_cache(maxsize=None)
def graphs(name):
    """-> dict(spec: the shape's spec, specs: one per graph, inputs: one oracle inputs dict per graph, roots, start:
    [B][n_msgs][X] or None, base_start: start before the patterns went in, slots: the slots the patterns went into)."""
    c = CASES[name]
    X, B = c['X'], c['B']
    spec = SPECS[c['shape']](X)
    trainmp = spec['style'] == 'trainmp'
    roots = ROOTS[c['shape']][:c.get('sweeps', 4)]
    inputs = [C.make_inputs(spec, 7000 + s, c.get('kind') or 'uniform') for s in range(B)]
    specs = [spec] * B
    if trainmp:
        rs = np.random.RandomState(7100)
        specs = [_instance_spec(spec, rs) for _ in range(B)]
        F = c.get('F', (3, 6))
        for i in inputs:                            # the feature tensors are the batch's: graph 0's; the pots stay each graph's own
            for k in ('phi_en_en', 'phi_en_en_w1'):
                i[k] = inputs[0][k][:, :, :F[0]]
            i['phi_en_de'] = inputs[0]['phi_en_de'][:, :, :F[1]]
            i['theta_en_en'], i['theta_en_de'] = i['theta_en_en'][:, :F[0]], i['theta_en_de'][:, :F[1]]
            if c.get('shared'):
                i['pot_en_en'], i['pot_en_en_w1'] = inputs[0]['pot_en_en'], inputs[0]['pot_en_en_w1']
        if c.get('zero_w1') is not None:
            inputs[c['zero_w1']]['pot_en_en_w1'] = np.zeros((X, X))
    if c.get('sparse_unary'):                       # unary tables with 30 non-zero entries: messages with fewer than 100
        rs = np.random.RandomState(7200)
        for i in inputs:
            tabs = list(i['tables'])
            for f in spec['factors']:
                if len(f['vars']) == 1:
                    t = np.zeros((X, 1))
                    t[rs.choice(X, c['sparse_unary'], replace=False), 0] = rs.rand(c['sparse_unary']) + 0.01
                    tabs[f['table']] = t
            i['tables'] = tabs
    start = base = slots = None
    if c.get('start'):
        n_msgs = len(C.msg_keys(spec))
        base = np.random.RandomState(7300).rand(B, n_msgs, X) + 0.05
        start = base.copy()
        if c['start'] == 'patterns':
            assert B == len(START_PATTERNS)
            slots = _selected_first(spec, inputs[0], roots, base[0])
            for b, pattern in enumerate(START_PATTERNS):
                assert _selected_first(specs[b], inputs[b], roots, base[b]) == slots
                for s in slots:
                    _apply_pattern(start[b, s], pattern)
        else:                                       # a NaN in a message a pairwise factor's beliefs read, graphs 0 and 1
            g = O.Graph(spec)
            keys = C.msg_keys(spec)
            pair = [f for f in g.factors if len(f['vars']) == 2][0]
            slots = [keys.index(('X_%d' % v, 'F_%d' % pair['id'])) for v in pair['vars']]
            start[0, slots[0], 17] = np.nan
            start[1, slots[1], [0, 200]] = np.nan
    return dict(spec=spec, specs=specs, inputs=inputs, roots=roots, start=start, base_start=base, slots=slots)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The walk of every graph of a case (computed once, never modified)."""
    G = graphs(name)
    beliefs = bool(CASES[name].get('beliefs'))
    return [A.walk(G['specs'][b], G['inputs'][b], G['roots'], start=None if G['start'] is None else G['start'][b],
                   approx_beliefs=beliefs) for b in range(CASES[name]['B'])]


def _decided(name):
    """The precondition, on every compared graph; prints the case's smallest gap."""
    ref = reference(name)
    gap = min(A.smallest_gap(w['records']) for w in ref)
    print('%s: smallest compared gap %.3g over %d selections' % (name, gap, sum(len(w['records']) for w in ref)))
    for b, w in enumerate(ref):
        assert A.decided(w['records']), (name, b)
    return ref


# ---- device side -----------------------------------------------------------------------------------------------------
def _ffi():
    from macaronicusermodeling_amd import _ffi
    return _ffi


def _tables(G, topo):
    pair, unary = [], []
    for s, i in zip(G['specs'], G['inputs']):
        p, u = batch_tables(s, topo, [i])
        pair.append(p); unary.append(u)
    return np.concatenate(pair), np.concatenate(unary)


def _grad_meta(spec, topo):
    by_id = {f['id']: f for f in spec['factors']}
    pair_phi = [0 if by_id[topo.factor_ids[j]]['gap'] > 1 else 1 for j in topo.pair_factors]
    kinds, obs = [], []
    for j in topo.unary_factors:
        f = by_id[topo.factor_ids[j]]
        kinds.append(2 if f['factor_type'] == 'en_de' else (0 if f['gap'] > 1 else 1))
        obs.append(f['observed_dim'])
    label_of = dict(zip(spec['var_ids'], spec['labels']))
    return pair_phi, kinds, obs, [label_of[v] for v in topo.var_ids]


class _Batch:
    """The device batch of a case: tables, and for a train_mp-style shape features and observations."""

    def __init__(self, name, inference=True, beliefs=None, shared_tab=None, only=None):
        from macaronicusermodeling_amd.batch import FactorGraphBatch
        from macaronicusermodeling_amd.topology import GraphTopology
        G = graphs(name)
        if only is not None:                      # the graphs `only` of the case, as a batch of their own
            G = dict(G, specs=[G['specs'][b] for b in only], inputs=[G['inputs'][b] for b in only])
        c = CASES[name]
        self.name, self.G, self.spec = name, G, G['spec']
        self.B, self.X = len(G['specs']), c['X']
        self.topo = topo = GraphTopology.from_spec(self.spec)
        assert topo.slot_keys() == C.msg_keys(self.spec) and list(topo.var_ids) == list(O.Graph(self.spec).var_order)
        self.trainmp = self.spec['style'] == 'trainmp'
        beliefs = bool(c.get('beliefs')) if beliefs is None else beliefs
        fb = self.fb = FactorGraphBatch(topo, self.X, self.B, use_approx_inference=inference, use_approx_beliefs=beliefs)
        pair, unary = _tables(G, topo)
        if shared_tab is None:
            shared_tab = bool(c.get('shared'))
        if shared_tab:                              # pair_tab names graph 0's two pots
            pair_phi = _grad_meta(self.spec, topo)[0]
            i0 = G['inputs'][0]
            fb.set_pair_tables(np.stack([i0['pot_en_en'], i0['pot_en_en_w1']]), np.tile(pair_phi, (self.B, 1)))
            assert fb.pair_tables_shared
        else:
            fb.set_pair_tables(pair)
        fb.set_unary_tables(unary)
        self.marg = torch.full((self.B, topo.n_vars, self.X), float('nan'), dtype=torch.float64, device=fb.device)
        if self.trainmp:
            meta = [_grad_meta(s, topo) for s in G['specs']]
            i0 = G['inputs'][0]
            fb.set_features(i0['phi_en_en'], i0['phi_en_en_w1'], i0['phi_en_de'], meta[0][0], meta[0][1])
            fb.set_observations(np.array([m[3] for m in meta]), np.array([m[2] for m in meta]))
            self.F = (i0['phi_en_en'].shape[2], i0['phi_en_de'].shape[2])
        fb.msgs.fill_(float('nan'))

    def grad_out(self):
        return tuple(torch.full((self.B, f), float('nan'), dtype=torch.float64, device=self.fb.device) for f in self.F)

    def sweep(self, roots=None, **kw):
        """One sweep call (from uniform messages unless init is given), the launch log reset before it -> Program."""
        kw.setdefault('init', True)
        kw.setdefault('marginals', self.marg)
        K.reset()
        prog = self.fb.sweep(self.G['roots'] if roots is None else roots, **kw)
        self.launched, self.everything = K.launched(), K.all_launched()
        assert prog.status() == 0, _ffi().lib.mlbp_last_error()
        return prog

    def messages(self):
        return self.fb.msgs.cpu().numpy()

    def check_sweeps(self, ref, graphs_of=None):
        got, marg = self.messages(), self.marg.cpu().numpy()
        for b in (range(self.B) if graphs_of is None else graphs_of):
            np.testing.assert_allclose(got[b], ref[b]['messages'], rtol=RTOL, atol=1e-300, err_msg='%s: messages of graph %d' % (self.name, b))
            np.testing.assert_allclose(marg[b], ref[b]['marginals'], rtol=RTOL, atol=1e-300, err_msg='%s: marginals of graph %d' % (self.name, b))

    def assert_wide(self, X=None):
        """The call ran on the wide kernel, the case's instance, in one launch."""
        assert _ffi().lib.mlbp_last_sweep_kernel() == 4
        assert self.launched[:1] == [wide_instance(self.X if X is None else X)], self.launched
        assert [k[0] for k in self.everything].count('sweep_wide_kernel') == 1, self.everything


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).tobytes()


# ---- A: every normalised float64 wide instance under selection ------------------------------------------------------
@pytest.mark.parametrize('name', sorted(n for names in APPROX_CASES.values() for n in names))
def test_wide_instance_under_selection(name):
    ref = _decided(name)
    inst = [i for i, names in APPROX_CASES.items() if name in names]
    assert inst == [wide_instance(CASES[name]['X'])]
    bt = _Batch(name)
    bt.sweep()
    bt.assert_wide()
    assert bt.launched == inst
    bt.check_sweeps(ref)
    if CASES[name]['shape'] == 'ring3':           # a loop: the first sweep selected from uniform messages
        assert all(any(r['cls'] == 'uniform' for r in w['records']) for w in ref)


def test_a_tree_has_the_unpatched_oracle_as_reference_too():
    name = 'chain3_x300_lognormal'
    ref = _decided(name)
    assert all({r['cls'] for r in w['records']} == {'gap'} for w in ref)
    bt = _Batch(name)
    bt.sweep()
    G = graphs(name)
    got = bt.messages()
    for b in range(bt.B):
        _, msgs, _ = O.run(G['spec'], G['inputs'][b], G['roots'], 4, force_loopy=True, approx=True)
        want = np.stack([msgs[k] for k in C.msg_keys(G['spec'])])
        assert want.tobytes() == ref[b]['messages'].tobytes()
        np.testing.assert_allclose(got[b], want, rtol=RTOL, atol=1e-300)


# ---- B: the boundary of K --------------------------------------------------------------------------------------------
def test_x100_keeps_everything_and_equals_the_exact_call():
    name = 'ring3_x100_uniform'
    ref = _decided(name)
    assert all({r['cls'] for r in w['records']} == {'all'} for w in ref)
    approx, exact = _Batch(name), _Batch(name, inference=False)
    approx.sweep()
    exact.sweep()
    assert approx.launched == exact.launched == [('sweep_wide_kernel', (True, 1, 'double', 2, 1))]
    assert _bits(approx.fb.msgs) == _bits(exact.fb.msgs) and _bits(approx.marg) == _bits(exact.marg)
    approx.check_sweeps(ref)


@pytest.mark.parametrize('X', [99, 64])
def test_fewer_than_100_states_are_refused_before_anything_launches(X):
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(C.ring_spec(3, X))
    fb = FactorGraphBatch(topo, X, 3, use_approx_inference=True)
    fb.set_pair_tables(np.ones((3 * topo.P, X, X))); fb.set_unary_tables(np.ones((3 * topo.U, X)))
    fb.msgs.fill_(7.0)
    K.reset()
    with pytest.raises(_ffi().MlbpError, match='out of bounds'):
        fb.sweep([0, 2, 1, 0], init=True)
    assert K.all_launched() == [] and _ffi().lib.mlbp_launch_log(None, 0) == 0
    assert float(fb.msgs.min()) == 7.0 == float(fb.msgs.max())


# ---- C: ties and sparse messages -------------------------------------------------------------------------------------
def test_uniform_first_selections_at_300():
    """Where argpartition and the rule part ways: the walk recorded uniform selections, and the unpatched oracle differs."""
    name = 'ring3_x300_uniform'
    ref = _decided(name)
    G = graphs(name)
    for b, w in enumerate(ref):
        assert sum(r['cls'] == 'uniform' for r in w['records']) >= 2
    plain = A.walk(G['spec'], G['inputs'][0], G['roots'], rule=False)
    assert not np.allclose(plain['messages'], ref[0]['messages'], rtol=1e-6, atol=0)
    bt = _Batch(name)
    bt.sweep()
    bt.check_sweeps(ref)


def test_sparse_messages_pad_the_selection_with_zeros():
    name = 'ring3_x300_sparse'
    ref = _decided(name)
    for w in ref:
        assert sum(r['cls'] == 'zero' for r in w['records']) > 0
    bt = _Batch(name)
    bt.sweep()
    bt.assert_wide()
    bt.check_sweeps(ref)
    assert np.isfinite(bt.messages()).all()


def test_object_api_selects_by_the_same_rule():
    """The product's other approximate path -- LBP.FactorGraph with use_approx_inference, one mlbp_topk_f64 per update -- on
    graph 0 of the X = 300 ring: the batched messages at 1e-10."""
    import importlib
    import macaronicusermodeling_amd.LBP as mod
    from test_gpu_dropin_lbp import Roots
    name = 'ring3_x300_uniform'
    ref = _decided(name)
    G = graphs(name)
    bt = _Batch(name)
    bt.sweep()
    L = importlib.reload(mod)
    try:
        roots = Roots(L)                          # (replaces the module's random.sample draw of the roots)
        fg = C.build_graph(L, G['spec'], G['inputs'][0])
        fg.use_approx_inference = True
        roots.queue = [G['roots'][0]]
        fg.initialize()
        assert fg.isLoopy
        roots.queue = list(G['roots'])
        fg.treelike_inference(len(G['roots']))
        assert roots.queue == []
        got = np.stack([fg.messages[k].m.reshape(-1) for k in C.msg_keys(G['spec'])])
    finally:
        importlib.reload(mod)
    np.testing.assert_allclose(got, bt.messages()[0], rtol=RTOL, atol=1e-300)
    np.testing.assert_allclose(got, ref[0]['messages'], rtol=RTOL, atol=1e-300)


# ---- D: messages the caller supplies ---------------------------------------------------------------------------------
def test_supplied_messages_with_ties_nans_and_infs():
    """init=False, one sweep: the loop-closing slots are selected from before anything writes them, so the selection reads
    the caller's bits -- exact duplicates across the 100th place, three NaNs among numbers, more NaNs than X - 100 (NaNs must
    be selected, lowest index first), +inf entries, an all-zero message: one graph each, and one untouched graph whose bits
    equal a run without the edited neighbours.  (Before ranks_above put NaN below every number the fused selection kept every
    NaN: the three_nans graph then had the uniform message where the rule, the object API and the reference give a finite
    one.)"""
    name = 'ring3_x201_start'
    ref = _decided(name)
    G = graphs(name)
    assert len(G['slots']) >= 1
    for b, w in enumerate(ref):
        first = [r for r in w['records'] if r['supplied']]
        assert len(first) == len(G['slots']) and {r['slot'] for r in first} <= set(G['slots'])     # (equal vectors share a slot number)
        want = {'duplicates': 'gap', 'three_nans': 'nan', 'mostly_nans': 'nan', 'infs': 'gap', 'zeros': 'uniform',
                'untouched': 'gap'}[START_PATTERNS[b]]
        assert {r['cls'] for r in first} == {want}, (START_PATTERNS[b], first)
    assert all(r['gap'] == 0.0 for r in ref[0]['records'] if r['supplied'])          # the duplicates straddle the 100th place
    bt = _Batch(name)
    bt.fb.msgs.copy_(torch.from_numpy(G['start']))
    bt.sweep(init=False)
    bt.assert_wide()
    got = bt.messages()
    for b, pattern in enumerate(START_PATTERNS):
        print('%s: max |difference| from the walk %.3g' % (pattern, np.nanmax(np.abs(got[b] - ref[b]['messages']))))
    bt.check_sweeps(ref)
    # three NaNs are dropped: the result is finite where it does not simply carry the caller's own NaNs
    written = np.array([not np.array_equal(got[1][s], G['start'][1][s], equal_nan=True) for s in range(got.shape[1])])
    assert written.any() and np.isfinite(got[1][written]).all()
    plain = _Batch(name)
    plain.fb.msgs.copy_(torch.from_numpy(G['base_start']))
    plain.sweep(init=False)
    u = START_PATTERNS.index('untouched')
    assert got[u].tobytes() == plain.messages()[u].tobytes() and _bits(bt.marg[u]) == _bits(plain.marg[u])


# ---- E: approximate beliefs in the gradient --------------------------------------------------------------------------
def _gradient_both_ways(bt):
    """The sweeps, then the gradient stand-alone and as the tail of the sweep call: the same bits -> (g_ee, g_ed) numpy."""
    bt.sweep()
    bt.assert_wide()
    K.reset()
    g_ee, g_ed = bt.fb.gradient()
    alone = K.launched()
    assert _ffi().lib.mlbp_gradient_status() == 0
    msgs = _bits(bt.fb.msgs)
    f_ee, f_ed = bt.grad_out()
    bt.sweep(gradient=(f_ee, f_ed))
    assert _ffi().lib.mlbp_gradient_status() == 0
    inst = ('gradient_kernel', bt.F)
    assert alone == [inst] and bt.launched == [wide_instance(bt.X), inst], (alone, bt.launched)
    assert not [k for k in bt.everything if 'contract' in k[0]], bt.everything
    assert _bits(bt.fb.msgs) == msgs and _bits(f_ee) == _bits(g_ee) and _bits(f_ed) == _bits(g_ed)
    return g_ee.cpu().numpy(), g_ed.cpu().numpy()


def _check_gradient(name, g_ee, g_ed, ref, graphs_of=None):
    for b in (range(len(ref)) if graphs_of is None else graphs_of):
        np.testing.assert_allclose(g_ee[b], ref[b]['gradient'][0], err_msg='%s: en_en gradient of graph %d' % (name, b), **GRAD_TOL)
        np.testing.assert_allclose(g_ed[b], ref[b]['gradient'][1], err_msg='%s: en_de gradient of graph %d' % (name, b), **GRAD_TOL)


@pytest.mark.parametrize('name', ['user_k3_x101', 'user_k3_x201', 'user_k3_x300', 'user_k3_x201_f11', 'user_k3_x201_f22'])
def test_approximate_beliefs_gradient(name):
    ref = _decided(name)
    assert all(len(w['records']) > w['n_sweep_records'] for w in ref)         # the beliefs selected too
    G = graphs(name)
    assert len({tuple(s['labels']) for s in G['specs']}) == 3                   # labels and observed columns differ per graph
    bt = _Batch(name)
    assert bt.F == CASES[name].get('F', (3, 6))
    g_ee, g_ed = _gradient_both_ways(bt)
    bt.check_sweeps(ref)
    _check_gradient(name, g_ee, g_ed, ref)


def test_approximate_beliefs_at_x100_are_the_exact_beliefs():
    name = 'user_k3_x100'
    ref = _decided(name)
    approx, exact = _Batch(name), _Batch(name, inference=False, beliefs=False)
    a_ee, a_ed = _gradient_both_ways(approx)
    exact.sweep()
    e_ee, e_ed = exact.fb.gradient()
    assert _bits(approx.fb.msgs) == _bits(exact.fb.msgs)
    assert a_ee.tobytes() == _bits(e_ee) and a_ed.tobytes() == _bits(e_ed)
    _check_gradient(name, a_ee, a_ed, ref)


def test_approximate_beliefs_with_shared_pairwise_tables():
    """pair_tab naming graph 0's two pots: the wide kernel sweeps and the per-graph gradient kernel follows (the contraction
    forms take no approximate call); the same bits as unique copies of those tables."""
    name = 'user_k3_x201_shared'
    ref = _decided(name)
    shared, unique = _Batch(name), _Batch(name, shared_tab=False)
    assert shared.fb.pair_tables_shared and not unique.fb.pair_tables_shared
    s_ee, s_ed = _gradient_both_ways(shared)
    u_ee, u_ed = _gradient_both_ways(unique)
    assert _bits(shared.fb.msgs) == _bits(unique.fb.msgs) and _bits(shared.marg) == _bits(unique.marg)
    assert s_ee.tobytes() == u_ee.tobytes() and s_ed.tobytes() == u_ed.tobytes()
    shared.check_sweeps(ref)
    _check_gradient(name, s_ee, s_ed, ref)


def test_approximate_beliefs_drop_a_nan_in_a_supplied_message():
    """gradient() on messages the caller supplied, a NaN in a variable -> factor message a pairwise factor's beliefs read
    (graph 0: one on the factor's axis-0 side, graph 1: two on the other side, graph 2: none).  NaN ranks below every number,
    so it is dropped and the factor's beliefs are those of the 100 largest numbers -- before ranks_above it was kept, the
    factor's sum was NaN and its beliefs fell to zero (an en_en gradient off by 0.5)."""
    name = 'user_k3_x201_nan'
    ref = _decided(name)
    G = graphs(name)
    assert [sum(r['cls'] == 'nan' for r in w['records']) for w in ref] == [1, 1, 0]
    bt = _Batch(name)
    bt.fb.msgs.copy_(torch.from_numpy(G['start']))
    K.reset()
    g_ee, g_ed = bt.fb.gradient()
    assert K.launched() == [('gradient_kernel', (3, 6))] and _ffi().lib.mlbp_gradient_status() == 0
    g_ee, g_ed = g_ee.cpu().numpy(), g_ed.cpu().numpy()
    print('%s: en_en gradient of graph 0 %s, the walk %s' % (name, g_ee[0], ref[0]['gradient'][0]))
    assert np.isfinite(ref[0]['gradient'][0]).all() and np.isfinite(ref[1]['gradient'][0]).all()
    _check_gradient(name, g_ee, g_ed, ref)


def test_approximate_beliefs_of_an_all_zero_table_are_zero():
    """Graph 1's pot_en_en_w1 -- the table of the pairwise factor (1, 2) -- is all zero.  The reference's sparse_normalize has
    no zero-sum guard and yields NaN; the kernel yields zero beliefs, the exact path's rule (au.normalize;
    test_zero_table_gives_zero_beliefs_like_au_normalize): that factor's gradient is its observed cell's features."""
    name = 'user_k3w_x201_zero'
    ref = _decided(name)
    G = graphs(name)
    z = CASES[name]['zero_w1']
    assert np.isnan(ref[z]['gradient'][0]).all() and np.isfinite(ref[z]['gradient'][1]).all()
    bt = _Batch(name)
    g_ee, g_ed = _gradient_both_ways(bt)
    bt.check_sweeps(ref)
    _check_gradient(name, g_ee, g_ed, ref, graphs_of=[b for b in range(bt.B) if b != z])
    # graph z by the kernel's rule: every other factor as the reference has it, the zero-table factor with zero beliefs
    g = O.Graph(G['specs'][z])
    inputs = G['inputs'][z]
    msgs = dict(zip(C.msg_keys(G['spec']), ref[z]['messages']))
    want = np.zeros(3)
    with A.ruled_topk():
        for f in g.factors:
            if f['factor_type'] != 'en_en':
                continue
            if len(f['vars']) == 2 and f['gap'] == 1:
                l0, l1 = O.observed_cell(g, f)
                want += inputs['phi_en_en_w1'][l0, l1]
            else:
                want += O.factor_gradient(g, inputs, msgs, f['id'], True).reshape(-1)
    np.testing.assert_allclose(g_ee[z], want, **GRAD_TOL)
    np.testing.assert_allclose(g_ed[z], ref[z]['gradient'][1], **GRAD_TOL)


# The gradient kernel holds both selected messages on chip: 2 X doubles of dynamic LDS beside its own 800 bytes, 64 KiB in
# all -> X <= (65536 - 800) / 16 = 4046 (MLBP_APPROX_BELIEFS_MAX_X).
MAX_X = 4046


def _two_variable_batch(X, host):
    """B = 1, variables 0 and 1 with a unary en_de factor each and the pairwise factor (0, 1); one feature per kind.  host:
    the inputs are made on the host (and returned); else uninitialised device memory (a call that must be refused)."""
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    spec = C.user_spec(2, [0, 1], X, 2, seed=1)
    topo = GraphTopology.from_spec(spec)
    assert (topo.P, topo.U, topo.n_vars) == (1, 2, 2)
    fb = FactorGraphBatch(topo, X, 1, use_approx_beliefs=True)
    dev = fb.device
    inputs = None
    if host:
        rs = np.random.RandomState(X)
        phi = rs.rand(X, X, 1)
        inputs = dict(phi=phi, phi_ed=rs.rand(X, 2, 1), T=np.exp(rs.rand(X, X)), unary=rs.rand(2, X) + 0.01,
                      msgs=rs.rand(topo.n_msgs, X) + 0.05)
        fb.set_pair_tables(inputs['T'][None])
        fb.set_unary_tables(inputs['unary'])
        fb.set_features(phi, phi, inputs['phi_ed'], [1], [2, 2])
        fb.msgs.copy_(torch.from_numpy(inputs['msgs'][None]))
    else:
        fb.set_pair_tables(torch.zeros(1, X, X, dtype=torch.float64, device=dev))
        fb.set_unary_tables(torch.zeros(2, X, dtype=torch.float64, device=dev))
        phi = torch.zeros(X, X, 1, dtype=torch.float64, device=dev)
        fb.set_features(phi, phi, torch.zeros(X, 2, 1, dtype=torch.float64, device=dev), [1], [2, 2])
        fb.msgs.fill_(1.0 / X)
    fb.set_observations([[3, X - 1]], [[0, 1]])
    return spec, topo, fb, inputs


def test_approximate_beliefs_at_the_largest_x_that_fits():
    X = MAX_X
    spec, topo, fb, inp = _two_variable_batch(X, host=True)
    K.reset()
    g_ee, g_ed = fb.gradient()
    assert K.launched() == [('gradient_kernel', (1, 1))] and _ffi().lib.mlbp_gradient_status() == 0
    keys = C.msg_keys(spec)
    pair = [f for f in spec['factors'] if len(f['vars']) == 2][0]
    c, r = (inp['msgs'][keys.index(('X_%d' % v, 'F_%d' % pair['id']))] for v in pair['vars'])
    assert A.decided([A.classify(c, supplied=True), A.classify(r, supplied=True)])
    print('X = %d: gaps %.3g, %.3g' % (X, A.classify(c)['gap'], A.classify(r)['gap']))
    ci, ri = np.sort(A.select(c)), np.sort(A.select(r))
    blk = np.ix_(ci, ri)
    w = np.outer(c[ci], r[ri]) * inp['T'][blk]
    want_ee = inp['phi'][3, X - 1, 0] - (w * inp['phi'][:, :, 0][blk]).sum() / w.sum()
    want_ed = sum(inp['phi_ed'][lab, u, 0] - (inp['unary'][u] * inp['phi_ed'][:, u, 0]).sum() / inp['unary'][u].sum()
                  for u, lab in enumerate((3, X - 1)))
    np.testing.assert_allclose(g_ee.cpu().numpy(), [[want_ee]], **GRAD_TOL)
    np.testing.assert_allclose(g_ed.cpu().numpy(), [[want_ed]], **GRAD_TOL)


def test_approximate_beliefs_beyond_the_on_chip_bound_are_refused():
    """X = 4047 is the first size whose two selected messages do not fit: MLBP_EUNSUPPORTED from gradient() and from
    sweep(gradient=...), before anything is enqueued."""
    X = MAX_X + 1
    spec, topo, fb, _ = _two_variable_batch(X, host=False)
    ffi = _ffi()
    K.reset()
    with pytest.raises(ffi.MlbpError, match='approximate beliefs hold both selected messages on chip') as e:
        fb.gradient()
    assert e.value.code == ffi.MLBP_EUNSUPPORTED and K.all_launched() == []
    out = tuple(torch.zeros(1, 1, dtype=torch.float64, device=fb.device) for _ in range(2))
    with pytest.raises(ffi.MlbpError, match='approximate beliefs hold both selected messages on chip') as e:
        fb.sweep([0], init=True, gradient=out)
    assert e.value.code == ffi.MLBP_EUNSUPPORTED and K.all_launched() == [] and ffi.lib.mlbp_launch_log(None, 0) == 0
    fb.use_approx_beliefs = False                  # the exact beliefs have no such bound
    K.reset()
    fb.gradient()
    assert K.launched() == [('gradient_kernel', (1, 1))] and ffi.lib.mlbp_gradient_status() == 0


# ---- F: the call around it -------------------------------------------------------------------------------------------
def test_split_calls_skip_unchanged_and_posterior_change_no_bit():
    name = 'ring3_x201_uniform'
    ref = _decided(name)
    G = graphs(name)
    roots = G['roots']
    whole = _Batch(name)
    whole.sweep()
    whole.assert_wide()
    whole.check_sweeps(ref)
    split = _Batch(name)
    split.sweep(roots[:1])
    split.sweep(roots[1:], init=False)
    assert _bits(split.fb.msgs) == _bits(whole.fb.msgs) and _bits(split.marg) == _bits(whole.marg)
    skip = _Batch(name)
    skip.sweep(skip_unchanged=True)
    skip.assert_wide()
    assert _bits(skip.fb.msgs) == _bits(whole.fb.msgs) and _bits(skip.marg) == _bits(whole.marg)
    post = _Batch(name)
    labels = np.random.RandomState(9).randint(0, 201, size=(post.B, post.topo.n_vars)).astype(np.int32)
    out = torch.full((post.B,), float('nan'), dtype=torch.float64, device=post.fb.device)
    tot = torch.full((1,), float('nan'), dtype=torch.float64, device=post.fb.device)
    post.sweep(posterior=(torch.from_numpy(labels).to(post.fb.device), out, tot))
    post.assert_wide()
    assert _bits(post.fb.msgs) == _bits(whole.fb.msgs) and _bits(post.marg) == _bits(whole.marg)
    want = np.array([sum(np.log(ref[b]['marginals'][v, labels[b, v]]) for v in range(post.topo.n_vars)) for b in range(post.B)])
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=RTOL)
    np.testing.assert_allclose(float(tot.item()), want.sum(), rtol=RTOL)


def test_a_batch_of_one():
    name = 'ring3_x201_b1'
    ref = _decided(name)
    bt = _Batch(name)
    assert bt.B == 1
    bt.sweep()
    bt.assert_wide()
    bt.check_sweeps(ref)
