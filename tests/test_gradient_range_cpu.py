"""The gradient away from unit magnitude, without a GPU: the inputs of tests/test_gpu_gradient_range.py parts B, C and D, and the
preconditions under which the float64 oracle's gradient (oracle/lbp_oracle.py: unregularized_gradient) is ground truth for them.

The oracle forms a pairwise belief as normalize((c r^T) * T) in float64, the reference's order.  With wide-range tables that is
where float64 and the mathematics could part (a product c_i r_j that leaves the normal range, a total that loses its small
terms), so `gradient_statement` restates the gradient of one graph in the log domain -- pairwise b_ij proportional to
exp(log c_i + log T_ij + log r_j - max), unary b_x proportional to T_x, every sum in np.longdouble (float64 where longdouble is
no wider) -- on the ORACLE'S messages, and every case of part B and part D first passes

    max |unregularized_gradient - gradient_statement| <= 1e-12       (BAR, absolute; the gradient's entries are O(1))

for EVERY graph of its batch: no graph is exempt, a later change of seeds cannot move a case out of that regime unnoticed.

Part C's inputs (one entry -100 or NaN, tests/test_gpu_exponent_range.py: HAND_OVER) are outside the log domain; for them the
file pins what the oracle's gradient IS: au.normalize sends a NaN or non-positive total to zero beliefs, so that factor
contributes phi[label] alone; a positive total with a negative entry gives finite beliefs with a negative one.  The oracle
raises nothing on any of them, and no component of its gradient is NaN.

Part D's inputs are user_k3 at X = 65, 97, 201 (the contraction path's padded sizes) with the last real state carrying most of
the mass and the labels of every other graph on that state.
"""
import copy
import functools

import numpy as np
import pytest

import cases as C
import test_range_cpu as R
from oracle import lbp_oracle as O

BAR = 1e-12
LD = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64
PHI = ('phi_en_en', 'phi_en_en_w1', 'phi_en_de')

SHARED_NAMES = ('user_k2', 'user_k3_gaps_3_6', 'user_k3_gaps_1_2_3', 'user_k4', 'user_k5')
SHARED_CASES = [(n, w) for n in SHARED_NAMES for w in R.SHARED_WIDTHS]
OWN_NAMES = ('user_k2', 'user_p2', 'user_k3')
OWN_CASES = [(n, w) for n in OWN_NAMES for w in R.SHARED_WIDTHS]
OWN_B, OWN_SEED = 13, 4100
PADDED_X = (65, 97, 201)
PADDED_B, PADDED_SEED = 19, 4200
HAND_OVER = {'negative': -100.0, 'nan': float('nan')}       # == test_gpu_exponent_range.HAND_OVER
HAND_OVER_CASES = ('lean_user_k3', 'shared_user_k3_gaps_3_6', 'shared_user_k4')


# ------------------------------------------------------------------------------------------------
# the statement
# ------------------------------------------------------------------------------------------------
def _log(a):
    return np.log(np.asarray(a, dtype=LD))


def factor_statement(g, inputs, msgs, f):
    """The gradient of one factor (cell - E_b[phi]) in the log domain -> [F] in LD.  Tables and messages strictly positive."""
    T = O.factor_table(g, inputs, f)
    phi = np.asarray(O.factor_phi(g, inputs, f), dtype=LD)
    if len(f['vars']) == 1:
        lw = _log(T.reshape(-1))
        feat = phi[:, f['observed_dim'], :]
        cell = feat[g.label[f['vars'][0]]]
    else:
        by_axis = {g.dim_of(f, v): v for v in f['vars']}
        c = msgs['X_%d' % by_axis[0], 'F_%d' % f['id']].reshape(-1)
        r = msgs['X_%d' % by_axis[1], 'F_%d' % f['id']].reshape(-1)
        lw = _log(c)[:, None] + _log(T) + _log(r)[None, :]
        feat = phi
        cell = phi[O.observed_cell(g, f)]
    w = np.exp(lw - np.max(lw))
    b = w / np.sum(w)
    return cell - np.tensordot(b, feat, axes=b.ndim)


def gradient_statement(g, inputs, msgs):
    """-> (g_ee [F_ee], g_ed [F_ed]) in LD: unregularized_gradient with every belief formed in the log domain."""
    out = {'en_en': np.zeros(inputs['theta_en_en'].size, dtype=LD), 'en_de': np.zeros(inputs['theta_en_de'].size, dtype=LD)}
    for f in g.factors:
        out[f['factor_type']] += factor_statement(g, inputs, msgs, f)
    return out['en_en'], out['en_de']


def oracle_gradient(g, inputs, msgs):
    """unregularized_gradient as two flat float64 vectors."""
    with np.errstate(all='ignore'):
        ee, ed = O.unregularized_gradient(g, inputs, msgs)
    return np.asarray(ee, dtype=np.float64).reshape(-1), np.asarray(ed, dtype=np.float64).reshape(-1)


def statement_distance(g, inputs, msgs):
    """max |oracle - statement| over both gradient vectors."""
    ee, ed = oracle_gradient(g, inputs, msgs)
    see, sed = gradient_statement(g, inputs, msgs)
    return float(max(np.max(np.abs(ee - see)), np.max(np.abs(ed - sed))))


# ------------------------------------------------------------------------------------------------
# the inputs
# ------------------------------------------------------------------------------------------------
def _batch_features(inputs):
    """The feature tensors are inputs of the batch (FactorGraphBatch.set_features): graph 0's behind every graph.  The pots stay
    each graph's own."""
    for inp in inputs[1:]:
        for k in PHI:
            inp[k] = inputs[0][k]
    return inputs


def shared_inputs(name, width, B=None):
    """test_range_cpu.range_inputs(name, width) -- graph 0's en_en pots behind every graph, own unary pots -- with the batch's
    feature tensors: dict(spec, roots, inputs)."""
    case = R.range_inputs(name, width, B=B)
    _batch_features(case['inputs'])
    return case


def own_spec(name, X=64):
    import test_gpu_instances as TI
    return TI.SPECS[name](X), list(TI.ROOTS[name])


def own_inputs(name, width, B=OWN_B, seed=OWN_SEED, X=64):
    """Own tables per graph: cases.make_inputs(spec, seed + 1000 b) with scale_thetas applied to each graph ALONE (no pot is
    shared), the batch's feature tensors behind all."""
    spec, roots = own_spec(name, X)
    inputs = [C.make_inputs(spec, seed + 1000 * b) for b in range(B)]
    for inp in inputs:
        R.scale_thetas([inp], width)
    return dict(spec=spec, roots=roots, inputs=_batch_features(inputs))


def padded_inputs(X, B=PADDED_B, seed=PADDED_SEED):
    """user_k3 at X states, the shared layout (graph 0's en_en pots, own pot_en_de as exp(0.5 N(0,1))): the last real state's row
    and column of both en_en pots and the last row of pot_en_de times 1e3; the labels of every odd graph on state X - 1.
    -> dict(spec, roots, inputs, labels [B][n_vars] in Graph.var_order)."""
    spec, roots = own_spec('user_k3', X)
    base = C.make_inputs(spec, seed + X)
    rs = np.random.RandomState(seed + X + 1)
    for k in ('pot_en_en', 'pot_en_en_w1'):
        base[k] = base[k].copy()
        base[k][X - 1, :] *= 1e3
        base[k][:, X - 1] *= 1e3
    inputs = []
    for b in range(B):
        i = dict(base)
        i['pot_en_de'] = np.exp(rs.randn(*base['pot_en_de'].shape) * 0.5)
        i['pot_en_de'][X - 1, :] *= 1e3
        inputs.append(i)
    order = O.Graph(spec).var_order
    label_of = dict(zip(spec['var_ids'], spec['labels']))
    labels = np.array([[X - 1 if b % 2 else label_of[v] for v in order] for b in range(B)], dtype=np.int64)
    return dict(spec=spec, roots=roots, inputs=inputs, labels=labels)


def spec_with_labels(spec, labels):
    """spec with the labels of one graph, given in Graph.var_order."""
    s = copy.deepcopy(spec)
    order = O.Graph(spec).var_order
    s['labels'] = [int(labels[order.index(v)]) for v in s['var_ids']]
    return s


def hand_over_inputs(case, what, B=None, b_edit=None):
    """-> dict(spec, roots, inputs, clean, b_edit, factor): `inputs` with ONE entry of graph b_edit set to HAND_OVER[what],
    `clean` without; `factor` the id of a factor that reads the entry.
    lean_user_k3: own tables, B = 13, entry (3, 9) of graph 5's pot_en_en (every pairwise factor of user_k3 has a gap > 1).
    shared_user_k3_gaps_3_6: B = 37, graph 21, row 5 of a column of its OWN pot_en_en_w1 that a unary gap-1 factor observes
      (the spec has no pairwise factor at gap 1: test_gpu_exponent_range.test_hand_over_shared).
    shared_user_k4: B = 37, graph 21, row 5 of the pot_en_de column its first en_de factor observes (user_k4 has a pairwise
      factor at gap 1, which reads graph 0's pot_en_en_w1 on the device: the graph's own entry sits in pot_en_de)."""
    value = HAND_OVER[what]
    if case == 'lean_user_k3':
        base = own_inputs('user_k3', 1, B=13 if B is None else B, seed=4300)
        b_edit, key, at = 5 if b_edit is None else b_edit, 'pot_en_en', (3, 9)
        fac = [f for f in base['spec']['factors'] if len(f['vars']) == 2][1]
        assert all(f['gap'] > 1 for f in base['spec']['factors'] if len(f['vars']) == 2)
    else:
        name = case[len('shared_'):]
        base = shared_inputs(name, 1, B=B)
        b_edit = 21 if b_edit is None else b_edit
        spec = base['spec']
        if name == 'user_k3_gaps_3_6':
            assert not [f for f in spec['factors'] if len(f['vars']) == 2 and f['gap'] == 1]
            fac = [f for f in spec['factors'] if len(f['vars']) == 1 and f['factor_type'] == 'en_en' and f['gap'] == 1][0]
            key = 'pot_en_en_w1'
        else:
            fac = [f for f in spec['factors'] if f['factor_type'] == 'en_de'][0]
            key = 'pot_en_de'
        at = (5, fac['observed_dim'])
    clean = [dict(i) for i in base['inputs']]
    inputs = [dict(i) for i in base['inputs']]
    inputs[b_edit][key] = inputs[b_edit][key].copy()
    inputs[b_edit][key][at] = value
    return dict(spec=base['spec'], roots=base['roots'], inputs=inputs, clean=clean, b_edit=b_edit, factor=fac['id'])


# ------------------------------------------------------------------------------------------------
# the references (computed once per process, shared by the tests that need them, never written to)
# ------------------------------------------------------------------------------------------------
def graph_reference(spec, inputs, roots, start=None):
    """One graph: test_range_cpu.oracle_is_normal plus the oracle's gradient ('g_ee', 'g_ed')."""
    pre = R.oracle_is_normal(spec, inputs, roots, start)
    pre['g_ee'], pre['g_ed'] = oracle_gradient(pre['g'], inputs, pre['msgs'])
    return pre


@functools.lru_cache(maxsize=None)
def shared_reference(name, width, B=None):
    case = shared_inputs(name, width, B)
    return case, [graph_reference(case['spec'], inp, case['roots']) for inp in case['inputs']]


@functools.lru_cache(maxsize=None)
def own_reference(name, width, B=OWN_B, X=64):
    case = own_inputs(name, width, B=B, X=X)
    return case, [graph_reference(case['spec'], inp, case['roots']) for inp in case['inputs']]


@functools.lru_cache(maxsize=None)
def padded_reference(X, B=PADDED_B):
    case = padded_inputs(X, B)
    refs = [graph_reference(spec_with_labels(case['spec'], case['labels'][b]), inp, case['roots']) for b, inp in enumerate(case['inputs'])]
    return case, refs


def assert_precondition(name, case, refs):
    """Every graph: the oracle stays normal and its gradient is the log-domain statement's to BAR.  Returns the worst distance."""
    worst, lo = 0.0, np.inf
    for b, (inp, pre) in enumerate(zip(case['inputs'], refs)):
        R.assert_normal('%s graph %d' % (name, b), pre)
        dist = statement_distance(pre['g'], inp, pre['msgs'])
        assert dist <= BAR, '%s graph %d: oracle gradient %.3g from the log-domain statement' % (name, b, dist)
        worst, lo = max(worst, dist), min(lo, pre['min_message'])
    print('%s: %d graphs, worst |oracle gradient - statement| %.2e, smallest message entry %.1e' % (name, len(refs), worst, lo))
    return worst


# ------------------------------------------------------------------------------------------------
# the statement itself
# ------------------------------------------------------------------------------------------------
def test_statement_is_the_oracle_gradient_at_unit_magnitude():
    """Mild tables (width 1): the two are one number far below BAR, on a pairwise-free graph (user_k1) too."""
    for name in ('user_k1', 'user_k2', 'user_k3'):
        case = own_inputs(name, 1, B=3)
        for inp in case['inputs']:
            pre = R.oracle_is_normal(case['spec'], inp, case['roots'])
            assert statement_distance(pre['g'], inp, pre['msgs']) <= 1e-14


def test_statement_does_not_feel_a_scale_the_float64_product_cannot_carry():
    """Messages scaled to 1e-170 each: c_i r_j underflows in the oracle's order, whose beliefs are then zero -- the statement is
    unchanged.  (Why the precondition is asserted and not assumed.)"""
    case = own_inputs('user_k2', 1, B=1)
    inp = case['inputs'][0]
    pre = R.oracle_is_normal(case['spec'], inp, case['roots'])
    want = gradient_statement(pre['g'], inp, pre['msgs'])
    tiny = {k: v * 1e-170 for k, v in pre['msgs'].items()}
    got = gradient_statement(pre['g'], inp, tiny)
    assert float(np.max(np.abs(got[0] - want[0]))) <= 1e-14
    assert statement_distance(pre['g'], inp, tiny) > 1e-3


# ------------------------------------------------------------------------------------------------
# part B: the preconditions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,width', SHARED_CASES)
def test_oracle_gradient_is_the_statement_on_the_shared_table_specs(name, width):
    case, refs = shared_reference(name, width)
    assert len(refs) == R.SHARED_B
    assert_precondition('%s thetas x %d' % (name, width), case, refs)


def test_standalone_x128_case_meets_the_precondition():
    """The standalone shared gradient's case of part B: user_k3 at X = 128, thetas times 8, B = 19 (graph 0's en_en pots)."""
    case, refs = standalone_x128_reference()
    assert_precondition('user_k3 x128 thetas x 8', case, refs)


@functools.lru_cache(maxsize=None)
def standalone_x128_reference(B=19, seed=4400):
    spec, roots = own_spec('user_k3', 128)
    inputs = [C.make_inputs(spec, seed + 1000 * b) for b in range(B)]
    R.scale_thetas(inputs, 8)
    case = dict(spec=spec, roots=roots, inputs=_batch_features(inputs))
    return case, [graph_reference(spec, inp, roots) for inp in inputs]


@pytest.mark.parametrize('name,width', OWN_CASES)
def test_oracle_gradient_is_the_statement_on_own_tables(name, width):
    case, refs = own_reference(name, width)
    assert len(refs) == OWN_B
    pots = [case['inputs'][b]['pot_en_en'] for b in range(OWN_B)]
    assert not any(np.array_equal(pots[0], p) for p in pots[1:])           # no pot is shared
    assert_precondition('own tables %s thetas x %d' % (name, width), case, refs)


# ------------------------------------------------------------------------------------------------
# part C: what the oracle's gradient is on the hand-over inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('what', list(HAND_OVER))
@pytest.mark.parametrize('case', HAND_OVER_CASES)
def test_oracle_gradient_is_defined_on_the_hand_over_inputs(case, what):
    h = hand_over_inputs(case, what)
    b = h['b_edit']
    got = graph_reference(h['spec'], h['inputs'][b], h['roots'])          # (raises nothing)
    clean = graph_reference(h['spec'], h['clean'][b], h['roots'])
    g, inp = got['g'], h['inputs'][b]
    assert not np.isnan(got['g_ee']).any() and not np.isnan(got['g_ed']).any()      # the statement: no NaN component
    assert np.isfinite(got['g_ee']).all() and np.isfinite(got['g_ed']).all()
    changed = not (np.array_equal(got['g_ee'], clean['g_ee']) and np.array_equal(got['g_ed'], clean['g_ed']))
    assert changed
    f = g.by_id[h['factor']]
    T = O.factor_table(g, inp, f)
    assert (np.isnan(T).any() if what == 'nan' else (T < 0).any())        # the factor reads the entry
    with np.errstate(all='ignore'):
        if len(f['vars']) == 1:
            total = np.sum(T)
        else:
            by_axis = {g.dim_of(f, v): v for v in f['vars']}
            c = got['msgs']['X_%d' % by_axis[0], 'F_%d' % f['id']].reshape(-1, 1)
            r = got['msgs']['X_%d' % by_axis[1], 'F_%d' % f['id']].reshape(1, -1)
            total = np.sum(c.dot(r) * T)
        fg = O.factor_gradient(g, inp, got['msgs'], f['id']).reshape(-1)
    phi = O.factor_phi(g, inp, f)
    alone = phi[g.label[f['vars'][0]], f['observed_dim']] if len(f['vars']) == 1 else phi[O.observed_cell(g, f)]
    print('%s %s: total of the edited factor %r; its gradient is phi[label] alone: %s' % (case, what, float(total), np.array_equal(fg, alone)))
    if not total > 0.0:                        # au.normalize: NaN or non-positive total -> zero beliefs
        assert np.array_equal(fg, alone)
    else:                                      # a positive total with a negative entry: finite beliefs, one of them negative
        assert np.isfinite(fg).all() and not np.array_equal(fg, alone)
    if what == 'nan':
        assert not total > 0.0
    for other in (0, len(h['inputs']) - 1):                               # the other graphs are untouched
        assert all(h['inputs'][other][k] is h['clean'][other][k] or np.array_equal(h['inputs'][other][k], h['clean'][other][k])
                   for k in ('pot_en_en', 'pot_en_en_w1', 'pot_en_de'))


# ------------------------------------------------------------------------------------------------
# part D: the padded cases
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('X', PADDED_X)
def test_oracle_gradient_is_the_statement_on_the_padded_cases(X):
    case, refs = padded_reference(X)
    assert len(refs) == PADDED_B
    assert (case['labels'][1::2] == X - 1).all() and not (case['labels'][0::2] == X - 1).all()
    assert_precondition('padded user_k3 x%d' % X, case, refs)
    # the last real state carries most of the mass: a padding bug would show at 1e-10
    heavy = min(float(pre['marginals'][:, X - 1].min()) for pre in refs)
    print('padded user_k3 x%d: smallest marginal of the last state %.3f' % (X, heavy))
    assert heavy > 0.5


# ------------------------------------------------------------------------------------------------
# a normaliser Z that is itself tiny, with tables and messages in range
# ------------------------------------------------------------------------------------------------
TINY_ENTRY, TINY_REST, TINY_STATE = 1e-225, 1e-240, 17


def tiny_normaliser_inputs(B=R.SHARED_B):
    """Shared user_k2 (one pairwise factor, test_gpu_shared.SPECS) at unit-magnitude thetas, edited so that the pairwise belief's
    normaliser Z = sum c_i T_ij r_j is about 1e-225 although every table entry, message and marginal is a normal number: both
    variables' unary products peak on state TINY_STATE (every other row of each graph's own pot_en_de times TINY_REST), and the
    shared pairwise table's entry (TINY_STATE, TINY_STATE) is TINY_ENTRY.  The belief then sits on that one cell: the terms
    c_s T_sj r_j are near TINY_REST and all others far below.  Uniform scaling cannot make such a Z -- the shared-table sweeps hand
    a graph over long before (their contraction of two scaled operands leaves the range) -- so this is the case that holds the
    epilogue's `Z > 0` against a small positive Z.  -> dict(spec, roots, inputs, factor)."""
    case = shared_inputs('user_k2', 1, B=B)
    spec, s = case['spec'], TINY_STATE
    pf = [f for f in spec['factors'] if len(f['vars']) == 2]
    assert len(pf) == 1 and pf[0]['gap'] == 1
    unary_w1 = [f['observed_dim'] for f in spec['factors'] if len(f['vars']) == 1 and f['factor_type'] == 'en_en' and f['gap'] == 1]
    assert s not in unary_w1                       # (no unary factor reads the edited entry's column)
    pot = case['inputs'][0]['pot_en_en_w1'].copy()
    pot[s, s] = TINY_ENTRY
    for inp in case['inputs']:
        inp['pot_en_en_w1'] = pot
        de = inp['pot_en_de'].copy()
        keep = de[s].copy()
        de *= TINY_REST
        de[s] = keep
        inp['pot_en_de'] = de
    case['factor'] = pf[0]['id']
    return case


@functools.lru_cache(maxsize=None)
def tiny_normaliser_reference(B=R.SHARED_B):
    case = tiny_normaliser_inputs(B)
    return case, [graph_reference(case['spec'], inp, case['roots']) for inp in case['inputs']]


def pair_normaliser(g, inputs, msgs, fid):
    """Z = sum c_i T_ij r_j of pairwise factor fid in float64, the reference's order."""
    f = g.by_id[fid]
    by_axis = {g.dim_of(f, v): v for v in f['vars']}
    c = msgs['X_%d' % by_axis[0], 'F_%d' % fid].reshape(-1, 1)
    r = msgs['X_%d' % by_axis[1], 'F_%d' % fid].reshape(1, -1)
    with np.errstate(all='ignore'):
        return float(np.sum(c.dot(r) * O.factor_table(g, inputs, f)))


def test_tiny_normaliser_case_is_in_range_and_its_oracle_gradient_is_the_statement():
    case, refs = tiny_normaliser_reference()
    worst, zs = 0.0, []
    for b, (inp, pre) in enumerate(zip(case['inputs'], refs)):
        assert pre['finite'] and not pre['uniform'] and pre['min_message'] >= 1e-300 and pre['min_marginal'] >= 1e-300, (b, pre['min_message'], pre['min_marginal'])
        dist = statement_distance(pre['g'], inp, pre['msgs'])
        assert dist <= BAR, (b, dist)
        worst = max(worst, dist)
        zs.append(pair_normaliser(pre['g'], inp, pre['msgs'], case['factor']))
    print('tiny normaliser: %d graphs, Z from %.2e to %.2e, worst |oracle gradient - statement| %.2e' % (len(refs), min(zs), max(zs), worst))
    assert 0.0 < min(zs) and max(zs) < 1e-210
