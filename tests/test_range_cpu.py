"""Exponent range without a GPU: the inputs of tests/test_gpu_exponent_range.py parts B and C, and the precondition under which
the float64 oracle is ground truth for them.

Wide-range potentials are where float64 semantics and the mathematics can part: an entry flushed to zero, or a message whose
total underflows and which the zero-sum -> uniform rule (Message.renormalize, LBP.py:655-657) then replaces.  Part B compares
every graph with the oracle, so it uses wide tables only where the oracle itself stays clear of both.  `oracle_is_normal` runs
the oracle on one graph and reports the smallest message and marginal entry, whether any message is the uniform vector, and
whether everything is finite; the tests here assert, for every (shape, width) of part B,

    smallest entry >= 1e-250, no uniform message, nothing non-finite,

and the GPU tests call the same function on the same inputs before they compare, so a later change of seeds cannot move a case
out of that regime unnoticed.  (Widths: explicit tables are exp(sigma N(0,1)), sigma 5 and 20 -- K3 at sigma 30 already has
entries flushed to zero in the oracle, at 60 the uniform rule acts; the train-layout inputs are cases.make_inputs with both
thetas multiplied by 8 or 64 and the pots rebuilt, at 64 the tables span 1e69.)

The file also states log Z in the log domain (every product a sum of logs, every sum a log-sum-exp) on the oracle's messages:
the reference of part B's log_partition cases, pinned here on the float64 statement of tests/test_logz_cpu.py."""
import numpy as np
import pytest

import cases as C
import test_logz_cpu as S
import test_map_cpu as W
from oracle import lbp_oracle as O

FLOOR = 1e-250          # the precondition's smallest entry
SHARED_B = 37
SHARED_SEED = 7

K7 = lambda: C.user_spec(12, [0, 1, 3, 5, 7, 9, 11], 64, 64, seed=5)           # noqa: E731  (test_gpu_logz.test_k7's graph)


def _explicit(spec):
    from test_gpu_lean_memory import _explicit as ex
    return ex(spec)


# name -> (spec, roots, graphs, seed): the lean kernel's shapes of test_gpu_lean_memory / test_gpu_lean_chain
LEAN = {
    'k3': (lambda: _explicit(C.user_spec(10, [1, 4, 7], 64, 40, seed=1)), [4, 1, 7, 4], 13, 3101),
    'star6': (lambda: C.star_spec(6, 64), [0, 3, 0, 5], 5, 3102),
    'chain8': (lambda: C.chain_spec(8, 64), [0, 7, 3, 0], 5, 3103),
    'k7': (lambda: _explicit(K7()), [0, 1, 3], 6, 3104),               # log_partition only (21 pairwise tables: the exact kernel sweeps)
}
LEAN_WIDTHS = (5, 20)
SHARED_WIDTHS = (8, 64)


def shared_specs():
    from test_gpu_shared import SPECS
    return SPECS


def scale_thetas(inputs, mult):
    """In place, on a list of trainmp inputs as test_gpu_shared._shared_batch builds it (graph 0's en_en pots behind every graph):
    both theta rows times `mult`, the pots rebuilt as cases.make_inputs forms them."""
    for inp in inputs:
        X = inp['phi_en_en'].shape[0]
        inp['theta_en_en'] = inp['theta_en_en'] * mult
        inp['theta_en_de'] = inp['theta_en_de'] * mult
        inp['pot_en_en'] = np.exp(inp['phi_en_en'].dot(inp['theta_en_en'].T).reshape(X, X))
        inp['pot_en_en_w1'] = np.exp(inp['phi_en_en_w1'].dot(inp['theta_en_en'].T).reshape(X, X))
        inp['pot_en_de'] = np.exp(inp['phi_en_de'].dot(inp['theta_en_de'].T).reshape(X, -1))
    for inp in inputs[1:]:
        inp['pot_en_en'] = inputs[0]['pot_en_en']
        inp['pot_en_en_w1'] = inputs[0]['pot_en_en_w1']


def range_inputs(name, width, B=None, seed=None):
    """-> dict(spec, roots, inputs): one oracle inputs dict per graph.
    name in LEAN: explicit tables exp(width N(0,1)), every graph its own.
    name in test_gpu_shared.SPECS: make_inputs(spec, seed + 1000 b) with the thetas times `width`, graph 0's en_en pots behind
    every graph (what _shared_batch(spec, B, seed, mutate=lambda i: scale_thetas(i, width)) puts on the device)."""
    if name in LEAN:
        make, roots, n, s = LEAN[name]
        spec = make()
        rs = np.random.RandomState((s if seed is None else seed) + int(width))
        X = spec['X']
        ntab = 1 + max(f['table'] for f in spec['factors'])
        shape = {f['table']: (X, X) if len(f['vars']) == 2 else (X, 1) for f in spec['factors']}
        inputs = [dict(tables=[np.exp(width * rs.randn(*shape[t])) for t in range(ntab)]) for _ in range(n if B is None else B)]
        return dict(spec=spec, roots=list(roots), inputs=inputs)
    spec = shared_specs()[name]()
    n = SHARED_B if B is None else B
    s = SHARED_SEED if seed is None else seed
    inputs = [C.make_inputs(spec, s + 1000 * b) for b in range(n)]
    scale_thetas(inputs, width)
    order = O.Graph(spec).var_order                   # == GraphTopology.var_ids
    return dict(spec=spec, roots=(list(order) * 3)[:3], inputs=inputs)


def start_messages(spec, B, seed):
    """Random positive messages [B][n_msgs][X] to start from (init=False), as test_gpu_lean_memory._Batch.start draws them."""
    return np.random.RandomState(seed).rand(B, len(C.msg_keys(spec)), spec['X']) + 0.05


def oracle_is_normal(spec, inputs, roots, start=None):
    """The oracle's sweeps on one graph (from uniform messages, or from start [n_msgs][X]) ->
    dict(min_message, min_marginal, uniform: some message equals the uniform vector, finite, messages [n_msgs][X] in
    cases.msg_keys order, marginals [n_vars][X] in Graph.var_order).  `ok` is the precondition of part B."""
    g = O.Graph(spec)
    keys = C.msg_keys(spec)
    msgs = O.init_messages(g)
    if start is not None:
        for i, k in enumerate(keys):
            msgs[k] = np.array(start[i], dtype=np.float64)
    with np.errstate(all='ignore'):
        for r in roots:
            O.sweep(g, inputs, msgs, r)
        marg = np.stack([O.marginal(g, msgs, v).reshape(-1) for v in g.var_order])
    m = np.stack([np.asarray(msgs[k]).reshape(-1) for k in keys])
    uni = 1.0 / g.X
    out = dict(min_message=float(np.min(m)), min_marginal=float(np.min(marg)),
               uniform=bool(np.any(np.all(m == uni, axis=1))), finite=bool(np.isfinite(m).all() and np.isfinite(marg).all()),
               messages=m, marginals=marg, msgs=msgs, g=g)
    out['ok'] = out['finite'] and not out['uniform'] and out['min_message'] >= FLOOR and out['min_marginal'] >= FLOOR
    return out


def assert_normal(name, got):
    assert got['finite'], name
    assert not got['uniform'], '%s: a message is the uniform vector (the zero-sum rule acted)' % name
    assert got['min_message'] >= FLOOR and got['min_marginal'] >= FLOOR, (name, got['min_message'], got['min_marginal'])


# ------------------------------------------------------------------------------------------------
# log Z in the log domain
# ------------------------------------------------------------------------------------------------
def _lse(a):
    m = np.max(a)
    return float(m + np.log(np.sum(np.exp(a - m))))


def log_partition_logdomain(g, inputs, msgs):
    """test_logz_cpu.log_partition with every product a sum of logs and every sum a log-sum-exp: no intermediate can leave
    the range whatever the tables' magnitude.  msgs: the oracle's message dict (strictly positive entries)."""
    def loo(v, skip=None):
        acc = np.zeros(g.X)
        for fid in g.facset[v]:
            if fid != skip:
                acc = acc + np.log(np.asarray(msgs['F_%d' % fid, 'X_%d' % v]).reshape(-1))
        return acc
    total = 0.0
    for f in g.factors:
        T = np.log(O.factor_table(g, inputs, f))
        if len(f['vars']) == 1:
            total += _lse(T.reshape(-1) + loo(f['vars'][0], f['id']))
        else:
            by_axis = {g.dim_of(f, v): v for v in f['vars']}
            total += _lse(loo(by_axis[0], f['id'])[:, None] + T + loo(by_axis[1], f['id'])[None, :])
    for v in g.var_order:
        d = len(g.facset[v])
        if d != 1:
            total -= (d - 1) * _lse(loo(v))
    return float(total)


def statement_bound(spec):
    """What the float64 statement may differ from the log-domain one by: the kernel bound of tests/test_gpu_logz.py (one sum of
    at most X^2 + 16 terms under each of the F + V logarithms, both summation orders) -- the statement is such an evaluation."""
    g = O.Graph(spec)
    return 2.0 * (len(g.factors) + len(g.var_order)) * (spec['X'] ** 2 + 16) * 2.0 ** -53


LOGZ_CASES = [('k3', 5), ('k3', 20), ('chain8', 5), ('chain8', 20), ('k7', 10)]
MAP_CASES = [('k3', 20), ('chain8', 20)]


# ------------------------------------------------------------------------------------------------
# the preconditions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', LEAN_WIDTHS)
@pytest.mark.parametrize('name', ['k3', 'star6', 'chain8'])
def test_oracle_stays_normal_on_the_lean_shapes(name, width):
    case = range_inputs(name, width)
    B = len(case['inputs'])
    starts = [None] + ([start_messages(case['spec'], B, 3200 + width)] if name == 'k3' else [])
    for start in starts:
        lo_m, lo_g = np.inf, np.inf
        for b, inp in enumerate(case['inputs']):
            got = oracle_is_normal(case['spec'], inp, case['roots'], None if start is None else start[b])
            assert_normal('%s sigma %d graph %d' % (name, width, b), got)
            lo_m, lo_g = min(lo_m, got['min_message']), min(lo_g, got['min_marginal'])
        print('%s sigma %d init=%s: %d graphs, smallest message entry %.1e, smallest marginal entry %.1e'
              % (name, width, start is None, B, lo_m, lo_g))


@pytest.mark.parametrize('width', SHARED_WIDTHS)
@pytest.mark.parametrize('name', ['user_k2', 'user_k3_gaps_3_6', 'user_k3_gaps_1_2_3', 'user_k4', 'user_k5', 'user_k6'])
def test_oracle_stays_normal_on_the_shared_table_specs(name, width):
    case = range_inputs(name, width)
    lo_m, lo_g = np.inf, np.inf
    for b, inp in enumerate(case['inputs']):
        got = oracle_is_normal(case['spec'], inp, case['roots'])
        assert_normal('%s thetas x %d graph %d' % (name, width, b), got)
        lo_m, lo_g = min(lo_m, got['min_message']), min(lo_g, got['min_marginal'])
    span = np.log10(max(i['pot_en_de'].max() for i in case['inputs']) / min(i['pot_en_de'].min() for i in case['inputs']))
    print('%s thetas x %d: %d graphs, smallest message entry %.1e, smallest marginal entry %.1e, unary pots span 1e%.0f'
          % (name, width, len(case['inputs']), lo_m, lo_g, span))


def test_the_limits_of_the_precondition_are_where_the_widths_stop():
    """K3 at sigma 30: entries flushed to zero in the oracle; at sigma 60 the uniform rule acts.  (Why K3 is capped at 20.)"""
    c30 = range_inputs('k3', 30)
    got = [oracle_is_normal(c30['spec'], inp, c30['roots']) for inp in c30['inputs']]
    assert any(r['min_message'] == 0.0 or r['min_marginal'] == 0.0 for r in got)
    c60 = range_inputs('k3', 60)
    got = [oracle_is_normal(c60['spec'], inp, c60['roots']) for inp in c60['inputs']]
    assert any(r['uniform'] for r in got) and not any(r['ok'] for r in got)


@pytest.mark.parametrize('name,width', MAP_CASES)
def test_max_product_walk_has_no_near_tie_at_wide_range(name, width):
    """The may-omit cap of tests/test_gpu_map.py stays 0 at sigma 20: the seeds here give no variable whose two largest
    max-marginal entries are within 1e-6 relative."""
    case = range_inputs(name, width)
    gaps = []
    for inp in case['inputs']:
        w = W.walk(case['spec'], inp, case['roots'])
        gaps += list(w['gap'].values())
        assert all(np.isfinite(m).all() for m in w['mm'].values())
    print('%s sigma %d: smallest gap of the walk %.2e' % (name, width, min(gaps)))
    assert min(gaps) >= 1e-6


@pytest.mark.parametrize('name,width', LOGZ_CASES + [('star6', 20)])
def test_log_domain_statement_equals_the_float64_statement(name, width):
    """Inside the limit of include/mlbp_logz.h (the product of d_v normalised messages stays normal) the two statements are one
    number."""
    case = range_inputs(name, width)
    bound = statement_bound(case['spec'])
    worst = 0.0
    for b, inp in enumerate(case['inputs']):
        got = oracle_is_normal(case['spec'], inp, case['roots'])
        assert_normal('%s sigma %d graph %d' % (name, width, b), got)
        lz = S.log_partition(got['g'], inp, got['msgs'])
        ld = log_partition_logdomain(got['g'], inp, got['msgs'])
        assert np.isfinite(lz) and np.isfinite(ld)
        worst = max(worst, abs(lz - ld))
        assert abs(lz - ld) <= bound + 1e-12 * abs(ld), (name, width, b, lz, ld)
    print('%s sigma %d: float64 statement against the log domain, worst |diff| %.2e (bound %.2e)' % (name, width, worst, bound))


def test_float64_statement_leaves_the_range_at_k7_sigma_20():
    """The limit itself, not pinned on the device: K7 (d_v = 12) at sigma 20 -- the product of twelve normalised messages
    underflows in the float64 statement, which then differs from the log domain or is not finite."""
    case = range_inputs('k7', 20)
    off = []
    with np.errstate(all='ignore'):
        for inp in case['inputs']:
            got = oracle_is_normal(case['spec'], inp, case['roots'])
            lz = S.log_partition(got['g'], inp, got['msgs'])
            ld = log_partition_logdomain(got['g'], inp, got['msgs']) if got['min_message'] > 0 else np.nan
            off.append(not np.isfinite(lz) or not np.isfinite(ld) or abs(lz - ld) > statement_bound(case['spec']) + 1e-12 * abs(ld))
    assert any(off)


def test_log_domain_statement_on_a_tree_is_brute_force():
    spec = C.chain_spec(5, 8)
    for seed in range(5):
        inputs = dict(tables=[np.exp(20 * np.random.RandomState(seed).randn(*t.shape)) for t in C.make_inputs(spec, seed)['tables']])
        g, msgs = S.sweeps(spec, inputs, [0])
        _, _, grid = W.brute_force(g, inputs)
        np.testing.assert_allclose(log_partition_logdomain(g, inputs, msgs), S.logsumexp(grid), rtol=1e-12)


# ------------------------------------------------------------------------------------------------
# part C: the oracle is defined on the edited inputs
# ------------------------------------------------------------------------------------------------
def edit_pair_entry(inputs, table, value, at=(3, 9)):
    """Explicit inputs with entry `at` of pairwise table `table` set to value (a copy)."""
    tabs = list(inputs['tables'])
    tabs[table] = tabs[table].copy()
    tabs[table][at] = value
    return dict(tables=tabs)


@pytest.mark.parametrize('value', [-0.25, float('nan')], ids=['negative', 'nan'])
def test_oracle_is_defined_on_the_edited_tables(value):
    spec = LEAN['k3'][0]()
    pf = [f for f in spec['factors'] if len(f['vars']) == 2]
    inp = edit_pair_entry(C.make_inputs(spec, 5), pf[1]['table'], value)
    got = oracle_is_normal(spec, inp, LEAN['k3'][1])
    assert got['messages'].shape == (len(C.msg_keys(spec)), 64)
    clean = oracle_is_normal(spec, C.make_inputs(spec, 5), LEAN['k3'][1])
    assert not np.array_equal(got['messages'], clean['messages'], equal_nan=True)
    if np.isnan(value):          # a NaN total is no positive total: the uniform vector
        assert got['uniform'] and got['finite']
