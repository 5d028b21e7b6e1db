"""The top-100 approximate paths without a GPU: the library's selection rule as a NumPy statement, the oracle's approximate
sweeps under that rule, and the precondition under which the result is ground truth for tests/test_gpu_approx.py.

Why the oracle alone is not a reference here.  `use_approx_inference` / `use_approx_beliefs` keep the 100 largest entries of a
message.  Where the 100th place is tied the answer depends on which of the tied entries are kept, and the reference leaves
that to np.argpartition (oracle/array_oracle.py:_topk_desc): NumPy's introselect, whose choice on a tied vector changes with
the vector's length.  Every loopy graph meets such a tie at once -- the loop-closing messages of the first sweep are still
the uniform vector when they are first selected from -- and on a uniform vector argpartition returns 0..99 at n = 101, 128
and 201 but not at n = 300, 451, 700, 1001 or 1024.  The library's rule (mlbp_device.h ranks_above, the order of
mlbp_topk_f64) is: by value descending, every NaN below every number, ties -- NaNs among themselves too -- to the lower
index.  `select` states it; `walk` runs the oracle with `_topk_desc` following it.

When the walk is ground truth.  Device and walk messages differ by rounding (about 1e-13 relative), so a selection is the
same on both sides when it is decided by the rule itself -- a tie of bit-equal values: the `uniform` and `zero` classes, and
any vector the caller supplied, whose bits the device reads as they are -- or by a gap between the 100th and 101st largest
entry that rounding cannot close.  `decided(records, floor=1e-8)` is that condition; the floor is a condition, not a
measurement, and leaves five orders of margin.  The GPU tests call it on the same inputs before they compare, and the tests
here assert it for every graph of every case of tests/test_gpu_approx.py."""
import contextlib

import numpy as np
import pytest

import cases as C
from oracle import array_oracle as AO
from oracle import lbp_oracle as O

K = AO.TOP_K
FLOOR = 1e-8


def select(vec, k=K):
    """Indices of the k largest entries of vec by the library's rule, best first: by value descending, every NaN below every
    number, ties (NaNs among themselves too) to the lower index.  (c_array_utils._top_k's lexsort with the NaN key added.)"""
    v = np.asarray(vec, dtype=np.float64).reshape(-1)
    nan = np.isnan(v)
    return np.lexsort((np.arange(v.size), np.where(nan, 0.0, -v), nan))[:k]


def classify(vec, k=K, supplied=False, slot=None):
    """What decides the selection from vec: dict(cls, gap, supplied, slot, n).
    nan: the vector holds a NaN;  all: n <= k, everything is kept;  uniform: all entries bit-equal;  zero: the k-th and
    (k+1)-th largest are both exactly 0;  gap: otherwise, with gap = (v_k - v_k+1) / v_k."""
    v = np.asarray(vec, dtype=np.float64).reshape(-1)
    rec = dict(cls='gap', gap=None, supplied=bool(supplied), slot=slot, n=v.size)
    if np.isnan(v).any():
        rec['cls'] = 'nan'
    elif v.size <= k:
        rec['cls'] = 'all'
    elif (v.view(np.int64) == v.view(np.int64)[0]).all():
        rec['cls'] = 'uniform'
    else:
        s = np.sort(v)[::-1]
        if s[k - 1] == 0.0 and s[k] == 0.0:
            rec['cls'] = 'zero'
        else:
            with np.errstate(all='ignore'):
                rec['gap'] = float((s[k - 1] - s[k]) / s[k - 1])
    return rec


@contextlib.contextmanager
def ruled_topk(records=None, supplied=None, rule=True):
    """array_oracle._topk_desc follows `select` for the duration (rule=False: left as it is, only recorded).  Where the
    rule's index set is the one argpartition chose, argpartition's own array is returned, so the sums downstream add in the
    reference's order and the walk equals the unpatched oracle bit for bit wherever the two agree.  records: a list that
    receives classify() of every vector selected from; supplied: {bytes of a vector the caller supplied: its slot}."""
    saved = AO._topk_desc
    supplied = supplied or {}

    def topk(vec1d):
        ref = saved(vec1d)                      # (raises for len < K like the reference)
        if records is not None:
            v = np.ascontiguousarray(vec1d, dtype=np.float64)
            slot = supplied.get(v.tobytes())
            records.append(classify(v, supplied=slot is not None, slot=slot))
        if not rule:
            return ref
        idx = select(vec1d)
        return ref if set(ref.tolist()) == set(idx.tolist()) else idx

    AO._topk_desc = topk
    try:
        yield
    finally:
        AO._topk_desc = saved


def walk(spec, inputs, roots, start=None, approx_beliefs=False, rule=True):
    """The oracle's approximate sweeps on one graph, rooted at `roots` in turn, with the top-100 following `select` ->
    dict(messages [n_msgs][X] in cases.msg_keys order, marginals [n_vars][X] in Graph.var_order, gradient (en_en, en_de) of
    unregularized_gradient(approx=approx_beliefs) for a train_mp-style spec else None, records: classify() of every vector
    selected from, n_sweep_records: how many of them the sweeps made).  start: optional [n_msgs][X] starting messages in
    cases.msg_keys order (init=False); a vector selected from while it still holds the bits of a starting message is
    recorded as supplied, with that message's slot."""
    g = O.Graph(spec)
    keys = C.msg_keys(spec)
    msgs = O.init_messages(g)
    if start is not None:
        for i, k in enumerate(keys):
            msgs[k] = np.array(start[i], dtype=np.float64)
    supplied = {np.ascontiguousarray(msgs[k]).tobytes(): i for i, k in enumerate(keys)}
    records = []
    with np.errstate(all='ignore'), ruled_topk(records, supplied, rule):
        for r in roots:
            O.sweep(g, inputs, msgs, r, True)
        n_sweep = len(records)
        messages = np.stack([msgs[k] for k in keys])
        marginals = np.stack([O.marginal(g, msgs, v).reshape(-1) for v in g.var_order])
        gradient = None
        if spec['style'] == 'trainmp':
            ee, ed = O.unregularized_gradient(g, inputs, msgs, approx_beliefs)
            gradient = (ee.reshape(-1), ed.reshape(-1))
    return dict(messages=messages, marginals=marginals, gradient=gradient, records=records, n_sweep_records=n_sweep)


def decided(records, floor=FLOOR):
    """True when every selection of the walk is the device's too: a vector the rule decides on bit-equal values (uniform,
    zero, all, or supplied by the caller: the device reads the same bits) or one whose gap is at least `floor`.  A NaN in a
    vector the sweeps COMPUTED is not decided (whether an entry is NaN there can hinge on rounding)."""
    for r in records:
        if r['supplied'] or r['cls'] in ('uniform', 'zero', 'all'):
            continue
        if r['cls'] == 'nan' or not (r['gap'] >= floor):
            return False
    return True


def smallest_gap(records):
    """The smallest gap among the records decided by a gap (inf when there is none)."""
    gaps = [r['gap'] for r in records if r['cls'] == 'gap' and not r['supplied']]
    return min(gaps) if gaps else float('inf')


# ---- the rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [100, 101, 300, 1024])
def test_select_is_argpartitions_set_without_ties(n):
    v = np.random.RandomState(n).rand(n)
    assert set(select(v).tolist()) == set(AO._topk_desc(v).tolist())
    assert (np.diff(v[select(v)]) < 0).all()                    # best first


def test_select_breaks_the_uniform_tie_by_index_and_argpartition_does_not():
    for n in (101, 128, 201, 300, 1024):
        np.testing.assert_array_equal(select(np.full(n, 1.0 / n)), np.arange(100))
    # the reason the walk exists: NumPy's introselect leaves 0..99 at n = 300, so a loopy graph's first sweep -- which selects
    # from uniform messages -- has no reference in the unpatched oracle at such a size
    assert set(AO._topk_desc(np.full(300, 1.0 / 300)).tolist()) != set(range(100))
    assert set(AO._topk_desc(np.full(128, 1.0 / 128)).tolist()) == set(range(100))      # (why the X = 128 fixtures agree)


def test_select_ties_and_zeros():
    v = np.zeros(300)
    v[[7, 250, 31]] = [3.0, 3.0, 5.0]
    np.testing.assert_array_equal(select(v, 5), [31, 7, 250, 0, 1])
    assert classify(v)['cls'] == 'zero'
    v[:] = np.arange(300, 0, -1)
    v[100] = v[99]                                              # the 100th and 101st largest are equal: index 99 wins
    np.testing.assert_array_equal(select(v), np.arange(100))
    assert classify(v) == dict(cls='gap', gap=0.0, supplied=False, slot=None, n=300)
    assert not decided([classify(v)]) and decided([classify(v, supplied=True)])
    assert classify(np.full(100, 0.01))['cls'] == 'all' and classify(np.full(101, 0.01))['cls'] == 'uniform'


def test_select_puts_nan_below_every_number():
    import test_gpu_kernels as GK
    for name, (v, k) in GK._nan_vectors().items():
        np.testing.assert_array_equal(select(v, k), GK._lexsort_topk(v, k), err_msg=name)
        assert classify(v)['cls'] == 'nan'
    v = np.array([np.nan, -np.inf, np.inf, 1.0, np.nan, -2.0])
    np.testing.assert_array_equal(select(v, 6), [2, 3, 5, 1, 0, 4])
    one, _ = GK._nan_vectors()['one_nan']
    assert set(select(one).tolist()) == set(AO._topk_desc(one).tolist())     # argpartition(-v) sorts NaN last too


# ---- the walk --------------------------------------------------------------------------------------------------------
def test_walk_is_the_oracle_on_a_tree():
    """chain3 at X = 300 has no tied selection, so the rule changes nothing: the same bits as the unpatched oracle."""
    spec = C.chain_spec(3, 300)
    inputs = C.make_inputs(spec, 7000, 'lognormal')
    a, b = walk(spec, inputs, [0, 2, 1, 0]), walk(spec, inputs, [0, 2, 1, 0], rule=False)
    assert a['messages'].tobytes() == b['messages'].tobytes() and a['marginals'].tobytes() == b['marginals'].tobytes()
    assert a['records'] == b['records'] and {r['cls'] for r in a['records']} == {'gap'} and decided(a['records'])
    g, msgs, _ = O.run(spec, inputs, [0, 2, 1, 0], 4, force_loopy=True, approx=True)
    assert np.stack([msgs[k] for k in C.msg_keys(spec)]).tobytes() == a['messages'].tobytes()


def test_walk_differs_from_the_oracle_on_a_loop_at_300():
    """ring3 at X = 300: the first sweep selects from uniform messages, the oracle keeps argpartition's set, the walk 0..99."""
    spec = C.ring_spec(3, 300)
    inputs = C.make_inputs(spec, 7000, 'uniform')
    a, b = walk(spec, inputs, [0, 2, 1, 0]), walk(spec, inputs, [0, 2, 1, 0], rule=False)
    assert sum(r['cls'] == 'uniform' for r in a['records']) > 0
    assert not np.allclose(a['messages'], b['messages'], rtol=1e-6, atol=0)
    assert ruled_is_restored()


def ruled_is_restored():
    return AO._topk_desc.__name__ == '_topk_desc'


def test_walk_restores_the_oracle_after_an_error():
    spec = C.ring_spec(3, 64)
    with pytest.raises(ValueError, match='out of bounds'):
        walk(spec, C.make_inputs(spec, 1), [0])
    assert ruled_is_restored()


def test_walk_records_supplied_vectors():
    spec = C.ring_spec(3, 201)
    start = np.random.RandomState(3).rand(len(C.msg_keys(spec)), 201) + 0.05
    w = walk(spec, C.make_inputs(spec, 7000), [0], start=start)
    assert any(r['supplied'] for r in w['records']) and not all(r['supplied'] for r in w['records'])
    assert decided(w['records'])


def test_every_gpu_case_is_decided():
    """The precondition of tests/test_gpu_approx.py, for every graph of every case of its table."""
    import test_gpu_approx as G
    assert len(G.CASES) >= 30
    for name in sorted(G.CASES):
        ref = G.reference(name)
        assert len(ref) == G.CASES[name]['B'], name
        for b, w in enumerate(ref):
            assert w['records'], (name, b)
            assert decided(w['records']), (name, b, smallest_gap(w['records']))
