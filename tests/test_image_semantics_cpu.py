"""What the images of the sweep-program compilers COMPUTE (csrc/mlbp_compile.cpp), on the CPU: the NumPy interpreters of
tests/image_interp.py run the pruned, the fused and the lean image of a program and must give the oracle's messages and
marginals.  tests/test_program_images.py pins the images word for word and so notices a change; this module judges whether the
words are right, also after a change made on purpose.

Cases: FAMILY_SIZE random (graph, roots) cases of image_interp.random_case -- 2-9 variables, trees plus up to three extra
factors, several unary factors on a variable, shuffled ids / creation order / axes, hubs with 5-8 pairwise factors, 1-6 roots
with repeats -- and the 55 shapes of make_program_images.shapes() (their graphs rebuilt at X = 5 with one table per factor; the
six hand-made op lists have no graph, and are held to the plain op list on random tables instead of the oracle).  X = 5,
C.make_inputs(..., 'uniform') tables, from uniform messages and continuing from the first call's messages, rtol 1e-10 /
atol 1e-300 (the project's bar for sums taken in another order).

No case is left out.  Where the lean kernel does not take a shape the test asserts why: the compiler's own refusals (ok = 0:
in-loop unary updates, a constant product of more than 15 messages; a read-out list of more than 15 entries) and the
launcher's (more than 8 pairwise factors: the micro-op's pair slot has three bits, lean_plan in csrc/mlbp_lean.hip); the
pruned and fused interpreters still run.

test_the_family_holds_every_form asserts what the cases reach (REQUIRED).  One form no graph reaches under the lean kernel: a
carry chain of THREE links needs a product of nine sources, a variable with nine pairwise factors, and the kernel takes eight
at the most; it is held by the hand-made list refuse_var_9_tiles (eight sources and the uniform base) and is not asked of the
GPU subset.  gpu_subset() is the smallest greedy cover of GPU_REQUIRED by family cases with every form held twice, at most 40;
tests/test_gpu_random_programs.py runs exactly these.
"""
import functools

import numpy as np
import pytest

import cases as C
import image_interp as I
import make_program_images as M
from helpers import batch_tables
from macaronicusermodeling_amd.topology import GraphTopology, program_images
from oracle import lbp_oracle as O

X = 5
FAMILY_SIZE = 256
RTOL, ATOL = 1e-10, 1e-300
PAIR_KINDS = ['TM|TM', 'MT|MT', 'TM|MT', 'MT|TM', 'TM|NOP', 'MT|NOP']
GPU_REQUIRED = PAIR_KINDS + ['VAR', '3SRC+VF', 'CARRY x2', 'odd n_bundles', 'even n_bundles', 'ends in VAR', 'ends in a contraction',
                             'n_cprod == 0', 'a variable without unary factor', 'a dead update dropped (differing roots)',
                             'a lone update kept (equal roots)', 'pruned drops nothing', 'pruned drops a whole sweep',
                             'lean refused: P > 8'] + ['P = %d' % p for p in range(1, 9)]
REQUIRED = GPU_REQUIRED + ['CARRY x3']


class Case:
    """One program: its op list and images, tables at X = 5, and the reference's messages and marginals after one call from
    uniform messages (first) and after a second call continuing from them (second)."""

    def __init__(self, name, shape, spec=None, roots=None, seed=0):
        self.name, self.shape, self.spec, self.roots = name, shape, spec, roots
        self.images = program_images(**shape)
        s = shape
        self.n_msgs, self.P, self.U = s['n_msgs'], s['P'], s['U']
        self.srcs = np.asarray(s['srcs'], dtype=np.int64).reshape(-1)
        self.in_off, self.in_slots = np.asarray(s['in_off']), np.asarray(s['in_slots'])
        if spec is not None:
            topo = GraphTopology.from_spec(spec)
            inputs = C.make_inputs(spec, 4000 + seed, 'uniform')
            self.pair, self.unary = batch_tables(spec, topo, [inputs])
            g, keys = O.Graph(spec), topo.slot_keys()
            msgs = O.init_messages(g)
            self.ref = []
            for _ in range(2):
                for r in roots:
                    O.sweep(g, inputs, msgs, r)
                self.ref.append((np.stack([msgs[k] for k in keys]), np.stack([O.marginal(g, msgs, v).reshape(-1) for v in topo.var_ids])))
        else:                                             # a hand-made op list: the plain list on random tables is the reference
            rs = np.random.RandomState(4000 + seed)
            self.pair, self.unary = rs.rand(self.P, X, X) + 0.01, rs.rand(self.U, X) + 0.01
            self.ref, start = [], None
            for _ in range(2):
                m = I.run_ops(s['ops'], self.srcs, s['sweeps'], self.n_msgs, self.pair, self.unary, start, start is None)
                self.ref.append((m, I.marginals_of(m, self.in_off, self.in_slots)))
                start = m
        self.fused, self.lean = I.parse_fused(self.images['fused']), I.parse_lean(self.images['lean'])
        self.readout_ok = int(self.images['lean_readout'][0])
        self.lean_decodable = bool(self.lean['ok']) and self.P <= 8

    def starts(self):
        """(what, start messages, init, reference) of the two calls."""
        return [('from uniform', None, True, self.ref[0]), ('continuing', self.ref[0][0], False, self.ref[1])]

    def forms(self):
        out = set()
        if self.lean_decodable and self.lean['n_bundles'] > 0 and 1 <= self.P:
            out |= I.lean_forms(self.lean['bundles'])
            out.add('P = %d' % self.P)
            if self.lean['n_cprod'] == 0:
                out.add('n_cprod == 0')
        if self.lean['ok'] and self.P > 8:
            out.add('lean refused: P > 8')
        if not self.lean['ok']:
            out.add('lean refused: ok = 0')
        ops, dropped = I.parse_pruned(self.images['pruned'])[::2]
        sweeps2 = I.parse_pruned(self.images['pruned'])[1]
        out.add('pruned drops nothing' if dropped == 0 else 'pruned drops updates')
        if len(sweeps2) and (sweeps2[:, 1] == 0).any():
            out.add('pruned drops a whole sweep')
        if self.spec is not None:
            with_unary = {f['vars'][0] for f in self.spec['factors'] if len(f['vars']) == 1}
            if set(self.spec['var_ids']) - with_unary:
                out.add('a variable without unary factor')
            # a sweep's variable updates all become fused headers unless dropped as dead
            all_ops, sw, fs, fops = np.asarray(self.shape['ops']).reshape(-1, 4), np.asarray(self.shape['sweeps']).reshape(-1, 2), self.fused['fsweeps'].reshape(-1, 2), self.fused['fops']
            for k in range(len(sw) - 1):
                n_var = int((all_ops[sw[k][0]:sw[k][0] + sw[k][1], 0] == I.OP_VAR).sum())
                kinds = fops[fs[k][0]:fs[k][0] + fs[k][1], 0] & 0xFF
                n_kept = int(np.isin(kinds, (I.FOP_VAR, I.FOP_VAR_PAIR_TM, I.FOP_VAR_PAIR_MT)).sum())
                if n_kept < n_var and self.roots[k] != self.roots[k + 1]:
                    out.add('a dead update dropped (differing roots)')
                if n_kept == n_var and self.roots[k] == self.roots[k + 1] and len(kinds) and kinds[-1] == I.FOP_VAR:
                    out.add('a lone update kept (equal roots)')
        return out


def _shape_of(spec, roots):
    topo = GraphTopology.from_spec(spec)
    ops, srcs, sweeps = topo.compile_program(roots)
    return dict(ops=ops, srcs=srcs, sweeps=sweeps, n_msgs=topo.n_msgs, P=topo.P, U=topo.U, n_vars=topo.n_vars, in_off=topo.in_off,
                in_slots=topo.in_slots)


@functools.lru_cache(maxsize=None)
def family():
    """The random cases, in seed order."""
    out = []
    for seed in range(FAMILY_SIZE):
        spec, roots = I.random_case(seed, X)
        out.append(Case(spec['name'], _shape_of(spec, roots), spec, roots, seed))
    return out


@functools.lru_cache(maxsize=None)
def fixture_shapes():
    """The 55 shapes of the word-for-word fixture: the graphs among them rebuilt at X = 5, the hand-made op lists as they are."""
    seen, graph = [], M._graph
    M._graph = lambda spec, roots: seen.append((spec, roots)) or graph(spec, roots)
    try:
        shapes = M.shapes()
    finally:
        M._graph = graph
    hand = M.refusals()
    assert len(shapes) == 55 and len(seen) == 55 - len(hand)
    graphs = iter(seen)
    out = []
    for k, (name, s) in enumerate(shapes.items()):
        if name in hand:
            out.append(Case(name, s, seed=500 + k))
            continue
        spec, roots = next(graphs)
        spec5 = I.explicit(spec, X)
        shape = _shape_of(spec5, roots)
        for key in ('ops', 'srcs', 'sweeps', 'in_off'):
            assert np.array_equal(np.asarray(shape[key]).reshape(-1), np.asarray(s[key]).reshape(-1)), (name, key)   # the same program
        out.append(Case(name, shape, spec5, list(roots), 500 + k))
    return out


def every_case():
    return family() + fixture_shapes()


def _close(got, want, what):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)
    return float(np.max(np.abs(got - want) / np.abs(want)))


def _sweep_all(run):
    """run(case, start, init) -> (messages or None, marginals or None) over every case and both starts; the worst distance."""
    worst, n = 0.0, 0
    for c in every_case():
        for what, start, init, (want_m, want_p) in c.starts():
            msgs, marg = run(c, start, init)
            if msgs is not None:
                worst = max(worst, _close(msgs, want_m, '%s, %s: messages' % (c.name, what)))
                n += 1
            if marg is not None:
                worst = max(worst, _close(marg, want_p, '%s, %s: marginals' % (c.name, what)))
    print('%d runs, worst relative distance %.3g' % (n, worst))
    assert n > 0
    return worst


def test_the_family_is_large_enough_and_reproducible():
    assert len(family()) >= 200 and len(fixture_shapes()) == 55
    a, b = I.random_case(17, X), I.random_case(17, X)
    assert a == b
    sizes = [len(c.spec['var_ids']) for c in family()]
    assert min(sizes) == 2 and max(sizes) == 9
    assert all(1 <= len(c.roots) <= 6 for c in family())
    assert any(len(set(c.roots)) < len(c.roots) for c in family())
    unary_per_var = [sum(1 for f in c.spec['factors'] if f['vars'] == [v]) for c in family() for v in c.spec['var_ids']]
    assert max(unary_per_var) >= 2 and min(unary_per_var) == 0
    degree = [sum(1 for f in c.spec['factors'] if len(f['vars']) == 2 and v in f['vars']) for c in family() for v in c.spec['var_ids']]
    assert {5, 6, 7, 8} <= set(degree), sorted(set(degree))


def test_plain_op_list_equals_the_oracle():
    """The interpreters' ground: the op list they all start from, run plainly, is the oracle's walk (hand-made lists: itself)."""
    def run(c, start, init):
        m = I.run_ops(c.shape['ops'], c.srcs, c.shape['sweeps'], c.n_msgs, c.pair, c.unary, start, init)
        return m, I.marginals_of(m, c.in_off, c.in_slots)
    _sweep_all(run)


def test_pruned_list_equals_the_oracle():
    """drop_unchanged_updates: the op list of MLBP_SWEEP_SKIP_UNCHANGED gives what the unpruned one gives."""
    def run(c, start, init):
        m = I.run_pruned(c.images['pruned'], c.srcs, c.n_msgs, c.pair, c.unary, start, init)
        return m, I.marginals_of(m, c.in_off, c.in_slots)
    _sweep_all(run)


def test_pruned_list_is_a_subsequence_with_the_count_it_reports():
    for c in every_case():
        ops2, sweeps2, dropped = I.parse_pruned(c.images['pruned'])
        ops, sweeps = np.asarray(c.shape['ops']).reshape(-1, 4), np.asarray(c.shape['sweeps']).reshape(-1, 2)
        assert len(sweeps2) == len(sweeps), c.name
        total = 0
        for (f, n), (f2, n2) in zip(sweeps, sweeps2):
            rest = iter(ops[f:f + n].tolist())
            assert all(any(o == r for r in rest) for o in ops2[f2:f2 + n2].tolist()), c.name       # in order, nothing invented
            total += n - n2
        assert total == dropped, c.name


@pytest.mark.parametrize('exact_lists', [False, True], ids=['fast_lists', 'exact_lists'])
def test_fused_image_equals_the_oracle(exact_lists):
    """build_fused_program: sinking, hoisting, constant products, fusion, dead updates, bundles, pairseq, written."""
    def run(c, start, init):
        m = I.run_fused(c.images['fused'], c.n_msgs, c.pair, c.unary, start, init, exact_lists=exact_lists)
        return m, I.marginals_of(m, c.in_off, c.in_slots)
    _sweep_all(run)


def _lean_refusal(c):
    """Why the lean kernel does not take the case, checked against the images; None when it does."""
    if not c.lean['ok']:
        cpw, at, longest = c.fused['cpw'], 0, 0
        while at < len(cpw):
            longest = max(longest, int(cpw[at]))
            at += 1 + int(cpw[at])
        assert c.fused['has_unary_fops'] or longest > 15, c.name
        assert len(c.lean['image']) == 0 and c.readout_ok == 0, c.name
        return 'compiler'
    if c.P > 8:
        return 'more than 8 pairwise factors'
    return None


def test_lean_image_equals_the_oracle():
    """build_lean_program and build_lean_readout: micro-ops, carry links, stored variable->factor messages, the per-wave lists,
    the ext slots, the written-slot rule, the read-out lists."""
    refused = {}

    def run(c, start, init):
        why = _lean_refusal(c)
        if why:
            refused[c.name] = why
            return None, None
        if not c.readout_ok:                              # more than 15 entries: messages only
            n_vary = [sum(1 for q in range(c.in_off[v], c.in_off[v + 1]) if not c.lean['hoisted'][c.in_slots[q]]) for v in range(len(c.in_off) - 1)]
            assert max(n_vary) > 14, c.name
            refused[c.name] = 'read-out'
            return I.run_lean(c.images['lean'], None, c.n_msgs, c.pair, c.unary, start, init)[0], None
        return I.run_lean(c.images['lean'], c.images['lean_readout'], c.n_msgs, c.pair, c.unary, start, init)
    _sweep_all(run)
    print('refused: %s' % sorted(refused.items()))
    hand = set(M.refusals())
    assert {n for n, w in refused.items() if w == 'compiler'} == {'refuse_cprod_16_messages', 'refuse_unary_two_tables_one_slot'}
    assert all(n not in hand for n, w in refused.items() if w != 'compiler')
    assert sum(1 for c in every_case() if c.name not in refused) >= 200


def test_lean_program_of_a_long_hand_made_product_has_three_links():
    """Nine sources (eight messages and the uniform base) are a chain of three links: the one carry length no graph that the
    lean kernel takes reaches."""
    c = [c for c in fixture_shapes() if c.name == 'refuse_var_9_tiles'][0]
    assert 'CARRY x3' in I.lean_forms(c.lean['bundles'])
    for what, start, init, (want_m, want_p) in c.starts():
        msgs, marg = I.run_lean(c.images['lean'], c.images['lean_readout'], c.n_msgs, c.pair, c.unary, start, init)
        _close(msgs, want_m, what)
        _close(marg, want_p, what)


def _counts(cases):
    counts = {}
    for c in cases:
        for f in c.forms():
            counts[f] = counts.get(f, 0) + 1
    return counts


def test_the_family_holds_every_form():
    counts = _counts(every_case())
    for f in sorted(counts):
        print('%-45s %d' % (f, counts[f]))
    missing = [f for f in REQUIRED if not counts.get(f)]
    assert not missing, missing
    fam = _counts(family())
    assert not [f for f in GPU_REQUIRED if not fam.get(f)], 'the random cases alone hold every form a graph can reach'


@functools.lru_cache(maxsize=None)
def gpu_subset():
    """Seeds of the family cases that tests/test_gpu_random_programs.py runs: a greedy cover of GPU_REQUIRED in which every form
    occurs TWICE (once where the family holds it once) -- the case that adds the most missing occurrences first, the lower seed
    on a tie.  Called when the GPU module is imported: it asserts nothing."""
    forms = [c.forms() & set(GPU_REQUIRED) for c in family()]
    have = _counts(family())
    need = {f: min(2, have.get(f, 0)) for f in GPU_REQUIRED}       # (a form the family has lost fails the tests below, not the import)
    chosen = []
    while any(need.values()):
        gain = [0 if k in chosen else sum(1 for f in fs if need[f]) for k, fs in enumerate(forms)]
        k = int(np.argmax(gain))
        assert gain[k] > 0, need
        chosen.append(k)
        for f in forms[k]:
            need[f] = max(0, need[f] - 1)
    return tuple(sorted(chosen))


def p3_seeds():
    """Seeds of the first three family cases with three pairwise factors: the ones the GPU module specialises."""
    return tuple(k for k, c in enumerate(family()) if c.P == 3)[:3]


def test_the_cases_to_specialise_have_three_tables_and_no_carry_links():
    seeds = p3_seeds()
    assert len(seeds) == 3
    for k in seeds:
        c = family()[k]
        forms = I.lean_forms(c.lean['bundles'])
        assert c.lean['ok'] and c.P == 3 and c.readout_ok and not [f for f in forms if f.startswith('CARRY')], (k, sorted(forms))
        print('family_%d: %d variables, %d unary factors, roots %s, %s' % (k, len(c.spec['var_ids']), c.U, c.roots, sorted(forms)))


def test_the_gpu_subset_is_small_and_still_holds_every_form():
    seeds = gpu_subset()
    print('GPU subset: seeds %s' % (seeds,))
    assert len(seeds) <= 40
    counts = _counts([family()[k] for k in seeds])
    assert not [f for f in GPU_REQUIRED if not counts.get(f)]
    assert sum(1 for k in seeds if 1 <= family()[k].P <= 4) >= 3          # the padded X = 20 instances have something to run
