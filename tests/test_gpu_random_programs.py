"""The compiled sweep programs of random graphs on the device: the cases of tests/test_image_semantics_cpu.py's family that its
gpu_subset() picks -- the smallest greedy cover of the forms a graph can reach (every pair of member kinds, lone variable
updates, a stored three-source product, carry chains, both parities of n_bundles, both endings, no constant product, dropped and
kept dead updates, every P from 1 to 8, pruned lists that drop nothing / a whole sweep, and a shape the lean kernel refuses) --
run through FactorGraphBatch against the oracle.  This module draws nothing itself.

Per case, X = 64 with B = 5 graphs of per-graph tables (is_loopy = True: a tree runs every sweep too): a single call, the same
with skip_unchanged, two groups of one sweep_groups launch (the second with the roots reversed and lognormal tables), a call
with keep_messages=False and marginals, and a call continuing from the first call's messages.  Messages and marginals equal the
oracle's at rtol 1e-10; the lean kernel ran (mlbp_last_sweep_kernel() == 7), flagged nothing (status() == 0, exact_count(B) ==
0: the tables are benign) and the launch log shows the sweep_x64_lean_kernel instance pick_lean chooses for the case's P, single
and grouped.  More than eight pairwise factors: the exact kernel with streamed tables ran instead, to the same parity.  The
cases with at most four pairwise factors also run at X = 20, on the padded lean instances.

Three cases with three pairwise factors (no carry links) are specialised: the static kernel against the interpreting instance
bit for bit (as tests/test_gpu_lean_static.py compares its hand-made programs), a specialised call captured into a
torch.cuda.graph and replayed with the tables changed in between, and the gradient, grouped and skip_unchanged calls of a
specialised program, which launch the compiled-in instances and give a never-specialised program's bytes.
"""
import functools

import numpy as np
import pytest

import cases as C
import image_interp as I
import test_image_semantics_cpu as S
from helpers import batch_tables
from macaronicusermodeling_amd import _ffi
from macaronicusermodeling_amd.topology import GraphTopology
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

LEAN, EXACT = 7, 2                 # MLBP_KERNEL_LEAN, MLBP_KERNEL_EXACT
B = 5
RTOL, ATOL = 1e-10, 1e-300
NAME = 'sweep_x64_lean_kernel'
STREAMED_EXACT = ('sweep_x64_fused_kernel', (True, 0, False))


def lean_instance(P, padx=False, multi=False, grad=False):
    """The instance <NT, PADX, MULTI, NL, GRAD> that pick_lean / pick_lean_grad (csrc/mlbp_lean.hip) choose."""
    if padx:
        return NAME, (min(P, 4), True, False, 0, False)
    return NAME, ({5: 6, 7: 6}.get(P, P), False, multi, 1 if P == 7 else 0, grad)


class Batch:
    """B graphs of family case `seed` at X states with tables of `kind`, on the device; the oracle's view of each."""

    def __init__(self, seed, X, kind='uniform', reverse=False):
        from macaronicusermodeling_amd.batch import FactorGraphBatch
        self.spec, roots = I.random_case(seed, X)
        self.roots = list(roots)[::-1] if reverse else list(roots)
        self.seed, self.X, self.kind = seed, X, kind
        self.topo = topo = GraphTopology.from_spec(self.spec)
        self.inputs = [C.make_inputs(self.spec, 6000 + seed + 1000 * i, kind) for i in range(B)]
        self.pair, self.unary = batch_tables(self.spec, topo, self.inputs)
        self.fb = fb = FactorGraphBatch(topo, X, B)
        fb.set_pair_tables(self.pair)
        if topo.U:
            fb.set_unary_tables(self.unary)
        fb.is_loopy = True
        self.marg = torch.full((B, topo.n_vars, X), float('nan'), dtype=torch.float64, device=fb.device)

    def oracle(self):
        """[(messages [B][n_msgs][X], marginals [B][n_vars][X])] after one call from uniform messages and after a second one."""
        return _oracle(self.seed, self.X, self.kind, tuple(self.roots))


@functools.lru_cache(maxsize=None)
def _oracle(seed, X, kind, roots):
    spec, _ = I.random_case(seed, X)
    topo, g = GraphTopology.from_spec(spec), O.Graph(spec)
    keys = topo.slot_keys()
    out = [[], []]
    for i in range(B):
        inputs = C.make_inputs(spec, 6000 + seed + 1000 * i, kind)
        msgs = O.init_messages(g)
        for call in range(2):
            for r in roots:
                O.sweep(g, inputs, msgs, r)
            out[call].append((np.stack([msgs[k] for k in keys]), np.stack([O.marginal(g, msgs, v).reshape(-1) for v in topo.var_ids])))
    return [(np.stack([m for m, _ in res]), np.stack([p for _, p in res])) for res in out]


_worst = {'distance': 0.0}


def _close(got, want, what):
    got = got.cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)
    _worst['distance'] = max(_worst['distance'], float(np.max(np.abs(got - want) / np.abs(want))))


def _log():
    import kernel_inventory as K
    handles = K.launched_handles()
    known = set(K._tables()['all_by_addr'])
    return K.launched(), [h for h in handles if h not in known]


def _verdict(bt, progs, expect_lean, what):
    """After a call on bt's shape: which kernel ran, that it flagged nothing, and what the launch log holds."""
    torch.cuda.synchronize()
    launched, foreign = _log()
    lean = [k for k in launched if k[0] == NAME]
    kernel = _ffi.lib.mlbp_last_sweep_kernel()
    assert all(p.status() == 0 for p in progs), what
    assert foreign == [], what
    if expect_lean is None:                           # more than eight pairwise factors at X = 64: the exact kernel, tables streamed
        assert bt.topo.P > 8 and kernel == EXACT and lean == [] and STREAMED_EXACT in launched, (what, kernel, launched)
        return
    assert kernel == LEAN and lean == expect_lean, (what, kernel, lean)
    assert all(p.exact_count(B) == 0 for p in progs), what     # benign tables: a flagged graph is a finding


def _run_modes(seed, X):
    import kernel_inventory as K
    from macaronicusermodeling_amd.batch import sweep_groups
    bt = Batch(seed, X)
    fb, roots, P = bt.fb, bt.roots, bt.topo.P
    padx = X < 64
    takes = 1 <= P <= (4 if padx else 8)
    assert takes or not padx, 'the X = 20 cases are the padded lean instances'
    single = [lean_instance(P, padx)] if takes else None
    (want_m, want_p), (next_m, next_p) = bt.oracle()
    what = 'family_%d at X = %d (P = %d, roots %s)' % (seed, X, P, roots)

    def call(mode, **kw):
        if kw.get('init'):
            fb.msgs.fill_(float('nan'))
        bt.marg.fill_(float('nan'))
        K.reset()
        prog = fb.sweep(roots, marginals=bt.marg, **kw)
        _verdict(bt, [prog], single, '%s, %s' % (what, mode))

    call('single', init=True)
    _close(fb.msgs, want_m, what + ', single: messages')
    _close(bt.marg, want_p, what + ', single: marginals')
    first = fb.msgs.clone()

    call('skip_unchanged', init=True, skip_unchanged=True)
    _close(fb.msgs, want_m, what + ', skip_unchanged: messages')
    _close(bt.marg, want_p, what + ', skip_unchanged: marginals')

    call('keep_messages=False', init=True, keep_messages=False)
    _close(bt.marg, want_p, what + ', keep_messages=False: marginals')

    fb.msgs.copy_(first)
    call('continuing', init=False)
    _close(fb.msgs, next_m, what + ', continuing: messages')
    _close(bt.marg, next_p, what + ', continuing: marginals')

    other = Batch(seed, X, kind='lognormal', reverse=True)
    for b in (bt, other):
        b.fb.msgs.fill_(float('nan'))
        b.marg.fill_(float('nan'))
    K.reset()
    progs = sweep_groups([fb, other.fb], [roots, other.roots], init=True, marginals=[bt.marg, other.marg])
    # one launch of the grouped instance at X = 64; below, a grouped call runs its groups one after the other
    grouped = None if not takes else ([lean_instance(P, multi=True)] if not padx else single * 2)
    _verdict(bt, progs, grouped, what + ', grouped')
    for b in (bt, other):
        m, p = b.oracle()[0]
        _close(b.fb.msgs, m, '%s, grouped (%s tables): messages' % (what, b.kind))
        _close(b.marg, p, '%s, grouped (%s tables): marginals' % (what, b.kind))
    print('%s: worst relative distance so far %.3g' % (what, _worst['distance']))


@pytest.mark.parametrize('seed', S.gpu_subset())
def test_random_program_at_x64_against_the_oracle(seed):
    _run_modes(seed, 64)


@pytest.mark.parametrize('seed', [k for k in S.gpu_subset() if 1 <= S.family()[k].P <= 4][:4])
def test_random_program_at_x20_on_the_padded_instances(seed):
    _run_modes(seed, 20)


# ---------------------------------------------------------------------------------------------------------------------------
# three pairwise factors: the static kernel
# ---------------------------------------------------------------------------------------------------------------------------
P3 = S.p3_seeds()
INTERPRETER = lean_instance(3)


@functools.lru_cache(maxsize=None)
def _pair(seed):
    """(interpreted, static): two batches of the same inputs, the second one's program specialised."""
    plain, forced = Batch(seed, 64), Batch(seed, 64)
    assert plain.topo.P == 3 and np.array_equal(plain.pair, forced.pair) and np.array_equal(plain.unary, forced.unary)
    prog = forced.fb.program(forced.roots)
    before = _ffi.lib.mlbp_lean_compile_count()
    prog.specialize()
    assert prog.specialized() == 1 and _ffi.lib.mlbp_lean_compile_count() > before
    print('family_%d: %s' % (seed, _ffi.lib.mlbp_last_error().decode()))
    return plain, forced


def _call(bt, init, start, keep, **kw):
    """One sweep call -> what it leaves, as bytes-comparable host arrays and integers."""
    import kernel_inventory as K
    fb = bt.fb
    if start is None:
        fb.msgs.fill_(float('nan'))
    else:
        fb.msgs.copy_(torch.from_numpy(start))
    bt.marg.fill_(float('nan'))
    K.reset()
    prog = fb.sweep(bt.roots, init=init, marginals=bt.marg, keep_messages=keep, **kw)
    torch.cuda.synchronize()
    launched, foreign = _log()
    out = dict(marg=bt.marg.cpu().numpy(), kernel=_ffi.lib.mlbp_last_sweep_kernel(), count=prog.exact_count(B), status=prog.status(),
               specialized=prog.specialized(), bail=prog.bail_codes(B), lean=[k for k in launched if k[0] == NAME], foreign=foreign)
    if keep:
        out['msgs'] = fb.msgs.cpu().numpy()
    return out


def _same_bytes(a, b, what):
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), '%s: %s differs' % (what, k)
    assert (a['kernel'], b['kernel']) == (LEAN, LEAN), what
    assert (a['count'], a['status']) == (b['count'], b['status']) == (0, 0), what


@pytest.mark.parametrize('seed', P3)
def test_static_kernel_equals_the_interpreter_bit_for_bit(seed):
    plain, forced = _pair(seed)
    first = None
    for init in (True, False):
        for keep in (True, False):
            start = None if init else first
            a, b = _call(plain, init, start, keep), _call(forced, init, start, keep)
            what = 'family_%d init=%s keep=%s' % (seed, init, keep)
            _same_bytes(a, b, what)
            assert (a['specialized'], b['specialized']) == (0, 1), what
            # the compiled-in instance and nothing foreign | no lean instance and one handle from outside the library
            assert a['lean'] == [INTERPRETER] and a['foreign'] == [], (what, a['lean'], a['foreign'])
            assert b['lean'] == [] and len(b['foreign']) == 1, (what, b['lean'], b['foreign'])
            if init and keep:
                first = a['msgs']
                want_m, want_p = plain.oracle()[0]
                np.testing.assert_allclose(a['msgs'], want_m, rtol=RTOL, atol=ATOL)
                np.testing.assert_allclose(a['marg'], want_p, rtol=RTOL, atol=ATOL)
    assert first is not None and np.isfinite(first).all()


def test_a_specialised_call_replays_from_a_captured_graph():
    """The module-launched static kernel inside a torch.cuda.graph: captured after a warm-up call, replayed twice with the
    tables changed in between; each replay gives the bytes of the eager call on the same tables."""
    _, forced = _pair(P3[0])
    fb = forced.fb
    other = Batch(P3[0], 64, kind='lognormal')
    tables = {'first': (fb.pair_tables.clone(), fb.unary_tables.clone() if forced.topo.U else None),
              'second': (other.fb.pair_tables, other.fb.unary_tables if forced.topo.U else None)}

    def load(which):
        fb.pair_tables.copy_(tables[which][0])
        if forced.topo.U:
            fb.unary_tables.copy_(tables[which][1])

    eager = {}
    for which in ('second', 'first'):                 # (the last one doubles as the warm-up call on the tables of the capture)
        load(which)
        eager[which] = _call(forced, True, None, True)
        assert len(eager[which]['foreign']) == 1 and eager[which]['lean'] == [] and eager[which]['count'] == 0
    assert eager['first']['msgs'].tobytes() != eager['second']['msgs'].tobytes()
    import kernel_inventory as K
    K.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        prog = fb.sweep(forced.roots, init=True, marginals=forced.marg)
    assert prog.specialized() == 1 and len(_log()[1]) == 1            # the capture recorded the module's function
    for which in ('first', 'second', 'first'):
        load(which)
        fb.msgs.fill_(float('nan'))
        forced.marg.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert fb.msgs.cpu().numpy().tobytes() == eager[which]['msgs'].tobytes(), which
        assert forced.marg.cpu().numpy().tobytes() == eager[which]['marg'].tobytes(), which
        assert prog.status() == 0 and prog.exact_count(B) == 0
    load('first')


def _with_features(bt):
    """Random feature tensors, selectors, labels and observed columns: what a gradient call needs beside the tables."""
    rs = np.random.RandomState(31)
    fb, topo, Vde = bt.fb, bt.topo, 40
    kinds = rs.randint(0, 3, size=topo.U)
    fb.set_features(rs.rand(64, 64, 3), rs.rand(64, 64, 3), rs.rand(64, Vde, 6), rs.randint(0, 2, size=topo.P), kinds)
    obs = np.stack([rs.randint(0, Vde if k == 2 else 64, size=B) for k in kinds], axis=1) if topo.U else np.zeros((B, 0))
    fb.set_observations(rs.randint(0, 64, size=(B, topo.n_vars)), obs)
    return (torch.full((B, 3), float('nan'), dtype=torch.float64, device=fb.device),
            torch.full((B, 6), float('nan'), dtype=torch.float64, device=fb.device))


def test_other_calls_of_a_specialised_program_launch_the_compiled_in_instances():
    """A gradient call, a grouped call and a skip_unchanged call do not take the static kernel: the launch log shows the
    library's own instances, and the bytes are a never-specialised program's."""
    import kernel_inventory as K
    from macaronicusermodeling_amd.batch import sweep_groups
    plain, forced = _pair(P3[0])
    # gradient: fused into the launch of the GRAD instance
    got = []
    for bt in (plain, forced):
        grads = _with_features(bt)
        out = _call(bt, True, None, True, gradient=grads)
        assert _ffi.lib.mlbp_last_sweep_fused_gradient() == 1
        out['ee'], out['ed'] = grads[0].cpu().numpy(), grads[1].cpu().numpy()
        assert out['lean'] == [lean_instance(3, grad=True)] and out['foreign'] == [], (out['lean'], out['foreign'])
        assert np.isfinite(out['ee']).all() and np.isfinite(out['ed']).all()
        got.append(out)
    _same_bytes(got[0], got[1], 'gradient')
    # skip_unchanged: the pruned twin keeps the interpreting kernel
    got = [_call(bt, True, None, True, skip_unchanged=True) for bt in (plain, forced)]
    for out in got:
        assert out['lean'] == [INTERPRETER] and out['foreign'] == [], (out['lean'], out['foreign'])
    _same_bytes(got[0], got[1], 'skip_unchanged')
    # grouped: one launch of the MULTI instance
    got = []
    for bt in (plain, forced):
        other = Batch(bt.seed, 64, kind='lognormal', reverse=True)
        for b in (bt, other):
            b.fb.msgs.fill_(float('nan'))
            b.marg.fill_(float('nan'))
        K.reset()
        progs = sweep_groups([bt.fb, other.fb], [bt.roots, other.roots], init=True, marginals=[bt.marg, other.marg])
        torch.cuda.synchronize()
        launched, foreign = _log()
        assert [k for k in launched if k[0] == NAME] == [lean_instance(3, multi=True)] and foreign == [], (launched, foreign)
        assert _ffi.lib.mlbp_last_sweep_kernel() == LEAN and all(p.status() == 0 and p.exact_count(B) == 0 for p in progs)
        got.append([t.cpu().numpy() for t in (bt.fb.msgs, bt.marg, other.fb.msgs, other.marg)])
    assert forced.fb.program(forced.roots).specialized() == 1 and plain.fb.program(plain.roots).specialized() == 0
    for a, b in zip(*got):
        assert a.tobytes() == b.tobytes() and np.isfinite(a).all()
