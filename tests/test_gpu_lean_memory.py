"""The memory side of the lean X = 64 kernel (csrc/mlbp_lean.hip): how a graph's unary rows come in (dense or through
unary_tab, up to eight rows per wave in registers and further rounds beyond), which message slots go back to memory and when
(the hoisted unary messages, the slots the sweeps wrote, the slots the program never touches, nothing at all when the
write-back is waived or the graph is skipped), and the three workgroup verdicts (bad index, prologue, final pass) that decide it.
None of this may show in a result, so every case compares

- messages and marginals with the float64 oracle (oracle/lbp_oracle.py) at 1e-10, and
- messages with the per-graph kernels on the same inputs (mlbp_set_sweep_variant(3)) at 1e-11,

and asserts that the lean kernel ran (mlbp_last_sweep_kernel() == 7).  Shapes: |X| = 64 (one case 33), 5 to 67 graphs.
The cases were written for 16-byte unary loads and an early write-back of the unary messages (LAB_NOTES R6.1: measured,
slower, not kept); they hold for the kernel as it is and for any later attempt at either.
"""
import numpy as np
import pytest

import cases as C
import test_gpu_instances as TI            # its workload batches (_Group) carry their own oracle inputs
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

RTOL = 1e-10
RTOL_EXACT = 1e-11
LEAN = 7


def _explicit(spec):
    """spec with one table per factor (table key = factor id): every graph of a batch brings its own tables."""
    return dict(name=spec['name'] + '_ex', style='explicit', X=spec['X'], var_ids=list(spec['var_ids']), labels=list(spec['labels']),
                factors=[dict(id=f['id'], vars=list(f['vars']), dims=list(f['dims']), table=f['id']) for f in spec['factors']])


def _many_unary(X, counts):
    """A chain over len(counts) variables, variable v carrying counts[v] unary factors."""
    n = len(counts)
    factors = []
    for v in range(n):
        for _ in range(counts[v]):
            factors.append(dict(id=len(factors), vars=[v], dims=[0], table=len(factors)))
    for v in range(n - 1):
        factors.append(dict(id=len(factors), vars=[v, v + 1], dims=[0, 1] if v % 2 else [1, 0], table=len(factors)))
    return dict(name='chain%d_u%d' % (n, sum(counts)), style='explicit', X=X, var_ids=list(range(n)), labels=[0] * n, factors=factors)


def _two_components(X):
    """chain5 without its (2, 3) factor: sweeps rooted in {0, 1, 2} never touch the messages of {3, 4}."""
    s = C.chain_spec(5, X, 'chain3_plus_chain2_x%d' % X)
    s['factors'] = [f for f in s['factors'] if f['vars'] != [2, 3]]
    return s


class _Batch:
    """B graphs of one explicit-style spec, each with its own random tables (unary rows optionally drawn from a shared pool
    through unary_tab), on the device, and the oracle's view of each graph."""

    def __init__(self, spec, roots, B, seed, unary_pool=None):
        from macaronicusermodeling_amd.batch import FactorGraphBatch
        from macaronicusermodeling_amd.topology import GraphTopology
        self.spec, self.roots, self.B, self.X = spec, list(roots), B, spec['X']
        X = self.X
        self.topo = topo = GraphTopology.from_spec(spec)
        self.g = O.Graph(spec)
        rs = np.random.RandomState(seed)
        self.pair = rs.rand(B, topo.P, X, X) + 0.01
        self.fb = fb = FactorGraphBatch(topo, X, B)
        fb.set_pair_tables(self.pair.reshape(B * topo.P, X, X))
        if unary_pool:
            pool = rs.rand(unary_pool, X) + 0.01
            tab = rs.randint(0, unary_pool, size=(B, topo.U))
            self.unary = pool[tab]
            fb.set_unary_tables(pool, tab)
        else:
            self.unary = rs.rand(B, topo.U, X) + 0.01
            fb.set_unary_tables(self.unary.reshape(B * topo.U, X))
        self.keys = C.msg_keys(spec)

    def upload(self):
        """(after editing self.pair / self.unary in place: dense layouts only)"""
        self.fb.set_pair_tables(self.pair.reshape(self.B * self.topo.P, self.X, self.X))
        self.fb.set_unary_tables(self.unary.reshape(self.B * self.topo.U, self.X))

    def oracle(self, b, start=None):
        """(messages [n_msgs][X], marginals [n_vars][X]) of graph b after the sweeps, from uniform messages or from start[b]."""
        by_id = {f['id']: f for f in self.spec['factors']}
        tables = [None] * (1 + max(f['table'] for f in self.spec['factors']))
        for p, j in enumerate(self.topo.pair_factors):
            tables[by_id[self.topo.factor_ids[j]]['table']] = self.pair[b, p]
        for u, j in enumerate(self.topo.unary_factors):
            tables[by_id[self.topo.factor_ids[j]]['table']] = self.unary[b, u].reshape(self.X, 1)
        msgs = O.init_messages(self.g)
        if start is not None:
            for i, k in enumerate(self.keys):
                msgs[k] = start[b, i].copy()
        with np.errstate(all='ignore'):
            for r in self.roots:
                O.sweep(self.g, dict(tables=tables), msgs, r)
            marg = np.stack([O.marginal(self.g, msgs, v).reshape(-1) for v in self.topo.var_ids])
        return np.stack([msgs[k].reshape(-1) for k in self.keys]), marg

    def start(self, seed):
        """Random positive messages to start from (init=False), as a host array."""
        return np.random.RandomState(seed).rand(self.B, self.topo.n_msgs, self.X) + 0.05

    def run(self, init, start=None, keep=True, variant=1):
        """One call; returns (program, messages, marginals) as host arrays."""
        fb = self.fb
        if start is None:
            fb.msgs.fill_(float('nan'))
        else:
            fb.msgs.copy_(torch.from_numpy(start))
        marg = torch.full((self.B, self.topo.n_vars, self.X), float('nan'), dtype=torch.float64, device=fb.device)
        prog = TI._with_variant(variant, lambda: fb.sweep(self.roots, init=init, marginals=marg, keep_messages=keep))
        torch.cuda.synchronize()
        return prog, fb.msgs.cpu().numpy(), marg.cpu().numpy()

    def check(self, init, start=None, exact=0, status=0, skipped=()):
        """The default path against the oracle and against the per-graph kernels; returns the default path's messages."""
        from macaronicusermodeling_amd import _ffi
        assert (start is None) == bool(init)
        prog, msgs, marg = self.run(init, start)
        assert _ffi.lib.mlbp_last_sweep_kernel() == LEAN
        assert prog.status() == status and prog.status() == 0
        count = prog.exact_count(self.B)
        print('%s init=%s: exact_count %d (expected %d)' % (self.spec['name'], init, count, exact))
        good = [b for b in range(self.B) if b not in skipped]
        worst = 0.0
        for b in good:
            want, wmarg = self.oracle(b, start)
            worst = max(worst, float(np.max(np.abs(msgs[b] - want) / np.maximum(np.abs(want), 1e-300))))
            np.testing.assert_allclose(msgs[b], want, rtol=RTOL, atol=1e-300, err_msg='messages of graph %d' % b)
            np.testing.assert_allclose(marg[b], wmarg, rtol=RTOL, atol=1e-300, err_msg='marginals of graph %d' % b)
        print('   largest relative message error against the oracle: %.3g' % worst)
        prog3, msgs3, _ = self.run(init, start, variant=3)
        assert prog3.status() == status
        np.testing.assert_allclose(msgs[good], msgs3[good], rtol=RTOL_EXACT, atol=1e-300)
        assert count == exact
        return msgs


def _user_k3(B, seed, **kw):
    return _Batch(_explicit(C.user_spec(10, [1, 4, 7], 64, 40, seed=1)), [4, 1, 7, 4], B, seed, **kw)


@pytest.mark.parametrize('init', [True, False])
def test_user_k3_dense_unique_tables(init):
    bt = _user_k3(13, 11)
    assert bt.topo.U == 24 and bt.topo.P == 3
    bt.check(init, None if init else bt.start(12))


@pytest.mark.parametrize('init', [True, False])
def test_slots_the_program_does_not_touch_keep_their_bytes(init):
    """Sweeps rooted in one component of a graph leave the other component's messages alone: uniform after an initialising
    call, the caller's bytes otherwise."""
    bt = _Batch(_two_components(64), [0, 2, 1], 9, 21)
    start = None if init else bt.start(22)
    msgs = bt.check(init, start)
    idle = [i for i, k in enumerate(bt.keys) if k[0] in ('X_3', 'X_4') or k[1] in ('X_3', 'X_4')]
    assert len(idle) == 6
    want = np.full_like(msgs[:, idle], 1.0 / 64) if init else start[:, idle]
    assert np.array_equal(msgs[:, idle], want)


@pytest.mark.parametrize('init', [True, False])
def test_indexed_unary_rows_from_a_shared_pool(init):
    bt = _user_k3(17, 31, unary_pool=192)
    assert not bt.fb._unary_dense
    bt.check(init, None if init else bt.start(32))


@pytest.mark.parametrize('pool', [None, 192])
def test_more_unary_rows_than_a_wave_holds_in_registers(pool):
    """38 unary factors: waves 0 and 1 take ten rows (a second round of two), waves 2 and 3 nine (a second round of one: the
    upper half-wave idle)."""
    bt = _Batch(_many_unary(64, [13, 13, 12]), [0, 2, 1, 0], 7, 41, unary_pool=pool)
    assert bt.topo.U == 38
    bt.check(True)
    bt.check(False, bt.start(42))


def test_three_unary_rows_leave_half_waves_idle():
    """ring3: one row in each of three waves, none in the fourth."""
    bt = _Batch(C.ring_spec(3, 64), [0, 2, 1, 0], 5, 51)
    bt.check(True)
    bt.check(False, bt.start(52))


@pytest.mark.parametrize('init', [True, False])
def test_waived_write_back_leaves_the_buffer_alone(init):
    from macaronicusermodeling_amd import _ffi
    bt = _user_k3(9, 61)
    before = bt.start(62)
    prog, msgs, marg = bt.run(init, before, keep=False)
    assert _ffi.lib.mlbp_last_sweep_kernel() == LEAN and prog.status() == 0 and prog.exact_count(bt.B) == 0
    assert np.array_equal(msgs, before)
    for b in range(bt.B):
        _, wmarg = bt.oracle(b, None if init else before)
        np.testing.assert_allclose(marg[b], wmarg, rtol=RTOL, atol=1e-300)


@pytest.mark.parametrize('init', [True, False])
def test_an_all_zero_pairwise_table_is_redone_by_the_exact_kernel(init):
    """One degenerate graph in a batch of 67, flagged in the main loop or the final pass (zero total -> uniform rule, which the
    scale-free representation hands to the exact kernel) -- after its unary messages have been stored."""
    bt = _user_k3(67, 71)
    bt.pair[41, 1] = 0.0
    bt.upload()
    bt.check(init, None if init else bt.start(72), exact=1)


@pytest.mark.parametrize('init', [True, False])
def test_an_all_zero_unary_row_is_redone_by_the_exact_kernel(init):
    """One graph with an all-zero unary row in a batch of 67: the zero total -> uniform rule (Message.renormalize,
    LBP.py:655-657) acts in the prologue, which flags the graph (bail code 1, nothing of it stored) as the main loop flags a
    zero-total update; the exact kernel redoes it."""
    bt = _user_k3(67, 73)
    bt.unary[41, 5] = 0.0
    bt.upload()
    bt.check(init, None if init else bt.start(74), exact=1)


@pytest.mark.parametrize('init', [True, False])
def test_a_negative_unary_entry_is_flagged_in_the_prologue(init):
    """A unary row the scale-free representation cannot carry (a negative entry): bail code 1, before anything of the graph is
    stored; the exact kernel redoes it."""
    bt = _user_k3(67, 75)
    bt.unary[23, 7, 9] = -0.25
    bt.upload()
    bt.check(init, None if init else bt.start(76), exact=1)


@pytest.mark.parametrize('init', [True, False])
@pytest.mark.parametrize('what', ['unary', 'pair'])
def test_an_out_of_range_index_skips_its_graph_only(what, init):
    bt = _user_k3(11, 81, unary_pool=192)
    b = 6
    if what == 'unary':
        bt.fb.unary_tab[b, 20] = 10 ** 6
    else:
        bt.fb.pair_tab[b, 2] = 10 ** 6
        bt.fb._pair_dense = False
    start = bt.start(82)
    msgs = bt.check(init, None if init else start, status=1, skipped=(b,))
    assert np.array_equal(msgs[b], np.full_like(msgs[b], 1.0 / 64) if init else start[b])


def test_grouped_call():
    """Two shapes in one launch (the MULTI instances read the write-back lists from the group table)."""
    from macaronicusermodeling_amd import _ffi
    from macaronicusermodeling_amd import batch as batch_mod
    groups = [TI._Group(dict(spec='chain2', X=64, B=5, layout='unique', kind='sweep'), 91),
              TI._Group(dict(spec='user_k3', X=64, B=7, layout='unique', kind='sweep'), 92)]
    progs = batch_mod.sweep_groups([g.fb for g in groups], [g.roots for g in groups], init=True, marginals=[g.marg for g in groups])
    torch.cuda.synchronize()
    assert _ffi.lib.mlbp_last_sweep_kernel() == LEAN and all(p.status() == 0 for p in progs)
    for g in groups:
        g.check()


def test_fused_gradient_call():
    from macaronicusermodeling_amd import _ffi
    gr = TI._Group(dict(spec='user_k3', X=64, B=9, layout='unique', kind='sweep', grad=True), 93)
    prog = gr.fb.sweep(gr.roots, **gr.sweep_kwargs())
    torch.cuda.synchronize()
    assert _ffi.lib.mlbp_last_sweep_kernel() == LEAN and prog.status() == 0 and prog.exact_count(gr.B) == 0
    gr.check()


def test_seven_table_chain():
    """chain8: six tables in registers, the seventh in LDS."""
    bt = _Batch(C.chain_spec(8, 64), [0, 7, 3, 0], 5, 94)
    assert bt.topo.P == 7
    bt.check(True)
    bt.check(False, bt.start(95))


def test_padded_state_space():
    """X = 33: rows are not 16-byte aligned; the instance keeps its 8-byte loads and its own write-back."""
    bt = _Batch(C.chain_spec(3, 33), [0, 2, 1, 0], 9, 96)
    bt.check(True)
    bt.check(False, bt.start(97))
