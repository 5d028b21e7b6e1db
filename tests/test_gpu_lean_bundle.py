"""One bundle of the lean X = 64 kernel (csrc/mlbp_lean.hip): its two members' gathers run ahead of either contraction
(the three-table instances), both members' partial sums come back in one LDS round trip behind the barrier and their rescale
chains run side by side, and the message write-back reads several slots before it stores them.  None of it may change a bit
of a result, so for every program below -- chosen so that together they hold every form the loop distinguishes, which the CPU
test asserts on the decoded micro-op images -- every call

- compares messages and marginals with the per-graph exact kernel (mlbp_set_sweep_variant(3)) at 1e-11 and with the float64
  oracle (oracle/lbp_oracle.py) at the tolerance of tests/test_gpu_lean_memory.py (1e-10),
- asserts that the lean kernel ran (mlbp_last_sweep_kernel() == 7), status() == 0 and the expected exact_count,

from uniform messages and continuing from the first call's messages, with and without the message write-back.  One graph of
the K3 batch carries an all-zero unary row and one a negative table entry: those two, and only those, go to the exact kernel.

Shapes: |X| = 64 (one case 48), 5 to 13 graphs.
"""
import functools

import numpy as np
import pytest

import cases as C
from macaronicusermodeling_amd import _ffi
from macaronicusermodeling_amd.topology import GraphTopology

RTOL = 1e-10            # tests/test_gpu_lean_memory.py: against the oracle
RTOL_EXACT = 1e-11      # ... and against the per-graph kernels
LEAN = 7

UOP_VAR, UOP_MT, UOP_NOP, UOP_STORE_VF, UOP_NSRC_SHIFT, UOP_CARRY_IN, UOP_CARRY_OUT = 1, 2, 32, 64, 8, 0x1000, 0x2000    # csrc/mlbp_internal.h


def _user_spec(K, X=64):
    return C.user_spec(10, [1, 4, 7, 8][:K], X, 40, seed=1)


# name -> (spec, roots, graphs, seed, pairwise factors): P picks the kernel instance -- 3 the one with the paired gather, 7 the
# one with a table in LDS, 1 and 2 the four- and five-workgroup ones
PROGRAMS = {
    'user_k3': (lambda: _user_spec(3), [1, 4, 7], 13, 201, 3),
    'user_k3_x48': (lambda: _user_spec(3, 48), [1, 4, 7], 9, 203, 3),
    'chain4': (lambda: C.chain_spec(4, 64), [0, 3, 1], 7, 205, 3),
    'star3': (lambda: C.star_spec(3, 64), [0, 2, 1], 7, 207, 3),
    'user_k4': (lambda: _user_spec(4), [1, 7, 8], 7, 209, 6),
    'chain2': (lambda: C.chain_spec(2, 64), [0, 1, 0], 5, 211, 1),
    'chain3': (lambda: C.chain_spec(3, 64), [0, 2, 0], 5, 213, 2),
    'ring7': (lambda: C.ring_spec(7, 64), [0, 3], 5, 215, 7),
    'star6': (lambda: C.star_spec(6, 64), [0, 3, 0, 5], 5, 217, 6),
}
# the graphs of user_k3 that the scale-free representation cannot hold
ZERO_ROW, NEGATIVE = 8, 3
FLAGGED = {'user_k3': (NEGATIVE, ZERO_ROW)}


def _forms(spec, roots):
    """What the main loop will meet in the lean program of (spec, roots): a set of names, from the decoded micro-op image
    (MLBP_IMAGE_LEAN: ok, n_bundles, HL, n_cprod, WL, then the image as a vector -- its first n_bundles x 16 words the bundles)."""
    w = GraphTopology.from_spec(spec).images(roots)['lean']
    assert w[0] == 1, 'no lean program for this shape'
    n = int(w[1])
    out = set()
    for r in w[6:6 + 16 * n].reshape(n, 16):
        fa, fb = int(r[0]), int(r[8])
        if fa & UOP_VAR:
            assert fb & UOP_NOP
            out.add('VAR')
            out.update(name for bit, name in ((UOP_CARRY_IN, 'CARRY_IN'), (UOP_CARRY_OUT, 'CARRY_OUT')) if fa & bit)
            continue
        assert not fa & UOP_NOP and not fb & UOP_VAR
        d = lambda f: 'MT' if f & UOP_MT else 'TM'      # noqa: E731
        out.add('%s|%s' % (d(fa), 'NOP' if fb & UOP_NOP else d(fb)))
        if fb & UOP_NOP:
            assert r[14] == 0       # word 6 of an empty member: a store would hit message slot 0
        for f in (fa,) if fb & UOP_NOP else (fa, fb):
            if ((f >> UOP_NSRC_SHIFT) & 15) > 2 and f & UOP_STORE_VF:
                out.add('3SRC+VF')
    return out


def test_the_programs_hold_every_form_of_the_loop():
    forms = {name: _forms(p[0](), p[1]) for name, p in PROGRAMS.items()}
    for name, f in sorted(forms.items()):
        print(name, sorted(f))
    assert {'TM|TM', 'MT|MT', 'TM|MT', 'MT|TM', 'VAR'} <= forms['user_k3']          # the four pairings and the lone products
    assert '3SRC+VF' in forms['user_k4']                                            # three sources, the product stored
    # the same in the instance with the paired gather (P = 3): beside an empty member, and three sources with the store
    assert {'TM|NOP', 'MT|NOP'} <= forms['chain4'] and '3SRC+VF' in forms['star3']
    assert {'TM|NOP', 'MT|NOP'} <= forms['chain3']
    assert {'CARRY_IN', 'CARRY_OUT', 'MT|NOP'} <= forms['star6']
    assert {'TM|TM', 'MT|MT', 'VAR'} <= forms['ring7']
    assert {'TM|MT', 'MT|TM'} <= forms['chain2'] and {'TM|TM', 'MT|MT', 'VAR'} <= forms['user_k3_x48']
    for name, p in PROGRAMS.items():
        assert GraphTopology.from_spec(p[0]()).P == p[4], name


# ---------------------------------------------------------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch(name):
    import test_gpu_lean_memory as TM          # its _Batch: per-graph random tables on the device and the oracle's view of each graph
    make, roots, B, seed, P = PROGRAMS[name]
    spec = make()
    bt = TM._Batch(spec if spec.get('style') == 'explicit' else TM._explicit(spec), roots, B, seed)
    assert bt.topo.P == P
    if name == 'user_k3':
        bt.unary[ZERO_ROW, 5] = 0.0                 # an all-zero unary row: flagged in the prologue
        # a negative table entry, large enough to outweigh the 63 positive terms beside it (the oracle's final messages of this
        # graph hold negative entries): a negative update result, flagged by rescale in the main loop
        bt.pair[NEGATIVE, 1, 17, 40] = -1000.0
        bt.upload()
    return bt


def _call(bt, init, start, keep=True, variant=1, skip_unchanged=False):
    """One sweep call -> (program, messages, marginals, last kernel); messages = the buffer after the call (host arrays)."""
    import torch
    import test_gpu_instances as TI
    fb = bt.fb
    if start is None:
        fb.msgs.fill_(float('nan'))
    else:
        fb.msgs.copy_(torch.from_numpy(start))
    marg = torch.full((bt.B, bt.topo.n_vars, bt.X), float('nan'), dtype=torch.float64, device=fb.device)
    prog = TI._with_variant(variant, lambda: fb.sweep(bt.roots, init=init, marginals=marg, keep_messages=keep, skip_unchanged=skip_unchanged))
    torch.cuda.synchronize()
    return prog, fb.msgs.cpu().numpy(), marg.cpu().numpy(), _ffi.lib.mlbp_last_sweep_kernel()


@functools.lru_cache(maxsize=None)
def _first(name):
    """The messages an initialising call of the default path leaves: where the continuing calls start."""
    return _call(_batch(name), True, None)[1]


@functools.lru_cache(maxsize=None)
def _reference(name, init):
    """(start, oracle messages, oracle marginals, exact-kernel messages, exact-kernel marginals) of one program, computed once.
    init=False: the second call, on the first call's messages."""
    bt = _batch(name)
    start = None if init else _first(name)
    want = [bt.oracle(b, start) for b in range(bt.B)]
    prog, msgs3, marg3, _ = _call(bt, init, start, variant=3)
    assert prog.status() == 0
    return start, np.stack([w[0] for w in want]), np.stack([w[1] for w in want]), msgs3, marg3


@pytest.mark.gpu
@pytest.mark.parametrize('keep', [True, False], ids=['keep', 'waived'])
@pytest.mark.parametrize('init', [True, False], ids=['init', 'continue'])
@pytest.mark.parametrize('name', sorted(PROGRAMS))
def test_bundle_forms_against_the_exact_kernel_and_the_oracle(name, init, keep):
    bt = _batch(name)
    start, want, wmarg, msgs3, marg3 = _reference(name, init)
    prog, msgs, marg, kernel = _call(bt, init, start, keep=keep)
    count = prog.exact_count(bt.B)
    flagged = FLAGGED.get(name, ())
    print('%s init=%s keep=%s: kernel %d, exact_count %d (expected %d)' % (name, init, keep, kernel, count, len(flagged)))
    assert kernel == LEAN and prog.status() == 0
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))       # noqa: E731
    print('   marginals: largest relative difference to the exact kernel %.3g, to the oracle %.3g' % (rel(marg, marg3), rel(marg, wmarg)))
    np.testing.assert_allclose(marg, marg3, rtol=RTOL_EXACT, atol=1e-300)
    np.testing.assert_allclose(marg, wmarg, rtol=RTOL, atol=1e-300)
    if keep:
        print('   messages: largest relative difference to the exact kernel %.3g, to the oracle %.3g' % (rel(msgs, msgs3), rel(msgs, want)))
        np.testing.assert_allclose(msgs, msgs3, rtol=RTOL_EXACT, atol=1e-300)
        np.testing.assert_allclose(msgs, want, rtol=RTOL, atol=1e-300)
    elif bt.X == 64:            # (a padded state space reads out in a launch of its own, over the messages in memory)
        good = [b for b in range(bt.B) if b not in flagged]
        assert np.array_equal(msgs[good], start[good]) if start is not None else np.isnan(msgs[good]).all()
    assert count == len(flagged)            # those two and only those (their results were compared with the exact kernel's above)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['user_k3', 'star3', 'user_k4'])
def test_skip_unchanged_equals_the_full_schedule_bit_for_bit(name):
    """(the graphs the exact kernel redoes are its own: it runs the pruned op list with its true normalisations, and agrees with
    its full schedule to rounding, not to the bit)"""
    bt = _batch(name)
    flagged = FLAGGED.get(name, ())
    good = [b for b in range(bt.B) if b not in flagged]
    prog, msgs, marg, kernel = _call(bt, True, None)
    assert kernel == LEAN and prog.status() == 0
    assert prog.skippable_updates() > 0
    prog, msgs_s, marg_s, kernel = _call(bt, True, None, skip_unchanged=True)
    assert kernel == LEAN and prog.status() == 0 and prog.exact_count(bt.B) == len(flagged)
    assert np.array_equal(msgs[good], msgs_s[good]) and np.array_equal(marg[good], marg_s[good])
    np.testing.assert_allclose(msgs_s, msgs, rtol=RTOL_EXACT, atol=1e-300)
    np.testing.assert_allclose(marg_s, marg, rtol=RTOL_EXACT, atol=1e-300)
