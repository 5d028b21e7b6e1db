"""The static form of the lean X = 64 kernel (csrc/mlbp_lean_device.h, sweep_x64_lean_static_kernel; csrc/mlbp_lean_jit.cpp):
one program's micro-ops compiled into the kernel at run time.  It must not change a bit of a result, so every program below is
run twice on the same inputs -- by the interpreting kernel of the build and by its own static kernel, forced with
mlbp_program_specialize -- and messages, marginals, log-posteriors, exact_count, status() and the bail bytes (mlbp_program_bail_codes) are compared bit
for bit: from uniform messages and continuing from the first call's own messages, with and without the message write-back, and
with the posterior.  Every batch carries an all-zero unary row, a negative unary entry, a pairwise entry of -1000 and a +inf
entry (the graphs without unary factors: the two pairwise ones).

The programs: user_k3 at three root sequences, chain4, star3 and chain3 + chain2 -- together a contraction beside an empty
member, three-source gathers with the stored product, both parities of n_bundles, and a program that ends in a lone variable
update (carry links -- a product of more than four sources -- do not occur in them: a variable of a graph with three pairwise
factors multiplies at most three messages and one constant product); the CPU test asserts that on the decoded images, compiles every program's static kernel (and the
benchmark's) for gfx950 without a device and reads registers and scratch from the code object.

Every call also reads the thread's launch log: the forced batch must have launched a handle that is no kernel of libmlbp.so
(the module's function) and no lean instance, the plain batch the <3, false, false, 0, false> instance -- so the comparison is
never the interpreter against itself.  chain4_u60 (60 unary factors, six sweeps) asks for more than 48 KB of dynamic LDS: a module function above
the 48 KB that need no grant.

Shapes: |X| = 64, 7 graphs; the policy test one batch of 4096.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import cases as C
from macaronicusermodeling_amd import _ffi
from macaronicusermodeling_amd.topology import GraphTopology

LEAN = 7
UOP_VAR, UOP_MT, UOP_NOP, UOP_STORE_VF, UOP_NSRC_SHIFT, UOP_CARRY_IN, UOP_CARRY_OUT = 1, 2, 32, 64, 8, 0x1000, 0x2000    # csrc/mlbp_uop.h
MAX_VGPRS = 168         # three workgroups of 256 threads per CU


def _user_spec():
    return C.user_spec(10, [1, 4, 7], 64, 40, seed=1)


def _two_components():
    """chain5 without its (2, 3) factor: chain3 + chain2, three pairwise factors in two components."""
    s = C.chain_spec(5, 64, 'chain3_plus_chain2_x64')
    s['factors'] = [f for f in s['factors'] if f['vars'] != [2, 3]]
    return s


def _many_unary(counts):
    """A chain over len(counts) variables, variable v carrying counts[v] unary factors (tests/test_gpu_lean_memory.py's)."""
    n = len(counts)
    factors = []
    for v in range(n):
        for _ in range(counts[v]):
            factors.append(dict(id=len(factors), vars=[v], dims=[0], table=len(factors)))
    for v in range(n - 1):
        factors.append(dict(id=len(factors), vars=[v, v + 1], dims=[0, 1] if v % 2 else [1, 0], table=len(factors)))
    return dict(name='chain%d_u%d' % (n, sum(counts)), style='explicit', X=64, var_ids=list(range(n)), labels=[0] * n, factors=factors)


# name -> (spec, roots, seed); every one has three pairwise factors: the instance that can be specialised
PROGRAMS = {
    'user_k3_147': (_user_spec, [1, 4, 7], 301),
    'user_k3_4174': (_user_spec, [4, 1, 7, 4], 302),
    'user_k3_77': (_user_spec, [7, 7], 303),
    'chain4': (lambda: C.chain_spec(4, 64), [0, 3, 1], 304),
    'star3': (lambda: C.star_spec(3, 64), [0, 2, 1], 305),
    'chain3_chain2': (_two_components, [0, 2, 4, 3], 306),
    'chain4_u60': (lambda: _many_unary([15] * 4), [0, 3, 1, 2, 0, 3], 307),
}
INTERPRETER = ('sweep_x64_lean_kernel', (3, False, False, 0, False))
BENCH = (lambda: C.user_spec(10, [1, 4, 7], 64, 64, seed=1), [1, 4, 7])      # bench.py's default workload
B = 7
ZERO_ROW, NEG_UNARY, NEG_PAIR, INF_PAIR = 1, 2, 3, 4       # the graphs that carry a bad entry


def _bundles(spec, roots):
    """The bundle words [n_bundles][16] of the lean program of (spec, roots) (MLBP_IMAGE_LEAN: ok, n_bundles, HL, n_cprod, WL,
    then the image as a vector whose first words they are)."""
    topo = GraphTopology.from_spec(spec)
    assert topo.P == 3
    w = topo.images(roots)['lean']
    assert w[0] == 1, 'no lean program for this shape'
    n = int(w[1])
    return np.ascontiguousarray(w[6:6 + 16 * n].reshape(n, 16), dtype=np.int32)


def _forms(bundles):
    out = set()
    for r in bundles:
        fa, fb = int(r[0]), int(r[8])
        if fa & UOP_VAR:
            out.add('VAR')
            out.update(name for bit, name in ((UOP_CARRY_IN, 'CARRY_IN'), (UOP_CARRY_OUT, 'CARRY_OUT')) if fa & bit)
            continue
        d = lambda f: 'MT' if f & UOP_MT else 'TM'      # noqa: E731
        out.add('%s|%s' % (d(fa), 'NOP' if fb & UOP_NOP else d(fb)))
        for f in (fa,) if fb & UOP_NOP else (fa, fb):
            if ((f >> UOP_NSRC_SHIFT) & 15) > 2 and f & UOP_STORE_VF:
                out.add('3SRC+VF')
    out.add('ends in VAR' if int(bundles[-1][0]) & UOP_VAR else 'ends in a contraction')
    out.add('odd' if len(bundles) % 2 else 'even')
    return out


def test_the_programs_hold_every_form_of_the_loop():
    forms = {name: _forms(_bundles(p[0](), p[1])) for name, p in PROGRAMS.items()}
    for name, f in sorted(forms.items()):
        print(name, sorted(f))
    every = set().union(*forms.values())
    assert {'TM|TM', 'MT|MT', 'TM|MT', 'MT|TM', 'TM|NOP', 'MT|NOP', 'VAR', '3SRC+VF'} <= every
    assert {'odd', 'even'} <= every and 'ends in VAR' in every and 'ends in a contraction' in every
    # the launch's dynamic LDS (lean_lds_bytes, csrc/mlbp_lean.hip): messages and ext slots, reduction buffers, micro-ops
    topo = GraphTopology.from_spec(PROGRAMS['chain4_u60'][0]())
    w = topo.images(PROGRAMS['chain4_u60'][1])['lean']
    lds = (topo.n_msgs + 2 + int(w[3])) * 512 + 8192 + 64 * (int(w[1]) + 1)
    print('chain4_u60: %d bytes of LDS' % lds)
    assert 48 * 1024 < lds <= 64 * 1024


def _note(code, key):
    """An unsigned integer of the code object's kernel metadata (msgpack: the key as a string, then the value).  The object
    holds one kernel, so the key occurs once."""
    at = [m.end() for m in re.finditer(re.escape(key.encode()), code)]
    assert len(at) == 1, (key, len(at))
    t = code[at[0]]
    if t < 0x80:
        return t
    width = {0xcc: 1, 0xcd: 2, 0xce: 4}[t]
    return int.from_bytes(code[at[0] + 1:at[0] + 1 + width], 'big')


@pytest.mark.parametrize('name', sorted(PROGRAMS) + ['bench'])
def test_static_kernel_compiles_without_a_device_within_the_register_budget(name):
    make, roots = PROGRAMS[name][:2] if name != 'bench' else BENCH
    b = _bundles(make(), roots)
    buf = ctypes.create_string_buffer(1 << 20)
    n = _ffi.check(_ffi.lib.mlbp_lean_static_code(_ffi.i32ptr(b.reshape(-1)), len(b), b'gfx950', buf, len(buf)))
    assert 0 < n <= len(buf)
    code = buf.raw[:n]
    assert code[:4] == b'\x7fELF' and b'sweep_x64_lean_static_kernel' in code
    vgprs, scratch = _note(code, '.vgpr_count'), _note(code, '.private_segment_fixed_size')
    print('%s: %d bundles, %d bytes of code object, %d VGPRs, %d bytes of scratch' % (name, len(b), n, vgprs, scratch))
    assert vgprs <= MAX_VGPRS and scratch == 0


# ---------------------------------------------------------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------------------------------------------------------
def _make_batch(name):
    import test_gpu_lean_memory as TM          # its _Batch: per-graph random tables on the device
    make, roots, seed = PROGRAMS[name]
    spec = make()
    bt = TM._Batch(spec if spec.get('style') == 'explicit' else TM._explicit(spec), roots, B, seed)
    assert bt.topo.P == 3
    if bt.topo.U:
        bt.unary[ZERO_ROW, bt.topo.U - 1] = 0.0
        bt.unary[NEG_UNARY, 0, 11] = -0.25
    bt.pair[NEG_PAIR, 1, 17, 40] = -1000.0
    bt.pair[INF_PAIR, 2, 5, 9] = np.inf
    bt.upload()
    return bt


@functools.lru_cache(maxsize=None)
def _pair(name):
    """(interpreted, static): two batches of the same inputs, the second one's program specialised."""
    plain, forced = _make_batch(name), _make_batch(name)
    assert np.array_equal(plain.pair, forced.pair) and np.array_equal(plain.unary, forced.unary)
    prog = forced.fb.program(forced.roots)
    before = _ffi.lib.mlbp_lean_compile_count()
    prog.specialize()
    assert prog.specialized() == 1
    print('%s: %s' % (name, _ffi.lib.mlbp_last_error().decode()))
    assert _ffi.lib.mlbp_lean_compile_count() > before
    return plain, forced


def _call(bt, init, start, keep, posterior):
    """One sweep call -> everything it leaves, as bytes-comparable host arrays and integers."""
    import torch
    fb = bt.fb
    if start is None:
        fb.msgs.fill_(float('nan'))
    else:
        fb.msgs.copy_(torch.from_numpy(start))
    marg = torch.full((bt.B, bt.topo.n_vars, bt.X), float('nan'), dtype=torch.float64, device=fb.device)
    post = None
    if posterior:
        labels = torch.from_numpy(np.random.RandomState(9).randint(0, bt.X, size=(bt.B, bt.topo.n_vars)).astype(np.int32)).to(fb.device)
        post = (labels, torch.full((bt.B,), float('nan'), dtype=torch.float64, device=fb.device),
                torch.full((1,), float('nan'), dtype=torch.float64, device=fb.device))
    import kernel_inventory as K
    K.reset()
    prog = fb.sweep(bt.roots, init=init, marginals=marg, keep_messages=keep, posterior=post)
    torch.cuda.synchronize()
    handles, lean = K.launched_handles(), [k for k in K.launched() if k[0] == 'sweep_x64_lean_kernel']
    known = set(K._tables()['all_by_addr'])
    kernel = _ffi.lib.mlbp_last_sweep_kernel()
    count = prog.exact_count(bt.B)
    reasons = _ffi.lib.mlbp_last_error().decode()           # exact_count's histogram of the bail codes
    out = dict(msgs=fb.msgs.cpu().numpy(), marg=marg.cpu().numpy(), kernel=kernel, count=count, reasons=reasons, status=prog.status(),
               specialized=prog.specialized(), bail=prog.bail_codes(bt.B), lean=lean, foreign=[h for h in handles if h not in known])
    if posterior:
        out['logp'], out['logp_sum'] = post[1].cpu().numpy(), post[2].cpu().numpy()
    return out


def _same(a, b, what):
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), '%s: %s differs' % (what, k)
    assert (a['kernel'], b['kernel']) == (LEAN, LEAN)
    assert (a['count'], a['reasons'], a['status']) == (b['count'], b['reasons'], b['status']), what
    assert (a['specialized'], b['specialized']) == (0, 1)       # an unforced small batch never compiles
    assert len(a['bail']) == B and int((a['bail'] != 0).sum()) == a['count']
    # what was launched: the compiled-in instance and nothing foreign | no lean instance and one handle from outside the library
    assert a['lean'] == [INTERPRETER] and a['foreign'] == [], (what, a['lean'], a['foreign'])
    assert b['lean'] == [] and len(b['foreign']) == 1, (what, b['lean'], b['foreign'])


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(PROGRAMS))
def test_static_kernel_equals_the_interpreter_bit_for_bit(name):
    plain, forced = _pair(name)
    first = None
    for init in (True, False):
        for keep in (True, False):
            for posterior in ((False, True) if keep else (False,)):
                start = None if init else first
                a, b = _call(plain, init, start, keep, posterior), _call(forced, init, start, keep, posterior)
                what = '%s init=%s keep=%s posterior=%s' % (name, init, keep, posterior)
                print('%s: exact_count %d, %s' % (what, a['count'], a['reasons']))
                _same(a, b, what)
                assert a['count'] >= 2 and a['status'] == 0           # (the bad entries reach the exact kernel on both sides)
                if init and keep and not posterior:
                    first = a['msgs']
    assert first is not None and np.isfinite(first[0]).all()


@pytest.mark.gpu
def test_a_second_forced_call_does_not_compile_again():
    _, forced = _pair('chain4')
    prog = forced.fb.program(forced.roots)
    before = _ffi.lib.mlbp_lean_compile_count()
    prog.specialize()
    _call(forced, True, None, True, False)
    assert prog.specialized() == 1 and _ffi.lib.mlbp_lean_compile_count() == before


@pytest.mark.gpu
def test_a_program_the_kernel_does_not_take_is_refused_with_a_reason():
    import test_gpu_lean_memory as TM
    bt = TM._Batch(C.chain_spec(3, 64), [0, 2, 0], 5, 311)       # two pairwise factors
    prog = bt.fb.program(bt.roots)
    with pytest.raises(Exception):
        prog.specialize()
    assert prog.specialized() == -1 and b'three pairwise factors' in _ffi.lib.mlbp_last_error()
    out = _call(bt, True, None, True, False)
    assert out['kernel'] == LEAN and out['status'] == 0 and np.isfinite(out['marg']).all()


@pytest.mark.gpu
def test_the_automatic_policy_compiles_at_4096_graphs_unless_disabled():
    import torch
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    spec, roots = _user_spec(), [1, 4, 7]
    topo = GraphTopology.from_spec(spec)
    n = 4096
    gen = torch.Generator(device='cuda:0').manual_seed(5)
    pair = torch.rand(n * topo.P, 64, 64, dtype=torch.float64, device='cuda:0', generator=gen) + 0.01
    unary = torch.rand(n * topo.U, 64, dtype=torch.float64, device='cuda:0', generator=gen) + 0.01

    def batch(graphs):
        fb = FactorGraphBatch(topo, 64, graphs)
        fb.set_pair_tables(pair[:graphs * topo.P])
        fb.set_unary_tables(unary[:graphs * topo.U])
        return fb

    def run(fb):
        marg = torch.empty(fb.B, topo.n_vars, 64, dtype=torch.float64, device=fb.device)
        prog = fb.sweep(roots, init=True, marginals=marg)
        torch.cuda.synchronize()
        assert _ffi.lib.mlbp_last_sweep_kernel() == LEAN and prog.status() == 0
        return prog, marg.cpu().numpy()

    saved = os.environ.get('MLBP_LEAN_SPECIALIZE')
    try:
        os.environ['MLBP_LEAN_SPECIALIZE'] = '0'
        off = batch(n)
        prog, want = run(off)
        assert prog.specialized() == 0
        os.environ.pop('MLBP_LEAN_SPECIALIZE')
        small = batch(n - 1)
        assert run(small)[0].specialized() == 0            # below the policy's batch size
        before = _ffi.lib.mlbp_lean_compile_count()
        on = batch(n)
        prog, got = run(on)
        assert prog.specialized() == 1 and _ffi.lib.mlbp_lean_compile_count() == before + 1
        print(_ffi.lib.mlbp_last_error().decode())
        assert got.tobytes() == want.tobytes()
        run(on)
        assert _ffi.lib.mlbp_lean_compile_count() == before + 1
    finally:
        if saved is None:
            os.environ.pop('MLBP_LEAN_SPECIALIZE', None)
        else:
            os.environ['MLBP_LEAN_SPECIALIZE'] = saved
