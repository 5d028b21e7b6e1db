#!/usr/bin/env python3
"""Pin the integer images of the sweep-program compilers (build_fused_program, build_lean_program / build_lean_readout,
build_shared_program / build_shared_readout, drop_unchanged_updates) word for word.

    python tests/golden/make_program_images.py              writes program_images.npz
    python tests/golden/make_program_images.py --check      compares what the library gives now with the committed file
    python tests/golden/make_program_images.py --dump FILE  writes the op lists of every shape as text (tools/compile_check.cpp reads it)

program_images.npz holds one int32 array per (shape, image): key '<shape>/<image>', the image names of _ffi.IMAGES, each in
mlbp_program_image's serialisation (include/mlbp.h).  It was written ONCE, by the compilers as they stood before they moved out
of the kernel files into csrc/mlbp_compile.cpp (that commit's parent with nothing but the mlbp_program_image entry point added),
and is what tests/test_program_images.py holds the library to: never regenerate it from later code -- a word that changes is a
change of what the X = 64 kernels read, to be argued on its own.  Reads nothing outside the repository; needs no GPU.

Shapes (three sweeps unless said): the clique sentences K1 to K12 with the trainer's roots; the calls of
test_host_logic.py::test_program_rewrites_plan; trees, rings and the shuffled graphs of cases.py; the 25 random graphs of
test_host_logic.py (seeds 9000 to 9024, the first variable as every root); single sweeps of K3 and K4; and hand-made op lists
that land on the refusals no graph above reaches (REFUSALS below)."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, 'tests'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import cases as C  # noqa: E402
from macaronicusermodeling_amd import _ffi  # noqa: E402
from macaronicusermodeling_amd.topology import GraphTopology, program_images  # noqa: E402

OUT = os.path.join(HERE, 'program_images.npz')
U_, TM, MT, VAR = _ffi.OP_UNARY, _ffi.OP_PAIR_TM, _ffi.OP_PAIR_MT, _ffi.OP_VAR

# Why build_shared_program declines a program: the SHARED image of a declined program carries the LENGTH of the reason.
SHARED_WHYS = ('unary messages are not all constant, or no / too many pairwise factors',
               'a unary message is folded into no variable update',
               'unsupported update kind or slot use',
               'more than 254 live tiles or 65535 message slots',
               'a variable update multiplies more than 8 tiles')
# ... and build_lean_program (the LEAN image has ok = 0; which of the two shows in the FUSED image's has_unary_fops)
LEAN_WHYS = ('in-loop unary updates (not hoistable)', 'a constant product of more than 15 messages')
N_SHARED_SCALARS = 28       # behind ok; of them (include/mlbp.h):
PF_OK, VF_DIRECT, P3_OK = 1 + 14, 1 + 21, 1 + 22


def _hand(ops, srcs, n_msgs, P, U, readout):
    """One sweep of a hand-made op list; readout: the incoming slots of each variable."""
    off = np.cumsum([0] + [len(r) for r in readout])
    return dict(ops=np.array(ops, dtype=np.int32).reshape(-1, 4), srcs=np.array(srcs, dtype=np.int32),
                sweeps=np.array([[0, len(ops)]], dtype=np.int32), n_msgs=n_msgs, P=P, U=U, n_vars=len(readout),
                in_off=off.astype(np.int32), in_slots=np.array([c for r in readout for c in r], dtype=np.int32))


def refusals():
    """The smallest op lists that land on the refusals none of the graphs reaches (no random spec does: a random variable has
    at most a handful of factors, every unary message of a graph is folded into its variable's updates, and one factor never
    writes one slot from two tables)."""
    out = {}
    # shared: 'a variable update multiplies more than 8 tiles' -- the uniform base and eight factor->variable messages
    ops = [[TM, 0, 0, 1 + i] for i in range(8)] + [[VAR, 0, 8, 9], [TM, 0, 9, 10]]
    out['refuse_var_9_tiles'] = _hand(ops, list(range(1, 9)), 11, 1, 0, [[1, 2], [10]])
    # lean: 'a constant product of more than 15 messages' -- sixteen unary messages into one variable
    ops = [[U_, i, 0, i] for i in range(16)] + [[VAR, 0, 16, 16], [TM, 0, 16, 17]]
    out['refuse_cprod_16_messages'] = _hand(ops, list(range(16)), 18, 1, 16, [list(range(16)), [17]])
    # lean and shared: an in-loop unary update that cannot be hoisted -- two unary tables writing one slot
    ops = [[U_, 0, 0, 0], [U_, 1, 0, 0], [VAR, 0, 1, 1], [TM, 0, 1, 2]]
    out['refuse_unary_two_tables_one_slot'] = _hand(ops, [0], 3, 1, 2, [[0], [2]])
    # shared: 'a unary message is folded into no variable update'
    out['refuse_unary_message_unread'] = _hand([[U_, 0, 0, 0], [TM, 0, 1, 2]], [], 3, 1, 1, [[0], [2]])
    # shared: 'unsupported update kind or slot use' -- a constant product whose only variable update is dropped as dead
    ops = [[U_, 0, 0, 0], [U_, 1, 0, 1], [VAR, 0, 1, 2], [VAR, 1, 1, 2], [TM, 0, 2, 3]]
    out['refuse_cprod_without_tile'] = _hand(ops, [0, 1], 4, 1, 2, [[0], [1, 3]])
    # shared: 'more than 254 live tiles' -- a chain of 255 factor updates through 256 slots
    ops = [[TM if i % 2 else MT, 0, i, i + 1] for i in range(255)]
    out['refuse_255_live_tiles'] = _hand(ops, [], 256, 1, 0, [[255]])
    return out


def _graph(spec, roots):
    topo = GraphTopology.from_spec(spec)
    ops, srcs, sweeps = topo.compile_program(roots)
    return dict(ops=ops, srcs=srcs, sweeps=sweeps, n_msgs=topo.n_msgs, P=topo.P, U=topo.U, n_vars=topo.n_vars,
                in_off=topo.in_off, in_slots=topo.in_slots)


def shapes():
    """{shape name: the arguments of topology.program_images}, in a fixed order."""
    from helpers import random_spec
    from test_host_logic import _clique_shapes
    out = {}
    for spec, roots in _clique_shapes():
        k = len(spec['var_ids'])
        assert 'clique_k%d' % k not in out
        out['clique_k%d' % k] = _graph(spec, roots)
    k3, k4 = C.user_spec(10, [1, 4, 7], 64, 64, seed=1), C.user_spec(9, [0, 2, 3, 7], 64, 64, seed=4)
    out['plan_k3_roots_1_4_7'] = _graph(k3, [1, 4, 7])
    out['plan_k3_roots_1_1_1'] = _graph(k3, [1, 1, 1])
    out['plan_k2_roots_0_1_0'] = _graph(C.user_spec(6, [0, 1], 64, 64, seed=3), [0, 1, 0])
    out['plan_k4_roots_0_2_3'] = _graph(k4, [0, 2, 3])
    out['plan_ring8_x64_roots_0_0_0'] = _graph(C.ring_spec(8, 64), [0, 0, 0])
    out['plan_k1_one_sweep'] = _graph(C.user_spec(5, [2], 64, 64, seed=5), [2])
    out['chain8_roots_0_0_0'] = _graph(C.chain_spec(8, 4), [0, 0, 0])
    out['star5_roots_0_2_0'] = _graph(C.star_spec(5, 4), [0, 2, 0])
    out['shuffled_x4_roots_11_5_7'] = _graph(C.shuffled_ids_spec(4), [11, 5, 7])
    out['shuffled_x64_roots_2_7_5'] = _graph(C.shuffled_ids_spec(64), [2, 7, 5])
    out['ring8_roots_0_3_0_0'] = _graph(C.ring_spec(8, 4), [0, 3, 0, 0])           # four sweeps, three of them share one op range
    for seed in range(25):
        spec = random_spec(np.random.RandomState(9000 + seed), 'random_%d' % seed)
        out['random_%d' % seed] = _graph(spec, [GraphTopology.from_spec(spec).var_ids[0]] * 3)
    out.update(refusals())
    out['single_sweep_k3'] = _graph(k3, [1])
    out['single_sweep_k4'] = _graph(k4, [0])
    return out


def generate():
    """{'<shape>/<image>': int32 array} from the library as built now."""
    arrays = {}
    for name, s in shapes().items():
        for which, a in program_images(**s).items():
            arrays['%s/%s' % (name, which)] = a
    return arrays


def check_coverage(arrays):
    """What the fixture must reach, as a condition on it."""
    names = sorted({k.split('/')[0] for k in arrays})
    lens = [len(w) for w in SHARED_WHYS]
    assert len(set(lens)) == len(lens), 'the reasons are told apart by their lengths'
    seen_shared, seen_lean, flags, dropped = set(), set(), {PF_OK: set(), VF_DIRECT: set(), P3_OK: set()}, 0
    for n in names:
        sh, ln, fu, pr = (arrays['%s/%s' % (n, w)] for w in ('shared', 'lean', 'fused', 'pruned'))
        if sh[0]:
            for f in flags:
                flags[f].add(int(sh[f]))
        else:
            assert len(sh) == 2
            seen_shared.add(SHARED_WHYS[lens.index(int(sh[1]))])
        if not ln[0]:
            seen_lean.add(LEAN_WHYS[0 if fu[-1] else 1])
        dropped += int(pr[-1]) > 0
    assert seen_shared == set(SHARED_WHYS), set(SHARED_WHYS) - seen_shared
    assert seen_lean == set(LEAN_WHYS), set(LEAN_WHYS) - seen_lean
    assert all(v == {0, 1} for v in flags.values()), flags
    assert dropped >= 1
    return len(names), dropped


def dump(path):
    """Text form of every shape: a header line `name n_ops n_srcs n_sweeps n_msgs P U n_vars n_in`, then the words of ops,
    srcs, sweeps, in_off and in_slots on one line each."""
    with open(path, 'w') as f:
        for name, s in shapes().items():
            arrs = [np.asarray(s[k], dtype=np.int32).reshape(-1) for k in ('ops', 'srcs', 'sweeps', 'in_off')]
            arrs.append(np.asarray(s['in_slots'], dtype=np.int32).reshape(-1)[:int(s['in_off'][-1])])
            f.write('%s %d %d %d %d %d %d %d %d\n' % (name, len(arrs[0]) // 4, len(arrs[1]), len(arrs[2]) // 2, s['n_msgs'], s['P'], s['U'],
                                                      s['n_vars'], len(arrs[4])))
            for a in arrs:
                f.write(' '.join(str(int(v)) for v in a) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--check', action='store_true', help='compare with the committed file instead of writing it')
    ap.add_argument('--dump', metavar='FILE', help='write the op lists as text and stop')
    a = ap.parse_args()
    if a.dump:
        dump(a.dump)
        return
    arrays = generate()
    n_shapes, dropped = check_coverage(arrays)
    if a.check:
        want = np.load(OUT)
        assert sorted(want.files) == sorted(arrays), set(want.files) ^ set(arrays)
        bad = [k for k in want.files if want[k].dtype != np.int32 or not np.array_equal(want[k], arrays[k])]
        assert not bad, 'images differ: %s' % bad
        print('program_images.npz reproduced: %d arrays of %d shapes equal' % (len(arrays), n_shapes))
        return
    np.savez_compressed(OUT, **arrays)
    print('wrote program_images.npz: %d arrays of %d shapes, %d words, %d bytes; %d shapes drop updates when pruned'
          % (len(arrays), n_shapes, sum(len(v) for v in arrays.values()), os.path.getsize(OUT), dropped))


if __name__ == '__main__':
    main()
