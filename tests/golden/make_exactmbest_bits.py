"""Records tests/golden/exactmbest_exact_bits.json: every output of exact_mbest(16) on the K3, X = 64 and K4, X = 4 batches of
tests/test_gpu_searchmbest.py (golden_batches), through a libmlbp_exactmbest.so built from the commit BEFORE the library had
a listed mode.  That library takes the args struct without N, configs and entries; bind_old() binds it under that layout
and old_library() routes FactorGraphBatch.exact_mbest through it, so the batches, the plan and the workspace are the ones the test uses.

    python tests/golden/make_exactmbest_bits.py --lib /path/to/the/old/libmlbp_exactmbest.so [--out FILE]

Needs an MI355X.  tests/test_gpu_searchmbest.py::test_the_exact_call_computes_the_bits_it_computed_before holds the current
library to the file."""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS, HERE]

LISTED_FIELDS = ('N', 'configs', 'entries')


def bind_old(path):
    """(library, args struct) of the library at `path` under the args struct as it was before the listed mode."""
    from macaronicusermodeling_amd import _sidelib, exactmbest as K

    class OldArgs(C.Structure):
        _fields_ = [f for f in K.ExactMbestArgs._fields_ if f[0] not in LISTED_FIELDS]
    signatures = dict(K.SIGNATURES)
    signatures['mlbp_exactmbest_f64'] = (C.c_int, [C.POINTER(OldArgs), C.c_void_p])
    return _sidelib.load(path, signatures), OldArgs


@contextlib.contextmanager
def old_library(bound):
    """Inside the block the exactmbest binding calls bind_old()'s library under its struct."""
    from macaronicusermodeling_amd import exactmbest as K
    saved = K.lib, K.ExactMbestArgs
    K.lib, K.ExactMbestArgs = bound
    try:
        yield K
    finally:
        K.lib, K.ExactMbestArgs = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', required=True, help='libmlbp_exactmbest.so built from the commit before the listed mode')
    ap.add_argument('--out', default=os.path.join(HERE, 'exactmbest_exact_bits.json'))
    args = ap.parse_args()
    import test_gpu_searchmbest as G
    with old_library(bind_old(os.path.abspath(args.lib))):
        record = {name: G.golden_record(fb) for name, fb in G.golden_batches().items()}
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
