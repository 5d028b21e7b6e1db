"""Records tests/golden/converge_sum_bits.json: every output of converge() on the sum-product batches of
tests/test_gpu_mapconverge.py (golden_batches: one per kernel instance), through a libmlbp_converge.so built from the commit
BEFORE the library had a max-product mode.  That library takes the args struct without max_product, assignment, score,
pair_axis_var and unary_var; bind_old() binds it under that layout and old_library() routes FactorGraphBatch.converge through
it, so the batches and the programs are the ones the test uses.

    python tests/golden/make_converge_bits.py --lib /path/to/the/old/libmlbp_converge.so [--out FILE]

Needs an MI355X.  tests/test_gpu_mapconverge.py::test_the_sum_mode_computes_the_bits_it_computed_before holds the current library
to the file."""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS, HERE]

MAX_FIELDS = ('max_product', 'assignment', 'score', 'pair_axis_var', 'unary_var')


def bind_old(path):
    """(library, args struct) of the library at `path` under the args struct as it was before the max-product mode."""
    from macaronicusermodeling_amd import _sidelib, converge as V

    class OldArgs(C.Structure):
        _fields_ = [f for f in V.ConvergeArgs._fields_ if f[0] not in MAX_FIELDS]
    signatures = dict(V.SIGNATURES)
    signatures['mlbp_converge_f64'] = (C.c_int, [C.POINTER(OldArgs), C.c_void_p])
    return _sidelib.load(path, signatures), OldArgs


@contextlib.contextmanager
def old_library(bound):
    """Inside the block the converge binding calls bind_old()'s library under its struct."""
    from macaronicusermodeling_amd import converge as V
    saved = V.lib, V.ConvergeArgs
    V.lib, V.ConvergeArgs = bound
    try:
        yield V
    finally:
        V.lib, V.ConvergeArgs = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', required=True, help='libmlbp_converge.so built from the commit before the max-product mode')
    ap.add_argument('--out', default=os.path.join(HERE, 'converge_sum_bits.json'))
    args = ap.parse_args()
    import test_gpu_mapconverge as G
    with old_library(bind_old(os.path.abspath(args.lib))):
        record = {name: G.golden_record(fb, max_rounds) for name, (fb, max_rounds) in G.golden_batches().items()}
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
