"""ctypes binding of libmlbp_exactmap.so (include/mlbp_exactmap.h): the exact MAP assignment and the max-marginals by cutset
conditioning.

The seventh library of the engine, with its own signature table.  There is no CPU fallback: the compute call on a machine
without an MI355X returns MLBP_ENODEVICE, raised as ExactMapError.

The call takes the packed plan of include/mlbp_cutset.h: `plan(topo, cutset, X, device)` derives it with cutset.choose /
cutset.plan_words, has THIS library validate it on the host, uploads it once and caches the device copy.
"""
import ctypes as C

from . import _sidelib
from . import cutset as _cutset
from ._sidelib import i32 as _i32, i32p as _i32p

LIB_PATH = _sidelib.lib_path('mlbp_exactmap')

KERNEL_NONE, KERNEL_X64, KERNEL_GENERIC = 0, 1, 2
PARTIAL_HEADER = 4              # include/mlbp_exactmap.h MLBP_EXACTMAP_PARTIAL_HEADER
DROP_BELOW = 1000
MAX_LISTED = 65536              # MLBP_EXACTMAP_MAX_LISTED: the most entries a listed call takes per graph
MAX_CUT = 16                    # MLBP_EXACTMAP_MAX_CUT: the most cutset variables of a listed call


class ExactMapError(_sidelib.SideError):
    LIB = 'libmlbp_exactmap'


class ExactMapArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('X', C.c_int32), ('n_vars', C.c_int32), ('P', C.c_int32), ('U', C.c_int32),
                ('n_cut', C.c_int32), ('n_free', C.c_int32), ('n_items', C.c_int32), ('n_consts', C.c_int32), ('n_forest', C.c_int32),
                ('n_pair_tables', C.c_int32), ('n_unary_tables', C.c_int32),
                ('plan_words', C.c_int32),
                ('N', C.c_int32),
                ('plan', C.c_void_p),
                ('pair_tables', C.c_void_p), ('pair_tab', C.c_void_p), ('unary_tables', C.c_void_p), ('unary_tab', C.c_void_p),
                ('configs', C.c_void_p),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_int64),
                ('assignment', C.c_void_p), ('score', C.c_void_p), ('max_marginals', C.c_void_p),
                ('entry', C.c_void_p)]


# name -> (restype, argtypes); mirrors include/mlbp_exactmap.h one to one (tests/test_side_libraries_cpu.py checks that).
SIGNATURES = {
    'mlbp_exactmap_f64': (C.c_int, [C.POINTER(ExactMapArgs), C.c_void_p]),
    'mlbp_exactmap_check_plan': (C.c_int, [_i32p, _i32, _i32]),
    'mlbp_exactmap_pick_kernel': (C.c_int, [_i32, _i32, _i32, _i32, _i32]),
    'mlbp_exactmap_chunks': (C.c_int, [_i32, _i32]),
    'mlbp_exactmap_workspace_bytes': (C.c_int64, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    'mlbp_exactmap_last_kernel': (C.c_int, []),
    'mlbp_exactmap_arch': (C.c_char_p, []),
    'mlbp_exactmap_last_error': (C.c_char_p, []),
}

lib = _sidelib.load(LIB_PATH, SIGNATURES)
last_error, check, last_kernel, pick_kernel = _sidelib.status_helpers(lib, ExactMapError)


def chunks(B, n_configs):
    """C of the launch grid (B, C): workgroup (g, k) walks configurations k, k + C, ... of graph g."""
    return check(lib.mlbp_exactmap_chunks(int(B), int(n_configs)))


def workspace_bytes(B, X, n_vars, P, U, n_forest, n_cut, max_marginals):
    return check(lib.mlbp_exactmap_workspace_bytes(int(B), int(X), int(n_vars), int(P), int(U), int(n_forest), int(n_cut),
                                                   1 if max_marginals else 0))


def listed_workspace_bytes(B, X, n_vars, P, U, n_forest, N):
    """Bytes of workspace a LISTED call (N > 0 entries per graph) needs: the header's formula, from the library's kernel pick
    and chunks rule and the constants shared with cutset.py.  mlbp_exactmap_workspace_bytes states the exact call alone."""
    which, n_chunks = pick_kernel(X, n_vars, P, U, n_forest), chunks(B, N)
    Xp = (int(X) + 1) // 2 * 2
    vectors = (5 * int(n_vars) + 2) * Xp
    ints = 4 * ((int(P) + int(U) + 16 + 3) // 4 * 4)
    per = PARTIAL_HEADER * (4 if which == KERNEL_X64 else 1)
    if which == KERNEL_GENERIC and vectors * 8 + 64 + ints > _cutset.GENERIC_LDS_BYTES:
        per += vectors
    return (int(B) * n_chunks * per + int(B) * (2 * int(n_vars) + 1) * Xp) * 8


check_plan, Plan, plan = _cutset.plan_functions(__name__)
