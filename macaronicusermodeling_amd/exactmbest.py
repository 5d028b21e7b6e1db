"""ctypes binding of libmlbp_exactmbest.so (include/mlbp_exactmbest.h): the M jointly most probable assignments of every
graph, ranked, by cutset conditioning, each with its score.

The tenth library of the engine, with its own signature table.  There is no CPU fallback: the compute call on a machine
without an MI355X returns MLBP_ENODEVICE, raised as ExactMbestError.

The call takes the packed plan of include/mlbp_cutset.h: `plan(topo, cutset, X, device)` derives it with cutset.choose /
cutset.plan_words, has THIS library validate it on the host, uploads it once and caches the device copy.
"""
import ctypes as C

from . import _sidelib
from . import cutset as _cutset
from ._sidelib import i32 as _i32, i32p as _i32p

LIB_PATH = _sidelib.lib_path('mlbp_exactmbest')

KERNEL_NONE, KERNEL_X64, KERNEL_GENERIC = 0, 1, 2
MAX_M = 16                      # include/mlbp_exactmbest.h MLBP_EXACTMBEST_MAX_M
LISTS_FIXED = 384               # MLBP_EXACTMBEST_LISTS_FIXED
MAX_LISTED = 65536              # MLBP_EXACTMBEST_MAX_LISTED: the most entries a listed call takes per graph
MAX_CUT = 16                    # MLBP_EXACTMBEST_MAX_CUT: the most cutset variables of a listed call


class ExactMbestError(_sidelib.SideError):
    LIB = 'libmlbp_exactmbest'


class ExactMbestArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('X', C.c_int32), ('n_vars', C.c_int32), ('P', C.c_int32), ('U', C.c_int32),
                ('n_cut', C.c_int32), ('n_free', C.c_int32), ('n_items', C.c_int32), ('n_consts', C.c_int32), ('n_forest', C.c_int32),
                ('n_pair_tables', C.c_int32), ('n_unary_tables', C.c_int32),
                ('plan_words', C.c_int32),
                ('M', C.c_int32),
                ('N', C.c_int32),
                ('plan', C.c_void_p),
                ('pair_tables', C.c_void_p), ('pair_tab', C.c_void_p), ('unary_tables', C.c_void_p), ('unary_tab', C.c_void_p),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_int64),
                ('assignments', C.c_void_p), ('scores', C.c_void_p), ('n_found', C.c_void_p),
                ('configs', C.c_void_p), ('entries', C.c_void_p)]


# name -> (restype, argtypes); mirrors include/mlbp_exactmbest.h one to one (tests/test_side_libraries_cpu.py checks that).
SIGNATURES = {
    'mlbp_exactmbest_f64': (C.c_int, [C.POINTER(ExactMbestArgs), C.c_void_p]),
    'mlbp_exactmbest_check_plan': (C.c_int, [_i32p, _i32, _i32]),
    'mlbp_exactmbest_pick_kernel': (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32]),
    'mlbp_exactmbest_chunks': (C.c_int, [_i32, _i32]),
    'mlbp_exactmbest_lists_bytes': (C.c_int64, [_i32, _i32, _i32]),
    'mlbp_exactmbest_workspace_bytes': (C.c_int64, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    'mlbp_exactmbest_last_kernel': (C.c_int, []),
    'mlbp_exactmbest_arch': (C.c_char_p, []),
    'mlbp_exactmbest_last_error': (C.c_char_p, []),
}

lib = _sidelib.load(LIB_PATH, SIGNATURES)
last_error, check, last_kernel, pick_kernel = _sidelib.status_helpers(lib, ExactMbestError)


def kernels(code):
    """(values kernel, lists kernel) of a pick_kernel / last_kernel code."""
    return code & 15, code >> 4


def chunks(B, n_configs):
    """min(n_configs, ceil(512 / B)): C of the values grid (B, C)."""
    return check(lib.mlbp_exactmbest_chunks(int(B), int(n_configs)))


def lists_bytes(X, n_vars, M):
    """The bytes of a lists task beside its fixed part: in LDS when they fit, else in the workspace."""
    return check(lib.mlbp_exactmbest_lists_bytes(int(X), int(n_vars), int(M)))


def workspace_bytes(B, X, n_vars, P, U, n_forest, n_cut, M):
    return check(lib.mlbp_exactmbest_workspace_bytes(int(B), int(X), int(n_vars), int(P), int(U), int(n_forest), int(n_cut), int(M)))


def listed_workspace_bytes(B, X, n_vars, P, U, n_forest, N, M):
    """Bytes of workspace a LISTED call (N > 0 entries per graph) needs: the header's formula with N in the place of the
    number of configurations, from the library's kernel pick, chunks rule and lists_bytes and the constants shared with
    cutset.py.  mlbp_exactmbest_workspace_bytes states the exact call alone."""
    B, X, n_vars, P, U, N, M = (int(v) for v in (B, X, n_vars, P, U, N, M))
    values, lists = kernels(pick_kernel(X, n_vars, P, U, n_forest, M))
    vectors = (5 * n_vars + 2) * ((X + 1) // 2 * 2)
    ints = 4 * ((P + U + 16 + 3) // 4 * 4)
    lb = lists_bytes(X, n_vars, M)
    words = B * N * 2 + B * (M + 1) + B * M * M * 2 + (B * M * M * n_vars + 1) // 2
    if values == KERNEL_GENERIC and vectors * 8 + 64 + ints > _cutset.GENERIC_LDS_BYTES:
        words += B * chunks(B, N) * vectors
    if lists == KERNEL_GENERIC and LISTS_FIXED + ints + lb > _cutset.GENERIC_LDS_BYTES:
        words += B * M * lb // 8
    return words * 8


check_plan, Plan, plan = _cutset.plan_functions(__name__)
