"""ctypes binding of libmlbp_exactsample.so (include/mlbp_exactsample.h): whole assignments drawn from the model itself by
cutset conditioning, with log p(x) = score(x) - log Z of every draw; and, over a caller's list of cutset states (N > 0), draws by
sampling-importance-resampling for the cutsets beyond the exact limit.

The ninth library of the engine, with its own signature table.  There is no CPU fallback: the compute call on a machine
without an MI355X returns MLBP_ENODEVICE, raised as ExactSampleError.

The call takes the packed plan of include/mlbp_cutset.h: `plan(topo, cutset, X, device)` derives it with cutset.choose /
cutset.plan_words, has THIS library validate it on the host, uploads it once and caches the device copy.
"""
import ctypes as C

from . import _sidelib
from . import cutset as _cutset
from ._sidelib import i32 as _i32, i32p as _i32p

LIB_PATH = _sidelib.lib_path('mlbp_exactsample')

KERNEL_NONE, KERNEL_X64, KERNEL_GENERIC = 0, 1, 2
HEAD = 4                        # include/mlbp_exactsample.h MLBP_EXACTSAMPLE_HEAD
MAX_LISTED = 65536              # MLBP_EXACTSAMPLE_MAX_LISTED: the most entries a listed call takes per graph


class ExactSampleError(_sidelib.SideError):
    LIB = 'libmlbp_exactsample'


class ExactSampleArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('X', C.c_int32), ('n_vars', C.c_int32), ('P', C.c_int32), ('U', C.c_int32),
                ('n_cut', C.c_int32), ('n_free', C.c_int32), ('n_items', C.c_int32), ('n_consts', C.c_int32), ('n_forest', C.c_int32),
                ('n_pair_tables', C.c_int32), ('n_unary_tables', C.c_int32),
                ('plan_words', C.c_int32),
                ('S', C.c_int32),
                ('N', C.c_int32),
                ('plan', C.c_void_p),
                ('pair_tables', C.c_void_p), ('pair_tab', C.c_void_p), ('unary_tables', C.c_void_p), ('unary_tab', C.c_void_p),
                ('uniforms', C.c_void_p),
                ('configs', C.c_void_p), ('log_q', C.c_void_p),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_int64),
                ('samples', C.c_void_p), ('logp', C.c_void_p), ('log_z', C.c_void_p), ('score', C.c_void_p),
                ('entry', C.c_void_p), ('ess', C.c_void_p)]


# name -> (restype, argtypes); mirrors include/mlbp_exactsample.h one to one (tests/test_side_libraries_cpu.py checks that).
SIGNATURES = {
    'mlbp_exactsample_f64': (C.c_int, [C.POINTER(ExactSampleArgs), C.c_void_p]),
    'mlbp_exactsample_check_plan': (C.c_int, [_i32p, _i32, _i32]),
    'mlbp_exactsample_pick_kernel': (C.c_int, [_i32, _i32, _i32, _i32, _i32]),
    'mlbp_exactsample_chunks': (C.c_int, [_i32, _i32]),
    'mlbp_exactsample_workspace_bytes': (C.c_int64, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    'mlbp_exactsample_last_kernel': (C.c_int, []),
    'mlbp_exactsample_arch': (C.c_char_p, []),
    'mlbp_exactsample_last_error': (C.c_char_p, []),
}

lib = _sidelib.load(LIB_PATH, SIGNATURES)
last_error, check, last_kernel, pick_kernel = _sidelib.status_helpers(lib, ExactSampleError)


def chunks(B, n):
    """min(n, ceil(512 / B)): C of the weights grid (B, C) with n = the configurations, of the draw grid with n = the samples
    (generic kernel) or ceil(samples / 4) (X = 64 kernel: a sample per wave)."""
    return check(lib.mlbp_exactsample_chunks(int(B), int(n)))


def workspace_bytes(B, S, X, n_vars, P, U, n_forest, n_cut):
    return check(lib.mlbp_exactsample_workspace_bytes(int(B), int(S), int(X), int(n_vars), int(P), int(U), int(n_forest), int(n_cut)))


def listed_workspace_bytes(B, S, X, n_vars, P, U, n_forest, N):
    """Bytes of workspace a LISTED call (N > 0 entries per graph, S samples) needs: the header's formula with N in the place of
    the configurations, from the library's kernel pick and chunks rule and the constants shared with cutset.py.
    mlbp_exactsample_workspace_bytes states the exact call alone."""
    which = pick_kernel(X, n_vars, P, U, n_forest)
    cw = chunks(B, N)
    cd = chunks(B, -(-int(S) // 4) if which == KERNEL_X64 else S)
    Xp = (int(X) + 1) // 2 * 2
    vectors = (5 * int(n_vars) + 2) * Xp
    ints = 4 * ((int(P) + int(U) + 16 + 3) // 4 * 4)
    spill = which == KERNEL_GENERIC and vectors * 8 + 64 + ints > _cutset.GENERIC_LDS_BYTES
    return (int(B) * int(N) * 3 + int(B) * HEAD + (int(B) * max(cw, cd) * vectors if spill else 0)) * 8


check_plan, Plan, plan = _cutset.plan_functions(__name__)
