"""ctypes binding of libmlbp_exactgrad.so (include/mlbp_exactgrad.h): the model's true pairwise marginals, expected features
and likelihood gradient by cutset conditioning; and, over a caller's list of cutset states (N > 0), their self-normalised
estimates for the cutsets beyond the exact limit.

The eighth library of the engine, with its own signature table.  There is no CPU fallback: the compute call on a machine
without an MI355X returns MLBP_ENODEVICE, raised as ExactGradError.

The call takes the packed plan of include/mlbp_cutset.h: `plan(topo, cutset, X, device)` derives it with cutset.choose /
cutset.plan_words, has THIS library validate it on the host, uploads it once and caches the device copy.
"""
import ctypes as C
import functools

from . import _sidelib
from . import cutset as _cutset
from ._sidelib import i32 as _i32, i32p as _i32p

LIB_PATH = _sidelib.lib_path('mlbp_exactgrad')

KERNEL_NONE, KERNEL_X64, KERNEL_GENERIC = 0, 1, 2
X64_MAX_FOREST = 2              # include/mlbp_exactgrad.h MLBP_EXACTGRAD_X64_MAX_FOREST
MIN_WORKGROUPS = 256
MAX_FEATURES = 64
MAX_LISTED = 65536              # MLBP_EXACTGRAD_MAX_LISTED: the most entries a listed call takes per graph
MAX_CUT = 16                    # MLBP_EXACTGRAD_MAX_CUT: the most cutset variables of a listed call


class ExactGradError(_sidelib.SideError):
    LIB = 'libmlbp_exactgrad'


class ExactGradArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('X', C.c_int32), ('n_vars', C.c_int32), ('P', C.c_int32), ('U', C.c_int32),
                ('n_cut', C.c_int32), ('n_free', C.c_int32), ('n_items', C.c_int32), ('n_consts', C.c_int32), ('n_forest', C.c_int32),
                ('n_pair_tables', C.c_int32), ('n_unary_tables', C.c_int32),
                ('plan_words', C.c_int32),
                ('F_ee', C.c_int32), ('F_ed', C.c_int32), ('Vde', C.c_int32),
                ('plan', C.c_void_p),
                ('pair_tables', C.c_void_p), ('pair_tab', C.c_void_p), ('unary_tables', C.c_void_p), ('unary_tab', C.c_void_p),
                ('phi_en_en', C.c_void_p), ('phi_en_en_w1', C.c_void_p), ('phi_en_de', C.c_void_p),
                ('pair_phi', C.c_void_p), ('unary_kind', C.c_void_p), ('unary_obs', C.c_void_p),
                ('labels', C.c_void_p),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_int64),
                ('log_z', C.c_void_p), ('marginals', C.c_void_p), ('pair_marginals', C.c_void_p),
                ('expect_ee', C.c_void_p), ('expect_ed', C.c_void_p), ('grad_ee', C.c_void_p), ('grad_ed', C.c_void_p)]


@functools.lru_cache(maxsize=None)
def listed_args():
    """The ctypes class of mlbp_exactgrad_listed_args: ExactGradArgs as `args`, then configs, log_q and N.  A listed call passes
    byref(a.args) with a.args.plan_words negated (the header's sign of a list behind the struct).  Made on first use: the module
    itself holds ONE Structure, the one that mirrors mlbp_exactgrad_args."""
    return type('ExactGradListedArgs', (C.Structure,),
                {'_fields_': [('args', ExactGradArgs), ('configs', C.c_void_p), ('log_q', C.c_void_p), ('N', C.c_int32)]})


# name -> (restype, argtypes); mirrors include/mlbp_exactgrad.h one to one (tests/test_side_libraries_cpu.py checks that).
SIGNATURES = {
    'mlbp_exactgrad_f64': (C.c_int, [C.POINTER(ExactGradArgs), C.c_void_p]),
    'mlbp_exactgrad_check_plan': (C.c_int, [_i32p, _i32, _i32]),
    'mlbp_exactgrad_pick_kernel': (C.c_int, [_i32, _i32, _i32, _i32, _i32]),
    'mlbp_exactgrad_chunks': (C.c_int, [_i32, _i32, _i32]),
    'mlbp_exactgrad_workspace_bytes': (C.c_int64, [_i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    'mlbp_exactgrad_last_kernel': (C.c_int, []),
    'mlbp_exactgrad_arch': (C.c_char_p, []),
    'mlbp_exactgrad_last_error': (C.c_char_p, []),
}

lib = _sidelib.load(LIB_PATH, SIGNATURES)
last_error, check, last_kernel, pick_kernel = _sidelib.status_helpers(lib, ExactGradError)


def chunks(B, n_configs, kernel):
    """C of the launch grid (B, C) for kernel = KERNEL_X64 or KERNEL_GENERIC."""
    return check(lib.mlbp_exactgrad_chunks(int(B), int(n_configs), int(kernel)))


def workspace_bytes(B, X, n_vars, P, U, n_forest, n_cut):
    return check(lib.mlbp_exactgrad_workspace_bytes(int(B), int(X), int(n_vars), int(P), int(U), int(n_forest), int(n_cut)))


def listed_workspace_bytes(B, X, n_vars, P, U, n_forest, N):
    """Bytes of workspace a LISTED call (N > 0 entries per graph) needs: the header's formula with N in the place of the
    configurations, from the library's kernel pick and chunks rule and the constants shared with cutset.py.
    mlbp_exactgrad_workspace_bytes states the exact call alone.  A partial holds X * X doubles per pairwise factor: K5 at X = 64
    is 330 256 bytes, four of them per graph on the X = 64 kernel."""
    which = pick_kernel(X, n_vars, P, U, n_forest)
    n_chunks = chunks(B, N, which)
    Xp = (int(X) + 1) // 2 * 2
    vectors = (5 * int(n_vars) + 2) * Xp
    ints = 4 * ((int(P) + int(U) + 16 + 3) // 4 * 4)
    per = 2 + int(n_vars) * int(X) + int(P) * int(X) * int(X)
    if which == KERNEL_X64:
        per *= 4
    elif vectors * 8 + 64 + ints > _cutset.GENERIC_LDS_BYTES:
        per += vectors
    return int(B) * n_chunks * per * 8


check_plan, Plan, plan = _cutset.plan_functions(__name__)
