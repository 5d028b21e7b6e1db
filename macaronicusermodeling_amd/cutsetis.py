"""ctypes binding of libmlbp_cutsetis.so (include/mlbp_cutsetis.h): an estimate of log Z and of the marginals by cutset
importance sampling, for the graphs whose cutset has more configurations than the exact libraries sum.

The eleventh library of the engine, with its own signature table.  There is no CPU fallback: the compute call on a machine
without an MI355X returns MLBP_ENODEVICE, raised as CutsetisError.

The call takes the packed plan of include/mlbp_cutset.h: `plan(topo, cutset, X, device)` derives it with cutset.choose /
cutset.plan_words, has THIS library validate it on the host -- no bound on X^|C|, at most MAX_CUT cutset variables -- uploads
it once and caches the device copy.
"""
import ctypes as C

from . import _sidelib
from . import cutset as _cutset
from ._sidelib import i32 as _i32, i32p as _i32p

LIB_PATH = _sidelib.lib_path('mlbp_cutsetis')

KERNEL_NONE, KERNEL_X64, KERNEL_GENERIC = 0, 1, 2
MAX_LISTED = 65536              # include/mlbp_cutsetis.h MLBP_CUTSETIS_MAX_LISTED
MAX_CUT = 16                    # MLBP_CUTSETIS_MAX_CUT
MIN_WORKGROUPS = 512            # MLBP_CUTSETIS_MIN_WORKGROUPS
MAX_ABS_LOG_Q = 1.0e6           # MLBP_CUTSETIS_MAX_ABS_LOG_Q


class CutsetisError(_sidelib.SideError):
    LIB = 'libmlbp_cutsetis'


class CutsetisArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('X', C.c_int32), ('n_vars', C.c_int32), ('P', C.c_int32), ('U', C.c_int32),
                ('n_cut', C.c_int32), ('n_free', C.c_int32), ('n_items', C.c_int32), ('n_consts', C.c_int32), ('n_forest', C.c_int32),
                ('n_pair_tables', C.c_int32), ('n_unary_tables', C.c_int32),
                ('plan_words', C.c_int32),
                ('N', C.c_int32),
                ('plan', C.c_void_p),
                ('pair_tables', C.c_void_p), ('pair_tab', C.c_void_p), ('unary_tables', C.c_void_p), ('unary_tab', C.c_void_p),
                ('configs', C.c_void_p), ('log_q', C.c_void_p),
                ('labels', C.c_void_p),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_int64),
                ('log_z_hat', C.c_void_p), ('marginals', C.c_void_p), ('ess', C.c_void_p), ('log_w', C.c_void_p),
                ('score', C.c_void_p), ('joint_logp', C.c_void_p)]


# name -> (restype, argtypes); mirrors include/mlbp_cutsetis.h one to one (tests/test_side_libraries_cpu.py checks that).
SIGNATURES = {
    'mlbp_cutsetis_f64': (C.c_int, [C.POINTER(CutsetisArgs), C.c_void_p]),
    'mlbp_cutsetis_check_plan': (C.c_int, [_i32p, _i32, _i32]),
    'mlbp_cutsetis_pick_kernel': (C.c_int, [_i32, _i32, _i32, _i32, _i32]),
    'mlbp_cutsetis_chunks': (C.c_int, [_i32, _i32]),
    'mlbp_cutsetis_workspace_bytes': (C.c_int64, [_i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    'mlbp_cutsetis_last_kernel': (C.c_int, []),
    'mlbp_cutsetis_arch': (C.c_char_p, []),
    'mlbp_cutsetis_last_error': (C.c_char_p, []),
}

lib = _sidelib.load(LIB_PATH, SIGNATURES)
last_error, check, last_kernel, pick_kernel = _sidelib.status_helpers(lib, CutsetisError)


def chunks(B, N):
    """min(N, ceil(512 / B)): C of the launch grid (B, C); workgroup (g, k) walks list entries k, k + C, ... of graph g."""
    return check(lib.mlbp_cutsetis_chunks(int(B), int(N)))


def workspace_bytes(B, X, n_vars, P, U, n_forest, N):
    return check(lib.mlbp_cutsetis_workspace_bytes(int(B), int(X), int(n_vars), int(P), int(U), int(n_forest), int(N)))


check_plan, Plan, plan = _cutset.plan_functions(__name__)
