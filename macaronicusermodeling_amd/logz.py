"""ctypes binding of libmlbp_logz.so (include/mlbp_logz.h): log Z and the joint log-likelihood of batched factor graphs.

The third library of the engine, with its own signature table (`_ffi.SIGNATURES` mirrors mlbp.h alone, `mapdecode.SIGNATURES`
mlbp_map.h).  There is no CPU fallback: the compute call on a machine without an MI355X returns MLBP_ENODEVICE, raised as
LogzError.

`readout(topo, device)` derives the read-out arrays of a topology -- each variable's in-slots, the variable on either table
axis of every pairwise factor, and the factor->variable slot of every (factor, variable) incidence (GraphTopology.f2v) -- has
the library validate them on the host, uploads them once and caches the device copies per (topology, device).
"""
import ctypes as C

import numpy as np

from . import _ffi, _sidelib
from ._sidelib import i32 as _i32, i32p as _i32p

LIB_PATH = _sidelib.lib_path('mlbp_logz')

KERNEL_NONE, KERNEL_X64, KERNEL_X64_SHARED, KERNEL_GENERIC = 0, 1, 2, 3
X64_LDS_BYTES = 65536           # include/mlbp_logz.h MLBP_LOGZ_X64_LDS_BYTES
MAX_X = 1024
GROUP = 16                      # graphs per workgroup of the shared-table kernel
SHARED_PAIR_TABLES = 1          # MLBP_LOGZ_SHARED_PAIR_TABLES


class LogzError(_sidelib.SideError):
    LIB = 'libmlbp_logz'


class LogzArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('X', C.c_int32), ('n_msgs', C.c_int32), ('P', C.c_int32), ('U', C.c_int32), ('n_vars', C.c_int32),
                ('n_pair_tables', C.c_int32), ('n_unary_tables', C.c_int32), ('flags', C.c_int32),
                ('pair_tables', C.c_void_p), ('pair_tab', C.c_void_p), ('unary_tables', C.c_void_p), ('unary_tab', C.c_void_p),
                ('msgs', C.c_void_p), ('in_off', C.c_void_p), ('in_slots', C.c_void_p),
                ('pair_axis_var', C.c_void_p), ('unary_var', C.c_void_p), ('pair_in_slot', C.c_void_p), ('unary_in_slot', C.c_void_p),
                ('labels', C.c_void_p), ('log_z', C.c_void_p), ('score', C.c_void_p), ('joint_logp', C.c_void_p), ('sum_out', C.c_void_p)]


# name -> (restype, argtypes); mirrors include/mlbp_logz.h one to one (tests/test_side_libraries_cpu.py checks that).
SIGNATURES = {
    'mlbp_logz_f64': (C.c_int, [C.POINTER(LogzArgs), C.c_void_p]),
    'mlbp_logz_check_readout': (C.c_int, [_i32, _i32p, _i32p, _i32, _i32, _i32p, _i32p, _i32, _i32p, _i32p]),
    'mlbp_logz_pick_kernel': (C.c_int, [_i32, _i32, _i32, _i32]),
    'mlbp_logz_last_kernel': (C.c_int, []),
    'mlbp_logz_arch': (C.c_char_p, []),
    'mlbp_logz_last_error': (C.c_char_p, []),
}

lib = _sidelib.load(LIB_PATH, SIGNATURES)
last_error, check, last_kernel, _pick_kernel = _sidelib.status_helpers(lib, LogzError)


def pick_kernel(X, n_in_slots, n_vars, flags=0):
    return _pick_kernel(X, n_in_slots, n_vars, flags)


def readout_arrays(topo):
    """(pair_axis_var [P][2], unary_var [U], pair_in_slot [P][2], unary_in_slot [U]) int32, in pair-slot / unary-slot order:
    the variable on table axis 0 / 1 of every pairwise factor (fac_dim) and the slot of the factor's message to it (f2v); the
    variable of every unary factor and the slot of its message."""
    pav = np.zeros((max(topo.P, 1), 2), dtype=np.int32)
    pis = np.zeros((max(topo.P, 1), 2), dtype=np.int32)
    for p, j in enumerate(topo.pair_factors):
        for k in range(2):
            axis = topo.fac_dim[2 * j + k]
            pav[p, axis] = topo.fac_var[2 * j + k]
            pis[p, axis] = topo.f2v[2 * j + k]
    uv = np.zeros(max(topo.U, 1), dtype=np.int32)
    uis = np.zeros(max(topo.U, 1), dtype=np.int32)
    for u, j in enumerate(topo.unary_factors):
        uv[u] = topo.fac_var[2 * j]
        uis[u] = topo.f2v[2 * j]
    return pav, uv, pis, uis


class Readout:
    """Validated device copies of one topology's read-out arrays."""

    def __init__(self, topo, device):
        import torch
        pav, uv, pis, uis = readout_arrays(topo)
        in_off = np.ascontiguousarray(topo.in_off, dtype=np.int32)
        in_slots = np.ascontiguousarray(topo.in_slots, dtype=np.int32)
        self.n_in_slots = int(in_off[-1])
        check(lib.mlbp_logz_check_readout(topo.n_vars, _ffi.i32ptr(in_off), _ffi.i32ptr(in_slots), topo.n_msgs, topo.P,
                                          _ffi.i32ptr(pav.reshape(-1)), _ffi.i32ptr(pis.reshape(-1)), topo.U, _ffi.i32ptr(uv),
                                          _ffi.i32ptr(uis)))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a.reshape(-1))).to(device)          # noqa: E731
        self.in_off, self.in_slots = up(in_off), up(in_slots)
        self.pair_axis_var, self.unary_var, self.pair_in_slot, self.unary_in_slot = up(pav), up(uv), up(pis), up(uis)


_readouts = _sidelib.Cache()


def readout(topo, device):
    """The cached Readout of (topology, device)."""
    return _readouts.get(topo, (str(device),), lambda: Readout(topo, device))
