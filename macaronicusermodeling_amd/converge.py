"""ctypes binding of libmlbp_converge.so (include/mlbp_converge.h): sum-product sweeps run to convergence.

The fifth library of the engine, with its own signature table (`_ffi.SIGNATURES` mirrors mlbp.h alone).  There is no
CPU fallback: a compute call on a machine without an MI355X returns MLBP_ENODEVICE, raised as ConvergeError.

`program(topo, roots, device)` compiles a root sequence with `GraphTopology.compile_program` -- the very op list the
sum-product sweeps run; here it is one ROUND -- has the library validate it on the host (index ranges, and that every
message slot is the destination of some op of the round), uploads (ops, srcs, sweeps) and the read-out arrays once, and
caches the device copies per (topology, roots, device).
"""
import ctypes as C

import numpy as np

from . import _ffi, _sidelib
from ._sidelib import i32 as _i32, i32p as _i32p

LIB_PATH = _sidelib.lib_path('mlbp_converge')

KERNEL_NONE, KERNEL_X64, KERNEL_GENERIC = 0, 1, 2
X64_LDS_BYTES = 81920           # include/mlbp_converge.h MLBP_CONVERGE_X64_LDS_BYTES
MAX_X = 1024
MAX_ROUNDS = 65535


class ConvergeError(_sidelib.SideError):
    LIB = 'libmlbp_converge'


class ConvergeArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('X', C.c_int32), ('n_msgs', C.c_int32), ('P', C.c_int32), ('U', C.c_int32), ('n_vars', C.c_int32),
                ('n_ops', C.c_int32), ('n_srcs', C.c_int32), ('n_sweeps', C.c_int32),
                ('n_pair_tables', C.c_int32), ('n_unary_tables', C.c_int32),
                ('normalize_messages', C.c_int32), ('init_messages', C.c_int32), ('max_rounds', C.c_int32),
                ('tol', C.c_double),
                ('ops', C.c_void_p), ('srcs', C.c_void_p), ('sweeps', C.c_void_p),
                ('pair_tables', C.c_void_p), ('pair_tab', C.c_void_p), ('unary_tables', C.c_void_p), ('unary_tab', C.c_void_p),
                ('in_off', C.c_void_p), ('in_slots', C.c_void_p),
                ('msgs', C.c_void_p), ('rounds', C.c_void_p), ('residual', C.c_void_p),
                ('marginals', C.c_void_p), ('history', C.c_void_p),
                ('max_product', C.c_int32), ('assignment', C.c_void_p), ('score', C.c_void_p),
                ('pair_axis_var', C.c_void_p), ('unary_var', C.c_void_p)]


# name -> (restype, argtypes); mirrors include/mlbp_converge.h one to one (tests/test_side_libraries_cpu.py checks that).
SIGNATURES = {
    'mlbp_converge_f64': (C.c_int, [C.POINTER(ConvergeArgs), C.c_void_p]),
    'mlbp_converge_check_program': (C.c_int, [_i32p, _i32, _i32p, _i32, _i32p, _i32, _i32, _i32, _i32]),
    'mlbp_converge_check_readout': (C.c_int, [_i32, _i32p, _i32p, _i32]),
    'mlbp_converge_pick_kernel': (C.c_int, [_i32, _i32, _i32]),
    'mlbp_converge_last_kernel': (C.c_int, []),
    'mlbp_converge_arch': (C.c_char_p, []),
    'mlbp_converge_last_error': (C.c_char_p, []),
}

lib = _sidelib.load(LIB_PATH, SIGNATURES)
last_error, check, last_kernel, pick_kernel = _sidelib.status_helpers(lib, ConvergeError)


def check_program(ops, srcs, sweeps, n_msgs, P, U):
    """mlbp_converge_check_program on host arrays: the status code (a negative one leaves its message in last_error())."""
    o, s, w = _sidelib.host_i32(ops), _sidelib.host_i32(srcs), _sidelib.host_i32(sweeps)
    s_arg = s if len(s) else np.zeros(1, dtype=np.int32)
    return lib.mlbp_converge_check_program(_ffi.i32ptr(o), len(o) // 4, _ffi.i32ptr(s_arg), len(s), _ffi.i32ptr(w), len(w) // 2,
                                           int(n_msgs), int(P), int(U))


def decode_arrays(topo):
    """(pair_axis_var [P][2], unary_var [U]) int32, what the max-product mode's decode reads: the variable index on table axis
    0 / 1 of every pairwise factor (fac_dim) and the variable of every unary factor, in pair-slot / unary-slot order."""
    pav = np.zeros((max(topo.P, 1), 2), dtype=np.int32)
    for p, j in enumerate(topo.pair_factors):
        for k in range(2):
            pav[p, topo.fac_dim[2 * j + k]] = topo.fac_var[2 * j + k]
    uv = np.zeros(max(topo.U, 1), dtype=np.int32)
    for u, j in enumerate(topo.unary_factors):
        uv[u] = topo.fac_var[2 * j]
    return pav, uv


class ConvergeProgram(_sidelib.Program):
    """Validated device copies of one root sequence's (ops, srcs, sweeps) -- one round -- and of the topology's read-out arrays,
    the decode's among them."""

    def __init__(self, topo, roots, device):
        roots = tuple(int(r) for r in roots)
        unknown = [r for r in roots if r not in topo.var_index]
        if unknown or not roots:
            raise ValueError('roots must name variables of the graph (unknown: %r)' % (unknown,))
        _sidelib.Program.__init__(self, topo, roots, device)

    def check_host(self):
        check(lib.mlbp_converge_check_program(*self.program_args()))
        check(lib.mlbp_converge_check_readout(*self.in_slot_args()))
        pav, uv = decode_arrays(self.topo)
        self._pav_h, self._uv_h = _sidelib.host_i32(pav), uv

    def upload(self):
        self.pair_axis_var, self.unary_var = self._up(self._pav_h), self._up(self._uv_h)


_programs = _sidelib.Cache()


def program(topo, roots, device):
    """The cached ConvergeProgram of (topology, roots, device)."""
    return _programs.program(ConvergeProgram, topo, roots, device)
