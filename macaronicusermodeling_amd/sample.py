"""ctypes binding of libmlbp_sample.so (include/mlbp_sample.h): posterior sampling of whole assignments.

The fourth library of the engine, with its own signature table (`_ffi.SIGNATURES` mirrors mlbp.h alone).  There is no
CPU fallback: a compute call on a machine without an MI355X returns MLBP_ENODEVICE, raised as SampleError.

`program(topo, roots, device)` compiles a root sequence with `GraphTopology.compile_program` -- the very op list the
sum-product sweeps run -- derives `slot_var` (the source variable of every variable->factor slot) from the topology, has
the library validate both on the host, uploads (ops, srcs, sweeps, slot_var) and the read-out arrays once, and caches the
device copies per (topology, roots, device).  The drawing order is an argument of a call, not of the program:
`SampleProgram.order(var_ids)` validates and caches its device copy.
"""
import ctypes as C

import numpy as np

from . import _ffi, _sidelib
from ._sidelib import i32 as _i32, i32p as _i32p

LIB_PATH = _sidelib.lib_path('mlbp_sample')

KERNEL_NONE, KERNEL_X64, KERNEL_GENERIC = 0, 1, 2
X64_LDS_BYTES = 81920           # include/mlbp_sample.h MLBP_SAMPLE_X64_LDS_BYTES
MAX_X = 1024
MIN_WORKGROUPS = 512


class SampleError(_sidelib.SideError):
    LIB = 'libmlbp_sample'


class SampleArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('X', C.c_int32), ('n_msgs', C.c_int32), ('P', C.c_int32), ('U', C.c_int32), ('n_vars', C.c_int32),
                ('n_ops', C.c_int32), ('n_srcs', C.c_int32), ('n_sweeps', C.c_int32),
                ('n_pair_tables', C.c_int32), ('n_unary_tables', C.c_int32),
                ('normalize_messages', C.c_int32), ('S', C.c_int32),
                ('ops', C.c_void_p), ('srcs', C.c_void_p), ('sweeps', C.c_void_p),
                ('pair_tables', C.c_void_p), ('pair_tab', C.c_void_p), ('unary_tables', C.c_void_p), ('unary_tab', C.c_void_p),
                ('in_off', C.c_void_p), ('in_slots', C.c_void_p), ('slot_var', C.c_void_p), ('order', C.c_void_p),
                ('uniforms', C.c_void_p), ('given', C.c_void_p),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_int64),
                ('samples', C.c_void_p), ('logq', C.c_void_p), ('cond_marginals', C.c_void_p)]


# name -> (restype, argtypes); mirrors include/mlbp_sample.h one to one (tests/test_side_libraries_cpu.py checks that).
SIGNATURES = {
    'mlbp_sample_f64': (C.c_int, [C.POINTER(SampleArgs), C.c_void_p]),
    'mlbp_sample_check_program': (C.c_int, [_i32p, _i32, _i32p, _i32, _i32p, _i32, _i32, _i32, _i32, _i32, _i32p, _i32p]),
    'mlbp_sample_check_readout': (C.c_int, [_i32, _i32p, _i32p, _i32]),
    'mlbp_sample_pick_kernel': (C.c_int, [_i32, _i32, _i32]),
    'mlbp_sample_chunks': (C.c_int, [_i32, _i32]),
    'mlbp_sample_workspace_bytes': (C.c_int64, [_i32, _i32, _i32, _i32, _i32]),
    'mlbp_sample_last_kernel': (C.c_int, []),
    'mlbp_sample_arch': (C.c_char_p, []),
    'mlbp_sample_last_error': (C.c_char_p, []),
}

lib = _sidelib.load(LIB_PATH, SIGNATURES)
last_error, check, last_kernel, pick_kernel = _sidelib.status_helpers(lib, SampleError)


def chunks(B, S):
    """C of the launch grid (B, C): workgroup (g, c) draws samples c, c + C, ... of graph g."""
    return check(lib.mlbp_sample_chunks(int(B), int(S)))


def workspace_bytes(B, S, X, n_msgs, n_vars):
    return check(lib.mlbp_sample_workspace_bytes(int(B), int(S), int(X), int(n_msgs), int(n_vars)))


def slot_var_array(topo):
    """int32 [n_msgs]: the source variable (index in var_ids order) of every variable->factor slot, -1 for a factor->variable
    slot -- from topo.v2f and topo.fac_var."""
    sv = np.full(topo.n_msgs, -1, dtype=np.int32)
    for j in range(topo.n_factors):
        for k in range(int(topo.fac_nvars[j])):
            if topo.v2f[2 * j + k] >= 0:
                sv[topo.v2f[2 * j + k]] = topo.fac_var[2 * j + k]
    return sv


class SampleProgram(_sidelib.Program):
    """Validated device copies of one root sequence's (ops, srcs, sweeps), of slot_var and of the topology's read-out arrays."""

    def check_host(self):
        self._slot_var_h = slot_var_array(self.topo)
        self._orders = {}
        check(lib.mlbp_sample_check_readout(*self.in_slot_args()))
        self.order(None)                                           # validates the program, with the default order

    def upload(self):
        self.slot_var = self._up(self._slot_var_h)

    def order(self, var_ids):
        """Device int32 [n_vars] of a drawing order given as variable ids (None: var_ids order), validated and cached."""
        topo = self.topo
        key = None if var_ids is None else tuple(int(v) for v in var_ids)
        if key not in self._orders:
            if key is None:
                idx = np.arange(topo.n_vars, dtype=np.int32)
            else:
                unknown = [v for v in key if v not in topo.var_index]
                if unknown:
                    raise ValueError('order names unknown variable ids %r' % (unknown,))
                idx = np.array([topo.var_index[v] for v in key], dtype=np.int32)
                if len(idx) != topo.n_vars:
                    raise ValueError('order must list every variable once (%d ids, %d variables)' % (len(idx), topo.n_vars))
            check(lib.mlbp_sample_check_program(*self.program_args(), topo.n_vars, _ffi.i32ptr(self._slot_var_h), _ffi.i32ptr(idx)))
            if len(self._orders) >= 64:
                self._orders.clear()
            self._orders[key] = self._up(idx)
        return self._orders[key]


_programs = _sidelib.Cache()


def program(topo, roots, device):
    """The cached SampleProgram of (topology, roots, device)."""
    return _programs.program(SampleProgram, topo, roots, device)
