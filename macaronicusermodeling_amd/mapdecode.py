"""ctypes binding of libmlbp_map.so (include/mlbp_map.h): max-product sweeps and MAP decoding.

The second library of the engine, with its own signature table (`_ffi.SIGNATURES` mirrors mlbp.h alone).  There is no
CPU fallback: a compute call on a machine without an MI355X returns MLBP_ENODEVICE, raised as MapError.

`program(topo, roots, device)` compiles a root sequence with `GraphTopology.compile_program` -- the very op list the
sum-product sweeps run -- has the library validate it on the host, uploads (ops, srcs, sweeps) and the read-out arrays
once, and caches the device copies per (topology, roots, device).
"""
import ctypes as C

import numpy as np

from . import _ffi, _sidelib
from ._sidelib import i32 as _i32, i32p as _i32p

LIB_PATH = _sidelib.lib_path('mlbp_map')

KERNEL_NONE, KERNEL_X64, KERNEL_GENERIC = 0, 1, 2
X64_LDS_BYTES = 81920           # include/mlbp_map.h MLBP_MAP_X64_LDS_BYTES
MAX_X = 1024


class MapError(_sidelib.SideError):
    LIB = 'libmlbp_map'


class MapArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('X', C.c_int32), ('n_msgs', C.c_int32), ('P', C.c_int32), ('U', C.c_int32), ('n_vars', C.c_int32),
                ('n_ops', C.c_int32), ('n_srcs', C.c_int32), ('n_sweeps', C.c_int32),
                ('n_pair_tables', C.c_int32), ('n_unary_tables', C.c_int32),
                ('init_messages', C.c_int32), ('normalize_messages', C.c_int32), ('write_messages', C.c_int32),
                ('ops', C.c_void_p), ('srcs', C.c_void_p), ('sweeps', C.c_void_p),
                ('pair_tables', C.c_void_p), ('pair_tab', C.c_void_p), ('unary_tables', C.c_void_p), ('unary_tab', C.c_void_p),
                ('msgs', C.c_void_p), ('in_off', C.c_void_p), ('in_slots', C.c_void_p),
                ('pair_axis_var', C.c_void_p), ('unary_var', C.c_void_p),
                ('max_marginals', C.c_void_p), ('assignment', C.c_void_p), ('score', C.c_void_p)]


# name -> (restype, argtypes); mirrors include/mlbp_map.h one to one (tests/test_side_libraries_cpu.py checks that).
SIGNATURES = {
    'mlbp_map_sweep_f64': (C.c_int, [C.POINTER(MapArgs), C.c_void_p]),
    'mlbp_map_check_program': (C.c_int, [_i32p, _i32, _i32p, _i32, _i32p, _i32, _i32, _i32, _i32]),
    'mlbp_map_check_readout': (C.c_int, [_i32, _i32p, _i32p, _i32, _i32, _i32p, _i32, _i32p]),
    'mlbp_map_pick_kernel': (C.c_int, [_i32, _i32, _i32]),
    'mlbp_map_last_kernel': (C.c_int, []),
    'mlbp_map_arch': (C.c_char_p, []),
    'mlbp_map_last_error': (C.c_char_p, []),
}

lib = _sidelib.load(LIB_PATH, SIGNATURES)
last_error, check, last_kernel, pick_kernel = _sidelib.status_helpers(lib, MapError)


def readout_arrays(topo):
    """(pair_axis_var [P][2], unary_var [U]) int32: the variable index on table axis 0 / 1 of every pairwise factor (fac_dim)
    and the variable of every unary factor, in pair-slot / unary-slot order."""
    pav = np.zeros((max(topo.P, 1), 2), dtype=np.int32)
    for p, j in enumerate(topo.pair_factors):
        for k in range(2):
            pav[p, topo.fac_dim[2 * j + k]] = topo.fac_var[2 * j + k]
    uv = np.zeros(max(topo.U, 1), dtype=np.int32)
    for u, j in enumerate(topo.unary_factors):
        uv[u] = topo.fac_var[2 * j]
    return pav, uv


class MapProgram(_sidelib.Program):
    """Validated device copies of one root sequence's (ops, srcs, sweeps) and of the topology's read-out arrays."""

    def check_host(self):
        topo = self.topo
        pav, uv = readout_arrays(topo)
        self._pav_h, self._uv_h = _sidelib.host_i32(pav), uv
        check(lib.mlbp_map_check_program(*self.program_args()))
        check(lib.mlbp_map_check_readout(*self.in_slot_args(), topo.P, _ffi.i32ptr(self._pav_h), topo.U, _ffi.i32ptr(uv)))

    def upload(self):
        self.pair_axis_var, self.unary_var = self._up(self._pav_h), self._up(self._uv_h)


_programs = _sidelib.Cache()


def program(topo, roots, device):
    """The cached MapProgram of (topology, roots, device)."""
    return _programs.program(MapProgram, topo, roots, device)
