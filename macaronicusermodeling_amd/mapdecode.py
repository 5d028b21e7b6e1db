"""ctypes binding of libmlbp_map.so (include/mlbp_map.h): max-product sweeps and MAP decoding.

The second library of the engine, with its own signature table (`_ffi.SIGNATURES` mirrors mlbp.h alone).  There is no
CPU fallback: a compute call on a machine without an MI355X returns MLBP_ENODEVICE, raised as MapError.

`program(topo, roots, device)` compiles a root sequence with `GraphTopology.compile_program` -- the very op list the
sum-product sweeps run -- has the library validate it on the host, uploads (ops, srcs, sweeps) and the read-out arrays
once, and caches the device copies per (topology, roots, device).
"""
import ctypes as C
import os
import threading

import numpy as np

from . import _ffi

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, 'libmlbp_map.so')

KERNEL_NONE, KERNEL_X64, KERNEL_GENERIC = 0, 1, 2
X64_LDS_BYTES = 81920           # include/mlbp_map.h MLBP_MAP_X64_LDS_BYTES
MAX_X = 1024


class MapError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, 'libmlbp_map error %d: %s' % (code, msg))
        self.code = code


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


_i32p = C.POINTER(C.c_int32)
_i32 = C.c_int32

# name -> (restype, argtypes); mirrors include/mlbp_map.h one to one (tests/test_map_cpu.py checks that).
SIGNATURES = {
    'mlbp_map_sweep_f64': (C.c_int, [C.POINTER(MapArgs), C.c_void_p]),
    'mlbp_map_check_program': (C.c_int, [_i32p, _i32, _i32p, _i32, _i32p, _i32, _i32, _i32, _i32]),
    'mlbp_map_check_readout': (C.c_int, [_i32, _i32p, _i32p, _i32, _i32, _i32p, _i32, _i32p]),
    'mlbp_map_pick_kernel': (C.c_int, [_i32, _i32, _i32]),
    'mlbp_map_last_kernel': (C.c_int, []),
    'mlbp_map_arch': (C.c_char_p, []),
    'mlbp_map_last_error': (C.c_char_p, []),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            'libmlbp_map.so not found at %s.  Build it with `python -m macaronicusermodeling_amd.build` '
            '(hipcc, gfx950).  There is no CPU fallback.' % LIB_PATH)
    import torch  # noqa: F401      (torch's HIP runtime must be the one mapped first: see _ffi._load)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header / library mismatch
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def last_error():
    return lib.mlbp_map_last_error().decode('utf-8', 'replace')


def check(rc):
    """Raises MapError for negative return codes; returns rc otherwise."""
    if rc < 0:
        raise MapError(rc, last_error())
    return rc


def last_kernel():
    """KERNEL_X64 / KERNEL_GENERIC: the kernel the calling thread's last map sweep enqueued (host-side record)."""
    return lib.mlbp_map_last_kernel()


def pick_kernel(X, n_msgs, n_vars):
    return check(lib.mlbp_map_pick_kernel(int(X), int(n_msgs), int(n_vars)))


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


class MapProgram:
    """Validated device copies of one root sequence's (ops, srcs, sweeps) and of the topology's read-out arrays."""

    def __init__(self, topo, roots, device):
        import torch
        self.roots = tuple(int(r) for r in roots)
        ops, srcs, sweeps = topo.compile_program(self.roots)
        ops = np.ascontiguousarray(ops.reshape(-1), dtype=np.int32)
        srcs_h = np.ascontiguousarray(srcs if len(srcs) else np.zeros(1), dtype=np.int32)
        sweeps = np.ascontiguousarray(sweeps.reshape(-1), dtype=np.int32)
        self.n_ops, self.n_srcs, self.n_sweeps = len(ops) // 4, len(srcs), len(sweeps) // 2
        check(lib.mlbp_map_check_program(_ffi.i32ptr(ops), self.n_ops, _ffi.i32ptr(srcs_h), self.n_srcs, _ffi.i32ptr(sweeps),
                                         self.n_sweeps, topo.n_msgs, topo.P, topo.U))
        pav, uv = readout_arrays(topo)
        in_off = np.ascontiguousarray(topo.in_off, dtype=np.int32)
        in_slots = np.ascontiguousarray(topo.in_slots, dtype=np.int32)
        check(lib.mlbp_map_check_readout(topo.n_vars, _ffi.i32ptr(in_off), _ffi.i32ptr(in_slots), topo.n_msgs, topo.P,
                                         _ffi.i32ptr(pav.reshape(-1)), topo.U, _ffi.i32ptr(uv)))
        up = lambda a: torch.from_numpy(a).to(device)          # noqa: E731
        self.ops, self.srcs, self.sweeps = up(ops), up(srcs_h), up(sweeps)
        self.in_off, self.in_slots = up(in_off), up(in_slots)
        self.pair_axis_var, self.unary_var = up(pav.reshape(-1).copy()), up(uv)


_programs = {}
_programs_lock = threading.Lock()
_PROGRAMS_MAX = 4096


def program(topo, roots, device):
    """The cached MapProgram of (topology, roots, device).  The topology is held by the cache entry, so its id stays its own."""
    key = (id(topo), tuple(int(r) for r in roots), str(device))
    with _programs_lock:
        hit = _programs.get(key)
        if hit is None:
            if len(_programs) >= _PROGRAMS_MAX:
                _programs.clear()
            hit = _programs[key] = (topo, MapProgram(topo, roots, device))
    return hit[1]
