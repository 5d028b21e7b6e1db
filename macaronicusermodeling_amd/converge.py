"""ctypes binding of libmlbp_converge.so (include/mlbp_converge.h): sum-product sweeps run to convergence.

The fifth library of the engine, with its own signature table (`_ffi.SIGNATURES` mirrors mlbp.h alone).  There is no
CPU fallback: a compute call on a machine without an MI355X returns MLBP_ENODEVICE, raised as ConvergeError.

`program(topo, roots, device)` compiles a root sequence with `GraphTopology.compile_program` -- the very op list the
sum-product sweeps run; here it is one ROUND -- has the library validate it on the host (index ranges, and that every
message slot is the destination of some op of the round), uploads (ops, srcs, sweeps) and the read-out arrays once, and
caches the device copies per (topology, roots, device).
"""
import ctypes as C
import os
import threading

import numpy as np

from . import _ffi

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, 'libmlbp_converge.so')

KERNEL_NONE, KERNEL_X64, KERNEL_GENERIC = 0, 1, 2
X64_LDS_BYTES = 81920           # include/mlbp_converge.h MLBP_CONVERGE_X64_LDS_BYTES
MAX_X = 1024
MAX_ROUNDS = 65535


class ConvergeError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, 'libmlbp_converge error %d: %s' % (code, msg))
        self.code = code


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
                ('marginals', C.c_void_p), ('history', C.c_void_p)]


_i32p = C.POINTER(C.c_int32)
_i32 = C.c_int32

# name -> (restype, argtypes); mirrors include/mlbp_converge.h one to one (tests/test_converge_cpu.py checks that).
SIGNATURES = {
    'mlbp_converge_f64': (C.c_int, [C.POINTER(ConvergeArgs), C.c_void_p]),
    'mlbp_converge_check_program': (C.c_int, [_i32p, _i32, _i32p, _i32, _i32p, _i32, _i32, _i32, _i32]),
    'mlbp_converge_check_readout': (C.c_int, [_i32, _i32p, _i32p, _i32]),
    'mlbp_converge_pick_kernel': (C.c_int, [_i32, _i32, _i32]),
    'mlbp_converge_last_kernel': (C.c_int, []),
    'mlbp_converge_arch': (C.c_char_p, []),
    'mlbp_converge_last_error': (C.c_char_p, []),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            'libmlbp_converge.so not found at %s.  Build it with `python -m macaronicusermodeling_amd.build` '
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
    return lib.mlbp_converge_last_error().decode('utf-8', 'replace')


def check(rc):
    """Raises ConvergeError for negative return codes; returns rc otherwise."""
    if rc < 0:
        raise ConvergeError(rc, last_error())
    return rc


def last_kernel():
    """KERNEL_X64 / KERNEL_GENERIC: the kernel the calling thread's last converge call enqueued (host-side record)."""
    return lib.mlbp_converge_last_kernel()


def pick_kernel(X, n_msgs, n_vars):
    return check(lib.mlbp_converge_pick_kernel(int(X), int(n_msgs), int(n_vars)))


def check_program(ops, srcs, sweeps, n_msgs, P, U):
    """mlbp_converge_check_program on host arrays: the status code (a negative one leaves its message in last_error())."""
    o = np.ascontiguousarray(np.asarray(ops, dtype=np.int32).reshape(-1))
    s = np.ascontiguousarray(np.asarray(srcs, dtype=np.int32).reshape(-1))
    w = np.ascontiguousarray(np.asarray(sweeps, dtype=np.int32).reshape(-1))
    s_arg = s if len(s) else np.zeros(1, dtype=np.int32)
    return lib.mlbp_converge_check_program(_ffi.i32ptr(o), len(o) // 4, _ffi.i32ptr(s_arg), len(s), _ffi.i32ptr(w), len(w) // 2,
                                           int(n_msgs), int(P), int(U))


class ConvergeProgram:
    """Validated device copies of one root sequence's (ops, srcs, sweeps) -- one round -- and of the topology's read-out arrays."""

    def __init__(self, topo, roots, device):
        import torch
        self.topo, self.device = topo, device
        self.roots = tuple(int(r) for r in roots)
        unknown = [r for r in self.roots if r not in topo.var_index]
        if unknown or not self.roots:
            raise ValueError('roots must name variables of the graph (unknown: %r)' % (unknown,))
        ops, srcs, sweeps = topo.compile_program(self.roots)
        ops_h = np.ascontiguousarray(ops.reshape(-1), dtype=np.int32)
        srcs_h = np.ascontiguousarray(srcs if len(srcs) else np.zeros(1), dtype=np.int32)
        sweeps_h = np.ascontiguousarray(sweeps.reshape(-1), dtype=np.int32)
        self.n_ops, self.n_srcs, self.n_sweeps = len(ops_h) // 4, len(srcs), len(sweeps_h) // 2
        check(check_program(ops_h, srcs, sweeps_h, topo.n_msgs, topo.P, topo.U))
        in_off = np.ascontiguousarray(topo.in_off, dtype=np.int32)
        in_slots = np.ascontiguousarray(topo.in_slots, dtype=np.int32)
        check(lib.mlbp_converge_check_readout(topo.n_vars, _ffi.i32ptr(in_off), _ffi.i32ptr(in_slots), topo.n_msgs))
        up = lambda a: torch.from_numpy(a).to(device)          # noqa: E731
        self.ops, self.srcs, self.sweeps = up(ops_h), up(srcs_h), up(sweeps_h)
        self.in_off, self.in_slots = up(in_off), up(in_slots)


_programs = {}
_programs_lock = threading.Lock()
_PROGRAMS_MAX = 4096


def program(topo, roots, device):
    """The cached ConvergeProgram of (topology, roots, device).  The topology is held by the cache entry, so its id stays its own."""
    key = (id(topo), tuple(int(r) for r in roots), str(device))
    with _programs_lock:
        hit = _programs.get(key)
        if hit is None:
            if len(_programs) >= _PROGRAMS_MAX:
                _programs.clear()
            hit = _programs[key] = (topo, ConvergeProgram(topo, roots, device))
    return hit[1]
