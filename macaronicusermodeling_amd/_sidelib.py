"""What the ctypes bindings of the side libraries share (the binding modules of build.SIDE_LIBRARIES): loading a library
against its signature table, its error class and status helpers, the per-topology cache of device copies, and the base of the
`*Program` classes.  Each binding keeps its own SIGNATURES, constants and args struct: they mirror its header.
"""
import ctypes as C
import os
import threading

import numpy as np

from . import _ffi

_PKG = os.path.dirname(os.path.abspath(__file__))

i32p = C.POINTER(C.c_int32)
i32 = C.c_int32


def lib_path(name):
    return os.path.join(_PKG, 'lib%s.so' % name)


def load(path, signatures):
    if not os.path.exists(path):
        raise ImportError(
            '%s not found at %s.  Build it with `python -m macaronicusermodeling_amd.build` '
            '(hipcc, gfx950).  There is no CPU fallback.' % (os.path.basename(path), path))
    import torch  # noqa: F401      (torch's HIP runtime must be the one mapped first: see _ffi._load)
    lib = C.CDLL(path)
    for name, (res, args) in signatures.items():
        fn = getattr(lib, name)          # AttributeError here = header / library mismatch
        fn.restype = res
        fn.argtypes = args
    return lib


class SideError(RuntimeError):
    """Base of the one error class of every binding of build.SIDE_LIBRARIES; LIB is the library's name without its suffix."""
    LIB = None

    def __init__(self, code, msg):
        RuntimeError.__init__(self, '%s error %d: %s' % (self.LIB, code, msg))
        self.code = code


def status_helpers(lib, error):
    """(last_error, check, last_kernel, pick_kernel) of a loaded library whose functions are named <error.LIB minus 'lib'>_*."""
    fn = lambda name: getattr(lib, '%s_%s' % (error.LIB[3:], name))          # noqa: E731

    def last_error():
        return fn('last_error')().decode('utf-8', 'replace')

    def check(rc):
        """Raises the library's error for negative return codes; returns rc otherwise."""
        if rc < 0:
            raise error(rc, last_error())
        return rc

    def last_kernel():
        """KERNEL_*: the kernel the calling thread's last compute call enqueued (host-side record)."""
        return fn('last_kernel')()

    def pick_kernel(*shape):
        return check(fn('pick_kernel')(*[int(v) for v in shape]))

    return last_error, check, last_kernel, pick_kernel


def host_i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))


class Cache:
    """Device copies per (topology, key), made on first use.  The topology is held by the cache entry, so its id stays its own."""
    MAX = 4096

    def __init__(self):
        self._entries, self._lock = {}, threading.Lock()

    def get(self, topo, key, make):
        key = (id(topo),) + tuple(key)
        with self._lock:
            hit = self._entries.get(key)
            if hit is None:
                if len(self._entries) >= self.MAX:
                    self._entries.clear()
                hit = self._entries[key] = (topo, make())
        return hit[1]

    def program(self, cls, topo, roots, device):
        """The cached cls(topo, roots, device)."""
        return self.get(topo, (tuple(int(r) for r in roots), str(device)), lambda: cls(topo, roots, device))


class Program:
    """Validated device copies of one root sequence's (ops, srcs, sweeps) and of the topology's in-slots: compile, contiguous
    int32, the library's host checks, upload.  A subclass validates in check_host() and adds its own arrays in upload()."""

    def __init__(self, topo, roots, device):
        import torch
        self.topo, self.device = topo, device
        self.roots = tuple(int(r) for r in roots)
        ops, srcs, sweeps = topo.compile_program(self.roots)
        self._ops_h, self._sweeps_h = host_i32(ops), host_i32(sweeps)
        self._srcs_h = host_i32(srcs if len(srcs) else np.zeros(1))
        self.n_ops, self.n_srcs, self.n_sweeps = len(self._ops_h) // 4, len(srcs), len(self._sweeps_h) // 2
        self._in_off_h, self._in_slots_h = host_i32(topo.in_off), host_i32(topo.in_slots)
        self._up = lambda a: torch.from_numpy(host_i32(a)).to(device)          # noqa: E731
        self.check_host()
        self.ops, self.srcs, self.sweeps = self._up(self._ops_h), self._up(self._srcs_h), self._up(self._sweeps_h)
        self.in_off, self.in_slots = self._up(self._in_off_h), self._up(self._in_slots_h)
        self.upload()

    def program_args(self):
        """The leading arguments of a library's check_program."""
        t = self.topo
        return (_ffi.i32ptr(self._ops_h), self.n_ops, _ffi.i32ptr(self._srcs_h), self.n_srcs, _ffi.i32ptr(self._sweeps_h), self.n_sweeps,
                t.n_msgs, t.P, t.U)

    def in_slot_args(self):
        """The leading arguments of a library's check_readout."""
        return (self.topo.n_vars, _ffi.i32ptr(self._in_off_h), _ffi.i32ptr(self._in_slots_h), self.topo.n_msgs)

    def check_host(self):
        raise NotImplementedError

    def upload(self):
        pass
