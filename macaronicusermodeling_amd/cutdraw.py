"""ctypes binding of libmlbp_cutdraw.so (include/mlbp_cutdraw.h): a proposal for cutset importance sampling drawn from the
messages a sweep left behind -- joint states of the cutset and the log-probability the proposal gave each -- in one launch.

The twelfth library of the engine, with its own signature table.  There is no CPU fallback: the compute call on a machine
without an MI355X returns MLBP_ENODEVICE, raised as CutdrawError.

`plan_words(topo, cutset)` derives the packed draw plan the header describes from the topology's own arrays -- per cut
position the message slots it multiplies and the table rows that reach an earlier position -- and `plan(topo, cutset, X,
device)` has the library validate it on the host, uploads it once and caches the device copy.  The cutset must be one the
estimate accepts, so plan() also obtains cutsetis.plan() for it: an invalid cutset fails with that library's words.
"""
import ctypes as C

import numpy as np

from . import _ffi, _sidelib
from . import cutset as _cutset
from . import cutsetis as _cutsetis
from ._sidelib import i32 as _i32, i32p as _i32p

LIB_PATH = _sidelib.lib_path('mlbp_cutdraw')

KERNEL_NONE, KERNEL_X64, KERNEL_GENERIC = 0, 1, 2
MAX_LISTED = 65536              # include/mlbp_cutdraw.h MLBP_CUTDRAW_MAX_LISTED
MAX_CUT = 16                    # MLBP_CUTDRAW_MAX_CUT
MAX_X = 1024                    # MLBP_CUTDRAW_MAX_X
MIN_WORKGROUPS = 512            # MLBP_CUTDRAW_MIN_WORKGROUPS
PLAN_HEADER = 8                 # MLBP_CUTDRAW_PLAN_HEADER


class CutdrawError(_sidelib.SideError):
    LIB = 'libmlbp_cutdraw'


class CutdrawArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('X', C.c_int32), ('n_msgs', C.c_int32), ('P', C.c_int32),
                ('n_cut', C.c_int32),
                ('n_pair_tables', C.c_int32),
                ('plan_words', C.c_int32),
                ('N', C.c_int32),
                ('plan', C.c_void_p),
                ('pair_tables', C.c_void_p), ('pair_tab', C.c_void_p),
                ('msgs', C.c_void_p),
                ('uniforms', C.c_void_p),
                ('configs_in', C.c_void_p),
                ('configs', C.c_void_p),
                ('log_q', C.c_void_p)]


# name -> (restype, argtypes); mirrors include/mlbp_cutdraw.h one to one (tests/test_side_libraries_cpu.py checks that).
SIGNATURES = {
    'mlbp_cutdraw_f64': (C.c_int, [C.POINTER(CutdrawArgs), C.c_void_p]),
    'mlbp_cutdraw_check_plan': (C.c_int, [_i32p, _i32, _i32, _i32]),
    'mlbp_cutdraw_pick_kernel': (C.c_int, [_i32]),
    'mlbp_cutdraw_chunks': (C.c_int, [_i32, _i32]),
    'mlbp_cutdraw_last_kernel': (C.c_int, []),
    'mlbp_cutdraw_arch': (C.c_char_p, []),
    'mlbp_cutdraw_last_error': (C.c_char_p, []),
}

lib = _sidelib.load(LIB_PATH, SIGNATURES)
last_error, check, last_kernel, pick_kernel = _sidelib.status_helpers(lib, CutdrawError)


def chunks(B, N):
    """min(N, ceil(512 / B)): C of the launch grid (B, C), the rule of cutsetis.chunks."""
    return check(lib.mlbp_cutdraw_chunks(int(B), int(N)))


def plan_items(topo, cutset):
    """Per cut position (base message slots, rows [(pair slot, earlier position, axis of this variable)]), both in the
    variable's facset order, for a cutset given as variable indices."""
    cutpos = {int(v): k for k, v in enumerate(cutset)}
    out = []
    for k, a in enumerate(int(v) for v in cutset):
        base, rows = [], []
        for j in topo.facsets[a]:
            e = 0 if topo.fac_var[2 * j] == a else 1
            if topo.fac_nvars[j] == 2:
                other = cutpos.get(int(topo.fac_var[2 * j + 1 - e]), k)
                if other < k:
                    rows.append((int(topo.pair_slot[j]), other, int(topo.fac_dim[2 * j + e])))
                    continue
            base.append(int(topo.f2v[2 * j + e]))
        out.append((base, rows))
    return out


def plan_words(topo, cutset):
    """The packed draw plan of include/mlbp_cutdraw.h for a cutset given as variable indices: int32 array."""
    cutset = [int(v) for v in cutset]
    items = plan_items(topo, cutset)
    base_off, row_off = [0], [0]
    for base, rows in items:
        base_off.append(base_off[-1] + len(base))
        row_off.append(row_off[-1] + len(rows))
    words = [topo.n_vars, topo.P, topo.n_msgs, len(cutset), base_off[-1], row_off[-1], 0, 0]
    words += cutset + base_off + [s for base, _ in items for s in base] + row_off + [x for _, rows in items for r in rows for x in r]
    return np.array(words, dtype=np.int32)


def check_plan(words, X, n_msgs):
    """Raises CutdrawError unless the packed draw plan `words` is valid for X states and n_msgs message slots."""
    check(lib.mlbp_cutdraw_check_plan(_ffi.i32ptr(words), len(words), int(X), int(n_msgs)))


class Plan:
    """A validated draw plan and its device copy; `walk` is the estimate's plan of the same cutset (cutsetis.plan)."""

    def __init__(self, topo, cutset, X, device):
        import torch
        self.walk = _cutsetis.plan(topo, cutset, X, device)     # refuses what is no cutset, in that library's words
        self.cutset = tuple(int(v) for v in cutset)
        self.words = plan_words(topo, self.cutset)
        check_plan(self.words, X, topo.n_msgs)
        self.n_cut = len(self.cutset)
        self.dev = torch.from_numpy(self.words).to(device) if device is not None else None


_plans = _sidelib.Cache()


def plan(topo, cutset, X, device):
    """The cached Plan of (topology, cutset, X, device); cutset None: cutset.choose(topo)."""
    cutset = tuple(_cutset.choose(topo) if cutset is None else (int(v) for v in cutset))
    return _plans.get(topo, (cutset, int(X), str(device)), lambda: Plan(topo, cutset, X, device))
