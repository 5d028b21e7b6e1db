"""ctypes binding of libmlbp_cutset.so (include/mlbp_cutset.h): the model's true marginals and log Z by cutset conditioning.

The sixth library of the engine, with its own signature table.  There is no CPU fallback: the compute call on a machine
without an MI355X returns MLBP_ENODEVICE, raised as CutsetError.

`choose(topo)` picks the cutset (variable indices, GraphTopology.var_ids order), `plan_words(topo, cutset)` derives the packed
plan the header describes -- elimination order, parent links, the cutset-incident and cutset-internal factor lists --
and `plan(topo, cutset, X, device)` has the library validate it on the host, uploads it once and caches the device copy.
"""
import ctypes as C
import sys

import numpy as np

from . import _ffi, _sidelib
from ._sidelib import i32 as _i32, i32p as _i32p

LIB_PATH = _sidelib.lib_path('mlbp_cutset')

KERNEL_NONE, KERNEL_X64, KERNEL_GENERIC = 0, 1, 2
X64_LDS_BYTES = 131072          # include/mlbp_cutset.h MLBP_CUTSET_X64_LDS_BYTES
GENERIC_LDS_BYTES = 65536
MAX_X = 1024
MAX_CONFIGS = 65536
MIN_WORKGROUPS = 512
PLAN_HEADER = 16
ITEM_UNARY, ITEM_COL, ITEM_ROW = 0, 1, 2
CONST_UNARY, CONST_PAIR = 0, 1


class CutsetError(_sidelib.SideError):
    LIB = 'libmlbp_cutset'


class CutsetArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('X', C.c_int32), ('n_vars', C.c_int32), ('P', C.c_int32), ('U', C.c_int32),
                ('n_cut', C.c_int32), ('n_free', C.c_int32), ('n_items', C.c_int32), ('n_consts', C.c_int32), ('n_forest', C.c_int32),
                ('n_pair_tables', C.c_int32), ('n_unary_tables', C.c_int32),
                ('plan_words', C.c_int32),
                ('plan', C.c_void_p),
                ('pair_tables', C.c_void_p), ('pair_tab', C.c_void_p), ('unary_tables', C.c_void_p), ('unary_tab', C.c_void_p),
                ('labels', C.c_void_p),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_int64),
                ('log_z', C.c_void_p), ('marginals', C.c_void_p), ('score', C.c_void_p), ('joint_logp', C.c_void_p)]


# name -> (restype, argtypes); mirrors include/mlbp_cutset.h one to one (tests/test_side_libraries_cpu.py checks that).
SIGNATURES = {
    'mlbp_cutset_f64': (C.c_int, [C.POINTER(CutsetArgs), C.c_void_p]),
    'mlbp_cutset_check_plan': (C.c_int, [_i32p, _i32, _i32]),
    'mlbp_cutset_pick_kernel': (C.c_int, [_i32, _i32, _i32, _i32, _i32]),
    'mlbp_cutset_chunks': (C.c_int, [_i32, _i32]),
    'mlbp_cutset_workspace_bytes': (C.c_int64, [_i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    'mlbp_cutset_last_kernel': (C.c_int, []),
    'mlbp_cutset_arch': (C.c_char_p, []),
    'mlbp_cutset_last_error': (C.c_char_p, []),
}

lib = _sidelib.load(LIB_PATH, SIGNATURES)
last_error, check, last_kernel, pick_kernel = _sidelib.status_helpers(lib, CutsetError)


def chunks(B, n_configs):
    """C of the launch grid (B, C): workgroup (g, k) walks configurations k, k + C, ... of graph g."""
    return check(lib.mlbp_cutset_chunks(int(B), int(n_configs)))


def workspace_bytes(B, X, n_vars, P, U, n_forest, n_cut):
    return check(lib.mlbp_cutset_workspace_bytes(int(B), int(X), int(n_vars), int(P), int(U), int(n_forest), int(n_cut)))


def pair_edges(topo):
    """[(variable on axis 0, variable on axis 1)] of every pairwise factor, in pair-slot order (variable indices)."""
    edges = []
    for j in topo.pair_factors:
        ends = [0, 0]
        for k in range(2):
            ends[int(topo.fac_dim[2 * j + k])] = int(topo.fac_var[2 * j + k])
        edges.append(tuple(ends))
    return edges


def two_core(n_vars, edges, removed):
    """(core variables, their degree within the core) of the multigraph of `edges` over the variables not in `removed`:
    variables of degree <= 1 are dropped until none is left.  Degree counts factors."""
    alive = [v not in removed for v in range(n_vars)]
    while True:
        deg = [0] * n_vars
        for a, b in edges:
            if alive[a] and alive[b]:
                deg[a] += 1
                deg[b] += 1
        drop = [v for v in range(n_vars) if alive[v] and deg[v] <= 1]
        if not drop:
            return [v for v in range(n_vars) if alive[v]], deg
        for v in drop:
            alive[v] = False


def choose(topo):
    """The cutset of a topology, as variable indices in the order they were taken: while the pairwise multigraph over the
    variables not yet taken has a cycle, the variable of its 2-core with the highest degree (ties: the lowest position in
    var_ids) joins the cutset.  K_n -> the first n - 2 variables, a ring -> its first variable, a tree -> []."""
    edges, cut = pair_edges(topo), []
    while True:
        core, deg = two_core(topo.n_vars, edges, set(cut))
        if not core:
            return cut
        cut.append(max(core, key=lambda v: (deg[v], -v)))


def plan_words(topo, cutset):
    """The packed plan of include/mlbp_cutset.h for a cutset given as variable indices: int32 array.  The forest over the free
    variables is walked breadth-first from the lowest free variable of every tree; `order` is that walk reversed.  A
    remainder with a cycle is packed as it is walked (the closing factor is in no list): check_plan names the cycle."""
    cutset = [int(v) for v in cutset]
    n, P, U = topo.n_vars, topo.P, topo.U
    cutpos = {v: q for q, v in enumerate(cutset)}
    edges = pair_edges(topo)
    unary_var = [int(topo.fac_var[2 * j]) for j in topo.unary_factors]
    free = [v for v in range(n) if v not in cutpos]
    adj = {v: [] for v in free}
    for p, (a, b) in enumerate(edges):
        if a in adj and b in adj:
            adj[a].append((p, b))
            adj[b].append((p, a))
    parent, bfs, used = {}, [], set()
    for root in free:
        if root in parent:
            continue
        parent[root] = (-1, -1)
        queue = [root]
        while queue:
            v = queue.pop(0)
            bfs.append(v)
            for p, w in adj[v]:
                if w not in parent:
                    parent[w] = (p, v)
                    used.add(p)
                    queue.append(w)
    order = bfs[::-1]
    fslot = [-1] * P
    for v in order:
        if parent[v][0] >= 0:
            fslot[parent[v][0]] = sum(1 for s in fslot if s >= 0)
    items, item_off, consts = [], [0], []
    for v in range(n):
        if v not in cutpos:
            for u, w in enumerate(unary_var):
                if w == v:
                    items.append((ITEM_UNARY, u, 0))
            for p, (a, b) in enumerate(edges):
                if a == v and b in cutpos:
                    items.append((ITEM_COL, p, cutpos[b]))
                elif b == v and a in cutpos:
                    items.append((ITEM_ROW, p, cutpos[a]))
        item_off.append(len(items))
    for u, w in enumerate(unary_var):
        if w in cutpos:
            consts.append((CONST_UNARY, u, cutpos[w], -1))
    for p, (a, b) in enumerate(edges):
        if a in cutpos and b in cutpos:
            consts.append((CONST_PAIR, p, cutpos[a], cutpos[b]))
    n_forest = sum(1 for s in fslot if s >= 0)
    words = [n, P, U, len(cutset), len(free), len(items), len(consts), n_forest] + [0] * (PLAN_HEADER - 8)
    words += cutset + order
    for v in range(n):
        words += list(parent.get(v, (-1, -1)))
    words += item_off + [x for it in items for x in it] + [x for c in consts for x in c]
    words += [x for e in edges for x in e] + unary_var + fslot
    return np.array(words, dtype=np.int32)


def check_plan(words, X):
    """Raises CutsetError unless the packed plan `words` is valid for X states."""
    check(lib.mlbp_cutset_check_plan(_ffi.i32ptr(words), len(words), int(X)))


class Plan:
    """A validated plan and its device copy.  binding: the module whose check_plan validates -- this one, or a plan-taking
    binding of build.SIDE_LIBRARIES."""

    def __init__(self, topo, cutset, X, device, binding=None):
        import torch
        seen = set()
        for v in cutset:
            if not 0 <= int(v) < topo.n_vars or int(v) in seen:
                raise ValueError('cutset names variable index %r twice or out of range' % (v,))
            seen.add(int(v))
        self.words = plan_words(topo, cutset)
        (binding or sys.modules[__name__]).check_plan(self.words, X)
        (self.n_vars, self.P, self.U, self.n_cut, self.n_free, self.n_items, self.n_consts, self.n_forest) = (int(w) for w in self.words[:8])
        self.n_configs = int(X) ** self.n_cut
        self.dev = torch.from_numpy(self.words).to(device) if device is not None else None


_plans = _sidelib.Cache()


def plan(topo, cutset, X, device, binding=None):
    """The cached Plan of (topology, cutset, X, device, validating binding); cutset None: choose(topo)."""
    cutset = tuple(choose(topo) if cutset is None else (int(v) for v in cutset))
    key = (cutset, int(X), str(device), (binding or sys.modules[__name__]).__name__)
    return _plans.get(topo, key, lambda: Plan(topo, cutset, X, device, binding))


def plan_functions(module_name):
    """(check_plan, Plan, plan) of the plan-taking binding being imported as `module_name`: this module's three, with that
    binding's library validating (its mlbp_<name>_check_plan, raised as its own error) and the binding in the cache key."""
    binding = sys.modules[module_name]
    entry = 'mlbp_%s_check_plan' % module_name.rsplit('.', 1)[-1]

    def check_plan(words, X):
        """Raises the binding's error unless the packed plan `words` is valid for X states."""
        binding.check(getattr(binding.lib, entry)(_ffi.i32ptr(words), len(words), int(X)))

    def bound_Plan(topo, cutset, X, device):
        """A plan validated by the binding's library and its device copy: cutset.Plan."""
        return Plan(topo, cutset, X, device, binding)

    def bound_plan(topo, cutset, X, device):
        """The cached Plan of (topology, cutset, X, device); cutset None: choose(topo)."""
        return plan(topo, cutset, X, device, binding)

    return check_plan, bound_Plan, bound_plan
