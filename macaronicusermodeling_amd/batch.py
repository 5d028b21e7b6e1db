"""FactorGraphBatch: B independent factor graphs of one shape, resident in HBM, swept by libmlbp.so.

This is the performance form of `FactorGraph.initialize` + `treelike_inference` +
`get_marginal` / `get_posterior_probs` (LBP.py:192-259): the same algorithm and update order,
batched over graphs.  torch is used only to own device memory and the HIP stream; every number is
produced by the HIP kernels behind the C ABI (include/mlbp.h).

HBM layout (all float64, the reference dtype):
    pair_tables  [n_pair_tables][X][X]   row-major; a graph's pairwise factor p reads table
                                         pair_tab[b][p]  (unique per (graph, factor), or shared)
    unary_tables [n_unary_tables][X]     a unary factor's (X,1) table as one contiguous row
    msgs         [B][n_msgs][X]          slot order = GraphTopology.slot_keys()
"""
import ctypes as C
import threading

import numpy as np
import torch

from . import _ffi
from .topology import GraphTopology


# cutset_proposal(): the most bytes of sample()'s cond_marginals buffer ([S][B][n_vars][X] doubles) alive at once; the draws
# are taken in slices of S that stay under it (one draw at the least)
CUTSET_PROPOSAL_BYTES = 256 << 20


def _stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ---- the argument checks every batch call shares (no device needed: tests/test_batch_args_cpu.py) --------------------------
_DTYPE_WORD = {torch.float64: 'float64', torch.int32: 'int32'}


def _device_tensor(t, shape, dtype, device, what, shape_text=None, message=None):
    """t.data_ptr() of a caller's tensor that a kernel is about to read or write, after checking that it IS a tensor, of
    `dtype`, on `device`, contiguous, and of `shape`: a tuple to be met exactly -- None admits any size on that axis -- or an
    int, the least number of elements in any shape.  Anything else raises ValueError('<what> must be a contiguous <dtype>
    device tensor <shape_text>'), or `message` where a call words it differently."""
    ok = torch.is_tensor(t) and t.dtype == dtype and t.device == device and t.is_contiguous()
    if ok and isinstance(shape, int):
        ok = t.numel() >= shape
    elif ok:
        ok = t.dim() == len(shape) and all(s is None or s == d for s, d in zip(shape, t.shape))
    if not ok:
        raise ValueError(message or '%s must be a contiguous %s device tensor %s' % (what, _DTYPE_WORD[dtype], shape_text))
    return t.data_ptr()


def _rows_i32(rows, shape, device, what):
    """rows (`shape` integers: a tensor, an array or nested lists) as a contiguous int32 tensor on `device`; one that already
    is comes back as it is."""
    if torch.is_tensor(rows) and rows.dtype == torch.int32 and rows.device == device and rows.is_contiguous():
        out = rows
    else:
        host = rows.cpu().numpy() if torch.is_tensor(rows) else np.asarray(rows)
        out = torch.from_numpy(np.ascontiguousarray(host.astype(np.int64).astype(np.int32))).to(device)
    if tuple(out.shape) != tuple(shape):
        raise ValueError('%s must be [B][n_vars]' % what)
    return out


def _listed_count(n, K, word='n_samples'):
    """int(n), the entries per graph of a list handed to binding K: within [1, K.MAX_LISTED]."""
    n = int(n)
    if not 1 <= n <= K.MAX_LISTED:
        raise ValueError('%s must be in [1, %d]' % (word, K.MAX_LISTED))
    return n


def _exactly_one(seed, uniforms):
    if (seed is None) == (uniforms is None):
        raise ValueError('give exactly one of seed and uniforms')


def _fill_program(a, prog):
    """The compiled root sequence and the in-slots of a _sidelib.Program into the args of a program-taking library."""
    a.n_ops, a.n_srcs, a.n_sweeps = prog.n_ops, prog.n_srcs, prog.n_sweeps
    a.ops, a.srcs, a.sweeps = prog.ops.data_ptr(), prog.srcs.data_ptr(), prog.sweeps.data_ptr()
    a.in_off, a.in_slots = prog.in_off.data_ptr(), prog.in_slots.data_ptr()


class Program:
    """Validated device-resident op list for one root sequence (mlbp_program_create)."""

    def __init__(self, topo, roots, max_graphs=0):
        self.roots = tuple(int(r) for r in roots)
        ops, srcs, sweeps = topo.compile_program(self.roots)
        self.n_ops = len(ops)
        self.ops, self.srcs, self.sweeps = ops, srcs, sweeps
        h = C.c_void_p()
        ops_c = np.ascontiguousarray(ops.reshape(-1))
        srcs_c = np.ascontiguousarray(srcs if len(srcs) else np.zeros(1, dtype=np.int32))
        sw_c = np.ascontiguousarray(sweeps.reshape(-1))
        _ffi.check(_ffi.lib.mlbp_program_create(_ffi.i32ptr(ops_c), len(ops), _ffi.i32ptr(srcs_c), len(srcs),
                                                _ffi.i32ptr(sw_c), len(sweeps), topo.n_msgs, topo.P, topo.U,
                                                C.byref(h)))
        self.handle = h
        _ffi.check(_ffi.lib.mlbp_program_set_readout(h, topo.n_vars, _ffi.i32ptr(topo.in_off), _ffi.i32ptr(topo.in_slots)))
        if max_graphs > 0:
            _ffi.check(_ffi.lib.mlbp_program_reserve(h, int(max_graphs)))

    def status(self):
        return _ffi.check(_ffi.lib.mlbp_program_status(self.handle))

    def exact_count(self, B):
        """Graphs of the last launch that needed the exact kernel (mlbp_program_exact_count)."""
        return _ffi.check(_ffi.lib.mlbp_program_exact_count(self.handle, B))

    def bail_codes(self, B):
        """The per-graph flag bytes of the last launch as a uint8 array (mlbp_program_bail_codes): 0 = the fast kernel's result
        stands, else why the graph went to the exact kernel."""
        out = np.zeros(int(B), dtype=np.uint8)
        n = _ffi.check(_ffi.lib.mlbp_program_bail_codes(self.handle, int(B), out.ctypes.data))
        return out[:n]

    def skippable_updates(self):
        """Updates of the root sequence that skip_unchanged drops (mlbp_program_skippable_updates)."""
        return _ffi.check(_ffi.lib.mlbp_program_skippable_updates(self.handle))

    def specialize(self):
        """Compiles the program's micro-ops into the default X = 64 kernel now (mlbp_program_specialize); raises when the
        program cannot be specialised."""
        _ffi.check(_ffi.lib.mlbp_program_specialize(self.handle))

    def specialized(self):
        """1 = the last call's program runs its own compiled kernel, 0 = not attempted, -1 = attempted and fell back
        (mlbp_program_specialized)."""
        return int(_ffi.lib.mlbp_program_specialized(self.handle))

    def __del__(self):
        h = getattr(self, 'handle', None)
        lib = getattr(_ffi, 'lib', None) if _ffi is not None else None      # module may be gone at interpreter exit
        if h is not None and h.value and lib is not None:
            lib.mlbp_program_destroy(h)
            self.handle = None


# Programs shared between the one-graph batches of the object API (LBP.py drop-in): every TrainingInstance of one sentence
# shape builds the same topology and draws its roots from the same few variables, and creating a Program costs a dozen
# synchronous allocations and copies.  Per thread (a program's scratch buffers belong to one stream at a time,
# include/mlbp.h), keyed by the topology's integer description, the device and the root sequence; bounded.
_shared_programs = threading.local()
_SHARED_PROGRAMS_MAX = 512


def _topology_signature(topo):
    return (topo.n_vars, tuple(topo.var_ids), topo.fac_nvars.tobytes(), topo.fac_var.tobytes(), topo.fac_dim.tobytes(),
            tuple(tuple(f) for f in topo.facsets))



class FactorGraphBatch:
    def __init__(self, topo, X, B, device='cuda:0', normalize_messages=True, use_approx_inference=False, use_approx_beliefs=False,
                 share_programs=False):
        if not isinstance(topo, GraphTopology):
            raise TypeError('topo must be a GraphTopology')
        self.topo, self.X, self.B = topo, int(X), int(B)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('FactorGraphBatch lives on an MI355X; there is no CPU path')
        self.normalize_messages = bool(normalize_messages)
        # FactorGraph.use_approx_inference / use_approx_beliefs (LBP.py:52-53): top-100 variants, selected on the device
        self.use_approx_inference, self.use_approx_beliefs = bool(use_approx_inference), bool(use_approx_beliefs)
        self.skip_unchanged = False       # MLBP_SWEEP_SKIP_UNCHANGED on every sweep (same output bits, fewer updates)
        self.msgs = torch.empty(self.B, topo.n_msgs, self.X, dtype=torch.float64, device=self.device)
        self.pair_tables = self.pair_tab = self.unary_tables = self.unary_tab = None
        self._in_off = torch.from_numpy(topo.in_off).to(self.device)
        self._in_slots = torch.from_numpy(topo.in_slots).to(self.device)
        self._programs = {}
        self._share_programs = bool(share_programs)     # the object API: Programs come from the per-thread shared cache
        self.is_loopy = None

    # ---- tables -------------------------------------------------------------------------------
    @staticmethod
    def _as_index(idx, B, n, limit, what, device):
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(B, n))
        if idx.size and (idx.min() < 0 or idx.max() >= limit):
            raise IndexError('%s index out of range [0, %d)' % (what, limit))
        return torch.from_numpy(idx.astype(np.int32)).to(device)

    def set_pair_tables(self, tables, pair_tab=None, dtype=torch.float64):
        """tables: [n][X][X] float64 (numpy or torch; copied to the device if needed).
        pair_tab: [B][P] integer table index per graph and pair slot; default = unique tables
        b*P + p.  dtype=torch.float32 keeps the tables in float32 on the device (X = 256 or 512 only:
        the large-state mode, half the bytes per update; sweeps and marginals only)."""
        if dtype not in (torch.float64, torch.float32):
            raise TypeError('pair tables are float64 or float32')
        if dtype == torch.float32 and self.X not in (256, 512):
            raise ValueError('float32 pair tables need X = 256 or 512')
        t = torch.as_tensor(tables).to(self.device).to(dtype).contiguous()
        if t.dim() != 3 or t.shape[1] != self.X or t.shape[2] != self.X:
            raise ValueError('pair tables must be [n][X][X]')
        self._pair_dense = pair_tab is None          # identity index: stated to the kernel (MLBP_SWEEP_DENSE_TABLES)
        if pair_tab is None:
            if t.shape[0] != self.B * self.topo.P:
                raise ValueError('need B*P tables when pair_tab is omitted')
            pair_tab = np.arange(self.B * self.topo.P).reshape(self.B, self.topo.P)
        host_tab = np.asarray(pair_tab).reshape(self.B, self.topo.P)
        # every graph reads the same table for factor p (the reference's layout: one pot array behind all
        # pairwise factors): eligible for the shared-table kernel, which re-checks it on the device
        self.pair_tables_shared = bool(self.topo.P) and bool((host_tab == host_tab[:1]).all())
        self._pair_row_host = np.ascontiguousarray(host_tab[0], dtype=np.int32) if self.pair_tables_shared else None
        self.pair_tab = self._as_index(host_tab, self.B, self.topo.P, t.shape[0], 'pair table', self.device)
        self.pair_tables = t

    def set_unary_tables(self, tables, unary_tab=None):
        t = torch.as_tensor(tables, dtype=torch.float64).to(self.device).contiguous()
        if t.dim() != 2 or t.shape[1] != self.X:
            raise ValueError('unary tables must be [n][X]')
        self._unary_dense = unary_tab is None
        if unary_tab is None:
            if t.shape[0] != self.B * self.topo.U:
                raise ValueError('need B*U tables when unary_tab is omitted')
            unary_tab = np.arange(self.B * self.topo.U).reshape(self.B, self.topo.U)
        self.unary_tab = self._as_index(unary_tab, self.B, self.topo.U, t.shape[0], 'unary table', self.device)
        self.unary_tables = t

    # ---- FactorGraph.initialize (LBP.py:192-216) ----------------------------------------------------
    def initialize(self, loop_root=None):
        root = self.topo.var_ids[0] if loop_root is None else loop_root
        self.is_loopy = self.topo.has_loops(root)
        _ffi.check(_ffi.lib.mlbp_init_messages_f64(self.msgs.data_ptr(), self.B * self.topo.n_msgs, self.X,
                                                   _stream_ptr(self.device)))

    # ---- FactorGraph.treelike_inference (LBP.py:218-245) ------------------------------------------
    def program(self, roots):
        key = tuple(int(r) for r in roots)
        if key not in self._programs:
            if self._share_programs:
                cache = getattr(_shared_programs, 'by_key', None)
                if cache is None:
                    cache = _shared_programs.by_key = {}
                if not hasattr(self, '_topo_sig'):
                    self._topo_sig = (_topology_signature(self.topo), self.device.index)
                full = (self._topo_sig, key)
                prog = cache.get(full)
                if prog is None:
                    if len(cache) >= _SHARED_PROGRAMS_MAX:
                        cache.clear()             # programs still referenced by a batch's own dict live on
                    prog = cache[full] = Program(self.topo, key, max_graphs=self.B)
                self._programs[key] = prog
            else:
                self._programs[key] = Program(self.topo, key, max_graphs=self.B)
        return self._programs[key]

    def sweep(self, roots, init=False, marginals=None, gradient=None, keep_messages=True, skip_unchanged=None, posterior=None, _collect=None):
        """Runs len(roots) sweeps, sweep s rooted at variable id roots[s], on every graph, in one
        launch.  init=True starts from uniform messages (initialize() fused into the launch);
        marginals: optional [B][n_vars][X] device tensor that receives every variable's marginal
        after the last sweep, read out of the on-chip messages in the same launch; gradient: optional
        (out_ee [B][F_ee], out_ed [B][F_ed]) device tensors that receive the per-graph gradients
        (set_features / set_observations first), fused into the launch when the kernel allows;
        keep_messages=False lets a launch whose read-outs (marginals, gradient) are fused skip the write-back of
        self.msgs (their contents are then undefined); posterior: optional (labels int32 [B][n_vars], out [B], sum_out [1] or
        None) device tensors -- get_posterior_probs of every graph (LBP.py:247-259) and their batch sum behind the sweeps of
        the same call (needs `marginals`; on the fast X = 64 paths the fix-up launch takes it);
        skip_unchanged (default: self.skip_unchanged, False) drops the
        updates of the root sequence that would recompute a message from unchanged inputs (MLBP_SWEEP_SKIP_UNCHANGED:
        same output bits, fewer updates)."""
        prog = self.program(roots)
        a = _ffi.SweepArgs()
        a.B, a.X = self.B, self.X
        if self.topo.P:
            if self.pair_tables is None:
                raise RuntimeError('set_pair_tables() first')
            a.n_pair_tables = self.pair_tables.shape[0]
            a.pair_tab = self.pair_tab.data_ptr()
            if self.pair_tables.dtype == torch.float32:
                a.pair_tables_f32 = self.pair_tables.data_ptr()
                a.flags |= _ffi.SWEEP_PAIR_TABLES_F32
            else:
                a.pair_tables = self.pair_tables.data_ptr()
        if self.topo.U:
            if self.unary_tables is None:
                raise RuntimeError('set_unary_tables() first')
            a.n_unary_tables = self.unary_tables.shape[0]
            a.unary_tables, a.unary_tab = self.unary_tables.data_ptr(), self.unary_tab.data_ptr()
        a.msgs = self.msgs.data_ptr()
        a.normalize_messages = 1 if self.normalize_messages else 0
        a.init_messages = 1 if init else 0
        if self.use_approx_inference:
            a.flags |= _ffi.SWEEP_APPROX_INFERENCE
        if getattr(self, 'skip_unchanged', False) if skip_unchanged is None else skip_unchanged:
            a.flags |= _ffi.SWEEP_SKIP_UNCHANGED
        if (getattr(self, '_pair_dense', False) or not self.topo.P) and (getattr(self, '_unary_dense', False) or not self.topo.U):
            a.flags |= _ffi.SWEEP_DENSE_TABLES
        if getattr(self, 'pair_tables_shared', False):
            a.flags |= _ffi.SWEEP_SHARED_PAIR_TABLES
            if getattr(self, '_pair_row_host', None) is not None:       # X >= 128: the update-by-update contraction path needs the row on the host
                a.pair_tab_host = self._pair_row_host.ctypes.data
        if not keep_messages and (marginals is not None or gradient is not None):
            a.flags |= _ffi.SWEEP_NO_MESSAGE_WRITEBACK      # honoured by the kernels whose read-outs are fused (lean, shared)
        if marginals is not None:
            if tuple(marginals.shape) != (self.B, self.topo.n_vars, self.X) or marginals.dtype != torch.float64:
                raise ValueError('marginals must be float64 [B][n_vars][X]')
            a.marginals = marginals.data_ptr()
        ga = pa = None
        if gradient is not None:
            ga = self._gradient_args(*gradient)
            a.gradient = C.addressof(ga)
        if posterior is not None:
            lab, out, tot = posterior
            if marginals is None or lab.dtype != torch.int32 or tuple(lab.shape) != (self.B, self.topo.n_vars) or out.numel() < self.B:
                raise ValueError('posterior needs marginals, int32 labels [B][n_vars] and an output of B doubles')
            pa = _ffi.PosteriorArgs()
            pa.labels, pa.out, pa.sum_out = lab.data_ptr(), out.data_ptr(), None if tot is None else tot.data_ptr()
            a.posterior = C.addressof(pa)
        if _collect is not None:                  # sweep_groups(): gather instead of launching
            _collect.append((prog, a, (ga, pa)))      # (the argument structs a points to stay alive with it)
            return prog
        _ffi.check(_ffi.lib.mlbp_sweep_f64(prog.handle, C.byref(a), _stream_ptr(self.device)))
        return prog

    # ---- what the calls into the side libraries share ---------------------------------------------------------
    def _tensor(self, t, shape, what, shape_text=None, dtype=torch.float64, message=None):
        return _device_tensor(t, shape, dtype, self.device, what, shape_text, message)

    def _rows_i32(self, rows, what):
        return _rows_i32(rows, (self.B, self.topo.n_vars), self.device, what)

    def _fill_tables(self, a, pair=True, unary=True):
        """The table fields of a side library's args; the tables must have been set."""
        if pair and self.topo.P:
            if self.pair_tables is None:
                raise RuntimeError('set_pair_tables() first')
            a.n_pair_tables = self.pair_tables.shape[0]
            a.pair_tables, a.pair_tab = self.pair_tables.data_ptr(), self.pair_tab.data_ptr()
        if unary and self.topo.U:
            if self.unary_tables is None:
                raise RuntimeError('set_unary_tables() first')
            a.n_unary_tables = self.unary_tables.shape[0]
            a.unary_tables, a.unary_tab = self.unary_tables.data_ptr(), self.unary_tab.data_ptr()

    def _uniforms(self, seed, uniforms, shape, shape_text):
        """The uniforms of a drawing call, float64 `shape`: the caller's, checked, or torch.rand from `seed`."""
        _exactly_one(seed, uniforms)
        if uniforms is None:
            gen = torch.Generator(self.device).manual_seed(int(seed))
            return torch.rand(shape, dtype=torch.float64, device=self.device, generator=gen)
        self._tensor(uniforms, shape, 'uniforms', shape_text)
        return uniforms

    def _workspace(self, a, need):
        """Allocates the `need` bytes a library asked for and states them in a; the caller holds the tensor until its launch
        is enqueued."""
        work = torch.empty(need // 8, dtype=torch.float64, device=self.device)
        a.workspace, a.workspace_bytes = work.data_ptr(), need
        return work

    def _cutset_indices(self, cutset):
        """A cutset given as variable ids as variable indices (None stays None: the library's own choice)."""
        if cutset is None:
            return None
        unknown = [v for v in cutset if v not in self.topo.var_index]
        if unknown:
            raise ValueError('cutset names unknown variable ids %r' % (unknown,))
        return [self.topo.var_index[v] for v in cutset]

    # ---- max-product: the jointly most probable assignment (include/mlbp_map.h) ------------------
    def map_sweep(self, roots, init=True, max_marginals=None, keep_messages=True):
        """Runs len(roots) MAX-product sweeps -- sweep()'s schedule with max_j in place of sum_j in every pairwise update --
        and decodes: returns (assignment int32 [B][n_vars], score float64 [B]) device tensors, variables in
        GraphTopology.var_ids order.  assignment[v] is the argmax of v's max-marginal (ties to the lowest index); score is
        the sum over factors of the log table entry at the assignment (the tables as given).  Exact MAP on a tree whenever
        it is unique, the usual max-product approximation on a loopy graph.  Tables and self.msgs are used as sweep() uses
        them; max_marginals: optional [B][n_vars][X] device tensor; keep_messages=False leaves self.msgs undefined."""
        from . import mapdecode as M
        if self.use_approx_inference:
            raise NotImplementedError('max-product has no top-100 approximate form')
        if self.pair_tables is not None and self.pair_tables.dtype != torch.float64:
            raise NotImplementedError('max-product needs float64 pairwise tables')
        topo = self.topo
        prog = M.program(topo, roots, self.device)
        a = M.MapArgs()
        a.B, a.X, a.n_msgs, a.P, a.U, a.n_vars = self.B, self.X, topo.n_msgs, topo.P, topo.U, topo.n_vars
        _fill_program(a, prog)
        self._fill_tables(a)
        if topo.P:
            a.pair_axis_var = prog.pair_axis_var.data_ptr()
        if topo.U:
            a.unary_var = prog.unary_var.data_ptr()
        a.msgs = self.msgs.data_ptr()
        a.init_messages, a.normalize_messages = (1 if init else 0), (1 if self.normalize_messages else 0)
        a.write_messages = 1 if keep_messages else 0
        if max_marginals is not None:
            a.max_marginals = self._tensor(max_marginals, (self.B, topo.n_vars, self.X), 'max_marginals',
                                           message='max_marginals must be float64 [B][n_vars][X]')
        assignment = torch.empty(self.B, topo.n_vars, dtype=torch.int32, device=self.device)
        score = torch.empty(self.B, dtype=torch.float64, device=self.device)
        a.assignment, a.score = assignment.data_ptr(), score.data_ptr()
        M.check(M.lib.mlbp_map_sweep_f64(C.byref(a), _stream_ptr(self.device)))
        return assignment, score

    # ---- log Z and the joint log-likelihood (include/mlbp_logz.h) -----------------------------------
    def log_partition(self, roots=None, init=True, labels=None, sum_out=None, score=None):
        """log Z of every graph from the factor->variable messages: exact on a tree, the Bethe value on a loopy graph.
        With `roots` it first runs self.sweep(roots, init=init) with the messages kept; without, it reads self.msgs as the
        last sweep (sum-product, exact or approximate) left them.  Returns log_z [B], or (log_z, joint_logp) when `labels`
        ([B][n_vars] integers, GraphTopology.var_ids order; an int32 device tensor is used as it is) is given:
        joint_logp = score(labels) - log_z, the log-probability of the whole assignment, where score is map_sweep's -- the sum
        over factors of the log table entry.  Device tensors.  A label outside [0, X) gives NaN for that graph, a zero table
        entry at the labels -inf.  sum_out: optional [2] float64 device tensor that receives the batch sums of log_z and
        joint_logp (added in a fixed order by one more launch); score: optional [B] float64 device tensor that receives
        score(labels)."""
        from . import logz as L
        if self.pair_tables is not None and self.pair_tables.dtype != torch.float64:
            raise NotImplementedError('log_partition needs float64 pairwise tables')
        topo = self.topo
        if roots is not None:
            self.sweep(roots, init=init, keep_messages=True)
        ro = L.readout(topo, self.device)
        a = L.LogzArgs()
        a.B, a.X, a.n_msgs, a.P, a.U, a.n_vars = self.B, self.X, topo.n_msgs, topo.P, topo.U, topo.n_vars
        self._fill_tables(a)
        if topo.P:
            a.pair_axis_var, a.pair_in_slot = ro.pair_axis_var.data_ptr(), ro.pair_in_slot.data_ptr()
            if getattr(self, 'pair_tables_shared', False):
                a.flags |= L.SHARED_PAIR_TABLES
        if topo.U:
            a.unary_var, a.unary_in_slot = ro.unary_var.data_ptr(), ro.unary_in_slot.data_ptr()
        a.msgs = self.msgs.data_ptr()
        a.in_off, a.in_slots = ro.in_off.data_ptr(), ro.in_slots.data_ptr()
        log_z = torch.empty(self.B, dtype=torch.float64, device=self.device)
        a.log_z = log_z.data_ptr()
        joint = lab = None
        if labels is not None:
            lab = self._rows_i32(labels, 'labels')
            joint = torch.empty(self.B, dtype=torch.float64, device=self.device)
            a.labels, a.joint_logp = lab.data_ptr(), joint.data_ptr()
            if score is not None:
                a.score = self._tensor(score, self.B, 'score', message='score must be a float64 device tensor of B elements')
        elif score is not None:
            raise ValueError('score needs labels')
        if sum_out is not None:
            a.sum_out = self._tensor(sum_out, 2, 'sum_out', message='sum_out must be a float64 device tensor of two elements')
        L.check(L.lib.mlbp_logz_f64(C.byref(a), _stream_ptr(self.device)))
        return log_z if labels is None else (log_z, joint)

    # ---- posterior sampling of whole assignments (include/mlbp_sample.h) -----------------------------
    def sample(self, roots, n_samples=1, seed=None, uniforms=None, order=None, given=None, cond_marginals=None):
        """Draws n_samples whole assignments per graph by sequential conditioning: draw a variable from its marginal, clamp it,
        run sweep(roots, init=True) again on the clamped model, draw the next.  Returns (samples int32 [S][B][n_vars] in
        GraphTopology.var_ids order, logq float64 [S][B]) device tensors; logq is the exact log-probability of the draw under
        the sampler -- score - log Z on a tree, a proper proposal distribution on a loopy graph.  Exactly one of `seed` and
        `uniforms`: uniforms is a float64 [S][B][n_vars] device tensor of numbers in [0, 1), indexed by step; seed means
        torch.rand((S, B, n_vars), dtype=float64, device=..., generator=torch.Generator(device).manual_seed(seed)).  order: a
        list of variable ids (default: var_ids order), step k handles order[k]; given: [B][n_vars] integers, a state fixes
        the variable, -1 draws it; cond_marginals: optional float64 [S][B][n_vars][X] device tensor that receives, per
        variable, the conditional marginal it was drawn from.  self.msgs is left untouched."""
        from . import sample as S_
        if self.use_approx_inference:
            raise NotImplementedError('sampling has no top-100 approximate form')
        if self.pair_tables is not None and self.pair_tables.dtype != torch.float64:
            raise NotImplementedError('sampling needs float64 pairwise tables')
        _exactly_one(seed, uniforms)
        topo, S = self.topo, int(n_samples)
        if S <= 0:
            raise ValueError('n_samples must be positive')
        uniforms = self._uniforms(seed, uniforms, (S, self.B, topo.n_vars), '[n_samples][B][n_vars]')
        prog = S_.program(topo, roots, self.device)
        a = S_.SampleArgs()
        a.B, a.X, a.n_msgs, a.P, a.U, a.n_vars, a.S = self.B, self.X, topo.n_msgs, topo.P, topo.U, topo.n_vars, S
        _fill_program(a, prog)
        self._fill_tables(a)
        a.normalize_messages = 1 if self.normalize_messages else 0
        a.slot_var = prog.slot_var.data_ptr()
        a.order = prog.order(order).data_ptr()
        a.uniforms = uniforms.data_ptr()
        giv = None
        if given is not None:
            giv = self._rows_i32(given, 'given')
            a.given = giv.data_ptr()
        need = S_.workspace_bytes(self.B, S, self.X, topo.n_msgs, topo.n_vars)
        work = self._workspace(a, need) if need else None
        if cond_marginals is not None:
            a.cond_marginals = self._tensor(cond_marginals, (S, self.B, topo.n_vars, self.X), 'cond_marginals', '[n_samples][B][n_vars][X]')
        samples = torch.empty(S, self.B, topo.n_vars, dtype=torch.int32, device=self.device)
        logq = torch.empty(S, self.B, dtype=torch.float64, device=self.device)
        a.samples, a.logq = samples.data_ptr(), logq.data_ptr()
        S_.check(S_.lib.mlbp_sample_f64(C.byref(a), _stream_ptr(self.device)))
        return samples, logq

    # ---- sweeps to convergence (include/mlbp_converge.h) ---------------------------------------------
    def converge(self, roots=None, tol=1e-6, max_rounds=50, init=True, marginals=None, history=False):
        """Repeats the sum-product sweeps of `roots` (default: every variable once, GraphTopology.var_ids order) -- one ROUND --
        until a whole round changes no message entry by more than tol, graph by graph, in one launch; a graph that has
        settled stops on its own.  Returns (rounds int32 [B], residual float64 [B]) device tensors -- the rounds each graph ran
        (at most max_rounds) and its last round's residual, so residual <= tol says it converged -- or (rounds, residual,
        history float64 [B][max_rounds]) with history=True: the residual of every round run, -1.0 beyond rounds.  The final
        messages are left in self.msgs: marginals(), log_partition(roots=None), pair_beliefs() and gradient() then read the
        converged messages.  init=False continues from what self.msgs holds; marginals: optional [B][n_vars][X] device tensor.
        tol = 0 stops only at an exact fixed point (a tree reaches one in its second round)."""
        return self._converge('converge', roots, tol, max_rounds, init, marginals, 'marginals', history, decode=False)

    def map_converge(self, roots=None, tol=1e-6, max_rounds=50, init=True, max_marginals=None, history=False):
        """converge() with MAX-product rounds -- map_sweep()'s updates, repeated until a whole round changes no message entry by
        more than tol, graph by graph, in one launch -- and map_sweep()'s decode from the final messages.  Returns (assignment
        int32 [B][n_vars], score float64 [B], rounds int32 [B], residual float64 [B]) device tensors, plus history float64
        [B][max_rounds] with history=True.  residual <= tol says the messages the assignment was read from had settled;
        max-product need not settle, and a graph that oscillates runs max_rounds rounds.  One round from uniform messages is
        map_sweep(roots) bit for bit.  The final messages are left in self.msgs; init=False continues from what it holds;
        max_marginals: optional [B][n_vars][X] device tensor.  Refuses what converge() refuses."""
        return self._converge('map_converge', roots, tol, max_rounds, init, max_marginals, 'max_marginals', history, decode=True)

    def _converge(self, what, roots, tol, max_rounds, init, marginals, marginals_word, history, decode):
        """The one call of libmlbp_converge.so: sum-product rounds, or (decode) max-product rounds and the decoded assignment."""
        from . import converge as V
        if self.use_approx_inference:
            raise NotImplementedError('%s has no top-100 approximate form' % what)
        if self.pair_tables is not None and self.pair_tables.dtype != torch.float64:
            raise NotImplementedError('%s needs float64 pairwise tables' % what)
        if not self.normalize_messages:
            raise ValueError('%s needs normalised messages: a residual on unnormalised messages has no scale' % what)
        topo = self.topo
        prog = V.program(topo, topo.var_ids if roots is None else roots, self.device)
        a = V.ConvergeArgs()
        a.B, a.X, a.n_msgs, a.P, a.U, a.n_vars = self.B, self.X, topo.n_msgs, topo.P, topo.U, topo.n_vars
        _fill_program(a, prog)
        self._fill_tables(a)
        a.normalize_messages, a.init_messages = 1, (1 if init else 0)
        a.max_rounds, a.tol = int(max_rounds), float(tol)
        a.msgs = self.msgs.data_ptr()
        if marginals is not None:
            a.marginals = self._tensor(marginals, (self.B, topo.n_vars, self.X), marginals_word, '[B][n_vars][X]')
        rounds = torch.empty(self.B, dtype=torch.int32, device=self.device)
        residual = torch.empty(self.B, dtype=torch.float64, device=self.device)
        a.rounds, a.residual = rounds.data_ptr(), residual.data_ptr()
        out = (rounds, residual)
        if decode:
            assignment = torch.empty(self.B, topo.n_vars, dtype=torch.int32, device=self.device)
            score = torch.empty(self.B, dtype=torch.float64, device=self.device)
            a.max_product, a.assignment, a.score = 1, assignment.data_ptr(), score.data_ptr()
            if topo.P:
                a.pair_axis_var = prog.pair_axis_var.data_ptr()
            if topo.U:
                a.unary_var = prog.unary_var.data_ptr()
            out = (assignment, score) + out
        if history:
            if not 1 <= int(max_rounds) <= V.MAX_ROUNDS:
                raise ValueError('max_rounds must be in [1, %d]' % V.MAX_ROUNDS)
            hist = torch.empty(self.B, int(max_rounds), dtype=torch.float64, device=self.device)
            a.history = hist.data_ptr()
            out = out + (hist,)
        V.check(V.lib.mlbp_converge_f64(C.byref(a), _stream_ptr(self.device)))
        return out

    # ---- what the six cutset-conditioning calls share -----------------------------------------------------
    def _cutset_args(self, K, Args, cutset, refusal):
        """(plan, args) of a call into binding K (cutset, or a plan-taking binding of build.SIDE_LIBRARIES): the cutset's
        variable ids translated, the plan validated by K's library, and the sizes, plan and table fields of an Args() filled.  refusal: the message for pairwise
        tables that are not float64."""
        if self.pair_tables is not None and self.pair_tables.dtype != torch.float64:
            raise NotImplementedError(refusal)
        topo = self.topo
        pl = K.plan(topo, self._cutset_indices(cutset), self.X, self.device)
        a = Args()
        a.B, a.X, a.n_vars, a.P, a.U = self.B, self.X, topo.n_vars, topo.P, topo.U
        a.n_cut, a.n_free, a.n_items, a.n_consts, a.n_forest = pl.n_cut, pl.n_free, pl.n_items, pl.n_consts, pl.n_forest
        a.plan, a.plan_words = pl.dev.data_ptr(), len(pl.words)
        self._fill_tables(a)
        return pl, a

    # ---- the model's true marginals and log Z (include/mlbp_cutset.h) --------------------------------
    def exact_inference(self, labels=None, marginals=None, cutset=None):
        """The TRUE log Z and marginals of every graph by cutset conditioning -- what sweep() and log_partition() approximate
        on a loopy graph.  Returns (log_z [B], marginals [B][n_vars][X]) device tensors, or (log_z, marginals, joint_logp [B])
        when `labels` ([B][n_vars] integers, GraphTopology.var_ids order) is given: joint_logp = score(labels) - log_z, the true
        log-probability of the assignment.  marginals: optional contiguous float64 [B][n_vars][X] device tensor to write into.
        cutset: a list of variable ids that replaces cutset.choose(topo); the pairwise factors among the other variables
        must form a forest, and X^len(cutset) may not pass 65536 (CutsetError otherwise).  Any valid cutset gives the same
        values up to rounding.  self.msgs is neither read nor written."""
        from . import cutset as K
        topo = self.topo
        pl, a = self._cutset_args(K, K.CutsetArgs, cutset, 'exact_inference needs float64 pairwise tables')
        if marginals is None:
            marginals = torch.empty(self.B, topo.n_vars, self.X, dtype=torch.float64, device=self.device)
        else:
            self._tensor(marginals, (self.B, topo.n_vars, self.X), 'marginals', '[B][n_vars][X]')
        a.marginals = marginals.data_ptr()
        log_z = torch.empty(self.B, dtype=torch.float64, device=self.device)
        a.log_z = log_z.data_ptr()
        joint = lab = None
        if labels is not None:
            lab = self._rows_i32(labels, 'labels')
            joint = torch.empty(self.B, dtype=torch.float64, device=self.device)
            a.labels, a.joint_logp = lab.data_ptr(), joint.data_ptr()
        work = self._workspace(a, K.workspace_bytes(self.B, self.X, topo.n_vars, topo.P, topo.U, pl.n_forest, pl.n_cut))
        K.check(K.lib.mlbp_cutset_f64(C.byref(a), _stream_ptr(self.device)))
        return (log_z, marginals) if labels is None else (log_z, marginals, joint)

    # ---- log Z and marginals by cutset importance sampling (include/mlbp_cutsetis.h) -------------------
    def cutset_proposal(self, roots, n_samples, seed=None, uniforms=None, cutset=None):
        """The default proposal of cutset_estimate(): n_samples joint states of the cutset per graph, drawn by sample() --
        sequential conditioning on loopy-BP marginals after sweep(roots, init=True) -- with the cutset variables first in
        its order.  Returns (configs int32 [B][N][n_cut], log_q float64 [B][N]) device tensors: configs[b][i][q] is the state
        of cutset variable q in draw i, log_q the natural log of the probability the sampler gave that joint state: the sum
        over the cutset variables, in cutset order, of the log of the conditional marginal each was drawn from.  Exactly one
        of `seed` and `uniforms`, as in sample() ([N][B][n_vars]; the columns behind the cutset's draw the free variables and
        do not move configs or log_q).  sample() is called on slices of the draws so that its cond_marginals buffer stays
        under CUTSET_PROPOSAL_BYTES; the uniforms are made once for the whole call and the result does not depend on the
        bound.  cutset: as in exact_inference, without its limit on X^len(cutset).  On a tree configs is [B][N][0] and log_q 0."""
        from . import cutset as K0, cutsetis as K
        _exactly_one(seed, uniforms)
        topo, N = self.topo, _listed_count(n_samples, K)
        pl, _ = self._cutset_args(K, K.CutsetisArgs, cutset, 'cutset_proposal needs float64 pairwise tables')
        cut = [int(v) for v in pl.words[K0.PLAN_HEADER:K0.PLAN_HEADER + pl.n_cut]]
        configs = torch.empty(self.B, N, pl.n_cut, dtype=torch.int32, device=self.device)
        log_q = torch.zeros(self.B, N, dtype=torch.float64, device=self.device)
        if not cut:
            return configs, log_q
        uniforms = self._uniforms(seed, uniforms, (N, self.B, topo.n_vars), '[n_samples][B][n_vars]')
        order = [topo.var_ids[v] for v in cut] + [topo.var_ids[v] for v in range(topo.n_vars) if v not in set(cut)]
        step = max(1, CUTSET_PROPOSAL_BYTES // (self.B * topo.n_vars * self.X * 8))
        cols = torch.tensor(cut, dtype=torch.int64, device=self.device)
        for lo in range(0, N, step):
            hi = min(N, lo + step)
            cond = torch.empty(hi - lo, self.B, topo.n_vars, self.X, dtype=torch.float64, device=self.device)
            samples, _ = self.sample(roots, hi - lo, uniforms=uniforms[lo:hi], order=order, cond_marginals=cond)
            drawn = samples.index_select(2, cols)                                          # [S][B][n_cut]
            p = cond.index_select(2, cols).gather(3, drawn.long().unsqueeze(3)).squeeze(3)
            lq = p[:, :, 0].log()
            for q in range(1, len(cut)):                       # one addition per cut position: the same bits for every slice
                lq = lq + p[:, :, q].log()
            configs[:, lo:hi] = drawn.permute(1, 0, 2)
            log_q[:, lo:hi] = lq.t()
        return configs, log_q

    # ---- the proposal drawn from the held messages (include/mlbp_cutdraw.h) -------------------------------------------
    def _cutdraw_refuse(self, what):
        if self.use_approx_inference:
            raise NotImplementedError('sampling has no top-100 approximate form')
        if self.pair_tables is not None and self.pair_tables.dtype != torch.float64:
            raise NotImplementedError('%s needs float64 pairwise tables' % what)

    def _cutdraw_plan(self, cutset):
        """The draw plan of a cutset given as variable ids (None: cutset.choose)."""
        from . import cutdraw as K
        return K.plan(self.topo, self._cutset_indices(cutset), self.X, self.device)

    def _cutdraw(self, what, N, cutset, uniforms=None, configs_in=None):
        """One call into libmlbp_cutdraw.so: (configs or None, log_q).  N: entries per graph; uniforms: [B][N][n_cut], checked
        by the caller."""
        from . import cutdraw as K
        self._cutdraw_refuse(what)
        topo = self.topo
        pl = self._cutdraw_plan(cutset)
        shape = (self.B, N, pl.n_cut)
        log_q = torch.zeros(self.B, N, dtype=torch.float64, device=self.device)
        configs = None
        if configs_in is None:
            configs = torch.empty(shape, dtype=torch.int32, device=self.device)
        else:
            self._tensor(configs_in, shape, 'configs', '[B][N][n_cut]', dtype=torch.int32)
        if not pl.n_cut:                                        # a tree: the one empty configuration, nothing to launch
            return configs, log_q
        a = K.CutdrawArgs()
        a.B, a.X, a.n_msgs, a.P, a.n_cut, a.N = self.B, self.X, topo.n_msgs, topo.P, pl.n_cut, N
        a.plan, a.plan_words = pl.dev.data_ptr(), len(pl.words)
        self._fill_tables(a, unary=False)
        a.msgs, a.log_q = self.msgs.data_ptr(), log_q.data_ptr()
        if configs_in is None:
            a.uniforms, a.configs = uniforms.data_ptr(), configs.data_ptr()
        else:
            a.configs_in = configs_in.data_ptr()
        K.check(K.lib.mlbp_cutdraw_f64(C.byref(a), _stream_ptr(self.device)))
        return configs, log_q

    def cutset_draw(self, n_samples, seed=None, uniforms=None, cutset=None):
        """The proposal of cutset_estimate(proposal='messages'): n_samples joint states of the cutset per graph drawn from the
        messages self.msgs holds AS THEY STAND -- run sweep() or converge() first, as before marginals() -- in one launch and
        without sweeping again.  The cutset variables are drawn in cutset order, each from the product of its incoming
        messages with the messages from cutset variables already drawn replaced by the table's row or column at the drawn
        state (include/mlbp_cutdraw.h).  Returns (configs int32 [B][N][n_cut], log_q float64 [B][N]) device tensors, the list
        cutset_estimate(configs=..., log_q=...) takes.  Exactly one of `seed` and `uniforms`: uniforms is a contiguous float64
        [B][N][n_cut] device tensor of numbers in [0, 1); seed means torch.rand((B, N, n_cut), dtype=float64, device=...,
        generator=torch.Generator(device).manual_seed(seed)).  cutset: as in cutset_estimate.  The first cutset variable is
        drawn from its loopy-BP marginal; on a tree with converged messages and a connected cutset the proposal is Z_c / Z
        itself.  A tree (no cutset) gives configs [B][N][0] and log_q 0 without a launch.  self.msgs is read, not written."""
        from . import cutdraw as K
        _exactly_one(seed, uniforms)
        self._cutdraw_refuse('cutset_draw')
        N = _listed_count(n_samples, K)
        uniforms = self._uniforms(seed, uniforms, (self.B, N, self._cutdraw_plan(cutset).n_cut), '[B][n_samples][n_cut]')
        return self._cutdraw('cutset_draw', N, cutset, uniforms=uniforms)

    def cutset_logq(self, configs, cutset=None):
        """log_q float64 [B][N] of the joint states `configs` (contiguous int32 [B][N][n_cut] device tensor) under the proposal
        of cutset_draw() and the messages self.msgs holds: the second mode of include/mlbp_cutdraw.h.  Of a list cutset_draw()
        drew it returns that call's log_q bit for bit; a state outside [0, X) gives NaN for its entry."""
        from . import cutdraw as K
        if not torch.is_tensor(configs) or configs.dim() != 3 or not 1 <= int(configs.shape[1]) <= K.MAX_LISTED:
            raise ValueError('configs must be a contiguous int32 device tensor [B][N][n_cut] with N in [1, %d]' % K.MAX_LISTED)
        return self._cutdraw('cutset_logq', int(configs.shape[1]), cutset, configs_in=configs)[1]

    def cutset_estimate(self, roots=None, n_samples=None, seed=None, uniforms=None, configs=None, log_q=None, labels=None,
                        marginals=None, cutset=None, log_w=False, proposal='sample'):
        """An ESTIMATE of log Z and of the marginals of every graph by cutset importance sampling -- for the graphs whose
        cutset has more joint states than exact_inference() sums (more than 65536: K5 and up at X = 64).  N joint states c_i of
        the cutset are listed per graph with the log-probability a proposal q gave each; the conditioned forest is solved
        exactly for every entry, as exact_inference() does for every configuration, and weighted by w_i = Z_c / q(c_i).
        Returns (log_z_hat [B], marginals [B][n_vars][X], ess [B]) device tensors, then joint_logp [B] = score(labels) -
        log_z_hat when `labels` is given, then log_w [B][N] = ln Z_c - log_q with log_w=True.
        Either `configs` (int32 [B][N][n_cut], the state of every cutset variable in cutset order) and `log_q` (float64
        [B][N]), or `roots`, `n_samples` and one of `seed` / `uniforms`, which go through cutset_proposal().
        exp(log_z_hat) = mean of w_i is an unbiased estimate of Z for any proposal that is positive wherever Z_c is.  The
        marginals are self-normalised, sum of w_i m_c / sum of w_i: consistent, not unbiased.  ess = (sum w)^2 / sum w^2 is the
        effective sample size, N for a perfect proposal; the relative standard error of the estimate of Z it implies is
        sqrt(1 / ess - 1 / N).  A graph with a state outside [0, X) or a log_q that is not finite gets NaN and keeps its
        marginals.  cutset: as in exact_inference; at most 16 variables, no limit on X^len(cutset).  self.msgs is untouched.
        proposal='messages' makes the list with cutset_draw() in the place of cutset_proposal(): n_samples and one of seed /
        uniforms ([B][N][n_cut]) as cutset_draw() takes them.  Given `roots`, sweep(roots, init=True) runs first -- THAT WRITES
        self.msgs --; with roots=None the messages self.msgs holds are used as they stand."""
        from . import cutsetis as K
        topo = self.topo
        if proposal not in ('sample', 'messages'):
            raise ValueError("proposal must be 'sample' or 'messages', not %r" % (proposal,))
        if (configs is None) != (log_q is None):
            raise ValueError('give configs and log_q together')
        if configs is None and proposal == 'messages':
            if n_samples is None:
                raise ValueError('give configs and log_q, or n_samples and one of seed / uniforms')
            self._cutdraw_refuse('cutset_estimate')
            if roots is not None:
                self.sweep(roots, init=True)
            configs, log_q = self.cutset_draw(n_samples, seed=seed, uniforms=uniforms, cutset=cutset)
        elif configs is None:
            if roots is None or n_samples is None:
                raise ValueError('give configs and log_q, or roots, n_samples and one of seed / uniforms')
            configs, log_q = self.cutset_proposal(roots, n_samples, seed=seed, uniforms=uniforms, cutset=cutset)
        elif roots is not None or n_samples is not None or seed is not None or uniforms is not None:
            raise ValueError('configs and log_q replace roots, n_samples, seed and uniforms')
        pl, a = self._cutset_args(K, K.CutsetisArgs, cutset, 'cutset_estimate needs float64 pairwise tables')
        a.log_q = self._tensor(log_q, (self.B, None), 'log_q', '[B][N]')
        a.N = N = _listed_count(log_q.shape[1], K, 'N')
        configs_ptr = self._tensor(configs, (self.B, N, pl.n_cut), 'configs', '[B][N][n_cut]', dtype=torch.int32)
        if pl.n_cut:
            a.configs = configs_ptr
        if marginals is None:
            marginals = torch.empty(self.B, topo.n_vars, self.X, dtype=torch.float64, device=self.device)
        else:
            self._tensor(marginals, (self.B, topo.n_vars, self.X), 'marginals', '[B][n_vars][X]')
        a.marginals = marginals.data_ptr()
        log_z_hat = torch.empty(self.B, dtype=torch.float64, device=self.device)
        ess = torch.empty(self.B, dtype=torch.float64, device=self.device)
        a.log_z_hat, a.ess = log_z_hat.data_ptr(), ess.data_ptr()
        out = [log_z_hat, marginals, ess]
        lab = None
        if labels is not None:
            lab = self._rows_i32(labels, 'labels')
            out.append(torch.empty(self.B, dtype=torch.float64, device=self.device))
            a.labels, a.joint_logp = lab.data_ptr(), out[-1].data_ptr()
        if log_w:
            out.append(torch.empty(self.B, N, dtype=torch.float64, device=self.device))
            a.log_w = out[-1].data_ptr()
        work = self._workspace(a, K.workspace_bytes(self.B, self.X, topo.n_vars, topo.P, topo.U, pl.n_forest, N))
        K.check(K.lib.mlbp_cutsetis_f64(C.byref(a), _stream_ptr(self.device)))
        return tuple(out)

    # ---- the exact MAP assignment and the max-marginals (include/mlbp_exactmap.h) ----------------------
    def exact_map(self, max_marginals=None, cutset=None):
        """The TRUE jointly most probable assignment of every graph by cutset conditioning -- what map_sweep() approximates
        on a loopy graph.  Returns (assignment int32 [B][n_vars] in GraphTopology.var_ids order, score float64 [B]) device
        tensors -- score: the log-potential of the assignment, map_sweep's score --, and with max_marginals=True or a
        contiguous float64 [B][n_vars][X] device tensor to write into also that tensor: max_marginals[b][v][s] = the best
        score of any assignment with variable v in state s (natural log; -inf where none has a positive potential).  Ties
        are broken as include/mlbp_exactmap.h says; the bits of every output depend on the graph and the cutset alone.
        cutset: as in exact_inference.  self.msgs is neither read nor written."""
        from . import exactmap as K
        topo = self.topo
        pl, a = self._cutset_args(K, K.ExactMapArgs, cutset, 'exact_map needs float64 pairwise tables')
        if max_marginals is True:
            max_marginals = torch.empty(self.B, topo.n_vars, self.X, dtype=torch.float64, device=self.device)
        elif max_marginals is False:
            max_marginals = None
        if max_marginals is not None:
            a.max_marginals = self._tensor(max_marginals, (self.B, topo.n_vars, self.X), 'max_marginals',
                                           message='max_marginals must be True or a contiguous float64 device tensor [B][n_vars][X]')
        assignment = torch.empty(self.B, topo.n_vars, dtype=torch.int32, device=self.device)
        score = torch.empty(self.B, dtype=torch.float64, device=self.device)
        a.assignment, a.score = assignment.data_ptr(), score.data_ptr()
        work = self._workspace(a, K.workspace_bytes(self.B, self.X, topo.n_vars, topo.P, topo.U, pl.n_forest, pl.n_cut,
                                                    max_marginals is not None))
        K.check(K.lib.mlbp_exactmap_f64(C.byref(a), _stream_ptr(self.device)))
        return (assignment, score) if max_marginals is None else (assignment, score, max_marginals)

    # ---- the best assignment among listed cutset states (the listed mode of include/mlbp_exactmap.h) ----------
    def cutset_map(self, configs, cutset=None, entry=False):
        """The best assignment among ALL assignments whose cutset state is LISTED -- for the graphs whose cutset has more joint
        states than exact_map() walks (more than 65536: K5 and up at X = 64).  configs: contiguous int32 [B][N][n_cut] device
        tensor, configs[b][i][q] the state of cutset variable q (cutset order) in entry i; 1 <= N <= 65536.  For every entry
        the conditioned forest is completed optimally, as exact_map() does for every configuration; the entry of the largest
        value wins, ties to the lowest entry index, and then exact_map()'s tie rule.  Returns (assignment int32 [B][n_vars],
        score float64 [B]) device tensors, and with entry=True also entry int32 [B], the index of the winning entry.  A list
        that holds the cutset state of an assignment x returns a score no lower than x's; the full list in index order returns
        exact_map()'s bits.  The list may repeat a configuration.  A graph with a state outside [0, X) in its list gets
        assignment -1, score NaN and entry -1.  The bits depend on the graph, the cutset and the list alone.  cutset: as in
        exact_inference; at most 16 variables, no limit on X^len(cutset).  On a tree configs is [B][N][0].  self.msgs is
        neither read nor written."""
        from . import cutsetis as KP, exactmap as K
        topo = self.topo
        pl, a = self._cutset_args(KP, K.ExactMapArgs, cutset, 'cutset_map needs float64 pairwise tables')       # the listed check of the plan
        configs_ptr = self._tensor(configs, (self.B, None, pl.n_cut), 'configs', '[B][N][n_cut]', dtype=torch.int32)
        a.N = N = _listed_count(configs.shape[1], K, 'N')
        if pl.n_cut:
            a.configs = configs_ptr
        assignment = torch.empty(self.B, topo.n_vars, dtype=torch.int32, device=self.device)
        score = torch.empty(self.B, dtype=torch.float64, device=self.device)
        a.assignment, a.score = assignment.data_ptr(), score.data_ptr()
        won = None
        if entry:
            won = torch.empty(self.B, dtype=torch.int32, device=self.device)
            a.entry = won.data_ptr()
        work = self._workspace(a, K.listed_workspace_bytes(self.B, self.X, topo.n_vars, topo.P, topo.U, pl.n_forest, N))
        K.check(K.lib.mlbp_exactmap_f64(C.byref(a), _stream_ptr(self.device)))
        return (assignment, score, won) if entry else (assignment, score)

    def _search_list(self, roots, n_samples, seed, uniforms, cutset, entry0='sweeps', tol=1e-6, max_rounds=50):
        """The list of search_map(): (configs int32 [B][N][n_cut], the assignment of entry 0, its score[s]).  entry0 =
        'sweeps': map_sweep's assignment and its score; 'settled': map_converge's, and the scores are the pair (map_converge's,
        map_sweep's)."""
        from . import cutset as K0, cutsetis as KP
        if entry0 not in ('sweeps', 'settled'):
            raise ValueError("entry0 must be 'sweeps' or 'settled'")
        N = _listed_count(n_samples, KP)
        pl, _ = self._cutset_args(KP, KP.CutsetisArgs, cutset, 'search_map needs float64 pairwise tables')
        cut = [int(v) for v in pl.words[K0.PLAN_HEADER:K0.PLAN_HEADER + pl.n_cut]]
        x_bp, score_bp = self.map_sweep(roots, init=True)
        if entry0 == 'settled':
            x_bp, settled = self.map_converge(roots, tol=tol, max_rounds=max_rounds, init=True)[:2]
            score_bp = (settled, score_bp)
        configs = torch.empty(self.B, N, pl.n_cut, dtype=torch.int32, device=self.device)
        if cut:
            configs[:, 0] = x_bp.index_select(1, torch.tensor(cut, dtype=torch.int64, device=self.device))
            if N > 1:
                self.sweep(roots, init=True)                    # after map_sweep: both write self.msgs
                drawn, _ = self.cutset_draw(N - 1, seed=None if uniforms is not None else seed, uniforms=uniforms, cutset=cutset)
                configs[:, 1:] = drawn
        return configs, x_bp, score_bp

    def search_map(self, roots, n_samples=256, seed=0, uniforms=None, cutset=None, entry0='sweeps', tol=1e-6, max_rounds=50):
        """Search decoding beyond exact_map()'s limit: cutset_map() over a list made of the max-product answer and of draws
        from the sum-product messages.  Entry 0 of the list is the cutset state of map_sweep(roots)'s assignment; entries 1 to
        n_samples - 1 are cutset_draw(n_samples - 1, ...) on the messages of sweep(roots, init=True), which runs AFTER
        map_sweep -- both write self.msgs.  Returns (assignment int32 [B][n_vars], score float64 [B], score_bp float64 [B])
        device tensors, score_bp the score of map_sweep's assignment: score >= score_bp up to the rounding of the two sums of
        logarithms, because the max-product assignment is among those the list admits.  n_samples = 1 is the optimal
        completion of the max-product cutset state alone.  seed / uniforms ([B][n_samples - 1][n_cut]) as cutset_draw takes
        them; uniforms replaces seed.  cutset: as in cutset_map.
        entry0='settled' takes entry 0 from map_converge(roots, tol, max_rounds) in the place of map_sweep(roots): the call then
        returns (assignment, score, score_settled, score_bp), score >= score_settled in the same sense, and score_bp still
        map_sweep's score, so that a caller sees both.  The default call is untouched by this."""
        configs, _, score_bp = self._search_list(roots, n_samples, seed, uniforms, cutset, entry0, tol, max_rounds)
        assignment, score = self.cutset_map(configs, cutset=cutset)
        return (assignment, score) + (score_bp if entry0 == 'settled' else (score_bp,))

    # ---- the M best whole assignments, ranked (include/mlbp_exactmbest.h) ------------------------------------
    def exact_mbest(self, m, cutset=None):
        """The TRUE `m` jointly most probable assignments of every graph, best first, by cutset conditioning -- exact_map()
        returns the first of them alone.  Returns (assignments int32 [B][m][n_vars] in GraphTopology.var_ids order, scores
        float64 [B][m], n_found int32 [B]) device tensors: scores are the log-potentials of the rows, non-increasing;
        n_found = min(m, the number of assignments of positive potential), and the rows from n_found on read -1 and -inf.
        1 <= m <= 16.  The order among equal values is the one include/mlbp_exactmbest.h fixes; the bits of every output
        depend on the graph, the cutset and m's prefix alone: the first rows of a longer list are the shorter list.
        cutset: as in exact_inference.  self.msgs is neither read nor written."""
        from . import exactmbest as K
        if not 1 <= int(m) <= K.MAX_M:
            raise ValueError('m must be in [1, %d]' % K.MAX_M)
        topo, m = self.topo, int(m)
        pl, a = self._cutset_args(K, K.ExactMbestArgs, cutset, 'exact_mbest needs float64 pairwise tables')
        assignments = torch.empty(self.B, m, topo.n_vars, dtype=torch.int32, device=self.device)
        scores = torch.empty(self.B, m, dtype=torch.float64, device=self.device)
        n_found = torch.empty(self.B, dtype=torch.int32, device=self.device)
        a.M, a.assignments, a.scores, a.n_found = m, assignments.data_ptr(), scores.data_ptr(), n_found.data_ptr()
        work = self._workspace(a, K.workspace_bytes(self.B, self.X, topo.n_vars, topo.P, topo.U, pl.n_forest, pl.n_cut, m))
        K.check(K.lib.mlbp_exactmbest_f64(C.byref(a), _stream_ptr(self.device)))
        return assignments, scores, n_found

    # ---- the M best among listed cutset states (the listed mode of include/mlbp_exactmbest.h) ------------------
    def cutset_mbest(self, configs, m, cutset=None, entries=False):
        """The TRUE `m` best assignments among ALL assignments whose cutset state is LISTED, best first -- for the graphs whose
        cutset has more joint states than exact_mbest() walks (K5 and up at X = 64).  configs: contiguous int32 [B][N][n_cut]
        device tensor as cutset_map() takes it; 1 <= N <= 65536, 1 <= m <= 16.  Returns (assignments int32 [B][m][n_vars],
        scores float64 [B][m], n_found int32 [B]) device tensors as exact_mbest() does, and with entries=True also entries
        int32 [B][m]: the index of the list entry every row lies under, -1 behind n_found.  An entry whose cutset state repeats
        that of an entry of lower index is ignored, so the rows are pairwise distinct; ties go to the lower entry index, then to
        the lower rank inside the entry.  Row 0 is cutset_map()'s answer on the same list; the full list in index order
        returns exact_mbest()'s bits.  A graph with a state outside [0, X) in its list gets n_found -1, assignments -1,
        scores NaN and entries -1.  The bits depend on the graph, the cutset, the list and m's prefix alone.  cutset: as in
        cutset_map.  self.msgs is neither read nor written."""
        from . import cutsetis as KP, exactmbest as K
        if not 1 <= int(m) <= K.MAX_M:
            raise ValueError('m must be in [1, %d]' % K.MAX_M)
        topo, m = self.topo, int(m)
        pl, a = self._cutset_args(KP, K.ExactMbestArgs, cutset, 'cutset_mbest needs float64 pairwise tables')    # the listed check of the plan
        configs_ptr = self._tensor(configs, (self.B, None, pl.n_cut), 'configs', '[B][N][n_cut]', dtype=torch.int32)
        a.N = N = _listed_count(configs.shape[1], K, 'N')
        if pl.n_cut:
            a.configs = configs_ptr
        assignments = torch.empty(self.B, m, topo.n_vars, dtype=torch.int32, device=self.device)
        scores = torch.empty(self.B, m, dtype=torch.float64, device=self.device)
        n_found = torch.empty(self.B, dtype=torch.int32, device=self.device)
        a.M, a.assignments, a.scores, a.n_found = m, assignments.data_ptr(), scores.data_ptr(), n_found.data_ptr()
        under = None
        if entries:
            under = torch.empty(self.B, m, dtype=torch.int32, device=self.device)
            a.entries = under.data_ptr()
        work = self._workspace(a, K.listed_workspace_bytes(self.B, self.X, topo.n_vars, topo.P, topo.U, pl.n_forest, N, m))
        K.check(K.lib.mlbp_exactmbest_f64(C.byref(a), _stream_ptr(self.device)))
        return (assignments, scores, n_found, under) if entries else (assignments, scores, n_found)

    def search_mbest(self, roots, m, n_samples=256, seed=0, uniforms=None, cutset=None, entry0='sweeps', tol=1e-6, max_rounds=50):
        """Ranked search decoding beyond exact_mbest()'s limit: cutset_mbest() over search_map()'s list -- entry 0 the cutset
        state of map_sweep(roots)'s assignment, entries 1 to n_samples - 1 cutset_draw() draws on the messages of
        sweep(roots, init=True); both write self.msgs.  Returns (assignments int32 [B][m][n_vars], scores float64 [B][m],
        n_found int32 [B], score_bp float64 [B]) device tensors, score_bp the score of map_sweep's assignment:
        scores[:, 0] >= score_bp up to the rounding of the two sums of logarithms, because the max-product assignment is among
        those the list admits.  The rows are the true m best among the assignments whose cutset state was listed; the draws
        repeat states, and a repeat counts once.  seed / uniforms and cutset: as in search_map; so is entry0='settled', which
        returns (assignments, scores, n_found, score_settled, score_bp) with scores[:, 0] >= score_settled."""
        configs, _, score_bp = self._search_list(roots, n_samples, seed, uniforms, cutset, entry0, tol, max_rounds)
        assignments, scores, n_found = self.cutset_mbest(configs, m, cutset=cutset)
        return (assignments, scores, n_found) + (score_bp if entry0 == 'settled' else (score_bp,))

    # ---- whole assignments drawn from the model itself (include/mlbp_exactsample.h) ---------------------
    def exact_sample(self, n_samples=1, seed=None, uniforms=None, cutset=None, log_z=False, score=False):
        """Draws n_samples whole assignments per graph from the MODEL ITSELF by cutset conditioning -- what sample() does only
        on a tree: draw the cutset's joint state with probability Z_c / Z, solve the conditioned forest by one pass up, draw
        the free variables from the roots down.  Returns (samples int32 [S][B][n_vars] in GraphTopology.var_ids order, logp
        float64 [S][B]) device tensors; logp is the true log-probability of the draw, score(x) - log Z, on loopy graphs too
        -- it equals exact_inference(labels=samples[s])'s joint_logp.  log_z=True appends log Z [B], score=True the
        log-potential of every draw [S][B], in that order.  Exactly one of `seed` and `uniforms`, as in sample(): uniforms is
        a contiguous float64 [S][B][n_vars] device tensor of numbers in [0, 1) (entry 0 draws the cutset's state, entries
        1 .. len(cutset)-1 are not read, the rest draw the free variables); seed means torch.rand((S, B, n_vars),
        dtype=float64, device=..., generator=torch.Generator(device).manual_seed(seed)).  cutset: as in exact_inference.  A
        graph whose Z is zero or not finite gets samples -1 and logp NaN.  self.msgs is neither read nor written."""
        from . import exactsample as K
        _exactly_one(seed, uniforms)
        topo, S = self.topo, int(n_samples)
        if S <= 0:
            raise ValueError('n_samples must be positive')
        pl, a = self._cutset_args(K, K.ExactSampleArgs, cutset, 'exact_sample needs float64 pairwise tables')
        uniforms = self._uniforms(seed, uniforms, (S, self.B, topo.n_vars), '[n_samples][B][n_vars]')
        a.S, a.uniforms = S, uniforms.data_ptr()
        samples = torch.empty(S, self.B, topo.n_vars, dtype=torch.int32, device=self.device)
        logp = torch.empty(S, self.B, dtype=torch.float64, device=self.device)
        a.samples, a.logp = samples.data_ptr(), logp.data_ptr()
        out = [samples, logp]
        if log_z:
            out.append(torch.empty(self.B, dtype=torch.float64, device=self.device))
            a.log_z = out[-1].data_ptr()
        if score:
            out.append(torch.empty(S, self.B, dtype=torch.float64, device=self.device))
            a.score = out[-1].data_ptr()
        work = self._workspace(a, K.workspace_bytes(self.B, S, self.X, topo.n_vars, topo.P, topo.U, pl.n_forest, pl.n_cut))
        K.check(K.lib.mlbp_exactsample_f64(C.byref(a), _stream_ptr(self.device)))
        return tuple(out)

    # ---- draws beyond the exact limit: resampling listed cutset states (the listed mode of include/mlbp_exactsample.h) ----
    def cutset_resample(self, configs, log_q, n_samples=1, seed=None, uniforms=None, cutset=None, log_z=False, score=False,
                        entry=False, ess=False):
        """Draws n_samples whole assignments per graph by sampling-importance-resampling over a LIST of cutset states -- for
        the graphs whose cutset has more joint states than exact_sample() walks (more than 65536: K5 and up at X = 64).
        configs: contiguous int32 [B][N][n_cut] device tensor, configs[b][i][q] the state of cutset variable q (cutset order)
        in entry i; log_q: contiguous float64 [B][N], the natural log of the probability a proposal gave each entry -- the
        list cutset_draw() and cutset_proposal() return and cutset_estimate() takes; 1 <= N <= 65536.  For every entry the
        conditioned forest is solved exactly and weighted by w_i = Z_c / q(c_i); a draw picks entry i with probability
        w_i / sum w, sets the cutset variables to its row and draws the free variables from the conditioned forest exactly, as
        exact_sample() does.  Returns (samples int32 [S][B][n_vars], logp float64 [S][B]) device tensors, then with log_z=True
        log_z_hat [B] (cutset_estimate()'s estimate of log Z on the same list), with score=True the log-potential of every
        draw [S][B], with entry=True the drawn entry's index int32 [S][B], with ess=True the effective size of the list [B],
        in that order.  logp is the log-probability of the draw GIVEN THE LIST and the entry: logp = score - log_q[entry] -
        (log_z_hat + log N) up to rounding; score - log_z_hat estimates log p(x).  The draws follow a distribution that tends
        to the model's as N grows; ess says how close the list is.  With the full list in index order and log_q = 0 the
        samples, logp and score are exact_sample()'s bits.  Exactly one of `seed` and `uniforms`, as in exact_sample():
        uniforms [S][B][n_vars], entry 0 picks the list entry, entries n_cut.. draw the free variables.  A graph with a state
        outside [0, X) or a log_q that is not finite gets samples -1, entry -1 and NaN; one whose listed weights are all
        zero samples -1, logp NaN, log_z_hat -inf, ess 0.  The list may repeat a state.  cutset: as in exact_inference; at
        most 16 variables, no limit on X^len(cutset).  On a tree configs is [B][N][0].  self.msgs is neither read nor
        written."""
        from . import cutsetis as KP, exactsample as K
        _exactly_one(seed, uniforms)
        topo, S = self.topo, int(n_samples)
        if S <= 0:
            raise ValueError('n_samples must be positive')
        pl, a = self._cutset_args(KP, K.ExactSampleArgs, cutset, 'cutset_resample needs float64 pairwise tables')   # the listed check of the plan
        a.log_q = self._tensor(log_q, (self.B, None), 'log_q', '[B][N]')
        a.N = N = _listed_count(log_q.shape[1], K, 'N')
        configs_ptr = self._tensor(configs, (self.B, N, pl.n_cut), 'configs', '[B][N][n_cut]', dtype=torch.int32)
        if pl.n_cut:
            a.configs = configs_ptr
        uniforms = self._uniforms(seed, uniforms, (S, self.B, topo.n_vars), '[n_samples][B][n_vars]')
        a.S, a.uniforms = S, uniforms.data_ptr()
        samples = torch.empty(S, self.B, topo.n_vars, dtype=torch.int32, device=self.device)
        logp = torch.empty(S, self.B, dtype=torch.float64, device=self.device)
        a.samples, a.logp = samples.data_ptr(), logp.data_ptr()
        out = [samples, logp]
        if log_z:
            out.append(torch.empty(self.B, dtype=torch.float64, device=self.device))
            a.log_z = out[-1].data_ptr()
        if score:
            out.append(torch.empty(S, self.B, dtype=torch.float64, device=self.device))
            a.score = out[-1].data_ptr()
        if entry:
            out.append(torch.empty(S, self.B, dtype=torch.int32, device=self.device))
            a.entry = out[-1].data_ptr()
        if ess:
            out.append(torch.empty(self.B, dtype=torch.float64, device=self.device))
            a.ess = out[-1].data_ptr()
        work = self._workspace(a, K.listed_workspace_bytes(self.B, S, self.X, topo.n_vars, topo.P, topo.U, pl.n_forest, N))
        K.check(K.lib.mlbp_exactsample_f64(C.byref(a), _stream_ptr(self.device)))
        return tuple(out)

    def estimate_sample(self, roots=None, n_samples=1, n_list=256, seed=0, cutset=None, proposal='messages'):
        """Whole sets of guesses for the sentences beyond exact_sample()'s limit: cutset_resample() over a list of n_list
        cutset states drawn from loopy BP.  proposal='messages' makes the list with cutset_draw(n_list, seed=seed) on the
        messages self.msgs holds; given `roots`, sweep(roots, init=True) runs first -- THAT WRITES self.msgs --, with roots=None
        the messages are used as they stand.  proposal='sample' makes it with cutset_proposal(roots, n_list, seed=seed), which
        needs roots and sweeps for every draw.  The draws' uniforms are torch.rand((n_samples, B, n_vars), dtype=float64,
        device=..., generator=torch.Generator(device).manual_seed(seed + 1)).  Returns (samples int32 [S][B][n_vars],
        logp_hat float64 [S][B], log_z_hat [B], ess [B]) device tensors: logp_hat = score - log_z_hat, the estimate of the
        log-probability of every draw under the model (its error is log_z_hat's, the same for every draw of a graph);
        ess / n_list near 1 says the list stands in well for the cutset's distribution."""
        if proposal not in ('sample', 'messages'):
            raise ValueError("proposal must be 'sample' or 'messages', not %r" % (proposal,))
        if proposal == 'sample':
            if roots is None:
                raise ValueError("proposal='sample' needs roots")
            configs, log_q = self.cutset_proposal(roots, n_list, seed=int(seed), cutset=cutset)
        else:
            self._cutdraw_refuse('estimate_sample')
            if roots is not None:
                self.sweep(roots, init=True)
            configs, log_q = self.cutset_draw(n_list, seed=int(seed), cutset=cutset)
        samples, _, log_z_hat, score, ess = self.cutset_resample(configs, log_q, n_samples=n_samples, seed=int(seed) + 1, cutset=cutset,
                                                                 log_z=True, score=True, ess=True)
        return samples, score - log_z_hat.unsqueeze(0), log_z_hat, ess

    # ---- the exact pair marginals and the true gradient (include/mlbp_exactgrad.h) ---------------------
    def _exactgrad(self, cutset, marginals=None, pair_marginals=None, expect=None, grad=None, labels=None, listed=None):
        """One mlbp_exactgrad_f64 call: log_z [B], and whichever of the optional outputs is given (expect, grad: (ee, ed)).
        listed: (configs, log_q) of a listed call, which returns log_z_hat in the place of log_z."""
        from . import exactgrad as K
        topo = self.topo
        if listed is None:
            pl, a = self._cutset_args(K, K.ExactGradArgs, cutset, 'the exact pair marginals and gradient need float64 pairwise tables')
        else:
            from . import cutsetis as KP
            tail = K.listed_args()()                            # mlbp_exactgrad_listed_args: the exact call's args, then the list
            pl, a = self._cutset_args(KP, lambda: tail.args, cutset,                      # the listed check of the plan
                                      'the estimated pair marginals and gradient need float64 pairwise tables')
            configs, log_q = listed
            tail.log_q = self._tensor(log_q, (self.B, None), 'log_q', '[B][N]')
            tail.N = N = _listed_count(log_q.shape[1], K, 'N')
            configs_ptr = self._tensor(configs, (self.B, N, pl.n_cut), 'configs', '[B][N][n_cut]', dtype=torch.int32)
            if pl.n_cut:
                tail.configs = configs_ptr
            a.plan_words = -a.plan_words                        # the header's sign of a list behind the struct

        def checked(t, shape, what):                           # the message prints the sizes themselves
            return self._tensor(t, shape, what, list(shape))
        if marginals is not None:
            a.marginals = checked(marginals, (self.B, topo.n_vars, self.X), 'marginals')
        if pair_marginals is not None:
            a.pair_marginals = checked(pair_marginals, (self.B, topo.P, self.X, self.X), 'pair_marginals')
        keep = []
        if expect is not None or grad is not None:
            if getattr(self, 'phi_en_en', None) is None:
                raise RuntimeError('set_features() first')
            if topo.U and getattr(self, '_unary_obs', None) is None:
                raise RuntimeError('set_observations() first')
            a.F_ee, a.F_ed, a.Vde = int(self.phi_en_en.shape[2]), int(self.phi_en_de.shape[2]), int(self.phi_en_de.shape[1])
            a.phi_en_en, a.phi_en_en_w1, a.phi_en_de = self.phi_en_en.data_ptr(), self.phi_en_en_w1.data_ptr(), self.phi_en_de.data_ptr()
            a.pair_phi, a.unary_kind = self._pair_phi.data_ptr(), self._unary_kind.data_ptr()
            if topo.U:
                a.unary_obs = self._unary_obs.data_ptr()
            if expect is not None:
                a.expect_ee, a.expect_ed = checked(expect[0], (self.B, a.F_ee), 'out_ee'), checked(expect[1], (self.B, a.F_ed), 'out_ed')
            if grad is not None:
                a.grad_ee, a.grad_ed = checked(grad[0], (self.B, a.F_ee), 'out_ee'), checked(grad[1], (self.B, a.F_ed), 'out_ed')
                if labels is None and getattr(self, '_labels', None) is None:
                    raise RuntimeError('exact_gradient needs labels: pass them or set_observations() first')
                lab = self._rows_i32(self._labels if labels is None else labels, 'labels')
                keep.append(lab)
                a.labels = lab.data_ptr()
        log_z = torch.empty(self.B, dtype=torch.float64, device=self.device)
        a.log_z = log_z.data_ptr()
        shape = (self.B, self.X, topo.n_vars, topo.P, topo.U, pl.n_forest)
        work = self._workspace(a, K.workspace_bytes(*shape + (pl.n_cut,)) if listed is None else K.listed_workspace_bytes(*shape + (N,)))
        K.check(K.lib.mlbp_exactgrad_f64(C.byref(a), _stream_ptr(self.device)))
        return log_z

    def exact_pair_marginals(self, out=None, cutset=None):
        """The TRUE marginal of every pairwise factor by cutset conditioning -- what pair_beliefs() approximates on a loopy
        graph: float64 device tensor [B][P][X][X], out[b][p][i][j] = p(x_a = i, x_b = j) in the axes of factor p's table.
        out: optional contiguous float64 [B][P][X][X] device tensor to write into; cutset: as in exact_inference.  self.msgs is
        neither read nor written."""
        if out is None:
            out = torch.empty(self.B, self.topo.P, self.X, self.X, dtype=torch.float64, device=self.device)
        self._exactgrad(cutset, pair_marginals=out)
        return out

    def exact_gradient(self, labels=None, out_ee=None, out_ed=None, pair_marginals=None, marginals=None, cutset=None, expect_only=False):
        """The TRUE per-graph likelihood gradient -- what gradient() approximates from BP beliefs: (grad_ee [B][F_ee], grad_ed
        [B][F_ed], log_z [B]) device tensors, grad = observed features at `labels` - expected features under the model's own
        pair marginals and marginals (include/mlbp_exactgrad.h; the unary term uses the variable's true marginal, not the
        reference's normalised table).  With tables exp(phi . theta) this is the derivative of exact_inference's joint_logp in
        theta.  Features, selectors and observed columns are those of set_features() / set_observations(); labels=None uses
        the labels of set_observations().  expect_only=True returns the expected features instead of the gradient and needs no
        labels.  out_ee / out_ed, pair_marginals ([B][P][X][X]) and marginals ([B][n_vars][X]): optional contiguous float64
        device tensors to write into (the last two are written only when given).  cutset: as in exact_inference.  self.msgs is
        neither read nor written."""
        self._need_f64_tables('exact_gradient')
        if getattr(self, 'phi_en_en', None) is None:
            raise RuntimeError('set_features() first')
        F_ee, F_ed = int(self.phi_en_en.shape[2]), int(self.phi_en_de.shape[2])
        if out_ee is None:
            out_ee = torch.empty(self.B, F_ee, dtype=torch.float64, device=self.device)
        if out_ed is None:
            out_ed = torch.empty(self.B, F_ed, dtype=torch.float64, device=self.device)
        out = (out_ee, out_ed)
        log_z = self._exactgrad(cutset, marginals=marginals, pair_marginals=pair_marginals, expect=out if expect_only else None,
                                grad=None if expect_only else out, labels=labels)
        return out_ee, out_ed, log_z

    # ---- the gradient beyond the exact limit: listed cutset states (the listed mode of include/mlbp_exactgrad.h) ----------
    def cutset_pair_marginals(self, configs, log_q, out=None, cutset=None):
        """An ESTIMATE of the marginal of every pairwise factor over a LIST of cutset states -- for the graphs whose cutset has
        more joint states than exact_pair_marginals() walks (more than 65536: K5 and up at X = 64): float64 device tensor
        [B][P][X][X] in the axes of each factor's table.  configs (int32 [B][N][n_cut]) and log_q (float64 [B][N]) are the list
        cutset_draw() and cutset_proposal() return and cutset_estimate() takes; every entry's conditioned forest is solved
        exactly and weighted by w_i = Z_c / q(c_i), and the result is sum of w_i M_p|c_i / sum of w_i: self-normalised, consistent,
        not unbiased.  The full list in index order with log_q = 0 returns exact_pair_marginals()'s bits.  A graph with a state
        outside [0, X) or a log_q that is not finite keeps what `out` held.  out: optional contiguous float64 [B][P][X][X]
        device tensor to write into; cutset: as in exact_inference, at most 16 variables, no limit on X^len(cutset).
        self.msgs is neither read nor written."""
        if out is None:
            out = torch.empty(self.B, self.topo.P, self.X, self.X, dtype=torch.float64, device=self.device)
        self._exactgrad(cutset, pair_marginals=out, listed=(configs, log_q))
        return out

    def cutset_gradient(self, configs, log_q, labels=None, out_ee=None, out_ed=None, pair_marginals=None, marginals=None, cutset=None,
                        expect_only=False):
        """An ESTIMATE of the per-graph likelihood gradient over a LIST of cutset states -- exact_gradient() for the graphs
        beyond its limit: (grad_ee [B][F_ee], grad_ed [B][F_ed], log_z_hat [B]) device tensors.  The expected features are
        formed from the self-normalised estimates of the pair marginals and marginals (cutset_pair_marginals(),
        cutset_estimate()): grad = observed features at `labels` - sum of w_i E[features | c_i] / sum of w_i; log_z_hat =
        ln(mean of w_i) is cutset_estimate()'s estimate of log Z on the same list.  configs, log_q: as in
        cutset_pair_marginals(); the other arguments as in exact_gradient().  The full list in index order with log_q = 0
        returns exact_gradient()'s bits and log_z - ln N.  A graph with a state outside [0, X) or a log_q that is not finite gets
        NaN and keeps its pair_marginals and marginals; one whose listed weights are all zero gets exact_gradient()'s Z = 0
        answer.  The bits depend on the graph, the cutset and the list alone.  self.msgs is neither read nor written."""
        self._need_f64_tables('cutset_gradient')
        if getattr(self, 'phi_en_en', None) is None:
            raise RuntimeError('set_features() first')
        F_ee, F_ed = int(self.phi_en_en.shape[2]), int(self.phi_en_de.shape[2])
        if out_ee is None:
            out_ee = torch.empty(self.B, F_ee, dtype=torch.float64, device=self.device)
        if out_ed is None:
            out_ed = torch.empty(self.B, F_ed, dtype=torch.float64, device=self.device)
        out = (out_ee, out_ed)
        log_z_hat = self._exactgrad(cutset, marginals=marginals, pair_marginals=pair_marginals, expect=out if expect_only else None,
                                    grad=None if expect_only else out, labels=labels, listed=(configs, log_q))
        return out_ee, out_ed, log_z_hat

    def estimate_gradient(self, roots=None, n_list=256, seed=0, cutset=None, proposal='messages', labels=None):
        """The gradient for the sentences beyond exact_gradient()'s limit: cutset_gradient() over a list of n_list cutset states
        drawn from loopy BP, made as estimate_sample() makes its list.  proposal='messages': cutset_draw(n_list, seed=seed) on
        the messages self.msgs holds; given `roots`, sweep(roots, init=True) runs first -- THAT WRITES self.msgs --, with
        roots=None the messages are used as they stand.  proposal='sample': cutset_proposal(roots, n_list, seed=seed), which
        needs roots and sweeps for every draw.  Returns (grad_ee [B][F_ee], grad_ed [B][F_ed], log_z_hat [B]) device tensors."""
        if proposal not in ('sample', 'messages'):
            raise ValueError("proposal must be 'sample' or 'messages', not %r" % (proposal,))
        if proposal == 'sample':
            if roots is None:
                raise ValueError("proposal='sample' needs roots")
            configs, log_q = self.cutset_proposal(roots, n_list, seed=int(seed), cutset=cutset)
        else:
            self._cutdraw_refuse('estimate_gradient')
            if roots is not None:
                self.sweep(roots, init=True)
            configs, log_q = self.cutset_draw(n_list, seed=int(seed), cutset=cutset)
        return self.cutset_gradient(configs, log_q, labels=labels, cutset=cutset)

    def treelike_inference(self, iterations, roots):
        """`iterations` sweeps if the graph is loopy, else one (LBP.py:219); `roots` replaces the
        per-sweep random.sample draw (LBP.py:223).  Returns the number of sweeps run."""
        if self.is_loopy is None:
            raise RuntimeError('initialize() first')
        n = iterations if self.is_loopy else 1
        if len(roots) < n:
            raise ValueError('need %d roots, got %d' % (n, len(roots)))
        self.sweep(list(roots)[:n])
        return n

    # ---- read-outs --------------------------------------------------------------------------------
    def marginals(self, out=None):
        """[B][n_vars][X] in GraphTopology.var_ids order (VariableNode.get_marginal, LBP.py:392-400)."""
        if out is None:
            out = torch.empty(self.B, self.topo.n_vars, self.X, dtype=torch.float64, device=self.device)
        _ffi.check(_ffi.lib.mlbp_marginals_f64(self.msgs.data_ptr(), self.B, self.topo.n_msgs, self.X,
                                               self.topo.n_vars, self._in_off.data_ptr(),
                                               self._in_slots.data_ptr(), 1 if self.normalize_messages else 0,
                                               out.data_ptr(), _stream_ptr(self.device)))
        return out

    def log_posterior(self, labels, marginals=None):
        """[B] sum over variables of log marginal[label] (FactorGraph.get_posterior_probs,
        LBP.py:247-259).  labels: [B][n_vars] integer label indices."""
        lab = np.asarray(labels, dtype=np.int64).reshape(self.B, self.topo.n_vars)
        if lab.min() < 0 or lab.max() >= self.X:
            raise IndexError('label index out of range')
        lab_d = torch.from_numpy(lab.astype(np.int32)).to(self.device)
        m = self.marginals() if marginals is None else marginals
        out = torch.empty(self.B, dtype=torch.float64, device=self.device)
        _ffi.check(_ffi.lib.mlbp_log_posterior_f64(m.data_ptr(), lab_d.data_ptr(), self.B, self.topo.n_vars,
                                                   self.X, out.data_ptr(), _stream_ptr(self.device)))
        return out

    # ---- beliefs / gradient (LBP.py:528-619, 301-320) ---------------------------------------------
    def _need_f64_tables(self, what):
        if self.pair_tables is not None and self.pair_tables.dtype != torch.float64:
            raise NotImplementedError('%s needs float64 pairwise tables' % what)

    def _pair_slots(self):
        """device int32 [P] message slots of the dim-0 / dim-1 variable -> factor messages."""
        if not hasattr(self, '_c_slot'):
            topo = self.topo
            c, r = [], []
            for j in topo.pair_factors:
                k0 = 0 if topo.fac_dim[2 * j] == 0 else 1          # varset position sitting on table axis 0
                c.append(int(topo.v2f[2 * j + k0]))
                r.append(int(topo.v2f[2 * j + 1 - k0]))
            self._c_slot = torch.tensor(c or [0], dtype=torch.int32, device=self.device)
            self._r_slot = torch.tensor(r or [0], dtype=torch.int32, device=self.device)
        return self._c_slot, self._r_slot

    def pair_beliefs(self):
        self._need_f64_tables('pair_beliefs')
        """[B][P][X][X]: FactorNode.get_factor_beliefs of every pairwise factor (LBP.py:543-569)."""
        c, r = self._pair_slots()
        out = torch.empty(self.B, self.topo.P, self.X, self.X, dtype=torch.float64, device=self.device)
        _ffi.check(_ffi.lib.mlbp_pair_beliefs_f64(self.msgs.data_ptr(), self.B, self.topo.n_msgs, self.X, self.topo.P,
                                                  self.pair_tables.data_ptr(), self.pair_tab.data_ptr(),
                                                  self.pair_tables.shape[0], c.data_ptr(), r.data_ptr(),
                                                  out.data_ptr(), _stream_ptr(self.device)))
        return out

    def set_features(self, phi_en_en, phi_en_en_w1, phi_en_de, pair_phi, unary_kind, share_with=None):
        """Feature tensors (X,X,F_ee) x2 and (X,Vde,F_ed) shared by the batch, and the per-slot
        selector FactorNode.get_phi implies (LBP.py:469-480): pair_phi[p] in {0: gap > 1, 1: gap == 1},
        unary_kind[u] in {0, 1 (en_en by gap), 2 (en_de)}."""
        dev = self.device
        if share_with is not None:
            # the other batch's device copies (and their two re-layouts), read-only: the buckets of a TiDirTrainer -- one batch per
            # sentence shape, hundreds of them -- read ONE set of feature tensors, and a grouped launch writes the gradient's
            # weighted table fragments once per distinct set (mlbp_sweep_groups_f64), not once per bucket
            if share_with.device != dev:
                raise ValueError('feature tensors can only be shared by batches of one device')
            self.phi_en_en, self.phi_en_en_w1, self.phi_en_de = share_with.phi_en_en, share_with.phi_en_en_w1, share_with.phi_en_de
            self._phi_t, self._phi_p = share_with._phi_t, share_with._phi_p
        else:
            self.phi_en_en = torch.as_tensor(phi_en_en, dtype=torch.float64).to(dev).contiguous()
            self.phi_en_en_w1 = torch.as_tensor(phi_en_en_w1, dtype=torch.float64).to(dev).contiguous()
            self.phi_en_de = torch.as_tensor(phi_en_de, dtype=torch.float64).to(dev).contiguous()
            # transposed copies [column][x][F] (a layout change only): contiguous feature slabs for unary factors
            self._phi_t = tuple(p.permute(1, 0, 2).contiguous() for p in (self.phi_en_en, self.phi_en_en_w1, self.phi_en_de))
            self._phi_p = tuple(p.permute(2, 0, 1).contiguous() for p in (self.phi_en_en, self.phi_en_en_w1))   # [F][X][X]
        X = self.X
        if tuple(self.phi_en_en.shape[:2]) != (X, X) or self.phi_en_en_w1.shape != self.phi_en_en.shape or \
                self.phi_en_de.shape[0] != X:
            raise ValueError('feature tensors must be (X,X,F_ee), (X,X,F_ee), (X,Vde,F_ed)')
        pp = np.asarray(pair_phi, dtype=np.int64).reshape(self.topo.P)
        uk = np.asarray(unary_kind, dtype=np.int64).reshape(self.topo.U)
        if (pp.size and (pp.min() < 0 or pp.max() > 1)) or (uk.size and (uk.min() < 0 or uk.max() > 2)):
            raise ValueError('pair_phi must be 0/1 and unary_kind 0/1/2')
        self._pair_phi = torch.from_numpy(np.ascontiguousarray(pp if pp.size else np.zeros(1)).astype(np.int32)).to(dev)
        self._unary_kind = torch.from_numpy(np.ascontiguousarray(uk if uk.size else np.zeros(1)).astype(np.int32)).to(dev)
        self._unary_kind_host = uk

    def set_observations(self, var_labels, unary_obs):
        """var_labels [B][n_vars]: supervised label index per variable (GraphTopology.var_ids order);
        unary_obs [B][U]: observed column of each unary factor (PotentialTable.observed_dim)."""
        topo, B, X = self.topo, self.B, self.X
        lab = np.asarray(var_labels, dtype=np.int64).reshape(B, topo.n_vars)
        obs = np.asarray(unary_obs, dtype=np.int64).reshape(B, topo.U)
        if lab.min() < 0 or lab.max() >= X:
            raise IndexError('label index out of range')
        Vde = int(self.phi_en_de.shape[1])
        for u in range(topo.U):
            lim = Vde if self._unary_kind_host[u] == 2 else X
            if obs[:, u].min() < 0 or obs[:, u].max() >= lim:
                raise IndexError('observed column out of range for unary slot %d' % u)
        pl = np.zeros((B, max(topo.P, 1), 2), dtype=np.int32)
        for p, j in enumerate(topo.pair_factors):
            k0 = 0 if topo.fac_dim[2 * j] == 0 else 1
            pl[:, p, 0] = lab[:, topo.fac_var[2 * j + k0]]
            pl[:, p, 1] = lab[:, topo.fac_var[2 * j + 1 - k0]]
        ul = np.zeros((B, max(topo.U, 1)), dtype=np.int32)
        for u, j in enumerate(topo.unary_factors):
            ul[:, u] = lab[:, topo.fac_var[2 * j]]
        dev = self.device
        self._labels = torch.from_numpy(lab.astype(np.int32)).to(dev)
        self._pair_label = torch.from_numpy(pl).to(dev)
        self._unary_label = torch.from_numpy(ul).to(dev)
        self._unary_obs = torch.from_numpy(np.ascontiguousarray(obs if topo.U else np.zeros((B, 1))).astype(np.int32)).to(dev)

    def set_unary_rows(self, row_kind, row_obs):
        """States, per row of the unary table array, the phi selector (0 / 1 / 2) and observed column of every
        factor that reads the row.  With shared pairwise tables the gradient then computes each row's expected
        features once (mlbp_unary_expectations_f64) and gathers them per factor."""
        n = int(self.unary_tables.shape[0])
        rk = np.asarray(row_kind, dtype=np.int32).reshape(-1)
        ro = np.asarray(row_obs, dtype=np.int32).reshape(-1)
        if rk.shape[0] != n or ro.shape[0] != n:
            raise ValueError('need one (kind, column) per unary table row')
        self._row_kind = torch.from_numpy(rk).to(self.device)
        self._row_obs = torch.from_numpy(ro).to(self.device)
        self._uexp = torch.zeros(n, 8, dtype=torch.float64, device=self.device)

    def _derive_unary_rows(self):
        """set_unary_rows() from (unary_tab, unary_kind, unary_obs) when every row has ONE (kind, column)."""
        if getattr(self, '_row_kind', None) is not None or not self.topo.U or self.X != 64:
            return
        tab = self.unary_tab.cpu().numpy().astype(np.int64)
        obs = self._unary_obs.cpu().numpy().astype(np.int64)
        kind = np.tile(np.asarray(self._unary_kind_host, dtype=np.int64), (self.B, 1))
        n = int(self.unary_tables.shape[0])
        rk, ro = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        rk[tab.ravel()], ro[tab.ravel()] = kind.ravel(), obs.ravel()
        if not ((rk[tab] == kind).all() and (ro[tab] == obs).all()):
            self._row_kind = False                      # a row is read with two different columns: no shortcut
            return
        rk[rk < 0], ro[ro < 0] = 0, 0
        self.set_unary_rows(rk, ro)

    def _gradient_args(self, out_ee, out_ed):
        self._need_f64_tables('the gradient')
        topo = self.topo
        F_ee, F_ed = int(self.phi_en_en.shape[2]), int(self.phi_en_de.shape[2])
        if tuple(out_ee.shape) != (self.B, F_ee) or tuple(out_ed.shape) != (self.B, F_ed):
            raise ValueError('gradient outputs must be [B][F_ee] and [B][F_ed]')
        c, r = self._pair_slots()
        a = _ffi.GradientArgs()
        a.B, a.X, a.n_msgs, a.P, a.U = self.B, self.X, topo.n_msgs, topo.P, topo.U
        a.F_ee, a.F_ed, a.Vde = F_ee, F_ed, int(self.phi_en_de.shape[1])
        a.msgs = self.msgs.data_ptr()
        if topo.P:
            a.n_pair_tables = self.pair_tables.shape[0]
            a.pair_tables, a.pair_tab = self.pair_tables.data_ptr(), self.pair_tab.data_ptr()
            a.pair_c_slot, a.pair_r_slot = c.data_ptr(), r.data_ptr()
            a.pair_phi, a.pair_label = self._pair_phi.data_ptr(), self._pair_label.data_ptr()
        if topo.U:
            a.n_unary_tables = self.unary_tables.shape[0]
            a.unary_tables, a.unary_tab = self.unary_tables.data_ptr(), self.unary_tab.data_ptr()
            a.unary_kind, a.unary_obs = self._unary_kind.data_ptr(), self._unary_obs.data_ptr()
            a.unary_label = self._unary_label.data_ptr()
        a.phi_en_en, a.phi_en_en_w1 = self.phi_en_en.data_ptr(), self.phi_en_en_w1.data_ptr()
        a.phi_en_de = self.phi_en_de.data_ptr()
        a.phi_en_en_t, a.phi_en_en_w1_t, a.phi_en_de_t = (p.data_ptr() for p in self._phi_t)
        if getattr(self, 'use_planar', True):
            a.phi_en_en_p, a.phi_en_en_w1_p = (p.data_ptr() for p in self._phi_p)
        a.grad_en_en, a.grad_en_de = out_ee.data_ptr(), out_ed.data_ptr()
        if self.use_approx_beliefs:
            a.flags |= _ffi.GRADIENT_APPROX_BELIEFS
        if getattr(self, 'pair_tables_shared', False) and getattr(self, 'use_shared_gradient', True) and not self.use_approx_beliefs:
            a.flags |= _ffi.GRADIENT_SHARED_PAIR_TABLES
            if getattr(self, '_pair_row_host', None) is not None:
                a.pair_tab_host = self._pair_row_host.ctypes.data
                if not hasattr(self, '_pair_slots_host'):      # host copy of the slot arrays: the X >= 128 gradient then only enqueues
                    self._pair_slots_host = np.ascontiguousarray(np.concatenate([
                        c.cpu().numpy(), r.cpu().numpy(), self._pair_phi.cpu().numpy()]).astype(np.int32))
                a.pair_slots_host = self._pair_slots_host.ctypes.data
            self._derive_unary_rows()
            if getattr(self, '_row_kind', None) is not None and self._row_kind is not False and F_ee == 3 and F_ed == 6:
                # rows [0, done) were written by the caller's potentials launch (mlbp_potentials_job.expect: the trainer's shared
                # pots); what is left -- all rows, or the trainer's private plane-patched ones -- is computed here
                done, n_rows = int(getattr(self, '_uexp_rows_done', 0)), int(self.unary_tables.shape[0])
                if done < n_rows:
                    _ffi.check(_ffi.lib.mlbp_unary_expectations_f64(
                        self.unary_tables[done:].data_ptr(), n_rows - done, self.X, self._row_kind[done:].data_ptr(),
                        self._row_obs[done:].data_ptr(), self._phi_t[0].data_ptr(), self._phi_t[1].data_ptr(), self._phi_t[2].data_ptr(),
                        F_ee, F_ed, int(self.phi_en_de.shape[1]), self._uexp[done:].data_ptr(), _stream_ptr(self.device)))
                a.unary_expect = self._uexp.data_ptr()
        return a

    def gradient(self, out_ee=None, out_ed=None):
        """Per-graph unregularised gradients ([B][F_ee], [B][F_ed]) from the messages in memory:
        FactorGraph.get_unregularized_gradeint (LBP.py:301-320), beliefs fused in.  (sweep(...,
        gradient=(out_ee, out_ed)) produces the same numbers inside the sweep launch.)"""
        F_ee, F_ed = int(self.phi_en_en.shape[2]), int(self.phi_en_de.shape[2])
        if out_ee is None:
            out_ee = torch.empty(self.B, F_ee, dtype=torch.float64, device=self.device)
        if out_ed is None:
            out_ed = torch.empty(self.B, F_ed, dtype=torch.float64, device=self.device)
        a = self._gradient_args(out_ee, out_ed)
        _ffi.check(_ffi.lib.mlbp_gradient_f64(C.byref(a), _stream_ptr(self.device)))
        return out_ee, out_ed

    def sum_rows(self, t, out=None):
        """Column sums of a [rows][cols] device tensor in a fixed order (mlbp_sum_rows_f64)."""
        t2 = t.reshape(t.shape[0], -1)
        if out is None:
            out = torch.empty(t2.shape[1], dtype=torch.float64, device=self.device)
        _ffi.check(_ffi.lib.mlbp_sum_rows_f64(t2.data_ptr(), t2.shape[0], t2.shape[1], out.data_ptr(),
                                              _stream_ptr(self.device)))
        return out


def sweep_groups(batches, roots, init=False, marginals=None, keep_messages=True, gradients=None, posteriors=None):
    """One minibatch of mixed graphs: batches[k] (a FactorGraphBatch: one topology, its tables and messages) is swept
    with its own root sequence roots[k] -- the reference draws roots per instance (LBP.py:223-225) and builds a
    different K_n per instance (train_mp.py:257-299).  Same results as batches[k].sweep(roots[k], ...) one by one, in fewer
    launches: the library (mlbp_sweep_groups_f64) decides group by group which fast kernel takes it, runs the groups each kernel
    takes in ONE launch sequence and the others as separate calls behind them.
    marginals: None or one [B_k][n_vars_k][X] tensor per group; gradients: None or one (g_en_en, g_en_de) pair per group
    (each group's gradient launch follows its sweeps, as in FactorGraphBatch.sweep(gradient=...)); posteriors: None or one
    (labels, out, sum_out) per group, as in FactorGraphBatch.sweep(posterior=...)."""
    if len(batches) != len(roots) or not batches:
        raise ValueError('one root sequence per batch')
    dev = batches[0].device
    got = []
    for k, fb in enumerate(batches):
        if fb.device != dev:
            raise ValueError('all groups live on one device')
        fb.sweep(roots[k], init=init, marginals=None if marginals is None else marginals[k], keep_messages=keep_messages,
                 gradient=None if gradients is None else gradients[k], posterior=None if posteriors is None else posteriors[k],
                 _collect=got)
    n = len(got)
    handles = (C.c_void_p * n)(*[p.handle for p, _, _ in got])
    args = (_ffi.SweepArgs * n)(*[a for _, a, _ in got])
    _ffi.check(_ffi.lib.mlbp_sweep_groups_f64(handles, args, n, _stream_ptr(dev)))
    return [p for p, _, _ in got]
