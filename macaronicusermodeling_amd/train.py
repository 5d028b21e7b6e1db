"""The train_mp.py-shaped outer step on the GPU: potentials -> sweeps -> gradient -> reduce -> theta.

Mirrors `batch_sgd` (train_mp.py:362-402) + `batch_sgd_accumulate` (train_mp.py:405-424) for a
whole shard of instances at once:

    pots   = exp(phi . theta^T)                       train_mp.py:220-255   mlbp_potentials_f64
    fg.initialize(); fg.treelike_inference(3)         train_mp.py:381-382   mlbp_sweep_f64 (init fused)
    g_en_en, g_en_de = fg.return_gradient()           train_mp.py:398       mlbp_gradient_f64
    p = fg.get_posterior_probs()                      train_mp.py:400       mlbp_marginals / log_posterior
    theta += sum_i lr (g_i - reg theta)               train_mp.py:405-424   mlbp_sum_rows_f64 + all-reduce

The reference applies each instance's step as its worker finishes (stale, asynchronous); here every
instance of a step sees the same theta and the steps are summed -- identical to the reference when
all tasks were pickled with the same theta.

Pairwise tables are the two shared pots (`pot_en_en`, `pot_en_en_w1`) referenced through the
table-index indirection; a unary factor's table is a COLUMN of a pot (LBP.py:702-703), read as a
row of the transposed pot the potentials kernel also writes -- no per-instance copies.
"""
import os

import numpy as np
import torch

from . import _ffi, dist as mdist
from .batch import FactorGraphBatch, _stream_ptr
from .topology import GraphTopology

# params and prediction files carry the adapt mode in their name (train_mp.py:654-656, 688-690)
ADAPT_EXT = {'user': '.user_adapt', 'experience': '.exp_adapt', None: ''}
SEARCH_ROSE = 1e-9              # search_decode: a score counts as risen above decode()'s beyond this, relative to max(1, |score|)


def _host(*tensors):
    """The tensors' host arrays."""
    return tuple(t.cpu().numpy() for t in tensors)


# ---- what TiDirTrainer's reports share: one walk over the sentence shapes, one reduction (tests/test_batch_args_cpu.py) ------
def _try(call, refused):
    """(call(), None), or (None, e) for the error e of class `refused` (None: no class) whose code says the library does not
    take this shape, MLBP_EUNSUPPORTED; every other error goes through."""
    try:
        return call(), None
    except refused or () as e:
        if e.code != _ffi.MLBP_EUNSUPPORTED:
            raise
        return None, e


def _per_shape(trainers, buckets, call, out=None, row=None, placeholder=None, refused=None, skipped=None, on_refused=None):
    """Walks the sentence shapes in `trainers` order and returns [(key, rows, result)] of the shapes that answered: result =
    call(i, trainer), i the shape's position in that order -- counted over every shape, answered or not --, rows =
    buckets[key]['rows'].  A shape whose call raises `refused` with MLBP_EUNSUPPORTED is noted in `skipped` as (predicted
    positions, instances, reason), then handed to on_refused(trainer, rows) if given; a call may also return None to pass over its
    shape unnoted.  With `out`, the per-instance list: out[row['index']] = (predicted positions,) + row(result, b) for instance b
    of a shape that answered, (predicted positions,) + placeholder for the others."""
    answered = []
    for i, (key, tr) in enumerate(trainers.items()):
        rows = buckets[key]['rows']
        res, e = _try(lambda: call(i, tr), refused)
        if e is not None:
            skipped.append((tuple(key[1]), len(rows), str(e)))
            if on_refused is not None:
                on_refused(tr, rows)
        for b, r in enumerate(rows if out is not None else ()):
            out[r['index']] = (tuple(key[1]),) + (placeholder if res is None else row(res, b))
        if res is not None:
            answered.append((key, rows, res))
    return answered


def _reduced(device, sums, maxima=()):
    """(sums, maxima) over ALL ranks as host float64 arrays: one fused all-reduce each (dist.all_reduce_sum_ / _max_), and none
    for an empty `maxima`."""
    tot = mdist.all_reduce_sum_(torch.tensor([float(v) for v in sums], dtype=torch.float64, device=device))
    top = torch.tensor([float(v) for v in maxima], dtype=torch.float64, device=device)
    return tot.cpu().numpy(), (mdist.all_reduce_max_(top) if len(maxima) else top).cpu().numpy()


class UserGraphTrainer:
    def __init__(self, spec, var_labels, unary_obs, phi_en_en, phi_en_en_w1, phi_en_de, theta_en_en, theta_en_de,
                 device='cuda:0', sweeps=3, roots=None, planes=None, domains=None, theta_dom_en_en=None,
                 theta_dom_en_de=None, skip_unchanged=False, member=False, features_of=None):
        """spec: a 'trainmp'-style spec (tests/golden/cases.py: factors carry factor_type / gap);
        var_labels [B][n_vars], unary_obs [B][U]: this rank's shard of instances.
        planes: optional per-instance sparse feature planes, a list (one entry per instance) of
        {(i, j, k): value} -- cell (i, j) of phi_en_de[:, :, k] for this instance only
        (train_mp.py:178-217 writes k = 2 'correct', 3 'full_history', 4 'hit_history').
        domains [B] + theta_dom_en_en [D][F_ee] + theta_dom_en_de [D][F_ed]: --user_adapt / --experience_adapt
        (train_mp.py:162-171, 226-247): instance i builds its potentials from theta_dom[domains[i]] INSTEAD of the
        global theta; the global theta still receives every instance's step.  Instances of one domain should be
        contiguous (groups of 16 consecutive graphs that share their tables run on the matrix cores).
        The pots, their transposed rows, the private rows and the per-instance outputs live in a _SharedTables, the only owner
        of per-step device state.  A standalone trainer is a set of one, built at the end of this constructor; member=True
        leaves that to the caller, which builds ONE set over many trainers (_BucketSet: the bucket trainers of a TiDirTrainer,
        one potentials launch, one patch launch and one statistics launch per step for all sentence shapes).
        skip_unchanged (off by default, like the C ABI: the default executes every update of the reference's schedule): the
        sweeps drop the updates of the root sequence that would recompute a message from unchanged inputs
        (MLBP_SWEEP_SKIP_UNCHANGED, include/mlbp.h) -- a third of a three-root user graph's contractions; statistics equal
        the full schedule's to rounding (tests/test_gpu_gradient.py)."""
        self.spec = spec
        self.topo = topo = GraphTopology.from_spec(spec)
        by_id = {f['id']: f for f in spec['factors']}
        X = spec['X']
        self.device = torch.device(device)
        B = int(np.asarray(var_labels).shape[0])
        self.batch = fb = FactorGraphBatch(topo, X, B, device=self.device)
        fb.skip_unchanged = bool(skip_unchanged)
        pair_phi, unary_kind = [], []
        for j in topo.pair_factors:
            f = by_id[topo.factor_ids[j]]
            if f['factor_type'] != 'en_en' or f['gap'] < 1:
                raise BaseException('only 2 kinds of distances are supported ...')      # LBP.py:463
            pair_phi.append(0 if f['gap'] > 1 else 1)
        for j in topo.unary_factors:
            f = by_id[topo.factor_ids[j]]
            if f['factor_type'] == 'en_de':
                unary_kind.append(2)
            elif f['factor_type'] == 'en_en' and f['gap'] >= 1:
                unary_kind.append(0 if f['gap'] > 1 else 1)
            else:
                raise BaseException('only two kinds of potentials are supported...')    # LBP.py:467
        # features_of: another trainer given the SAME feature tensors -- its device copies are used (the buckets of one TiDirTrainer)
        fb.set_features(phi_en_en, phi_en_en_w1, phi_en_de, pair_phi, unary_kind, share_with=features_of.batch if features_of is not None else None)
        fb.set_observations(var_labels, unary_obs)
        self.Vde = int(fb.phi_en_de.shape[1])
        self.F_ee, self.F_ed = int(fb.phi_en_en.shape[2]), int(fb.phi_en_de.shape[2])
        dev = self.device
        # theta may be passed as device tensors so that several shape buckets share one parameter vector
        self.theta_en_en = theta_en_en if isinstance(theta_en_en, torch.Tensor) else \
            torch.as_tensor(np.asarray(theta_en_en, dtype=np.float64).reshape(-1)).to(dev)
        self.theta_en_de = theta_en_de if isinstance(theta_en_de, torch.Tensor) else \
            torch.as_tensor(np.asarray(theta_en_de, dtype=np.float64).reshape(-1)).to(dev)
        # pots: [pot_en_en, pot_en_en_w1] as pairwise tables; their transposes + pot_en_de^T as unary rows
        as_theta = lambda t: t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t, dtype=np.float64)).to(dev)   # noqa: E731
        self.n_dom = 0
        self._dom_host = np.zeros(B, dtype=np.int64)
        if domains is not None:
            self.theta_dom_en_en, self.theta_dom_en_de = as_theta(theta_dom_en_en), as_theta(theta_dom_en_de)
            self.n_dom = int(self.theta_dom_en_en.shape[0])
            self._dom_host = np.asarray(domains, dtype=np.int64).reshape(B)
            if self.n_dom < 1 or self._dom_host.min() < 0 or self._dom_host.max() >= self.n_dom:
                raise IndexError('domain index out of range')
            if tuple(self.theta_dom_en_en.shape) != (self.n_dom, self.F_ee) or tuple(self.theta_dom_en_de.shape) != (self.n_dom, self.F_ed):
                raise ValueError('theta_dom_* must be [D][F]')
            self._dom = torch.from_numpy(self._dom_host.astype(np.int32)).to(dev)
        nd = max(self.n_dom, 1)
        self.rows_per_dom = 2 * X + self.Vde
        obs_np = np.asarray(unary_obs, dtype=np.int64).reshape(B, topo.U)
        self._plan_patches(planes, unary_kind, obs_np, np.asarray(var_labels, dtype=np.int64).reshape(B, topo.n_vars))
        self.n_shared_rows = self.rows_per_dom * nd
        self._pair_phi, self._unary_kind_list, self._obs_np = pair_phi, unary_kind, obs_np
        self.sweeps = int(sweeps)
        self.roots = list(roots) if roots is not None else [topo.var_ids[i % topo.n_vars] for i in range(self.sweeps)]
        fb.is_loopy = topo.has_loops(self.roots[0])
        self.n_sweeps_run = self.sweeps if fb.is_loopy else 1                            # LBP.py:219
        if not member:
            _SharedTables([self])

    def _join(self, shared, priv_row0, inst0):
        """The rest of the construction, called by the _SharedTables that takes this trainer in: the set's pots and rows, this
        trainer's private rows from row priv_row0 of the set's row array, its per-instance gradient rows and log-posteriors from
        instance inst0 of the set's arrays."""
        fb, topo, dev = self.batch, self.topo, self.device
        X, B = self.spec['X'], fb.B
        self.shared, self.priv_row0 = shared, int(priv_row0)
        self.pair_tables, self.unary_tables = shared.pair_tables, shared.unary_tables
        pair_phi, unary_kind = self._pair_phi, self._unary_kind_list
        fb.pair_tables = self.pair_tables
        ptab = np.tile(np.array(pair_phi or [0], dtype=np.int64), (B, 1)) + 2 * self._dom_host[:, None]
        fb.pair_tab = torch.from_numpy(ptab.astype(np.int32)).to(dev)
        fb.pair_tables_shared = bool(topo.P)      # every instance reads the two pots: the MFMA kernels apply
        # one row for every instance (no per-domain pots): at X >= 128 the sweeps can run as batched MFMA contractions
        fb._pair_row_host = np.ascontiguousarray(ptab[0], dtype=np.int32) if (topo.P and not self.n_dom) else None
        obs = self._obs_np
        base = np.array([0, X, 2 * X], dtype=np.int64)[np.array(unary_kind, dtype=np.int64)] if topo.U else np.zeros(0)
        fb.unary_tables = self.unary_tables
        utab = obs + base[None, :] + self.rows_per_dom * self._dom_host[:, None]
        for r, (b_i, u) in enumerate(self._priv_rows):          # patched factors read their private row
            utab[b_i, u] = self.priv_row0 + r
        fb.unary_tab = torch.from_numpy(utab.astype(np.int32)).to(dev)
        self._g_ee, self._g_ed = shared.g_ee[inst0:inst0 + B], shared.g_ed[inst0:inst0 + B]
        self._lp = shared.lp[inst0:inst0 + B]
        self._marg = torch.empty(B, topo.n_vars, X, dtype=torch.float64, device=dev)
        if shared.expect and topo.U:        # the set states the rows' (kind, column) and fills every row's expected features
            fb._row_kind, fb._row_obs, fb._uexp = shared.row_kind, shared.row_obs, shared.uexp
            fb._uexp_rows_done = int(shared.unary_tables.shape[0])

    def _plan_patches(self, planes, unary_kind, obs, labels):
        """Host-side integer work: which (instance, en_de factor) pairs see a plane cell in their
        observed column, and the CSR item lists the two patch kernels consume."""
        topo, X = self.topo, self.spec['X']
        rows, off, ix, ik, iv, rgraph, rlabel, rbase = [], [0], [], [], [], [], [], []
        if planes is not None:
            ed_slots = [u for u in range(topo.U) if unary_kind[u] == 2]
            for b_i, cells in enumerate(planes):
                if not cells:
                    continue
                for u in ed_slots:
                    col = int(obs[b_i, u])
                    items = [(i, k, v) for (i, j, k), v in sorted(cells.items()) if j == col and v != 0.0]
                    if not items:
                        continue
                    for i, k, v in items:
                        if not (0 <= i < X and 0 <= k < self.F_ed):
                            raise IndexError('feature-plane cell out of range')
                        ix.append(i); ik.append(k); iv.append(float(v))
                    rows.append((b_i, u)); off.append(len(ix))
                    rgraph.append(b_i); rbase.append(2 * X + col + self.rows_per_dom * int(self._dom_host[b_i]))
                    rlabel.append(int(labels[b_i, topo.fac_var[2 * topo.unary_factors[u]]]))
        self._priv_rows, self.n_priv = rows, len(rows)
        self._priv_cols = [b - 2 * X - self.rows_per_dom * int(self._dom_host[g_i]) for b, g_i in zip(rbase, rgraph)]   # observed column of each private row
        # private rows of one domain must be contiguous (their exponent uses that domain's theta): instances come
        # grouped by domain, so the row list already is; record the ranges
        row_dom = [int(self._dom_host[b_i]) for b_i, _ in rows]
        if any(row_dom[i] > row_dom[i + 1] for i in range(len(row_dom) - 1)):
            raise ValueError('instances with feature planes must be grouped by domain')
        self._priv_dom_ranges = []
        for d in sorted(set(row_dom)):
            lo = row_dom.index(d)
            self._priv_dom_ranges.append((d, lo, lo + row_dom.count(d)))
        self._patch_plan = (off, ix, ik, iv, rgraph, rlabel, rbase)      # (the set joins its trainers' plans and uploads them once)

    def build_potentials(self):
        """The pots under the current thetas, then this trainer's private rows (_SharedTables.build)."""
        self.shared.build([self])

    def capture(self):
        """Records local_statistics() into a HIP graph (torch.cuda.CUDAGraph over the library's stream-ordered
        launches): the step is a dozen short kernels, so replaying one graph instead of issuing them from Python
        removes the launch-bound host time.  theta is read from the same device tensors at every replay.  Call
        after one eager local_statistics() (first-use allocations and attribute calls must not be captured)."""
        self._graph = None
        self._local_statistics_eager()               # warm-up on the current stream
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._local_statistics_eager()
        self._graph = g
        return self

    def local_statistics(self):
        """Runs inference on this rank's shard and returns the fused statistics buffer (device):
        [sum_i grad_en_en (F_ee) | sum_i grad_en_de (F_ed) | sum_i log-posterior | instance count]."""
        if getattr(self, '_graph', None) is not None:
            self._graph.replay()
            return self.shared.stats_all
        return self._local_statistics_eager()

    def _sweep_with_gradient(self):
        self.batch.sweep(self.roots[:self.n_sweeps_run], init=True, marginals=self._marg, gradient=(self._g_ee, self._g_ed),
                         keep_messages=False)

    def _local_statistics_eager(self):
        if len(self.shared.trainers) != 1:
            raise RuntimeError('a bucket trainer has no statistics of its own: its set sums every bucket (TiDirTrainer)')
        self.build_potentials()
        self._sweep_with_gradient()
        return self.shared.statistics()

    def step(self, learning_rate, reg_param, reg_param_ua_scale=1.0):
        """One synchronous optimisation step over ALL ranks' shards: returns (mean log-posterior,
        theta_en_en, theta_en_de).  reg_param is FactorGraph.regularization_param, i.e. the reference's
        `--reg_param / N` (train_mp.py:160); with domains the per-domain thetas take their own instances' steps
        with the regulariser scaled by reg_param_ua_scale (train_mp.py:384-396, 413-415)."""
        stats = mdist.all_reduce_sum_(self.local_statistics())
        update_thetas(self, stats, learning_rate, reg_param, reg_param_ua_scale)
        n_stat = self.F_ee + self.F_ed + 2
        return float(stats[n_stat - 2].item() / stats[n_stat - 1].item()), self.theta_en_en, self.theta_en_de

    def predict(self, top=50, with_logs=False):
        """batch_predictions for the shard (train_mp.py:310-343): runs inference and returns
        (log-posterior per instance [B] (host), top-`top` word indices per predicted variable
        [B][n_vars][top] in descending probability (device top-K), their log-probabilities, and the
        precision counts (p@0, p@25, p@50, total) of FactorGraph.get_precision_counts, LBP.py:80-106)."""
        fb, topo = self.batch, self.topo
        self.build_potentials()
        fb.sweep(self.roots[:self.n_sweeps_run], init=True, marginals=self._marg, keep_messages=False)
        st = _stream_ptr(self.device)
        _ffi.check(_ffi.lib.mlbp_log_posterior_f64(self._marg.data_ptr(), fb._labels.data_ptr(), fb.B, topo.n_vars, fb.X,
                                                   self._lp.data_ptr(), st))
        idx = torch.empty(fb.B, topo.n_vars, top, dtype=torch.int32, device=self.device)
        _ffi.check(_ffi.lib.mlbp_topk_rows_f64(self._marg.data_ptr(), fb.B * topo.n_vars, fb.X, top, idx.data_ptr(), st))
        logm = torch.empty_like(self._marg)
        _ffi.check(_ffi.lib.mlbp_log_f64(self._marg.data_ptr(), logm.data_ptr(), self._marg.numel(), st))
        idx_h = idx.cpu().numpy().astype(np.int64)
        logs = np.take_along_axis(logm.cpu().numpy(), idx_h, axis=2)
        labels = fb._labels.cpu().numpy()
        # integer work: rank of the user's label among the top words of every en_de factor's variable
        by_id = {f['id']: f for f in self.spec['factors']}
        ed_vars = [int(topo.fac_var[2 * j]) for j in topo.unary_factors if by_id[topo.factor_ids[j]]['factor_type'] == 'en_de']
        hit = idx_h[:, ed_vars, :] == labels[:, ed_vars, None]
        rank = np.where(hit.any(-1), hit.argmax(-1), 10 ** 6)
        counts = (int((rank == 0).sum()), int((rank < 26).sum()), int((rank < 51).sum()), int(rank.size))
        if with_logs:       # + every variable's log-marginal vector and the log-probability of the user's label (the text formats)
            logm_h = logm.cpu().numpy()
            return self._lp.cpu().numpy(), idx_h, logs, counts, logm_h, np.take_along_axis(logm_h, labels[:, :, None], axis=2)[:, :, 0]
        return self._lp.cpu().numpy(), idx_h, logs, counts

    def decode(self):
        """The jointly most probable set of guesses of every instance under the current thetas (max-product sweeps over the
        predict() schedule, FactorGraphBatch.map_sweep): host (assignment int64 [B][n_vars] word indices in var_ids order,
        score float64 [B] -- the log-potential of the assignment)."""
        self.build_potentials()
        assignment, score = self.batch.map_sweep(self.roots[:self.n_sweeps_run], init=True, keep_messages=False)
        return assignment.cpu().numpy().astype(np.int64), score.cpu().numpy()

    def settled_decode(self, tol=1e-6, max_rounds=50, with_changed=False):
        """decode() run until its messages stop moving (FactorGraphBatch.map_converge; a round is the predict() schedule, so
        the first round is decode() itself): host (assignment int64 [B][n_vars] word indices in var_ids order, score float64
        [B], rounds int32 [B], residual float64 [B] -- residual <= tol: the set was read from settled messages --, gain
        float64 [B] -- score minus decode()'s score; max-product promises no sign for it); with_changed also changed bool [B],
        the set differs from decode()'s."""
        fb, roots = self.batch, self.roots[:self.n_sweeps_run]
        self.build_potentials()
        bp_x, bp_score = fb.map_sweep(roots, init=True, keep_messages=False)
        x, score, rounds, residual = fb.map_converge(roots, tol=tol, max_rounds=max_rounds, init=True)
        out = (x.cpu().numpy().astype(np.int64),) + _host(score, rounds, residual, score - bp_score)
        return out + _host((bp_x != x).any(dim=1)) if with_changed else out

    def sample(self, n_samples=1, seed=None, uniforms=None, given=None):
        """Whole sets of guesses drawn from the model under the current thetas (sequential conditioning over the predict()
        schedule, FactorGraphBatch.sample): host (samples int64 [S][B][n_vars] word indices in var_ids order, logq float64
        [S][B] -- the exact log-probability of each draw under the sampler).  Exactly one of seed and uniforms; given:
        [B][n_vars] word indices that are known, -1 for the words to draw."""
        self.build_potentials()
        samples, logq = self.batch.sample(self.roots[:self.n_sweeps_run], n_samples=n_samples, seed=seed, uniforms=uniforms, given=given)
        return samples.cpu().numpy().astype(np.int64), logq.cpu().numpy()

    def exact_sample(self, n_samples=1, seed=None, uniforms=None):
        """Whole sets of guesses drawn from the model ITSELF under the current thetas (FactorGraphBatch.exact_sample): host
        (samples int64 [S][B][n_vars] word indices in var_ids order, logp float64 [S][B] -- the true log-probability of each
        draw, score - log Z, on loopy sentence graphs too).  Exactly one of seed and uniforms.  Raises
        exactsample.ExactSampleError(MLBP_EUNSUPPORTED) for a shape above the configuration limit."""
        self.build_potentials()
        samples, logp = self.batch.exact_sample(n_samples=n_samples, seed=seed, uniforms=uniforms)
        return samples.cpu().numpy().astype(np.int64), logp.cpu().numpy()

    def estimated_sample(self, n_samples, n_list=256, seed=0, proposal='messages'):
        """The sentence shapes exact_sample() refuses: whole sets of guesses drawn by resampling a list of n_list cutset states
        under the current thetas (FactorGraphBatch.estimate_sample over the predict() schedule, which writes the batch's
        messages): host (samples int64 [S][B][n_vars] word indices in var_ids order, logp_hat float64 [S][B] -- the estimate
        score - log_z_hat of each draw's log-probability --, log_z_hat float64 [B], ess float64 [B] -- the effective size of
        the list out of n_list).  proposal: 'messages' or 'sample', as FactorGraphBatch.estimate_sample takes it.  Raises
        cutsetis.CutsetisError(MLBP_EUNSUPPORTED) for a shape the listed plan refuses (more than 16 cutset variables)."""
        self.build_potentials()
        samples, logp_hat, log_z_hat, ess = self.batch.estimate_sample(self.roots[:self.n_sweeps_run], n_samples=n_samples, n_list=n_list,
                                                                       seed=seed, proposal=proposal)
        return (samples.cpu().numpy().astype(np.int64),) + _host(logp_hat, log_z_hat, ess)

    def convergence(self, tol=1e-6, max_rounds=50):
        """What stopping at the trainer's own n_sweeps_run sweeps cost each instance, under the current thetas: host (rounds
        int32 [B], residual float64 [B], gap float64 [B]).  rounds and residual are FactorGraphBatch.converge's over rounds of
        every predicted variable as a root once (residual <= tol: the instance converged within max_rounds); gap is the
        largest |marginal after the predict() schedule - marginal at convergence| over variables and states."""
        fb = self.batch
        self.build_potentials()
        fb.sweep(self.roots[:self.n_sweeps_run], init=True, marginals=self._marg)
        stopped = self._marg.cpu().numpy()
        settled = torch.empty_like(self._marg)
        rounds, residual = fb.converge(tol=tol, max_rounds=max_rounds, init=True, marginals=settled)
        gap = np.abs(stopped - settled.cpu().numpy()).reshape(fb.B, -1).max(axis=1)
        return _host(rounds, residual) + (gap,)

    def joint_log_likelihood(self):
        """How probable the model finds each instance's whole set of stored labels, under the current thetas: host
        (joint_logp float64 [B], log_z float64 [B]).  Sum-product sweeps over the predict() schedule with the messages kept,
        then FactorGraphBatch.log_partition: joint_logp = score(labels) - log Z, exact where the graph is a tree (one
        predicted word: the log-posterior predict() reports), the Bethe value otherwise."""
        fb = self.batch
        self.build_potentials()
        log_z, joint = fb.log_partition(self.roots[:self.n_sweeps_run], init=True, labels=fb._labels)
        return _host(joint, log_z)

    def exact_inference(self):
        """How wrong the usual sweeps were for each instance, under the current thetas: host (log_z float64 [B] -- the model's
        true log Z by FactorGraphBatch.exact_inference --, bethe_gap float64 [B] -- log_partition after the predict() schedule
        minus log_z --, marginal_gap float64 [B] -- the largest |BP marginal - exact marginal| over variables and states --,
        top_agrees bool [B] -- every word's top guess is the same --, joint_logp float64 [B] -- the true log-probability of the
        stored labels).  Raises cutset.CutsetError(MLBP_EUNSUPPORTED) for a shape above the configuration limit."""
        fb = self.batch
        self.build_potentials()
        log_z, exact, joint = fb.exact_inference(labels=fb._labels)
        bethe = fb.log_partition(self.roots[:self.n_sweeps_run], init=True)
        bp = fb.marginals()
        gap = (bp - exact).abs().reshape(fb.B, -1).max(dim=1).values
        agrees = (bp.argmax(dim=2) == exact.argmax(dim=2)).all(dim=1)
        return _host(log_z, bethe - log_z, gap, agrees, joint)

    def estimated_inference(self, n_samples, seed, proposal='sample'):
        """The sentence shapes exact_inference() refuses: an ESTIMATE of each instance's log Z under the current thetas by
        cutset importance sampling (FactorGraphBatch.cutset_estimate with its default proposal over the predict() schedule):
        host (log_z_hat float64 [B], ess float64 [B] -- the effective sample size out of n_samples --, bethe_gap float64 [B] --
        log_partition after the predict() schedule minus log_z_hat --, marginals float64 [B][n_vars][X], self-normalised).
        proposal='messages': log_partition over the predict() schedule runs FIRST and the list is drawn by
        FactorGraphBatch.cutset_draw from the messages that call leaves -- the proposal then costs no sweep of its own.
        Raises cutsetis.CutsetisError(MLBP_EUNSUPPORTED) for a shape the estimating library refuses."""
        fb = self.batch
        self.build_potentials()
        roots = self.roots[:self.n_sweeps_run]
        if proposal == 'messages':
            bethe = fb.log_partition(roots, init=True)
            log_z_hat, marg, ess = fb.cutset_estimate(n_samples=n_samples, seed=seed, proposal='messages')
        elif proposal != 'sample':
            raise ValueError("proposal must be 'sample' or 'messages', not %r" % (proposal,))
        else:
            log_z_hat, marg, ess = fb.cutset_estimate(roots, n_samples=n_samples, seed=seed)
            bethe = fb.log_partition(roots, init=True)
        return _host(log_z_hat, ess, bethe - log_z_hat, marg)

    def _plane_share(self, belief):
        """The per-instance feature planes' share of the en_de gradient, host [B][F_ed]: for every plane cell (i, observed
        column, k) of value v on a patched factor, v * ([label == i] - belief[row][i]).  belief: host [n_priv][X], the belief
        of every private row's factor over its variable (what mlbp_patch_gradient_f64 adds from the normalised rows)."""
        out = np.zeros((self.batch.B, self.F_ed))
        off, ix, ik, iv, rgraph, rlabel, _ = self._patch_plan
        for r in range(self.n_priv):
            for q in range(off[r], off[r + 1]):
                out[rgraph[r], ik[q]] += iv[q] * ((1.0 if rlabel[r] == ix[q] else 0.0) - belief[r, ix[q]])
        return out

    def _bp_gradient(self):
        """What gradient() gives after the predict() schedule, planes included: host (bp_ee [B][F_ee], bp_ed [B][F_ed],
        log-posterior [B]).  The potentials are already built."""
        fb, topo = self.batch, self.topo
        fb.sweep(self.roots[:self.n_sweeps_run], init=True, marginals=self._marg)
        bp_ee, bp_ed = fb.gradient()
        lp = torch.empty(fb.B, dtype=torch.float64, device=self.device)
        _ffi.check(_ffi.lib.mlbp_log_posterior_f64(self._marg.data_ptr(), fb._labels.data_ptr(), fb.B, topo.n_vars, fb.X, lp.data_ptr(),
                                                   _stream_ptr(self.device)))
        bp_ee, bp_ed = bp_ee.cpu().numpy(), bp_ed.cpu().numpy()
        if self.n_priv:                                         # the reference's unary belief: the normalised table alone
            rows = self.unary_tables[self.priv_row0:self.priv_row0 + self.n_priv].cpu().numpy()
            bp_ed = bp_ed + self._plane_share(rows / rows.sum(axis=1, keepdims=True))
        return bp_ee, bp_ed, lp.cpu().numpy()

    def exact_gradient(self):
        """The gradient of the TRUE likelihood of each instance under the current thetas, beside the one the trainer follows:
        host (g_ee float64 [B][F_ee], g_ed float64 [B][F_ed] -- observed minus expected features under the model's own pair
        marginals and marginals, FactorGraphBatch.exact_gradient, the feature planes' share included: the derivative of
        joint_logp in the thetas --, joint_logp float64 [B] -- the true log-probability of the stored labels --, bp_ee, bp_ed
        -- what gradient() gives after the predict() schedule).  Raises exactgrad.ExactGradError(MLBP_EUNSUPPORTED) for a
        shape above the configuration limit."""
        fb, topo = self.batch, self.topo
        self.build_potentials()
        exact = torch.empty(fb.B, topo.n_vars, fb.X, dtype=torch.float64, device=self.device)
        g_ee, g_ed, _ = fb.exact_gradient(marginals=exact)
        joint = fb.exact_inference(labels=fb._labels)[2]
        g_ee, g_ed = g_ee.cpu().numpy(), g_ed.cpu().numpy()
        if self.n_priv:                                         # the true belief of a unary factor: its variable's marginal
            exact = exact.cpu().numpy()
            var_of = [int(topo.fac_var[2 * topo.unary_factors[u]]) for _, u in self._priv_rows]
            g_ed = g_ed + self._plane_share(np.stack([exact[b_i, v] for (b_i, _), v in zip(self._priv_rows, var_of)]))
        bp_ee, bp_ed, _ = self._bp_gradient()
        return g_ee, g_ed, joint.cpu().numpy(), bp_ee, bp_ed

    def estimated_gradient(self, n_list=256, seed=0, proposal='messages'):
        """The sentence shapes exact_gradient() refuses: an ESTIMATE of the gradient of the true likelihood of each instance
        under the current thetas over a list of n_list cutset states (FactorGraphBatch.cutset_gradient, the feature planes'
        share from the estimated marginals included): host (g_ee float64 [B][F_ee], g_ed float64 [B][F_ed], joint_logp_hat
        float64 [B] -- the log-potential of the stored labels minus log_z_hat --, log_z_hat float64 [B]).  log_partition over
        the predict() schedule runs first: it gives the labels' log-potential and leaves the messages the list is drawn from
        (proposal='messages': FactorGraphBatch.cutset_draw(n_list, seed=seed)); proposal='sample' draws the list with
        cutset_proposal(), which sweeps again for every draw.  Raises cutsetis.CutsetisError(MLBP_EUNSUPPORTED) for a shape the
        listed plan refuses (more than 16 cutset variables)."""
        if proposal not in ('sample', 'messages'):
            raise ValueError("proposal must be 'sample' or 'messages', not %r" % (proposal,))
        fb, topo = self.batch, self.topo
        self.build_potentials()
        roots = self.roots[:self.n_sweeps_run]
        score = torch.empty(fb.B, dtype=torch.float64, device=self.device)
        fb.log_partition(roots, init=True, labels=fb._labels, score=score)
        if proposal == 'messages':
            configs, log_q = fb.cutset_draw(n_list, seed=int(seed))
        else:
            configs, log_q = fb.cutset_proposal(roots, n_list, seed=int(seed))
        est = torch.empty(fb.B, topo.n_vars, fb.X, dtype=torch.float64, device=self.device)
        g_ee, g_ed, log_z_hat = fb.cutset_gradient(configs, log_q, marginals=est)
        g_ee, g_ed = g_ee.cpu().numpy(), g_ed.cpu().numpy()
        if self.n_priv:                                         # as exact_gradient(): the unary factor's belief is its variable's marginal
            est = est.cpu().numpy()
            var_of = [int(topo.fac_var[2 * topo.unary_factors[u]]) for _, u in self._priv_rows]
            g_ed = g_ed + self._plane_share(np.stack([est[b_i, v] for (b_i, _), v in zip(self._priv_rows, var_of)]))
        return g_ee, g_ed, (score - log_z_hat).cpu().numpy(), log_z_hat.cpu().numpy()

    def exact_decode(self):
        """The TRUE jointly most probable set of guesses of every instance under the current thetas
        (FactorGraphBatch.exact_map), and how decode() fared against it: host (assignment int64 [B][n_vars] word indices in
        var_ids order, score float64 [B] -- its log-potential --, margin float64 [B] -- score minus the best score of any
        assignment that differs in at least one word: the minimum over the words of score - the second-largest max-marginal
        --, bp_agrees bool [B] -- map_sweep over the predict() schedule returned the same assignment --, shortfall float64
        [B] >= 0 -- score minus map_sweep's score, 0 where they agree --, joint_logp float64 [B] -- the true log-probability
        of the assignment, by exact_inference).  Raises exactmap.ExactMapError(MLBP_EUNSUPPORTED) for a shape above the
        configuration limit."""
        fb = self.batch
        self.build_potentials()
        x, score, mm = fb.exact_map(max_marginals=True)
        second = mm.topk(2, dim=2).values[:, :, 1]
        margin = (score[:, None] - second).min(dim=1).values
        bp_x, bp_score = fb.map_sweep(self.roots[:self.n_sweeps_run], init=True, keep_messages=False)
        agrees = (bp_x == x).all(dim=1)
        shortfall = torch.where(agrees, torch.zeros_like(score), (score - bp_score).clamp(min=0.0))
        joint = fb.exact_inference(labels=x)[2]
        return (x.cpu().numpy().astype(np.int64),) + _host(score, margin, agrees, shortfall, joint)

    def search_decode(self, n_samples=256, seed=0, with_list=False):
        """The sentence shapes exact_decode() refuses, and the others beside it: the best set of guesses among those whose
        cutset state is on a list of n_samples -- decode()'s own cutset state first, then draws from the sum-product messages
        (FactorGraphBatch.search_map over the predict() schedule).  Host (assignment int64 [B][n_vars] word indices in
        var_ids order, score float64 [B] -- its log-potential --, score_bp float64 [B] -- decode()'s score, never above score
        but by the rounding of the two sums --, changed bool [B] -- the set differs from decode()'s); with_list also configs
        int32 [B][n_samples][n_cut], the list that was walked.  Up to 16 cutset variables: nothing is refused for its
        number of configurations."""
        fb = self.batch
        self.build_potentials()
        configs, bp_x, bp_score = fb._search_list(self.roots[:self.n_sweeps_run], n_samples, seed, None, None)
        x, score = fb.cutset_map(configs)
        out = (x.cpu().numpy().astype(np.int64),) + _host(score, bp_score, (bp_x != x).any(dim=1))
        return out + (configs.cpu().numpy(),) if with_list else out

    def exact_nbest(self, m):
        """The `m` TRULY most probable sets of guesses of every instance under the current thetas, ranked
        (FactorGraphBatch.exact_mbest), with the true probability of each: host (assignments int64 [B][m][n_vars] word
        indices in var_ids order, -1 in the rows a list does not have; scores float64 [B][m] -- the log-potentials, -inf
        there --; logp float64 [B][m] = score - log Z, log Z from one exact_inference call; covered float64 [B] -- the mass
        of the rows, sum exp(logp) --; label_rank int64 [B] -- the row that is the user's own labelled set of guesses, -1
        when it is not among them --; bp_rank int64 [B] -- the row decode()'s set is, -1 likewise).  1 <= m <= 16.  Raises
        exactmbest.ExactMbestError(MLBP_EUNSUPPORTED) for a shape above the configuration limit."""
        fb = self.batch
        self.build_potentials()
        x, score, _ = fb.exact_mbest(m)
        log_z = fb.exact_inference()[0]
        bp_x, _ = fb.map_sweep(self.roots[:self.n_sweeps_run], init=True, keep_messages=False)
        logp = score - log_z[:, None]
        covered = logp.exp().sum(dim=1)

        def rank_of(rows):
            hit = (x == rows[:, None, :].to(x.dtype)).all(dim=2)
            return torch.where(hit.any(dim=1), hit.to(torch.int64).argmax(dim=1), torch.full_like(hit[:, 0], -1, dtype=torch.int64))
        return (x.cpu().numpy().astype(np.int64),) + _host(score, logp, covered, rank_of(fb._labels), rank_of(bp_x))

    def search_nbest(self, m, n_samples=256, seed=0, with_list=False):
        """The sentence shapes exact_nbest() refuses, and the others beside it: the `m` best sets of guesses among those
        whose cutset state is on search_decode()'s list, ranked (FactorGraphBatch.cutset_mbest over that list).  Host
        (assignments int64 [B][m][n_vars] word indices in var_ids order, -1 in the rows a list does not have; scores float64
        [B][m], -inf there; n_found int64 [B]; label_rank int64 [B] -- the row that is the user's own labelled set of guesses,
        -1 when it is not among them --; bp_rank int64 [B] -- the row decode()'s set is: its cutset state is entry 0 of the
        list, so it is -1 only where m sets under the listed states score above it).  No logp: entry 0 of the list is no draw
        from a proposal, so the list carries no unbiased log Z.  with_list also configs int32 [B][n_samples][n_cut], the list
        that was walked.  1 <= m <= 16; up to 16 cutset variables, nothing is refused for its number of configurations."""
        fb = self.batch
        self.build_potentials()
        configs, bp_x, _ = fb._search_list(self.roots[:self.n_sweeps_run], n_samples, seed, None, None)
        x, score, n_found = fb.cutset_mbest(configs, m)

        def rank_of(rows):
            hit = (x == rows[:, None, :].to(x.dtype)).all(dim=2)
            return torch.where(hit.any(dim=1), hit.to(torch.int64).argmax(dim=1), torch.full_like(hit[:, 0], -1, dtype=torch.int64))
        out = (x.cpu().numpy().astype(np.int64),) + _host(score, n_found.to(torch.int64), rank_of(fb._labels), rank_of(bp_x))
        return out + (configs.cpu().numpy(),) if with_list else out


def apply_update(theta_en_en, theta_en_de, stats, F_ee, F_ed, learning_rate, reg_param):
    """theta += sum_i lr (g_i - reg theta) = lr (sum_i g_i - n reg theta): the sum of the per-instance
    steps `return_gradient` produces (LBP.py:293-299, 322-327) as `batch_sgd_accumulate` adds them
    (train_mp.py:419-424).  Works on CPU or device tensors (it is part of the gloo tests)."""
    n = stats[-1]
    theta_en_en += learning_rate * (stats[:F_ee] - n * reg_param * theta_en_en)
    theta_en_de += learning_rate * (stats[F_ee:F_ee + F_ed] - n * reg_param * theta_en_de)
    return theta_en_en, theta_en_de


def apply_domain_update(theta_dom_en_en, theta_dom_en_de, stats_dom, F_ee, F_ed, learning_rate, reg_param):
    """theta_d += lr (sum_{i in d} g_i - n_d reg theta_d): the per-domain half of batch_sgd_accumulate
    (train_mp.py:384-396, 413-415; `reg_param` already carries reg_param_ua_scale).  stats_dom: [D][F_ee+F_ed+2]."""
    n = stats_dom[:, -1:]
    theta_dom_en_en += learning_rate * (stats_dom[:, :F_ee] - n * reg_param * theta_dom_en_en)
    theta_dom_en_de += learning_rate * (stats_dom[:, F_ee:F_ee + F_ed] - n * reg_param * theta_dom_en_de)
    return theta_dom_en_en, theta_dom_en_de


def update_thetas(owner, stats, learning_rate, reg_param, reg_param_ua_scale):
    """The step of a trainer's thetas (owner: a UserGraphTrainer or a TiDirTrainer) from its fused statistics buffer
    [global statistics | per-domain statistics [D][F_ee+F_ed+2]]: apply_update, then apply_domain_update when the buffer
    carries per-domain rows."""
    F_ee, F_ed = len(owner.theta_en_en), len(owner.theta_en_de)
    n = F_ee + F_ed + 2
    apply_update(owner.theta_en_en, owner.theta_en_de, stats[:n], F_ee, F_ed, learning_rate, reg_param)
    if stats.numel() > n:
        apply_domain_update(owner.theta_dom_en_en, owner.theta_dom_en_de, stats[n:].view(-1, n), F_ee, F_ed, learning_rate,
                            reg_param * reg_param_ua_scale)


class _SharedTables:
    """The only owner of per-step device state, for one trainer (a standalone UserGraphTrainer) or the bucket trainers of one
    TiDirTrainer: the pots under the global theta (or every domain's) as pairwise tables and as transposed rows
    (train_mp.py:220-255 builds them per instance; they depend on theta alone), behind the shared rows every trainer's private
    plane-patched rows and their joined patch plan, the rows' expected features, the per-instance gradient rows and
    log-posteriors, and the statistics buffer.  One potentials launch and one expectations launch per step serve every sentence
    shape."""

    def __init__(self, trainers):
        t0 = trainers[0]
        self.trainers = list(trainers)
        self.device = dev = t0.device
        self.X = X = t0.spec['X']
        self.F_ee, self.F_ed, self.n_dom = t0.F_ee, t0.F_ed, t0.n_dom
        nd = max(self.n_dom, 1)
        self.n_shared_rows = t0.n_shared_rows
        self.n_priv = n_priv = sum(t.n_priv for t in trainers)
        self.n_inst = n_inst = sum(t.batch.B for t in trainers)
        self.pair_tables = torch.empty(2 * nd, X, X, dtype=torch.float64, device=dev)
        self.unary_tables = torch.empty(self.n_shared_rows + n_priv, X, dtype=torch.float64, device=dev)
        self.g_ee = torch.empty(n_inst, self.F_ee, dtype=torch.float64, device=dev)
        self.g_ed = torch.empty(n_inst, self.F_ed, dtype=torch.float64, device=dev)
        self.lp = torch.empty(n_inst, dtype=torch.float64, device=dev)
        # where every trainer's private rows and instances start, and the trainers' patch plans joined (item offsets, base rows
        # and graphs absolute): one upload for the set
        starts, row, inst = [], self.n_shared_rows, 0
        off, ix, ik, iv, rg, rl, rb = [0], [], [], [], [], [], []
        for t in trainers:
            starts.append((row, inst))
            o, x, k, v, g, l, b = t._patch_plan
            off += [len(ix) + e for e in o[1:]]
            ix += x; ik += k; iv += v; rl += l; rb += b
            rg += [inst + gi for gi in g]
            row += t.n_priv; inst += t.batch.B
        if n_priv:
            as_i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)          # noqa: E731
            self._p_off, self._p_x, self._p_k = as_i32(off), as_i32(ix), as_i32(ik)
            self._p_val = torch.tensor(iv, dtype=torch.float64, device=dev)
            self._p_graph, self._p_label, self._p_base = as_i32(rg), as_i32(rl), as_i32(rb)
        # X = 64, shared pots: the potentials launch also writes every shared row's expected features (the gradient's gather
        # table), build() those of the private rows -- decided once, for every trainer of the set
        self.expect = X == 64 and (self.F_ee, self.F_ed) == (3, 6) and any(t.topo.U for t in trainers)
        if self.expect:
            # every row's (phi selector, observed column): shared rows by their place in the layout, private rows their base row's
            rk = np.zeros(self.n_shared_rows + n_priv, dtype=np.int32)
            ro = np.zeros(self.n_shared_rows + n_priv, dtype=np.int32)
            for d in range(nd):
                o = d * t0.rows_per_dom
                rk[o + X:o + 2 * X] = 1; rk[o + 2 * X:o + t0.rows_per_dom] = 2
                ro[o:o + X] = np.arange(X); ro[o + X:o + 2 * X] = np.arange(X); ro[o + 2 * X:o + t0.rows_per_dom] = np.arange(t0.Vde)
            for t, (row, _) in zip(trainers, starts):
                rk[row:row + t.n_priv] = 2
                ro[row:row + t.n_priv] = np.asarray(t._priv_cols, dtype=np.int32).reshape(-1)
            self.row_kind = torch.from_numpy(rk).to(dev)
            self.row_obs = torch.from_numpy(ro).to(dev)
            self.uexp = torch.zeros(self.n_shared_rows + n_priv, 8, dtype=torch.float64, device=dev)
        for t, (row, inst) in zip(trainers, starts):
            t._join(self, row, inst)
        # one buffer for the single all-reduce of a step: [global statistics | per-domain statistics [D][n_stat]]
        n_stat = self.F_ee + self.F_ed + 2
        self.stats_all = torch.zeros(n_stat * (1 + self.n_dom), dtype=torch.float64, device=dev)
        # the group table of mlbp_log_posterior_groups_f64
        gt = np.zeros(len(trainers), dtype=[('m', '<u8'), ('l', '<u8'), ('nv', '<i4'), ('B', '<i4'), ('start', '<i8')])
        for i, (t, (row, inst)) in enumerate(zip(trainers, starts)):
            gt[i] = (t._marg.data_ptr(), t.batch._labels.data_ptr(), t.topo.n_vars, t.batch.B, inst)
        self._groups = torch.from_numpy(gt.view(np.uint8).reshape(-1).copy()).to(dev)
        if self.n_dom:      # per-instance rows summed by segment: the instance's domain, or a dump segment when not selected
            self.rows = torch.empty(n_inst, n_stat, dtype=torch.float64, device=dev)
            self._dom = torch.cat([t._dom for t in trainers])
            self._segsum = torch.zeros(nd + 1, n_stat, dtype=torch.float64, device=dev)
            self._seg = torch.empty(n_inst, dtype=torch.int32, device=dev)
            self._dump = torch.full((n_inst,), nd, dtype=torch.int32, device=dev)

    def statistics(self, select=None):
        """[sum g_ee | sum g_ed | sum log-posterior | count] (then the per-domain rows) over every instance of the set -- or over
        the instances select = (key, value) picks: key device int32 [n_inst], value device int32 [1], instance i counts when
        key[i] == value (a masked minibatch) -- behind the sweeps of all trainers: the planes' gradient share, the
        log-posteriors of every group and the sums, one launch each (one for the last two with a single trainer, every
        instance and no domains)."""
        st = _stream_ptr(self.device)
        if self.n_priv:
            _ffi.check(_ffi.lib.mlbp_patch_gradient_f64(
                self.unary_tables[self.n_shared_rows:].data_ptr(), self._p_off.data_ptr(), self._p_x.data_ptr(), self._p_k.data_ptr(),
                self._p_val.data_ptr(), self._p_graph.data_ptr(), self._p_label.data_ptr(), self.n_priv, self.X, self.F_ed,
                self.g_ed.data_ptr(), st))
        if len(self.trainers) == 1 and select is None and not self.n_dom:
            t = self.trainers[0]
            _ffi.check(_ffi.lib.mlbp_step_statistics_f64(self.g_ee.data_ptr(), self.F_ee, self.g_ed.data_ptr(), self.F_ed,
                                                         t._marg.data_ptr(), t.batch._labels.data_ptr(), t.topo.n_vars, self.X,
                                                         self.n_inst, self.lp.data_ptr(), self.stats_all.data_ptr(), st))
            return self.stats_all
        _ffi.check(_ffi.lib.mlbp_log_posterior_groups_f64(self._groups.data_ptr(), len(self.trainers), self.n_inst, self.X, self.lp.data_ptr(), st))
        if not self.n_dom:
            key, value = (None, None) if select is None else (select[0].data_ptr(), select[1].data_ptr())
            _ffi.check(_ffi.lib.mlbp_select_sum_rows_cat_f64(self.g_ee.data_ptr(), self.F_ee, self.g_ed.data_ptr(), self.F_ed, self.lp.data_ptr(), 1,
                                                             self.n_inst, key, value, 1, self.stats_all.data_ptr(), st))
            return self.stats_all
        n_stat, nd = self.F_ee + self.F_ed + 2, self.n_dom
        r = self.rows
        r[:, :self.F_ee] = self.g_ee
        r[:, self.F_ee:self.F_ee + self.F_ed] = self.g_ed
        r[:, -2] = self.lp
        r[:, -1] = 1.0
        code = self._dom
        if select is not None:
            torch.where(select[0] == select[1], code, self._dump, out=self._seg)
            code = self._seg
        _ffi.check(_ffi.lib.mlbp_segment_sum_rows_f64(r.data_ptr(), self.n_inst, n_stat, code.data_ptr(), nd + 1, self._segsum.data_ptr(), st))
        self.stats_all[n_stat:].view(nd, n_stat).copy_(self._segsum[:nd])
        torch.sum(self._segsum[:nd], dim=0, out=self.stats_all[:n_stat])
        return self.stats_all

    def build(self, trainers=None):
        """The pots (and the shared rows' expected features) under the current thetas, then the private rows of `trainers`
        (default: all) and THEIR expected features."""
        self._potentials()
        t0, X, st = self.trainers[0], self.X, _stream_ptr(self.device)

        def patch(r0, n, theta):        # private rows r0 .. r0 + n of the joined plan
            _ffi.check(_ffi.lib.mlbp_patch_unary_tables_f64(
                self.unary_tables.data_ptr(), self._p_base[r0:].data_ptr(), self._p_off[r0:].data_ptr(), self._p_x.data_ptr(),
                self._p_k.data_ptr(), self._p_val.data_ptr(), theta.data_ptr(), n, X,
                self.unary_tables[self.n_shared_rows + r0:].data_ptr(), st))
        trs = self.trainers if trainers is None else trainers
        if trainers is None and self.n_priv and not self.n_dom:      # every private row of every shape in one launch
            patch(0, self.n_priv, t0.theta_en_de)
        else:
            for t in trs:
                for d, lo, hi in t._priv_dom_ranges:        # one launch per domain present (its theta in the exponent)
                    patch(t.priv_row0 - self.n_shared_rows + lo, hi - lo, t.theta_dom_en_de[d] if self.n_dom else t.theta_en_de)
        if not self.expect:
            return
        spans = [(self.n_shared_rows, int(self.unary_tables.shape[0]))] if trainers is None else [(t.priv_row0, t.priv_row0 + t.n_priv) for t in trs]
        fb = t0.batch
        for lo, hi in spans:
            if hi > lo:
                _ffi.check(_ffi.lib.mlbp_unary_expectations_f64(
                    self.unary_tables[lo:].data_ptr(), hi - lo, X, self.row_kind[lo:].data_ptr(), self.row_obs[lo:].data_ptr(),
                    fb._phi_t[0].data_ptr(), fb._phi_t[1].data_ptr(), fb._phi_t[2].data_ptr(), self.F_ee, self.F_ed, t0.Vde,
                    self.uexp[lo:].data_ptr(), st))

    def _potentials(self):
        """All three pots, for the global theta or for every domain's (its theta REPLACES the global one, train_mp.py:226-247),
        in ONE launch: pot_en_en / pot_en_en_w1 as pairwise tables and transposed rows, pot_en_de as transposed rows only --
        and, self.expect, every shared row's expected features (what the gradient gathers per unary factor,
        mlbp_unary_expectations_f64) out of the same launch: a row of pot^T IS a unary factor's table."""
        t0, X = self.trainers[0], self.X
        fb, pt, ut, rpd = t0.batch, self.pair_tables, self.unary_tables, t0.rows_per_dom
        t_ee = t0.theta_dom_en_en if self.n_dom else t0.theta_en_en
        t_ed = t0.theta_dom_en_de if self.n_dom else t0.theta_en_de
        jobs = (_ffi.PotentialsJob * 3)()
        for j, (phi, th, F, cols, pot, pot_t, row0) in enumerate((
                (fb.phi_en_en, t_ee, self.F_ee, X, pt[0].data_ptr(), ut[0:X].data_ptr(), 0),
                (fb.phi_en_en_w1, t_ee, self.F_ee, X, pt[1].data_ptr(), ut[X:2 * X].data_ptr(), X),
                (fb.phi_en_de, t_ed, self.F_ed, t0.Vde, None, ut[2 * X:].data_ptr(), 2 * X))):
            jobs[j].phi, jobs[j].theta, jobs[j].pot, jobs[j].pot_t = phi.data_ptr(), th.data_ptr(), pot, pot_t
            jobs[j].theta_stride, jobs[j].pot_stride, jobs[j].pot_t_stride = F, 2 * X * X, rpd * X
            jobs[j].rows, jobs[j].cols, jobs[j].F = X, cols, F
            if self.expect:
                jobs[j].expect, jobs[j].expect_stride = self.uexp[row0:].data_ptr(), rpd * 8
        _ffi.check(_ffi.lib.mlbp_potentials_multi_f64(jobs, 3, max(self.n_dom, 1), _stream_ptr(self.device)))


class _BucketSet:
    """The bucket trainers (one UserGraphTrainer per sentence shape) of a list of instances, sharing the owner's thetas."""

    def __init__(self, owner, instances):
        from . import tidir
        self.buckets = tidir.bucket_instances(instances, owner.en, owner.de)
        self.trainers = {}
        o = owner
        dom_of = (lambda r: str(r['user_id'])) if o.adapt == 'user' else (lambda r: str(r['n_seen']))
        dom_index = {d: i for i, d in enumerate(o.domains)}
        for key, b in sorted(self.buckets.items()):
            roots = [key[1][i % len(key[1])] for i in range(o.sweeps)]
            extra = {}
            if o.adapt:   # group the bucket's instances by domain: groups of 16 graphs then share their tables
                dom = np.array([dom_index[dom_of(r)] for r in b['rows']], dtype=np.int64)
                order = np.argsort(dom, kind='stable')
                b['rows'] = [b['rows'][i] for i in order]
                b['var_labels'], b['unary_obs'] = b['var_labels'][order], b['unary_obs'][order]
                extra = dict(domains=dom[order], theta_dom_en_en=o.theta_dom_en_en, theta_dom_en_de=o.theta_dom_en_de)
            planes = None
            if o.use_planes:
                planes = []
                for r in b['rows']:
                    cells = {}
                    for name, k in o.plane_features.items():
                        for i, j, v in r['planes'][name]:
                            cells[(i, j, k)] = cells.get((i, j, k), 0.0) + v      # the reference accumulates (+=)
                    planes.append(cells)
            self.trainers[key] = UserGraphTrainer(b['spec'], b['var_labels'], b['unary_obs'], o.phi_ee, o.phi_w1, o.phi_ed_t,
                                                  o.theta_en_en, o.theta_en_de, device=o.device, sweeps=o.sweeps, roots=roots,
                                                  planes=planes, skip_unchanged=o.skip_unchanged, member=True,
                                                  features_of=next(iter(self.trainers.values()), None), **extra)
        self.shared = _SharedTables(list(self.trainers.values())) if self.trainers else None

    def statistics_into(self, stats, grouped_sweeps, select=None):
        """Adds the set's statistics to `stats`.  grouped_sweeps: the sweeps of ALL sentence shapes in one call
        (batch.sweep_groups -> mlbp_sweep_groups_f64: every bucket its own topology and roots; the library runs the buckets
        its fast kernels take in shared launches, the others one by one) instead of one call per bucket.  select: optional
        (key, value) -- key device int32 over the set's instances (bucket order), value device int32 [1]: only the instances
        with key == value enter the sums (masked minibatches).  One potentials launch in front of the sweeps and three launches
        behind them (planes' gradient share, log-posteriors, sums) serve every shape."""
        trs = list(self.trainers.values())
        if not trs:
            return
        self.shared.build()                           # ONE potentials launch (and one expectations launch) for every shape
        if grouped_sweeps and len(trs) >= 2:
            from .batch import sweep_groups
            sweep_groups([tr.batch for tr in trs], [tr.roots[:tr.n_sweeps_run] for tr in trs], init=True,
                         marginals=[tr._marg for tr in trs], gradients=[(tr._g_ee, tr._g_ed) for tr in trs], keep_messages=False)
        else:
            for tr in trs:
                tr._sweep_with_gradient()
        stats += self.shared.statistics(select)


class TiDirTrainer:
    """The outer loop of train_mp.py's __main__ (train_mp.py:560-690) over files in the reference's
    formats: vocabularies, feature matrices, JSON training instances -> one UserGraphTrainer per
    sentence shape sharing theta; one fused statistics buffer, one all-reduce and one update per epoch -- or, with
    `minibatch`, per minibatch of a shuffled epoch (the reference updates once per instance, train_mp.py:631-649 + 405-424:
    minibatch=1 in the limit); params written in the reference's text format, read back for a resumed run, predictions
    written in the reference's two text formats."""

    def __init__(self, ti_path, en_vocab, de_vocab, phi_pmi, phi_pmi_w1, phi_ed, phi_ped, device='cuda:0', sweeps=3,
                 rank=0, world=1, use_planes=True, adapt=None, domains=None, reg_param_ua_scale=1.0,
                 use_correct_feat=True, history=True, session_history=True, grouped_sweeps=True, skip_unchanged=False,
                 minibatch=None, shuffle_seed=None, load_params=None, share_params_with=None, minibatch_mode='masked'):
        """use_planes switches the three per-instance feature planes on as a whole; use_correct_feat / history /
        session_history gate them one by one as the reference's options of the same names do (train_mp.py:178, 192,
        206: the 'correct', 'full_history' and 'hit_history' planes).
        adapt: None, 'user' (--user_adapt: domain = ti.user_id) or 'experience' (--experience_adapt: domain =
        len(ti.past_sentences_seen)), train_mp.py:162-171; `domains`: the domain names in file order (the
        reference reads <ti>.users / <ti>.experience, train_mp.py:504-516) -- default: the names that occur.
        minibatch: instances per update (None = the whole file: one update per epoch).  Every epoch walks the instances in
        a shuffled order (`random.shuffle(training_instances)`, train_mp.py:631) -- a permutation seeded by (shuffle_seed,
        epoch), the same on every rank; shuffle_seed=None keeps the file order -- and cuts it into minibatches; a minibatch is
        sharded contiguously over the ranks, its statistics all-reduced once, theta updated once.
        minibatch_mode: 'masked' (default) -- the rank's whole shard stays resident as ONE set of bucket trainers (one HIP graph);
        every minibatch evaluates ALL of them under the current thetas and sums the statistics of the minibatch's instances only
        (a device-side selection: the epoch's permutation is uploaded once, a minibatch costs one graph replay and no host work
        per instance; the surplus evaluations are what a GPU that is idle anyway pays for having nothing rebuilt).  'rebuild' --
        round 3's form: the bucket trainers of every minibatch are built from its instances (shape compile, table upload,
        programs), which costs tens of milliseconds of host time per minibatch but evaluates nothing twice: for shards far
        larger than a minibatch times the number of minibatches one can afford to replay.
        load_params: a params file (tidir.save_params / the reference's save_params) to start from instead of zeros
        (--load_params, train_mp.py:528-542: the adapt mode's extension is tried first, then the bare name).
        skip_unchanged: the sweeps drop updates that would recompute a message from unchanged inputs (include/mlbp.h
        MLBP_SWEEP_SKIP_UNCHANGED; equal to the full schedule to rounding, off by default like the C ABI).
        share_params_with: another TiDirTrainer whose theta tensors (global and per-domain) this one READS instead of owning
        its own -- the tune-set evaluator of train(tune=...), train_mp.py:657-684: same vocabularies, features and adapt mode."""
        from . import tidir
        self._files = dict(en_vocab=en_vocab, de_vocab=de_vocab, phi_pmi=phi_pmi, phi_pmi_w1=phi_pmi_w1, phi_ed=phi_ed, phi_ped=phi_ped)
        self._options = dict(sweeps=sweeps, use_planes=use_planes, reg_param_ua_scale=reg_param_ua_scale, use_correct_feat=use_correct_feat,
                             history=history, session_history=session_history, grouped_sweeps=grouped_sweeps, skip_unchanged=skip_unchanged)
        if adapt not in (None, 'user', 'experience'):
            raise ValueError("adapt is None, 'user' or 'experience'")
        self.adapt, self.reg_param_ua_scale = adapt, float(reg_param_ua_scale)
        self.grouped_sweeps, self.sweeps, self.skip_unchanged = bool(grouped_sweeps), int(sweeps), bool(skip_unchanged)
        self.rank, self.world = int(rank), int(world)
        self.device = dev = torch.device(device)
        self.en, self.de = tidir.read_vocab(en_vocab), tidir.read_vocab(de_vocab)
        self.phi_ee, self.phi_w1, self.phi_ed_t = tidir.load_features(phi_pmi, phi_pmi_w1, phi_ed, phi_ped)
        self.instances = tidir.read_instances(ti_path)
        self.n_total = len(self.instances)
        self.use_planes = bool(use_planes)
        self.plane_features = {name: tidir.ED_NAMES.index(name)
                               for name, on in (('correct', use_correct_feat), ('full_history', history), ('hit_history', session_history)) if on}
        self.theta_en_en = torch.zeros(len(tidir.EE_NAMES), dtype=torch.float64, device=dev)   # train_mp.py:519-523
        self.theta_en_de = torch.zeros(len(tidir.ED_NAMES), dtype=torch.float64, device=dev)
        dom_of = (lambda r: str(r['user_id'])) if adapt == 'user' else (lambda r: str(r['n_seen']))
        self.domains = []
        if adapt:       # every rank needs the same list: it comes from ALL instances, not only this rank's shard
            if domains is None:
                en2id, de2id = {w: i for i, w in enumerate(self.en)}, {w: i for i, w in enumerate(self.de)}
                domains = sorted({dom_of(tidir.instance_shape(ti, en2id, de2id)[1]) for ti in self.instances})
            self.domains = [str(d) for d in domains]
            self.theta_dom_en_en = torch.zeros(len(self.domains), len(tidir.EE_NAMES), dtype=torch.float64, device=dev)  # train_mp.py:524-527
            self.theta_dom_en_de = torch.zeros(len(self.domains), len(tidir.ED_NAMES), dtype=torch.float64, device=dev)
        if share_params_with is not None:
            o = share_params_with
            if o.adapt != adapt or (adapt and list(o.domains) != list(self.domains)):
                raise ValueError('share_params_with: the other trainer has another adapt mode or domain list')
            self.theta_en_en, self.theta_en_de = o.theta_en_en, o.theta_en_de
            if adapt:
                self.theta_dom_en_en, self.theta_dom_en_de = o.theta_dom_en_en, o.theta_dom_en_de
        if load_params:
            self.load_params(load_params)
        self.minibatch = None if minibatch is None else max(1, int(minibatch))
        if minibatch_mode not in ('masked', 'rebuild'):
            raise ValueError("minibatch_mode is 'masked' or 'rebuild'")
        self.minibatch_mode = minibatch_mode
        self.shuffle_seed = shuffle_seed
        self.n_stat = len(tidir.EE_NAMES) + len(tidir.ED_NAMES) + 2
        self.stats = torch.zeros(self.n_stat * (1 + len(self.domains)), dtype=torch.float64, device=dev)
        self._epochs_done = 0
        # the whole shard as one set of buckets: full-batch epochs and the prediction pass
        lo, hi = mdist.shard_range(self.n_total, self.rank, self.world)
        self._shard = (lo, hi)
        self._full = _BucketSet(self, self.instances[lo:hi])
        self.buckets, self.trainers = self._full.buckets, self._full.trainers
        self._mini_sets = {}
        self._mgraph = None
        if self.minibatch is not None and self.minibatch_mode == 'masked':
            # device-side selection of a minibatch: which minibatch every instance of the file belongs to this epoch, the current
            # minibatch's number, and per bucket the file position of each of its instances
            self._mb_of = torch.zeros(max(self.n_total, 1), dtype=torch.int32, device=dev)
            self._m_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            self._acc = torch.zeros(2, dtype=torch.float64, device=dev)
            pos = [lo + r['index'] for key in self.trainers for r in self.buckets[key]['rows']]      # (bucket order = the set's instance order)
            self._file_pos = torch.from_numpy(np.array(pos, dtype=np.int64)).to(dev)
            self._key = torch.zeros(max(len(pos), 1), dtype=torch.int32, device=dev)      # minibatch of each resident instance this epoch

    # ---- parameters -----------------------------------------------------------------------------
    def load_params(self, path):
        """Starts from a params file (train_mp.py:528-542): '<path><ext>' with the adapt mode's extension first, then
        '<path>'.  Global thetas, and every adapted domain's thetas the file holds for a domain this run knows."""
        from . import tidir
        ext = ADAPT_EXT[self.adapt]
        chosen = path + ext if os.path.exists(path + ext) else path
        een, eet, edn, edt, d2t = tidir.read_params(chosen)
        if list(een) != list(tidir.EE_NAMES) or list(edn) != list(tidir.ED_NAMES):
            raise ValueError('params file %s names other features than this build' % chosen)
        self.theta_en_en.copy_(torch.from_numpy(np.asarray(eet, dtype=np.float64).reshape(-1)))
        self.theta_en_de.copy_(torch.from_numpy(np.asarray(edt, dtype=np.float64).reshape(-1)))
        for i, d in enumerate(self.domains):
            if ('en_en', d) in d2t:
                self.theta_dom_en_en[i].copy_(torch.from_numpy(np.asarray(d2t['en_en', d], dtype=np.float64).reshape(-1)))
            if ('en_de', d) in d2t:
                self.theta_dom_en_de[i].copy_(torch.from_numpy(np.asarray(d2t['en_de', d], dtype=np.float64).reshape(-1)))
        return chosen

    def domain_thetas(self):
        """{('en_en' | 'en_de', domain name): (1, F) array} as train_mp's domain2theta / the params file."""
        d2t = {}
        for i, d in enumerate(self.domains):
            d2t['en_en', d] = self.theta_dom_en_en[i].cpu().numpy().reshape(1, -1)
            d2t['en_de', d] = self.theta_dom_en_de[i].cpu().numpy().reshape(1, -1)
        return d2t

    # ---- statistics -----------------------------------------------------------------------------
    def capture(self):
        """Records local_statistics() -- every bucket's potentials, sweeps (grouped or not), gradients and sums -- into one
        HIP graph; later calls replay it.  theta is read from the same device tensors at every replay.  One eager pass
        first: first-use allocations, attribute calls and the group table's upload must not be captured."""
        self._graph = None
        self._local_statistics_eager()
        torch.cuda.synchronize(self.theta_en_en.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._local_statistics_eager()
        self._graph = g
        return self

    def local_statistics(self):
        """Sum of this rank's buckets' statistics over its whole shard."""
        if getattr(self, '_graph', None) is not None:
            self._graph.replay()
            return self.stats
        return self._local_statistics_eager()

    def _local_statistics_eager(self, bucket_set=None):
        self.stats.zero_()
        (bucket_set or self._full).statistics_into(self.stats, self.grouped_sweeps)
        return self.stats

    def _update(self, learning_rate, reg_param):
        """One all-reduce of the fused buffer (global and per-domain statistics), one update of every theta."""
        mdist.all_reduce_sum_(self.stats)
        update_thetas(self, self.stats, learning_rate, reg_param, self.reg_param_ua_scale)
        n = self.n_stat
        return float(self.stats[n - 2].item()), float(self.stats[n - 1].item())

    def epoch_order(self, epoch):
        """The order in which epoch `epoch` walks ALL instances (every rank computes the same one)."""
        if self.shuffle_seed is None:
            return np.arange(self.n_total)
        return np.random.RandomState([int(self.shuffle_seed) & 0x7FFFFFFF, int(epoch)]).permutation(self.n_total)

    def _minibatch_set(self, epoch, m, ids):
        """The bucket trainers of this rank's share of one minibatch (built once per (order, minibatch): a fixed order reuses
        them every epoch)."""
        key = (epoch if self.shuffle_seed is not None else 0, m)
        if key not in self._mini_sets:
            if self.shuffle_seed is not None:
                self._mini_sets = {k: v for k, v in self._mini_sets.items() if k[0] == key[0]}      # last epoch's sets go
            lo, hi = mdist.shard_range(len(ids), self.rank, self.world)
            self._mini_sets[key] = _BucketSet(self, [self.instances[int(i)] for i in ids[lo:hi]])
        return self._mini_sets[key]

    def _masked_statistics(self):
        """Statistics of the current minibatch (self._m_dev) over this rank's resident shard."""
        if self._mgraph is not None:
            self._mgraph.replay()
            return self.stats
        self.stats.zero_()
        self._full.statistics_into(self.stats, self.grouped_sweeps, select=(self._key, self._m_dev))
        return self.stats

    def capture_masked(self):
        """Records _masked_statistics() into one HIP graph: the minibatch number and the thetas are read from device tensors
        at every replay, so ONE graph serves every minibatch of every epoch."""
        self._mgraph = None
        self._masked_statistics()
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._masked_statistics()
        self._mgraph = g
        return self

    def _epoch_masked(self, epoch, learning_rate, reg_param):
        order = self.epoch_order(epoch)
        mb = np.empty(self.n_total, dtype=np.int32)
        mb[order] = np.arange(self.n_total, dtype=np.int64) // self.minibatch
        self._mb_of.copy_(torch.from_numpy(mb))                  # the epoch's permutation: one upload
        torch.index_select(self._mb_of, 0, self._file_pos, out=self._key)
        self._acc.zero_()
        for m in range((self.n_total + self.minibatch - 1) // self.minibatch):
            self._m_dev.fill_(m)
            self._masked_statistics()
            self._update_on_device(learning_rate, reg_param)
        lp, cnt = (float(v) for v in self._acc.cpu())                # (read once per epoch: no host round trip per minibatch)
        return lp / max(cnt, 1.0)

    def _update_on_device(self, learning_rate, reg_param):
        """_update() without its host read-back: all-reduce, theta updates, the running [sum log-posterior, count]."""
        mdist.all_reduce_sum_(self.stats)
        update_thetas(self, self.stats, learning_rate, reg_param, self.reg_param_ua_scale)
        self._acc += self.stats[self.n_stat - 2:self.n_stat]

    def epoch(self, learning_rate, reg_param):
        """One pass over the instances; returns the mean log-posterior (at the thetas each instance was evaluated under)."""
        epoch = self._epochs_done
        self._epochs_done += 1
        if self.minibatch is None:
            self.local_statistics()
            lp, n = self._update(learning_rate, reg_param)
            return lp / max(n, 1.0)
        if self.minibatch_mode == 'masked':
            return self._epoch_masked(epoch, learning_rate, reg_param)
        order = self.epoch_order(epoch)
        lp_sum, n_sum = 0.0, 0.0
        for m, m0 in enumerate(range(0, self.n_total, self.minibatch)):
            self._local_statistics_eager(self._minibatch_set(epoch, m, order[m0:m0 + self.minibatch]))
            lp, n = self._update(learning_rate, reg_param)
            lp_sum += lp; n_sum += n
        return lp_sum / max(n_sum, 1.0)

    def tune_evaluator(self, tune_path):
        """A second trainer over the instances of `tune_path` (--tune, train_mp.py:463, 571-580) that reads THIS trainer's thetas:
        its predict() is the per-epoch tune evaluation of train_mp.py:657-684."""
        return TiDirTrainer(tune_path, self._files['en_vocab'], self._files['de_vocab'], self._files['phi_pmi'], self._files['phi_pmi_w1'],
                            self._files['phi_ed'], self._files['phi_ped'], device=self.device, rank=self.rank, world=self.world,
                            adapt=self.adapt, domains=self.domains if self.adapt else None, share_params_with=self, **self._options)

    def train(self, epochs=3, reg_param=0.2, save_params=None, capture=True, tune=None):
        """lr = 0.1 / (1 + 0.3 epoch) (train_mp.py:627-630); regularisation reg_param / N (train_mp.py:160);
        params saved as <save_params><ext>.iter<epoch> and <save_params><ext> with ext = '.user_adapt' / '.exp_adapt' /
        '' by adapt mode (train_mp.py:654-656, 688-690).
        tune: a TI file (or a tune_evaluator()) evaluated after EVERY epoch under the thetas that epoch left (train_mp.py:657-684:
        `batch_predictions` over --tune, then the mean log-posterior and precision at 0 / 25 / 50); the per-epoch results --
        (mean log-posterior, (p@0, p@25, p@50, total)) -- are kept in self.tune_history.
        capture: whole-file epochs (minibatch=None) replay one HIP graph of the step's launches (capture(): same bits as the
        eager launches, 7 % less time per step at 8192 instances) when there are at least three of them."""
        from . import tidir
        if capture and self.minibatch is None and epochs >= 3 and getattr(self, '_graph', None) is None and self.trainers:
            self.capture()
        if capture and self.minibatch is not None and self.minibatch_mode == 'masked' and self._mgraph is None and self.trainers and \
                epochs * ((self.n_total + self.minibatch - 1) // self.minibatch) >= 3:
            self.capture_masked()
        if save_params:
            save_params = save_params + ADAPT_EXT[self.adapt]
        history = []
        tuner = self.tune_evaluator(tune) if isinstance(tune, str) else tune
        self.tune_history = []
        for epoch in range(epochs):
            history.append(self.epoch(0.1 / (1.0 + 0.3 * epoch), float(reg_param) / float(self.n_total)))
            if save_params and self.rank == 0:
                tidir.save_params('%s.iter%d' % (save_params, epoch), self.theta_en_en.cpu().numpy().reshape(1, -1),
                                  self.theta_en_de.cpu().numpy().reshape(1, -1), d2t=self.domain_thetas())
            if tuner is not None:
                self.tune_history.append(tuner.predict())
        if save_params and self.rank == 0:
            tidir.save_params(save_params, self.theta_en_en.cpu().numpy().reshape(1, -1),
                              self.theta_en_de.cpu().numpy().reshape(1, -1), d2t=self.domain_thetas())
        return history

    # ---- what the reports below share ------------------------------------------------------------------
    def _per_shape(self, call, empty=None, **how):
        """-> (per-instance list, [(key, rows, result)]): module-level _per_shape over this rank's shapes.  The list (None
        without `empty`) has one entry per instance of the shard in file order, `empty` for those that build no graph."""
        out = None if empty is None else [empty] * (self._shard[1] - self._shard[0])
        return out, _per_shape(self.trainers, self.buckets, call, out=out, **how)

    def _reduced(self, sums, maxima=()):
        return _reduced(self.device, sums, maxima)

    def _hit_counts(self, key, x):
        """decode()'s counts of one shape: (sentences all right, sentences, words right, words)."""
        hit = x == self.buckets[key]['var_labels']
        return np.array([int(hit.all(axis=1).sum()), hit.shape[0], int(hit.sum()), hit.size], dtype=np.int64)

    def _draws_row(self, r, b):
        """([[en words] per sample], [log-probability per sample]) of instance b from a shape's (samples [S][B][n_vars], logp [S][B])."""
        x, logp = r
        return [[self.en[w] for w in x[s, b]] for s in range(x.shape[0])], [float(logp[s, b]) for s in range(x.shape[0])]

    # ---- joint decoding (max-product; the reference has none) ---------------------------------------
    def decode(self):
        """-> (guesses, counts).  guesses[i], for instance i of this rank's shard in file order: (predicted positions, [en
        words], score) -- the whole set of guesses the model finds jointly most probable for the sentence
        (UserGraphTrainer.decode) and its log-potential; an instance without a predicted word builds no graph and gives
        ((), [], 0.0).  counts = (sentences whose every predicted word equals the user's guess, sentences with a predicted
        word, predicted words equal to the user's guess, predicted words) over ALL ranks' instances, reduced once."""
        guesses, shapes = self._per_shape(lambda i, tr: tr.decode(), empty=((), [], 0.0),
                                          row=lambda r, b: ([self.en[w] for w in r[0][b]], float(r[1][b])))
        counts = sum((self._hit_counts(key, x) for key, _, (x, _) in shapes), np.zeros(4, dtype=np.int64))
        return guesses, tuple(int(v) for v in self._reduced(counts)[0])

    def settled_decode(self, tol=1e-6, max_rounds=50):
        """-> (guesses, totals, reached).  guesses[i], for instance i of this rank's shard in file order: (predicted positions,
        [en words], score, rounds, residual, gain over decode()) as UserGraphTrainer.settled_decode gives them; an instance
        without a predicted word builds no graph and gives ((), [], 0.0, 0, 0.0, 0.0).  totals = (sentences decoded, sentences
        whose residual is at most tol, sentences whose score rose above decode()'s by more than SEARCH_ROSE relative to
        max(1, |score|), sentences whose score fell by more than that, sentences whose words changed).  reached = (sentences
        of the shapes exact_map() answers, those whose settled set is exact_map()'s, sum and largest of exact_map()'s score
        minus the settled score); the sentences of five and more predicted words are decoded and counted in totals, not in
        reached.  Over ALL ranks' instances, reduced once."""
        from . import exactmap as K

        def call(i, tr):
            r = tr.settled_decode(tol=tol, max_rounds=max_rounds, with_changed=True)
            best, _ = _try(lambda: tr.batch.exact_map(), K.ExactMapError)          # (the potentials are built)
            return r + (None if best is None else (best[0].cpu().numpy().astype(np.int64), best[1].cpu().numpy()),)
        guesses, shapes = self._per_shape(
            call, empty=((), [], 0.0, 0, 0.0, 0.0),
            row=lambda r, b: ([self.en[w] for w in r[0][b]], float(r[1][b]), int(r[2][b]), float(r[3][b]), float(r[4][b])))
        sums, worst = np.zeros(8), 0.0
        for _, _, (x, score, _, residual, gain, changed, best) in shapes:
            bar = SEARCH_ROSE * np.maximum(1.0, np.abs(score))
            sums[:5] += [len(score), int((residual <= tol).sum()), int((gain > bar).sum()), int((gain < -bar).sum()), int(changed.sum())]
            if best is not None:
                short = np.where((best[0] == x).all(axis=1), 0.0, np.maximum(best[1] - score, 0.0))
                sums[5:] += [len(score), int((best[0] == x).all(axis=1).sum()), float(short.sum())]
                worst = max(worst, float(short.max()))
        tot, top = self._reduced(sums, [worst])
        return guesses, tuple(int(v) for v in tot[:5]), (int(tot[5]), int(tot[6]), float(tot[7]), float(top[0]))

    # ---- posterior sampling of whole sets of guesses (the reference has none) --------------------------
    def sample(self, n_samples=1, seed=0):
        """-> per_instance.  per_instance[i], for instance i of this rank's shard in file order: (predicted positions, [[en
        words] per sample], [logq per sample]) -- n_samples whole sets of guesses drawn from the model for the sentence
        (UserGraphTrainer.sample) and the log-probability of each draw under the sampler; an instance without a predicted
        word builds no graph and gives ((), [], []).  The i-th sentence shape in self.trainers order draws with seed
        `seed + i`.  Every rank draws for its own shard: nothing is reduced."""
        return self._per_shape(lambda i, tr: tr.sample(n_samples=n_samples, seed=int(seed) + i), empty=((), [], []),
                               row=self._draws_row)[0]

    # ---- draws from the model itself (include/mlbp_exactsample.h) ----------------------------------------
    def exact_sample(self, n_samples=1, seed=0):
        """-> (per_instance, skipped).  per_instance[i], for instance i of this rank's shard in file order: (predicted
        positions, [[en words] per sample], [logp per sample]) -- n_samples whole sets of guesses drawn from the model itself
        for the sentence (UserGraphTrainer.exact_sample) and the true log-probability of each draw; an instance without a
        predicted word builds no graph and gives ((), [], []), one of a shape above the configuration limit (positions, None,
        None).  The i-th sentence shape in self.trainers order draws with seed `seed + i`, as sample() does.  skipped:
        [(predicted positions, instances, reason)] of this rank's shapes above the limit.  Every rank draws for its own
        shard: nothing is reduced."""
        from . import exactsample as K
        skipped = []
        per_instance, _ = self._per_shape(lambda i, tr: tr.exact_sample(n_samples=n_samples, seed=int(seed) + i), empty=((), [], []),
                                          row=self._draws_row, placeholder=(None, None), refused=K.ExactSampleError, skipped=skipped)
        return per_instance, skipped

    # ---- and draws for the longer sentences (the listed mode of include/mlbp_exactsample.h) ---------------------------------
    def estimated_sample(self, n_samples=1, n_list=256, seed=0):
        """-> (per_instance, skipped).  per_instance[i], for instance i of this rank's shard in file order: (predicted
        positions, [[en words] per sample], [logp_hat per sample], ess / n_list) -- n_samples whole sets of guesses drawn for
        the sentence by resampling a list of n_list cutset states (UserGraphTrainer.estimated_sample), the estimate of each
        draw's log-probability and the share of the list that is effective; the shapes exact_sample() skips for their size
        -- five and more predicted words -- are INCLUDED.  An instance without a predicted word builds no graph and gives
        ((), [], [], None), one of a shape the listed plan refuses (positions, None, None, None).  The i-th sentence shape in
        self.trainers order draws with seed `seed + 2 i` for its list and `seed + 2 i + 1` for its draws.  skipped:
        [(predicted positions, instances, reason)] of this rank's shapes the listed plan refuses (more than 16 cutset
        variables) -- none for the configuration limit.  Every rank draws for its own shard: nothing is reduced."""
        from . import cutsetis as K
        skipped = []
        per_instance, _ = self._per_shape(
            lambda i, tr: tr.estimated_sample(n_samples, n_list=n_list, seed=int(seed) + 2 * i), empty=((), [], [], None),
            row=lambda r, b: self._draws_row(r[:2], b) + (float(r[3][b]) / float(n_list),), placeholder=(None, None, None),
            refused=K.CutsetisError, skipped=skipped)
        return per_instance, skipped

    # ---- sweeps to convergence (the reference stops at three sweeps and never looks) -------------------
    def convergence_report(self, tol=1e-6, max_rounds=50):
        """-> (per_instance, totals).  per_instance[i], for instance i of this rank's shard in file order: (predicted
        positions, rounds, residual, gap) as UserGraphTrainer.convergence gives them; an instance without a predicted word
        builds no graph and gives ((), 0, 0.0, 0.0).  totals = (sentences with a predicted word, sentences whose residual is
        still above tol after max_rounds, sum of rounds, sum of gap) over ALL ranks' instances, reduced once."""
        per_instance, shapes = self._per_shape(lambda i, tr: tr.convergence(tol=tol, max_rounds=max_rounds), empty=((), 0, 0.0, 0.0),
                                               row=lambda r, b: (int(r[0][b]), float(r[1][b]), float(r[2][b])))
        seen = open_ = total_rounds = 0
        total_gap = 0.0
        for _, _, (rounds, residual, gap) in shapes:
            seen += rounds.shape[0]
            open_ += int((~(residual <= tol)).sum())
            total_rounds += int(rounds.sum())
            total_gap += float(gap.sum())
        tot, _ = self._reduced([seen, open_, total_rounds, total_gap])
        return per_instance, (int(tot[0]), int(tot[1]), int(tot[2]), float(tot[3]))

    # ---- how wrong was it: the sweeps against the model's true values (include/mlbp_cutset.h) ---------
    def exactness_report(self):
        """-> (per_instance, totals, skipped).  per_instance[i], for instance i of this rank's shard in file order: (predicted
        positions, exact log_z, Bethe gap, largest |BP marginal - exact marginal|, every top guess agrees) as
        UserGraphTrainer.exact_inference gives them; an instance without a predicted word builds no graph and gives
        ((), 0.0, 0.0, 0.0, True); an instance of a shape above the configuration limit gives (positions, None, None, None, None).
        totals = (sentences compared, sentences skipped, sum of |Bethe gap|, largest marginal gap, sentences whose top guesses
        all agree) over ALL ranks' instances, reduced once.  skipped: [(predicted positions, instances, reason)] of this rank's
        shapes above the limit."""
        from . import cutset as K
        skipped = []
        per_instance, shapes = self._per_shape(
            lambda i, tr: tr.exact_inference(), empty=((), 0.0, 0.0, 0.0, True), placeholder=(None,) * 4, refused=K.CutsetError,
            skipped=skipped, row=lambda r, b: (float(r[0][b]), float(r[1][b]), float(r[2][b]), bool(r[3][b])))
        seen = n_agree = 0
        sum_gap = worst = 0.0
        for _, rows, (_, bethe_gap, marg_gap, agrees, _) in shapes:
            seen += len(rows)
            sum_gap += float(np.abs(bethe_gap).sum())
            n_agree += int(agrees.sum())
            worst = max(worst, float(marg_gap.max()))
        tot, top = self._reduced([seen, sum(s[1] for s in skipped), sum_gap, n_agree], [worst])
        return per_instance, (int(tot[0]), int(tot[1]), float(tot[2]), float(top[0]), int(tot[3])), skipped

    # ---- and the longer sentences: log Z estimated by cutset importance sampling (include/mlbp_cutsetis.h) ---------------
    def estimate_report(self, n_samples=256, seed=0, proposal='sample'):
        """-> (per_instance, totals, skipped).  per_instance[i], for instance i of this rank's shard in file order: (predicted
        positions, log_z_hat, the relative standard error of the estimate of Z that its effective sample size implies,
        sqrt(1 / ess - 1 / n_samples), log_partition after the usual sweeps minus log_z_hat, the exact log_z where
        exact_inference() accepts the shape, else None) as UserGraphTrainer.estimated_inference gives them; an instance
        without a pairwise factor (at most one predicted word) is solved by the sweeps and gives ((positions), None, None,
        None, None).  The i-th sentence shape in self.trainers order draws with seed `seed + i`, as sample() does; proposal:
        'sample' or 'messages', handed to UserGraphTrainer.estimated_inference.  totals =
        (sentences estimated, sentences also solved exactly, sum and maximum of |log_z_hat - log_z| over those, sum of
        ess / n_samples) over ALL ranks' instances, reduced once.  skipped: [(predicted positions, instances, reason)] of this
        rank's shapes that the estimating library refuses -- none of the shapes the exact reports skip for their size."""
        from . import cutset as K0, cutsetis as K
        def call(i, tr):
            if not tr.topo.P:
                return None
            log_z_hat, ess, bethe_gap, _ = tr.estimated_inference(n_samples, int(seed) + i, proposal=proposal)
            exact, _ = _try(tr.exact_inference, K0.CutsetError)          # above the exact limit: estimated alone
            with np.errstate(divide='ignore', invalid='ignore'):
                rse = np.sqrt(np.maximum(1.0 / ess - 1.0 / float(n_samples), 0.0))
            return log_z_hat, rse, bethe_gap, None if exact is None else exact[0], ess

        skipped = []
        per_instance, shapes = self._per_shape(
            call, empty=((), None, None, None, None), placeholder=(None,) * 4, refused=K.CutsetisError, skipped=skipped,
            row=lambda r, b: (float(r[0][b]), float(r[1][b]), float(r[2][b]), None if r[3] is None else float(r[3][b])))
        seen = both = 0
        sum_err = sum_share = worst = 0.0
        for _, rows, (log_z_hat, _, _, log_z, ess) in shapes:
            seen += len(rows)
            sum_share += float(ess.sum()) / float(n_samples)
            if log_z is not None:
                err = np.abs(log_z_hat - log_z)
                both += len(rows)
                sum_err += float(err.sum())
                worst = max(worst, float(err.max()))
        tot, top = self._reduced([seen, both, sum_err, sum_share], [worst])
        return per_instance, (int(tot[0]), int(tot[1]), float(tot[2]), float(top[0]), float(tot[3])), skipped

    # ---- how wrong is the gradient the trainer follows, and a step on the true likelihood (include/mlbp_exactgrad.h) -----
    def _exact_statistics(self, on_limit='skip'):
        """This rank's sums over its shard, host: (exact [F_ee + F_ed] -- the true gradient --, bp [F_ee + F_ed] -- the BP
        gradient of the same instances --, sum of joint_logp, instances compared, fallback statistics [n_stat] of the shapes
        above the configuration limit when on_limit == 'bp', skipped [(predicted positions, instances, reason)]); on_limit ==
        'raise' lets the library's refusal of such a shape through."""
        from . import exactgrad as K
        F = self.n_stat - 2
        exact, bp, fall = np.zeros(F), np.zeros(F), np.zeros(self.n_stat)
        loglik, seen, skipped = 0.0, 0, []

        def bp_statistics(tr, rows):
            tr.build_potentials()
            bp_ee, bp_ed, lp = tr._bp_gradient()
            fall[:] += np.concatenate([bp_ee.sum(axis=0), bp_ed.sum(axis=0), [lp.sum(), float(len(rows))]])

        _, shapes = self._per_shape(lambda i, tr: tr.exact_gradient(), refused=None if on_limit == 'raise' else K.ExactGradError,
                                    skipped=skipped, on_refused=bp_statistics if on_limit == 'bp' else None)
        for _, rows, (g_ee, g_ed, joint, bp_ee, bp_ed) in shapes:
            seen += len(rows)
            loglik += float(joint.sum())
            exact += np.concatenate([g_ee.sum(axis=0), g_ed.sum(axis=0)])
            bp += np.concatenate([bp_ee.sum(axis=0), bp_ed.sum(axis=0)])
        return exact, bp, loglik, seen, fall, skipped

    def gradient_report(self):
        """-> (totals, skipped): how far the gradient step() and epoch() follow is from the gradient of the true likelihood,
        under the current thetas.  totals = (exact [F_ee + F_ed] -- the true gradient summed over the instances compared,
        UserGraphTrainer.exact_gradient --, bp [F_ee + F_ed] -- the BP gradient summed over the same instances --, their
        cosine, |bp - exact| / |exact|, the true total log-likelihood of the stored labels, instances compared, instances
        skipped) over ALL ranks' instances, reduced once.  skipped: [(predicted positions, instances, reason)] of this rank's
        shapes above the configuration limit; an instance without a predicted word builds no graph and is not counted."""
        exact, bp, loglik, seen, _, skipped = self._exact_statistics()
        F = self.n_stat - 2
        tot, _ = self._reduced(list(exact) + list(bp) + [loglik, seen, sum(s[1] for s in skipped)])
        exact, bp = tot[:F], tot[F:2 * F]
        ne, nb = float(np.linalg.norm(exact)), float(np.linalg.norm(bp))
        cosine = float(exact.dot(bp)) / (ne * nb) if ne > 0 and nb > 0 else float('nan')
        rel = float(np.linalg.norm(bp - exact)) / ne if ne > 0 else float('nan')
        return (exact, bp, cosine, rel, float(tot[2 * F]), int(tot[2 * F + 1]), int(tot[2 * F + 2])), skipped

    def exact_step(self, learning_rate, reg_param, fallback=None):
        """One eager, synchronous step on the TRUE likelihood over ALL ranks' shards: the statistics vector step() hands to
        update_thetas -- [sum g_ee | sum g_ed | sum log-likelihood | count] -- with the exact gradient sums and the sum of
        joint_logp in place of the BP ones, one all-reduce, one update of the global thetas.  A shape above the configuration
        limit raises exactgrad.ExactGradError, or with fallback='bp' contributes its BP statistics (gradient and
        log-posterior).  Returns (mean log-likelihood of the instances at the thetas they were evaluated under, instances that
        fell back to BP, over all ranks).  Per-domain thetas are not supported.  Not captured into the step graph; step() and
        epoch() are what they were."""
        if self.domains:
            raise NotImplementedError('exact_step does not update per-domain thetas')
        if fallback not in (None, 'bp'):
            raise ValueError("fallback is None or 'bp'")
        exact, _, loglik, seen, fall, _ = self._exact_statistics('bp' if fallback == 'bp' else 'raise')
        n = self.n_stat
        stats = torch.tensor(list(exact) + [loglik, float(seen)] + list(fall), dtype=torch.float64, device=self.device)
        mdist.all_reduce_sum_(stats)
        n_fallback = int(stats[2 * n - 1].item())
        stats = stats[:n] + stats[n:]
        update_thetas(self, stats, learning_rate, reg_param, self.reg_param_ua_scale)
        return float(stats[n - 2].item() / max(stats[n - 1].item(), 1.0)), n_fallback

    # ---- and a step for every sentence: the gradient estimated beyond the exact limit (the listed mode of include/mlbp_exactgrad.h) ----
    def estimated_step(self, learning_rate, reg_param, n_list=256, seed=0, proposal='messages'):
        """exact_step() for EVERY sentence: the same statistics vector and single all-reduce, where a shape the exact call
        admits contributes UserGraphTrainer.exact_gradient() and every other shape UserGraphTrainer.estimated_gradient(n_list,
        seed + i, proposal) -- i its position in self.trainers order --, its joint_logp_hat in the place of joint_logp.  No
        sentence falls back to BP and none is skipped; a shape the listed plan refuses (more than 16 cutset variables) raises
        cutsetis.CutsetisError.  On a file whose shapes the exact call admits it IS exact_step(): the same thetas bit for bit.
        Returns (mean log-likelihood of the instances at the thetas they were evaluated under -- estimated where the gradient
        is --, instances estimated, over all ranks).  Per-domain thetas are not supported.  Not captured into the step graph."""
        from . import exactgrad as K
        if self.domains:
            raise NotImplementedError('estimated_step does not update per-domain thetas')
        n = self.n_stat

        def call(i, tr):
            exact, e = _try(tr.exact_gradient, K.ExactGradError)
            if e is None:
                return exact[:3] + (0,)
            return tr.estimated_gradient(n_list=n_list, seed=int(seed) + i, proposal=proposal)[:3] + (1,)
        _, shapes = self._per_shape(call)
        grad, tail = np.zeros(n - 2), np.zeros(n)
        loglik, seen = 0.0, 0
        for _, rows, (g_ee, g_ed, joint, estimated) in shapes:
            seen += len(rows)
            loglik += float(joint.sum())
            grad += np.concatenate([g_ee.sum(axis=0), g_ed.sum(axis=0)])
            tail[n - 1] += estimated * len(rows)
        stats = torch.tensor(list(grad) + [loglik, float(seen)] + list(tail), dtype=torch.float64, device=self.device)
        mdist.all_reduce_sum_(stats)
        n_estimated = int(stats[2 * n - 1].item())
        stats = stats[:n] + torch.cat([stats[n:2 * n - 1], torch.zeros(1, dtype=torch.float64, device=self.device)])
        update_thetas(self, stats, learning_rate, reg_param, self.reg_param_ua_scale)
        return float(stats[n - 2].item() / max(stats[n - 1].item(), 1.0)), n_estimated

    def estimated_gradient_report(self, n_list=256, seed=0):
        """-> totals: the estimated gradient over ALL shapes under the current thetas, and how far it is from the true one
        where the exact call exists.  totals = (estimate [F_ee + F_ed] -- UserGraphTrainer.estimated_gradient(n_list, seed + i)
        summed over every instance --, exact [F_ee + F_ed] -- UserGraphTrainer.exact_gradient() summed over the instances of
        the shapes it admits --, the estimate summed over those same instances, the cosine of the last two, |estimate - exact|
        / |exact| of the same, sum of joint_logp_hat over every instance, instances, instances also solved exactly) over ALL
        ranks' instances, reduced once.  The two distances are figures to record: nothing bounds them."""
        from . import exactgrad as K
        F = self.n_stat - 2

        def call(i, tr):
            est = tr.estimated_gradient(n_list=n_list, seed=int(seed) + i)
            exact, _ = _try(tr.exact_gradient, K.ExactGradError)           # above the exact limit: estimated alone
            return est[:3] + (None if exact is None else exact[:2],)
        _, shapes = self._per_shape(call)
        est, exact, est_on = np.zeros(F), np.zeros(F), np.zeros(F)
        loglik, seen, both = 0.0, 0, 0
        for _, rows, (g_ee, g_ed, joint_hat, x) in shapes:
            g = np.concatenate([g_ee.sum(axis=0), g_ed.sum(axis=0)])
            seen += len(rows)
            loglik += float(joint_hat.sum())
            est += g
            if x is not None:
                both += len(rows)
                est_on += g
                exact += np.concatenate([x[0].sum(axis=0), x[1].sum(axis=0)])
        tot, _ = self._reduced(list(est) + list(exact) + list(est_on) + [loglik, seen, both])
        est, exact, est_on = tot[:F], tot[F:2 * F], tot[2 * F:3 * F]
        ne, no = float(np.linalg.norm(exact)), float(np.linalg.norm(est_on))
        cosine = float(exact.dot(est_on)) / (ne * no) if ne > 0 and no > 0 else float('nan')
        rel = float(np.linalg.norm(est_on - exact)) / ne if ne > 0 else float('nan')
        return est, exact, est_on, cosine, rel, float(tot[3 * F]), int(tot[3 * F + 1]), int(tot[3 * F + 2])

    # ---- which guesses are truly the best: exact joint decoding (include/mlbp_exactmap.h) ------------
    def exact_decode(self):
        """-> (guesses, counts, report, skipped).  guesses[i], for instance i of this rank's shard in file order: (predicted
        positions, [en words], score, margin, joint_logp) as UserGraphTrainer.exact_decode gives them -- the set of guesses
        that truly maximises the model, its log-potential, its lead over the best set that differs in a word and its true
        log-probability; an instance without a predicted word builds no graph and gives ((), [], 0.0, 0.0, 0.0), one of a shape
        above the configuration limit (positions, None, None, None, None).  counts: as decode() counts, over the exact
        guesses.  report = (sentences compared, sentences where map_sweep decoded the same set, sum of shortfall, largest
        shortfall) over ALL ranks' instances, reduced once.  skipped: [(predicted positions, instances, reason)] of this
        rank's shapes above the limit.  decode() itself is what it was."""
        from . import exactmap as K
        skipped = []
        guesses, shapes = self._per_shape(
            lambda i, tr: tr.exact_decode(), empty=((), [], 0.0, 0.0, 0.0), placeholder=(None,) * 4, refused=K.ExactMapError,
            skipped=skipped, row=lambda r, b: ([self.en[w] for w in r[0][b]], float(r[1][b]), float(r[2][b]), float(r[5][b])))
        counts = np.zeros(4, dtype=np.int64)
        seen = n_agree = 0
        sum_short = worst = 0.0
        for key, rows, (x, _, _, agrees, shortfall, _) in shapes:
            counts += self._hit_counts(key, x)
            seen += len(rows)
            n_agree += int(agrees.sum())
            sum_short += float(shortfall.sum())
            worst = max(worst, float(shortfall.max()))
        tot, top = self._reduced(list(counts) + [seen, n_agree, sum_short], [worst])
        return (guesses, tuple(int(v) for v in tot[:4]), (int(tot[4]), int(tot[5]), float(tot[6]), float(top[0])), skipped)

    # ---- search decoding beyond the exact limit (the listed mode of include/mlbp_exactmap.h) -----------------
    def search_decode(self, n_samples=256, seed=0):
        """-> (guesses, counts).  guesses[i], for instance i of this rank's shard in file order: (predicted positions, [en
        words], score, score - score_bp) as UserGraphTrainer.search_decode gives them -- the best set of guesses among those
        whose cutset state is listed, its log-potential and its gain over decode()'s set; an instance without a predicted
        word builds no graph and gives ((), [], 0.0, 0.0).  No shape is skipped for its number of configurations (up to 16
        cutset variables): the sentences exact_decode() lists as skipped are decoded here, the others too, so the two
        reports can be laid side by side.  The i-th sentence shape in self.trainers order draws with seed `seed + i`.
        counts = (sentences decoded, sentences whose score rose above decode()'s by more than SEARCH_ROSE relative to
        max(1, |score|) -- the rounding of the two sums of logarithms --, sentences whose words changed) over ALL ranks'
        instances, reduced once."""
        guesses, shapes = self._per_shape(
            lambda i, tr: tr.search_decode(n_samples=n_samples, seed=int(seed) + i), empty=((), [], 0.0, 0.0),
            row=lambda r, b: ([self.en[w] for w in r[0][b]], float(r[1][b]), float(r[1][b] - r[2][b])))
        counts = np.zeros(3, dtype=np.int64)
        for _, _, (_, score, score_bp, changed) in shapes:
            rose = score - score_bp > SEARCH_ROSE * np.maximum(1.0, np.abs(score))
            counts += np.array([len(score), int(rose.sum()), int(changed.sum())], dtype=np.int64)
        return guesses, tuple(int(v) for v in self._reduced(counts)[0])

    # ---- the ranked list of whole sets of guesses (include/mlbp_exactmbest.h) ---------------------------
    def exact_nbest(self, m):
        """-> (per_sentence, totals, skipped).  per_sentence[i], for instance i of this rank's shard in file order: (predicted
        positions, [[en words] per rank], [score], [logp]) -- the at most `m` sets of guesses the model truly ranks highest,
        best first, their log-potentials and true log-probabilities (UserGraphTrainer.exact_nbest; the lists end where the
        model has no further set of positive potential); an instance without a predicted word builds no graph and gives
        ((), [], [], []), one of a shape above the configuration limit (positions, None, None, None).  totals = (sentences
        compared, sum of `covered` -- the mass the lists hold --, recall [m]: recall[r] = sentences whose labelled set of
        guesses sits at rank <= r, sentences whose decode() set is in the list) over ALL ranks' instances, reduced once.
        skipped: as exact_decode gives it."""
        from . import exactmbest as K
        m = int(m)
        if not 1 <= m <= K.MAX_M:
            raise ValueError('m must be in [1, %d]' % K.MAX_M)
        def ranked(r, b):
            x, score, logp = r[:3]
            have = int((x[b, :, 0] >= 0).sum())
            return ([[self.en[w] for w in x[b, k]] for k in range(have)], [float(v) for v in score[b, :have]],
                    [float(v) for v in logp[b, :have]])

        skipped = []
        per_sentence, shapes = self._per_shape(lambda i, tr: tr.exact_nbest(m), empty=((), [], [], []), placeholder=(None,) * 3,
                                               refused=K.ExactMbestError, skipped=skipped, row=ranked)
        recall = np.zeros(m)
        seen = n_bp = 0
        covered_sum = 0.0
        for _, rows, (_, _, _, covered, label_rank, bp_rank) in shapes:
            seen += len(rows)
            n_bp += int((bp_rank >= 0).sum())
            covered_sum += float(covered.sum())
            for r in range(m):
                recall[r] += int(((label_rank >= 0) & (label_rank <= r)).sum())
        tot, _ = self._reduced([seen, covered_sum, n_bp] + list(recall))
        return per_sentence, (int(tot[0]), float(tot[1]), [int(v) for v in tot[3:]], int(tot[2])), skipped

    # ---- the ranked list beyond the exact limit (the listed mode of include/mlbp_exactmbest.h) ----------------
    def search_nbest(self, m, n_samples=256, seed=0):
        """-> (per_sentence, totals).  per_sentence[i], for instance i of this rank's shard in file order: (predicted
        positions, [[en words] per rank], [score]) -- the at most `m` best sets of guesses among those whose cutset state is
        on search_decode()'s list, best first, and their log-potentials (UserGraphTrainer.search_nbest); an instance without
        a predicted word builds no graph and gives ((), [], []).  No shape is skipped for its number of configurations (up to
        16 cutset variables): the sentences with five and more predicted words that exact_nbest() lists as skipped are ranked
        here, the others too.  The i-th sentence shape in self.trainers order draws with seed `seed + i`.  totals =
        (sentences ranked, recall [m]: recall[r] = sentences whose labelled set of guesses sits at rank <= r, sentences whose
        decode() set is in the list) over ALL ranks' instances, reduced once.  No logp is returned: entry 0 of a list is
        decode()'s cutset state and no draw from a proposal, so the list carries no unbiased log Z."""
        from . import exactmbest as K
        m = int(m)
        if not 1 <= m <= K.MAX_M:
            raise ValueError('m must be in [1, %d]' % K.MAX_M)

        def ranked(r, b):
            x, score, n_found = r[:3]
            have = max(int(n_found[b]), 0)
            return [[self.en[w] for w in x[b, k]] for k in range(have)], [float(v) for v in score[b, :have]]

        per_sentence, shapes = self._per_shape(lambda i, tr: tr.search_nbest(m, n_samples=n_samples, seed=int(seed) + i),
                                               empty=((), [], []), row=ranked)
        recall = np.zeros(m)
        seen = n_bp = 0
        for _, rows, (_, _, _, label_rank, bp_rank) in shapes:
            seen += len(rows)
            n_bp += int((bp_rank >= 0).sum())
            for r in range(m):
                recall[r] += int(((label_rank >= 0) & (label_rank <= r)).sum())
        tot, _ = self._reduced([seen, n_bp] + list(recall))
        return per_sentence, (int(tot[0]), [int(v) for v in tot[2:]], int(tot[1]))

    # ---- joint log-likelihood (log Z; the reference has only the sum of per-word log-marginals) ------
    def joint_log_likelihood(self):
        """-> (per_instance, totals).  per_instance[i], for instance i of this rank's shard in file order: (predicted
        positions, joint_logp, log_z) -- the log-probability of the user's whole set of guesses for the sentence
        (UserGraphTrainer.joint_log_likelihood) and the sentence graph's log Z; an instance without a predicted word builds
        no graph and gives ((), 0.0, 0.0).  totals = (sum of joint_logp, sentences with a predicted word) over ALL ranks'
        instances, reduced once."""
        per_instance, shapes = self._per_shape(lambda i, tr: tr.joint_log_likelihood(), empty=((), 0.0, 0.0),
                                               row=lambda r, b: (float(r[0][b]), float(r[1][b])))
        total, seen = 0.0, 0
        for _, _, (joint, _) in shapes:
            total += float(joint.sum())
            seen += joint.shape[0]
        tot, _ = self._reduced([total, seen])
        return per_instance, (float(tot[0]), int(tot[1]))

    # ---- prediction pass (train_mp.py:310-343, 692-770) -------------------------------------------
    def predict(self, save_predictions=None):
        """-> (mean log-posterior, (p@0, p@25, p@50, total)) over ALL ranks' instances (train_mp.py:666-684: sums reduced once).
        save_predictions: the '*SENT_ID:' blocks go to '<path><ext>' and the '.dist' lines to '<path><ext>.dist', one block per
        instance in file order, exactly the text `batch_predictions` returns (train_mp.py:337-338, 752-757) -- formed from the
        batched top-50 indices and log-marginals, no per-instance graph.  With several ranks every rank writes its shard
        ('.rank<r>') and rank 0 joins the shards into the ONE pair of files the reference writes (train_mp.py:740-760)."""
        from . import tidir
        lp, counts = 0.0, np.zeros(4, dtype=np.int64)
        blocks = {}
        ext = ADAPT_EXT[self.adapt]
        for key, tr in self.trainers.items():
            l, idx, logs, c, logm, label_logs = tr.predict(top=min(50, tr.batch.X), with_logs=True)
            lp += float(l.sum()); counts += np.array(c)
            if save_predictions:
                rows = self.buckets[key]['rows']
                for b, row in enumerate(rows):
                    blocks[row['index']] = tidir.prediction_text(row, list(key[1]), self.en, idx[b], logs[b], label_logs[b], logm[b])
        # the mean's denominator is every instance of the shard -- `/ float(len(testing_instances))`, train_mp.py:684, 764 -- also
        # the ones without a predicted word, which build no graph here (the reference's workers fail on them and the pool drops
        # the task silently, train_mp.py:666-680; LBP.py:193-194)
        n = self._shard[1] - self._shard[0]
        if save_predictions:
            import codecs
            tail = '.rank%d' % self.rank if self.world > 1 else ''
            with codecs.open(save_predictions + ext + tail, 'w', 'utf8') as w, codecs.open(save_predictions + ext + '.dist' + tail, 'w', 'utf8') as wd:
                for i in sorted(blocks):
                    w.write(blocks[i][0] + '\n')
                    wd.write(blocks[i][1] + '\n')
        tot = torch.tensor([lp, float(n)] + [float(v) for v in counts], dtype=torch.float64, device=self.device)
        mdist.all_reduce_sum_(tot)
        tot = tot.cpu().numpy()
        if save_predictions and self.world > 1:
            # ONE '<path><ext>' and one '.dist' in instance order, as the reference writes them (train_mp.py:740-760) and eval.py /
            # get_acc.py read them: the shards are contiguous, so rank order is instance order.  (The all-reduce above is the
            # barrier: every rank has closed its files.)
            import shutil
            if self.rank == 0:
                for suffix in ('', '.dist'):
                    with open(save_predictions + ext + suffix, 'wb') as out:
                        for r in range(self.world):
                            part = '%s%s%s.rank%d' % (save_predictions, ext, suffix, r)
                            with open(part, 'rb') as f:
                                shutil.copyfileobj(f, out)
                            os.remove(part)
            mdist.barrier()
        return float(tot[0] / max(tot[1], 1.0)), tuple(int(v) for v in tot[2:])
