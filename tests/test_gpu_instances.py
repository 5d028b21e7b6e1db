"""GPU parity per compiled kernel instance: every instance of the sweep and contraction families that the dispatch code can
reach has a case here (COVERED; tests/test_kernel_inventory.py checks the list against the built library).  Each case runs a
workload that reaches its instance, checks in the launch log (mlbp_launch_log) that the instance ran, and compares the
call's outputs with the float64 oracle (oracle/lbp_oracle.py); the kernels that run only inside such calls (COMPOUND) are
checked the same way, through the all-kernel launch log.  Tolerances:

- messages, marginals, log-posteriors and their batch sum: 1e-10 relative;
- gradients (unregularized_gradient): 1e-8;
- float32 pairwise tables: against the oracle on the float32-rounded tables, 1e-5 (messages) / 5e-6 (marginals);
- unnormalised messages: against the oracle with Message.renormalize replaced by the identity.

Workloads are shared by the instances they reach and run once per module.  Batch sizes leave a ragged last workgroup for
the instance's graphs per workgroup (16 for the shared-table and contraction kernels, 32 for the two-tile contraction, 64
for the fix-up pass); the large batches of the two-tile contraction are compared with the oracle on a sample and in full
with the per-graph kernels (mlbp_set_sweep_variant(3)).
"""
import copy
import functools

import numpy as np
import pytest

import cases as C
import kernel_inventory as K
from helpers import batch_tables
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

RTOL = 1e-10
GRAD_RTOL = 1e-8


# ---- topologies ------------------------------------------------------------------------------------------------------
def _user_p2(X):
    """A trainmp-style graph with exactly two pairwise factors: K3 without its (first, last) factor."""
    s = C.user_spec(10, [1, 4, 7], X, 40, seed=1, name='user_p2_x%d' % X)
    s['factors'] = [f for f in s['factors'] if f['vars'] != [1, 7]]
    return s


def _no_unary(s, v):
    """Spec s without the unary factors of variable v: v has no constant product, so a call that asks for the marginals keeps
    the shared-table kernel off its product-fused and three-source forms."""
    s = copy.deepcopy(s)
    s['name'] += '_nou%d' % v
    s['factors'] = [f for f in s['factors'] if f['vars'] != [v]]
    if s['style'] == 'explicit':           # (table keys stay contiguous)
        keys = sorted({f['table'] for f in s['factors']})
        for f in s['factors']:
            f['table'] = keys.index(f['table'])
    return s


def _parallel(X, n):
    """Two variables joined by n parallel pairwise factors (each variable update multiplies n tiles), unary factors on both."""
    s = C.chain_spec(2, X, 'parallel%d_x%d' % (n, X))
    for k in range(1, n):
        s['factors'].append(dict(id=3 + k - 1, vars=[0, 1], dims=[0, 1] if k % 2 else [1, 0], table=3 + k - 1))
    return s


SPECS = {
    'chain2': lambda X: C.chain_spec(2, X),
    'chain3': lambda X: C.chain_spec(3, X),
    'chain5': lambda X: C.chain_spec(5, X),
    'chain9': lambda X: C.chain_spec(9, X),
    'ring3': lambda X: C.ring_spec(3, X),
    'ring4': lambda X: C.ring_spec(4, X),
    'ring5': lambda X: C.ring_spec(5, X),
    'ring7': lambda X: C.ring_spec(7, X),
    'ring8': lambda X: C.ring_spec(8, X),
    'star5': lambda X: C.star_spec(5, X),
    'chain2_nou1': lambda X: _no_unary(C.chain_spec(2, X), 1),
    'ring3_nou1': lambda X: _no_unary(C.ring_spec(3, X), 1),
    'parallel3_nou1': lambda X: _no_unary(_parallel(X, 3), 1),
    'user_k2_nou1': lambda X: _no_unary(C.user_spec(6, [0, 1], X, 40, seed=3), 1),
    'user_k3_nou4': lambda X: _no_unary(C.user_spec(10, [1, 4, 7], X, 40, seed=1), 4),
    'user_k1': lambda X: C.user_spec(6, [2], X, 40, seed=3),
    'user_k2': lambda X: C.user_spec(6, [0, 1], X, 40, seed=3),
    'user_p2': _user_p2,
    'user_k3': lambda X: C.user_spec(10, [1, 4, 7], X, 40, seed=1),
    'user_k4': lambda X: C.user_spec(9, [0, 2, 3, 7], X, 40, seed=4),
    'user_k5': lambda X: C.user_spec(9, [0, 2, 3, 5, 8], X, 40, seed=6),
}
ROOTS = {   # a root sequence with a repeat and at least three sweeps, by variable id
    'chain2': [0, 1, 0], 'chain3': [0, 2, 1, 0], 'chain5': [0, 4, 2, 0], 'chain9': [0, 8, 4, 0],
    'ring3': [0, 2, 1, 0], 'ring4': [0, 2, 3, 0], 'ring5': [0, 3, 1, 0], 'ring7': [0, 4, 6, 0],
    'ring8': [0, 5, 2, 0], 'star5': [0, 3, 5, 0], 'chain2_nou1': [0, 1, 0], 'ring3_nou1': [0, 2, 1, 0], 'parallel3_nou1': [0, 1, 0],
    'user_k2_nou1': [0, 1, 0], 'user_k3_nou4': [4, 1, 7, 4],
    'user_k1': [2, 2, 2], 'user_k2': [0, 1, 0], 'user_p2': [4, 1, 7, 4], 'user_k3': [4, 1, 7, 4], 'user_k4': [2, 7, 0, 2],
    'user_k5': [3, 8, 0, 3],
}


# ---- workloads -------------------------------------------------------------------------------------------------------
# name -> dict: spec, X, B, layout ('unique': every graph its own tables, 'shared': graph 0's pairwise tables for all),
# f32 (float32 pairwise tables), norm, variant (1: default dispatch, 3: per-graph kernels), grad (the call's gradient),
# post (posterior), zero (graph whose first pairwise table -- own tables -- or unary table -- shared pairwise tables -- is all
# zero: flagged by the fast kernels, redone by the exact one),
# heavy_last (explicit tables scaled by 1e3 in the last real state's rows and columns), F (feature counts of a standalone
# gradient call), groups (list of sub-workloads for mlbp_sweep_groups_f64), sample
# (graphs compared with the oracle), full_check (compare every graph with the per-graph kernels' result).
WORKLOADS = {}


def _w(name, **kw):
    assert name not in WORKLOADS
    kw.setdefault('kind', 'sweep')
    WORKLOADS[name] = kw


# X = 64: exact kernel on every graph (variant 3), normalised and not, tables in registers (P = 1..3) or streamed
for _s in ('chain2', 'chain3', 'ring3', 'ring5'):
    _w('exact_%s' % _s, spec=_s, X=64, B=5, layout='unique', variant=3, post=True)
    _w('exact_unnorm_%s' % _s, spec=_s, X=64, B=5, layout='unique', variant=3, norm=False)
_w('exact_b1_ring3', spec='ring3', X=64, B=1, layout='unique', variant=3)
# ... with the gradient as its epilogue (F = (3, 6), at most three pairwise factors)
for _s in ('user_k1', 'user_k2', 'user_p2', 'user_k3'):
    _w('exact_grad_%s' % _s, spec=_s, X=64, B=5, layout='unique', variant=3, grad=True)
# ... as the fix-up pass behind the fast kernels (64 graphs per workgroup: B = 67 leaves a ragged one)
_w('fixup_lean_ring3', spec='ring3', X=64, B=67, layout='unique', zero=66, post=True)
_w('fixup_lean_grad_user_k3', spec='user_k3', X=64, B=67, layout='unique', zero=65, grad=True)
_w('fixup_shared_grad_user_k4', spec='user_k4', X=64, B=67, layout='shared', zero=64, grad=True)
# lean kernel: one call
for _s in ('chain2', 'chain3', 'ring3', 'ring4', 'ring5', 'ring7', 'chain9'):
    _w('lean_%s' % _s, spec=_s, X=64, B=7, layout='unique')
_w('lean_b1_ring3', spec='ring3', X=64, B=1, layout='unique', unshared=True)
for _s in ('user_k2', 'user_p2', 'user_k3'):
    _w('lean_grad_%s' % _s, spec=_s, X=64, B=9, layout='unique', grad=True)
for _s, _x in (('chain2', 16), ('chain3', 33), ('ring3', 48), ('chain5', 17)):
    _w('lean_small_%s_x%d' % (_s, _x), spec=_s, X=_x, B=9, layout='unique')
# lean kernel: grouped calls (the kernel instance follows the largest P of the groups)
for _big in ('chain2', 'chain3', 'ring3', 'ring4', 'ring5', 'ring7', 'ring8'):
    _w('lean_groups_%s' % _big, kind='groups', groups=[dict(spec='chain2', X=64, B=3, layout='unique'),
                                                      dict(spec=_big, X=64, B=5, layout='unique')])
# shared-table kernel (X = 64, shared pairwise tables, 16 graphs per workgroup)
for _s in ('user_k2', 'user_k3', 'user_k4', 'user_k5', 'ring8', 'chain2_nou1', 'ring3_nou1', 'parallel3_nou1'):
    _w('shared_%s' % _s, spec=_s, X=64, B=19, layout='shared', post=_s.startswith('user'))
_w('shared_b1_user_k3', spec='user_k3', X=64, B=1, layout='shared')
for _s in ('user_k2', 'user_k3', 'user_k4', 'user_k5', 'user_k2_nou1', 'user_k3_nou4'):
    _w('shared_grad_%s' % _s, spec=_s, X=64, B=19, layout='shared', grad=True)
_SHARED_GROUPS = {          # (a launch takes one instance per form: product-fused, three-source, general)
    'k2': ['user_k2'], 'k2_k3': ['user_k2', 'user_k3'], 'k2_k4': ['user_k2', 'user_k4'], 'k5': ['user_k5'],
    'k2_k5': ['user_k2', 'user_k5'], 'k3_k4_k5': ['user_k3', 'user_k4', 'user_k5'], 'ring8': ['ring8'],
    'c2nou': ['chain2_nou1'], 'c2nou_ring8': ['chain2_nou1', 'ring8'], 'r3nou': ['ring3_nou1'], 'par3nou': ['parallel3_nou1'],
    'uk2nou': ['user_k2_nou1'], 'uk3nou': ['user_k3_nou4'],
}
for _n, _ss in _SHARED_GROUPS.items():
    if _n not in ('k2_k5', 'uk2nou', 'uk3nou'):
        _w('shared_groups_%s' % _n, kind='groups', groups=[dict(spec=s, X=64, B=17 + 2 * i, layout='shared') for i, s in enumerate(_ss)])
    if all(s.startswith('user') for s in _ss) and _n != 'k5':
        _w('shared_groups_grad_%s' % _n, kind='groups',
           groups=[dict(spec=s, X=64, B=17 + 2 * i, layout='shared', grad=True) for i, s in enumerate(_ss)])
# wide kernel: X = 128 / 256 / 512 exactly (float64 and float32 tables, normalised and not), and padded (normalised, float64)
for _x in (128, 256, 512):
    _w('wide_x%d' % _x, spec='ring5', X=_x, B=3, layout='unique', post=True)
    _w('wide_unnorm_x%d' % _x, spec='ring5', X=_x, B=3, layout='unique', norm=False)
for _x in (256, 512):
    _w('wide_f32_x%d' % _x, spec='ring5', X=_x, B=3, layout='unique', f32=True)
    _w('wide_f32_unnorm_x%d' % _x, spec='ring5', X=_x, B=3, layout='unique', f32=True, norm=False)
for _x in (97, 100, 201, 200, 300, 301, 450, 451, 700, 701, 800, 801):
    _w('wide_pad_x%d' % _x, spec='ring3', X=_x, B=2, layout='unique', heavy_last=True)
_w('wide_b1_x128', spec='ring5', X=128, B=1, layout='unique', variant=3)
# generic kernel: X < 64 and X > 1024 (normalised or not), messages in LDS or in global memory
_w('generic_x16', spec='ring5', X=16, B=3, layout='unique', variant=3)
_w('generic_unnorm_x4', spec='star5', X=4, B=3, layout='unique', norm=False)
_w('generic_x1100', spec='ring5', X=1100, B=2, layout='unique')
_w('generic_unnorm_x700', spec='ring5', X=700, B=2, layout='unique', norm=False)
_w('generic_b1_x16', spec='ring5', X=16, B=1, layout='unique', variant=3)
# contraction kernels (shared tables, 65 <= X <= 4096): one image, padded, chunked in 2 .. 4 passes, float32 tables
for _x in (128, 256, 384, 512, 97, 201, 300, 450, 600, 700, 850, 1000, 1100, 1700, 2100, 2500, 3000, 4096):
    _w('gemm_x%d' % _x, spec='ring3', X=_x, B=19, layout='shared', post=_x <= 512, heavy_last=True)
_w('gemm_b1_x128', spec='ring3', X=128, B=1, layout='shared')
for _x in (256, 512):
    _w('gemm_f32_x%d' % _x, spec='ring3', X=_x, B=19, layout='shared', f32=True)
for _x in (128, 256):      # 32 graphs per workgroup from 16384 graphs on: the ragged last workgroup holds 19
    _w('gemm_big_x%d' % _x, spec='chain2', X=_x, B=16384 + 19, layout='shared', full_check=True,
       sample=list(range(0, 40)) + [32 * k + j for k in (101, 257) for j in (0, 15, 16, 31)] + list(range(16384 - 13, 16384 + 19)))
for _x in (128, 384, 2100):
    _w('gemm_grad_x%d' % _x, spec='user_k3', X=_x, B=19, layout='shared', grad=True)
# standalone gradient calls, each feature count (F_ee, F_ed) the kernels are compiled for
for _f in ((1, 1), (2, 2), (3, 6)):
    _w('gradient_x64_f%d%d' % _f, kind='gradient', spec='user_k3', X=64, B=5, layout='unique', F=_f)
    _w('gradient_x128_f%d%d' % _f, kind='gradient', spec='user_k3', X=128, B=5, layout='unique', F=_f)
_w('gradient_b1_x64', kind='gradient', spec='user_k3', X=64, B=1, layout='unique', F=(3, 6), unshared=True)
_w('gradient_b1_x128', kind='gradient', spec='user_k3', X=128, B=1, layout='unique', F=(3, 6))
# ... with shared pairwise tables: the pairwise part on the matrix cores (X = 64) or as contractions (X = 128)
_w('gradient_shared_x64', kind='gradient', spec='user_k3', X=64, B=19, layout='shared', F=(3, 6))
_w('gradient_shared_x128', kind='gradient', spec='user_k3', X=128, B=19, layout='shared', F=(3, 6))


# ---- running a workload ----------------------------------------------------------------------------------------------
class _Group:
    """One batch of a workload: its spec, per-graph oracle inputs, device batch and outputs."""

    def __init__(self, w, seed, mutate=None):
        from macaronicusermodeling_amd.batch import FactorGraphBatch
        from macaronicusermodeling_amd.topology import GraphTopology
        X, B = w['X'], w['B']
        self.w, self.X, self.B = w, X, B
        self.spec = spec = SPECS[w['spec']](X)
        self.roots = ROOTS[w['spec']]
        self.topo = topo = GraphTopology.from_spec(spec)
        self.trainmp = spec['style'] == 'trainmp'
        self.norm = w.get('norm', True)
        F = w.get('F', (3, 6))
        base = C.make_inputs(spec, seed)
        rs = np.random.RandomState(seed + 1)
        inputs = []
        for b in range(B):
            if self.trainmp:
                i = dict(base)
                if w['layout'] == 'unique':          # own pots per graph, the batch's feature tensors
                    i['pot_en_en'] = np.exp(rs.randn(X, X) * 0.5)
                    i['pot_en_en_w1'] = np.exp(rs.randn(X, X) * 0.5)
                i['pot_en_de'] = np.exp(rs.randn(*base['pot_en_de'].shape) * 0.5)
                if F != (3, 6):
                    i['phi_en_en'], i['phi_en_en_w1'] = base['phi_en_en'][:, :, :F[0]], base['phi_en_en_w1'][:, :, :F[0]]
                    i['phi_en_de'] = base['phi_en_de'][:, :, :F[1]]
                    i['theta_en_en'], i['theta_en_de'] = base['theta_en_en'][:, :F[0]], base['theta_en_de'][:, :F[1]]
            else:
                tabs = list(base['tables'])
                for f in spec['factors']:
                    if len(f['vars']) == 1 or (w['layout'] == 'unique' and b > 0):
                        tabs[f['table']] = rs.rand(*tabs[f['table']].shape) + 0.01
                if w['layout'] == 'shared':          # every pairwise factor reads one of graph 0's first two tables
                    pf = [f for f in spec['factors'] if len(f['vars']) == 2]
                    for p, f in enumerate(pf):
                        tabs[f['table']] = base['tables'][pf[p % 2]['table']]
                i = dict(tables=tabs)
            inputs.append(i)
        if w.get('heavy_last'):               # the last real state carries most of every message: padding bugs show at 1e-10
            for i in inputs:
                tabs = [t.copy() for t in i['tables']]
                for t in tabs:
                    t[X - 1, :] *= 1e3
                    if t.shape[1] > 1:
                        t[:, X - 1] *= 1e3
                i['tables'] = tabs
        if w.get('zero') is not None:         # graph b's first pairwise table (own tables) or unary one (shared tables) all zero
            b = w['zero']
            if w['layout'] == 'unique' and self.trainmp:
                inputs[b]['pot_en_en'] = inputs[b]['pot_en_en'] * 0.0
                inputs[b]['pot_en_en_w1'] = inputs[b]['pot_en_en_w1'] * 0.0
            elif w['layout'] == 'unique':
                t = [f for f in spec['factors'] if len(f['vars']) == 2][0]['table']
                inputs[b]['tables'] = list(inputs[b]['tables'])
                inputs[b]['tables'][t] = inputs[b]['tables'][t] * 0.0
            elif self.trainmp:
                col = [f for f in spec['factors'] if f.get('factor_type') == 'en_de'][0]['observed_dim']
                inputs[b]['pot_en_de'] = inputs[b]['pot_en_de'].copy()
                inputs[b]['pot_en_de'][:, col] = 0.0
            else:
                t = [f for f in spec['factors'] if len(f['vars']) == 1][0]['table']
                inputs[b]['tables'] = list(inputs[b]['tables'])
                inputs[b]['tables'][t] = inputs[b]['tables'][t] * 0.0
        if mutate:                            # (a caller's own inputs or edits, in place, before anything is derived from them)
            mutate(inputs)
        self.inputs = inputs
        g = self.g = O.Graph(spec)
        pair, unary = batch_tables(spec, topo, inputs)
        fb = self.fb = FactorGraphBatch(topo, X, B, normalize_messages=self.norm)
        dtype = torch.float32 if w.get('f32') else torch.float64
        by_id = {f['id']: f for f in spec['factors']}
        if topo.P:
            if w['layout'] == 'shared':
                if self.trainmp:
                    pair_phi = [0 if by_id[topo.factor_ids[j]]['gap'] > 1 else 1 for j in topo.pair_factors]
                    fb.set_pair_tables(np.stack([inputs[0]['pot_en_en'], inputs[0]['pot_en_en_w1']]), np.tile(pair_phi, (B, 1)), dtype=dtype)
                else:                            # graph 0's first two tables, alternating (the kernels hold two)
                    pick = [p % 2 for p in range(topo.P)]
                    fb.set_pair_tables(pair[:min(topo.P, 2)], np.tile(pick, (B, 1)), dtype=dtype)
                assert fb.pair_tables_shared
            else:
                fb.set_pair_tables(pair, dtype=dtype)
                if w.get('unshared'):            # B = 1 with its own tables: not stated shared (the per-graph kernels)
                    fb.pair_tables_shared, fb._pair_row_host = False, None
                assert fb.pair_tables_shared == (B == 1 and not w.get('unshared'))
        if topo.U:
            fb.set_unary_tables(unary)
        if w.get('f32'):                           # the oracle reads the float32-rounded tables
            for i in inputs:
                if self.trainmp:
                    i['pot_en_en'] = i['pot_en_en'].astype(np.float32).astype(np.float64)
                    i['pot_en_en_w1'] = i['pot_en_en_w1'].astype(np.float32).astype(np.float64)
                else:
                    i['tables'] = [t.astype(np.float32).astype(np.float64) if t.shape[1] > 1 else t for t in i['tables']]
        self.grad = w.get('grad') or w.get('kind') == 'gradient'
        if self.grad:
            pair_phi = [0 if by_id[topo.factor_ids[j]]['gap'] > 1 else 1 for j in topo.pair_factors]
            kinds, obs = [], []
            for j in topo.unary_factors:
                f = by_id[topo.factor_ids[j]]
                kinds.append(2 if f['factor_type'] == 'en_de' else (0 if f['gap'] > 1 else 1))
                obs.append(f['observed_dim'])
            i0 = inputs[0]
            fb.set_features(i0['phi_en_en'], i0['phi_en_en_w1'], i0['phi_en_de'], pair_phi, kinds)
            label_of = dict(zip(spec['var_ids'], spec['labels']))
            fb.set_observations(np.tile([label_of[v] for v in topo.var_ids], (B, 1)), np.tile(obs, (B, 1)))
            dev = fb.device
            self.g_ee = torch.full((B, F[0]), float('nan'), dtype=torch.float64, device=dev)
            self.g_ed = torch.full((B, F[1]), float('nan'), dtype=torch.float64, device=dev)
        dev = fb.device
        self.marg = torch.full((B, topo.n_vars, X), float('nan'), dtype=torch.float64, device=dev) if self.norm else None
        self.post = None
        if w.get('post'):
            label_of = dict(zip(spec['var_ids'], spec['labels']))
            lab = torch.from_numpy(np.tile([label_of[v] for v in topo.var_ids], (B, 1)).astype(np.int32)).to(dev)
            self.post = (lab, torch.full((B,), float('nan'), dtype=torch.float64, device=dev),
                         torch.full((1,), float('nan'), dtype=torch.float64, device=dev))
        fb.msgs.fill_(float('nan'))

    def sweep_kwargs(self):
        kw = dict(init=True, marginals=self.marg)
        if self.grad:
            kw['gradient'] = (self.g_ee, self.g_ed)
        if self.post is not None:
            kw['posterior'] = self.post
        return kw

    def oracle(self, b):
        """(messages [n_msgs][X], marginals [n_vars][X], log-posterior, (g_ee, g_ed)) of graph b."""
        g, inputs = self.g, self.inputs[b]
        msgs = O.init_messages(g)
        saved = O.renormalize
        if not self.norm:
            O.renormalize = lambda m: m
        try:
            for r in self.roots:
                O.sweep(g, inputs, msgs, r)
        finally:
            O.renormalize = saved
        want = np.stack([msgs[k] for k in C.msg_keys(self.spec)])
        if not self.norm:
            return want, None, None, None
        marg = np.stack([O.marginal(g, msgs, v).reshape(-1) for v in self.topo.var_ids])
        lp = O.log_posterior(g, msgs)
        grad = O.unregularized_gradient(g, inputs, msgs) if self.grad else None
        return want, marg, lp, grad

    def check(self, sample=None):
        w = self.w
        B = self.B
        f32 = w.get('f32')
        rtol, mrtol = (1e-5, 5e-6) if f32 else (RTOL, RTOL)
        msgs = self.fb.msgs.cpu().numpy()
        marg = self.marg.cpu().numpy() if self.marg is not None else None
        lp_all = []
        for b in (sample if sample is not None else range(B)):
            want, wm, wlp, wg = self.oracle(b)
            np.testing.assert_allclose(msgs[b], want, rtol=rtol, atol=1e-300, err_msg='messages of graph %d' % b)
            if wm is not None:
                np.testing.assert_allclose(marg[b], wm, rtol=mrtol, atol=1e-300, err_msg='marginals of graph %d' % b)
            if self.post is not None:
                np.testing.assert_allclose(float(self.post[1][b]), wlp, rtol=RTOL, err_msg='log-posterior of graph %d' % b)
                lp_all.append(wlp)
            if wg is not None:
                np.testing.assert_allclose(self.g_ee[b].cpu().numpy(), wg[0].reshape(-1), rtol=GRAD_RTOL, atol=1e-11,
                                           err_msg='en_en gradient of graph %d' % b)
                np.testing.assert_allclose(self.g_ed[b].cpu().numpy(), wg[1].reshape(-1), rtol=GRAD_RTOL, atol=1e-11,
                                           err_msg='en_de gradient of graph %d' % b)
        if self.post is not None and sample is None:
            np.testing.assert_allclose(float(self.post[2].item()), sum(lp_all), rtol=RTOL, err_msg='batch sum of log-posteriors')


def _with_variant(variant, fn):
    from macaronicusermodeling_amd import _ffi
    _ffi.check(_ffi.lib.mlbp_set_sweep_variant(variant))
    try:
        return fn()
    finally:
        _ffi.check(_ffi.lib.mlbp_set_sweep_variant(1))


@functools.lru_cache(maxsize=None)
def run_workload(name):
    """Runs workload `name` once: (instances launched, exact-kernel redo counts, failure or None, every kernel launched)."""
    from macaronicusermodeling_amd import _ffi
    from macaronicusermodeling_amd import batch as batch_mod
    w = WORKLOADS[name]
    seed = 1000 + sorted(WORKLOADS).index(name)
    K.reset()
    try:
        if w['kind'] == 'groups':
            groups = [_Group(dict(g, kind='sweep'), seed + 100 * k) for k, g in enumerate(w['groups'])]
        else:
            groups = [_Group(w, seed)]
        variant = w.get('variant', 1)
        K.reset()
        if w['kind'] == 'gradient':
            gr = groups[0]
            _with_variant(variant, lambda: gr.fb.sweep(gr.roots, init=True, marginals=gr.marg))
            K.reset()
            gr.fb.gradient(gr.g_ee, gr.g_ed)
            launched, everything = K.launched(), K.all_launched()
            torch.cuda.synchronize()
            assert _ffi.lib.mlbp_gradient_status() == 0
        elif w['kind'] == 'groups':
            kws = [g.sweep_kwargs() for g in groups]
            progs = _with_variant(variant, lambda: batch_mod.sweep_groups(
                [g.fb for g in groups], [g.roots for g in groups], init=True, marginals=[k['marginals'] for k in kws],
                gradients=[k['gradient'] for k in kws] if groups[0].grad else None,
                posteriors=[k['posterior'] for k in kws] if groups[0].post is not None else None))
            launched, everything = K.launched(), K.all_launched()
            torch.cuda.synchronize()
            for p in progs:
                assert p.status() == 0
        else:
            gr = groups[0]
            prog = _with_variant(variant, lambda: gr.fb.sweep(gr.roots, **gr.sweep_kwargs()))
            launched, everything = K.launched(), K.all_launched()
            torch.cuda.synchronize()
            assert prog.status() == 0, _ffi.lib.mlbp_last_error()
        redo = []
        for g in groups:
            if g.w['kind'] == 'sweep' and g.X == 64:
                redo.append(g.fb.program(g.roots).exact_count(g.B))
        for g in groups:
            g.check(w.get('sample'))
        if w.get('full_check'):         # every graph against the per-graph kernels on the same inputs
            gr = groups[0]
            got = gr.fb.msgs.clone()
            _with_variant(3, lambda: gr.fb.sweep(gr.roots, init=True))
            np.testing.assert_allclose(got.cpu().numpy(), gr.fb.msgs.cpu().numpy(), rtol=1e-11, atol=1e-300)
        return frozenset(launched), tuple(redo), None, frozenset(everything)
    except Exception as e:         # (kept for every instance case of this workload)
        return frozenset(K.launched()), (), e, frozenset(K.all_launched())


# ---- the instance table ----------------------------------------------------------------------------------------------
# instance -> the workloads that reach it (tests/test_kernel_inventory.py: together with UNREACHABLE there, every instance of the
# built library)
COVERED = {
    ('contract_chunked_kernel', ('double', 10, 8)): ['gemm_x1100'],
    ('contract_chunked_kernel', ('double', 12, 16)): ['gemm_x2100', 'gemm_grad_x2100'],
    ('contract_chunked_kernel', ('double', 14, 8)): ['gemm_x1700', 'gemm_x2500'],
    ('contract_chunked_kernel', ('double', 16, 16)): ['gemm_x3000', 'gemm_x4096'],
    ('contract_kernel', ('double', 10, 1, 2, 8, True)): ['gemm_x600'],
    ('contract_kernel', ('double', 12, 1, 2, 16, True)): ['gemm_x700'],
    ('contract_kernel', ('double', 14, 1, 2, 8, True)): ['gemm_x850'],
    ('contract_kernel', ('double', 16, 1, 2, 16, True)): ['gemm_x1000'],
    ('contract_kernel', ('double', 2, 1, 2, 8, False)): ['gemm_x128', 'gemm_b1_x128', 'gemm_grad_x128'],
    ('contract_kernel', ('double', 2, 1, 2, 8, True)): ['gemm_x97'],
    ('contract_kernel', ('double', 2, 2, 4, 4, False)): ['gemm_big_x128'],
    ('contract_kernel', ('double', 4, 1, 2, 8, False)): ['gemm_x256'],
    ('contract_kernel', ('double', 4, 1, 2, 8, True)): ['gemm_x201'],
    ('contract_kernel', ('double', 4, 2, 4, 4, False)): ['gemm_big_x256'],
    ('contract_kernel', ('double', 6, 1, 2, 8, False)): ['gemm_x384', 'gemm_grad_x384'],
    ('contract_kernel', ('double', 6, 1, 2, 8, True)): ['gemm_x300'],
    ('contract_kernel', ('double', 8, 1, 2, 8, False)): ['gemm_x512'],
    ('contract_kernel', ('double', 8, 1, 2, 8, True)): ['gemm_x450'],
    ('contract_kernel', ('float', 4, 1, 4, 8, False)): ['gemm_f32_x256'],
    ('contract_kernel', ('float', 8, 1, 4, 8, False)): ['gemm_f32_x512'],
    ('gradient_kernel', (1, 1)): ['gradient_x128_f11'],
    ('gradient_kernel', (2, 2)): ['gradient_x128_f22'],
    ('gradient_kernel', (3, 6)): ['gradient_x128_f36', 'gradient_b1_x128'],
    ('gradient_x64_kernel', (1, 1)): ['gradient_x64_f11'],
    ('gradient_x64_kernel', (2, 2)): ['gradient_x64_f22'],
    ('gradient_x64_kernel', (3, 6)): ['gradient_x64_f36', 'gradient_b1_x64', 'fixup_shared_grad_user_k4'],
    ('shared_prepare_kernel', (False,)): ['shared_user_k3'],
    ('shared_prepare_kernel', (True,)): ['shared_groups_k3_k4_k5', 'shared_groups_grad_k3_k4_k5'],
    ('sweep_generic_kernel', (False, False)): ['generic_unnorm_x700'],
    ('sweep_generic_kernel', (False, True)): ['generic_unnorm_x4'],
    ('sweep_generic_kernel', (True, False)): ['generic_x1100'],
    ('sweep_generic_kernel', (True, True)): ['generic_x16', 'generic_b1_x16'],
    ('sweep_wide_kernel', (False, 1, 'double', 2, 0)): ['wide_unnorm_x128'],
    ('sweep_wide_kernel', (False, 1, 'float', 4, 0)): ['wide_f32_unnorm_x256'],
    ('sweep_wide_kernel', (False, 2, 'double', 2, 0)): ['wide_unnorm_x256'],
    ('sweep_wide_kernel', (False, 2, 'float', 4, 0)): ['wide_f32_unnorm_x512'],
    ('sweep_wide_kernel', (False, 4, 'double', 2, 0)): ['wide_unnorm_x512'],
    ('sweep_wide_kernel', (True, 1, 'double', 2, 0)): ['wide_x128', 'wide_b1_x128'],
    ('sweep_wide_kernel', (True, 1, 'double', 2, 1)): ['wide_pad_x100'],
    ('sweep_wide_kernel', (True, 1, 'double', 2, 2)): ['wide_pad_x97'],
    ('sweep_wide_kernel', (True, 1, 'float', 4, 0)): ['wide_f32_x256'],
    ('sweep_wide_kernel', (True, 2, 'double', 2, 0)): ['wide_x256'],
    ('sweep_wide_kernel', (True, 2, 'double', 2, 1)): ['wide_pad_x200'],
    ('sweep_wide_kernel', (True, 2, 'double', 2, 2)): ['wide_pad_x201'],
    ('sweep_wide_kernel', (True, 2, 'float', 4, 0)): ['wide_f32_x512'],
    ('sweep_wide_kernel', (True, 3, 'double', 2, 1)): ['wide_pad_x300'],
    ('sweep_wide_kernel', (True, 3, 'double', 2, 2)): ['wide_pad_x301'],
    ('sweep_wide_kernel', (True, 4, 'double', 2, 0)): ['wide_x512'],
    ('sweep_wide_kernel', (True, 4, 'double', 2, 1)): ['wide_pad_x450'],
    ('sweep_wide_kernel', (True, 4, 'double', 2, 2)): ['wide_pad_x451'],
    ('sweep_wide_kernel', (True, 6, 'double', 2, 1)): ['wide_pad_x700'],
    ('sweep_wide_kernel', (True, 6, 'double', 2, 2)): ['wide_pad_x701'],
    ('sweep_wide_kernel', (True, 8, 'double', 2, 1)): ['wide_pad_x800'],
    ('sweep_wide_kernel', (True, 8, 'double', 2, 2)): ['wide_pad_x801'],
    ('sweep_x64_fused_kernel', (False, 0, False)): ['exact_unnorm_ring5'],
    ('sweep_x64_fused_kernel', (False, 1, False)): ['exact_unnorm_chain2'],
    ('sweep_x64_fused_kernel', (False, 2, False)): ['exact_unnorm_chain3'],
    ('sweep_x64_fused_kernel', (False, 3, False)): ['exact_unnorm_ring3'],
    ('sweep_x64_fused_kernel', (True, 0, False)): ['exact_ring5', 'fixup_shared_grad_user_k4'],
    ('sweep_x64_fused_kernel', (True, 0, True)): ['exact_grad_user_k1'],
    ('sweep_x64_fused_kernel', (True, 1, False)): ['exact_chain2'],
    ('sweep_x64_fused_kernel', (True, 1, True)): ['exact_grad_user_k2'],
    ('sweep_x64_fused_kernel', (True, 2, False)): ['exact_chain3'],
    ('sweep_x64_fused_kernel', (True, 2, True)): ['exact_grad_user_p2'],
    ('sweep_x64_fused_kernel', (True, 3, False)): ['exact_ring3', 'exact_b1_ring3', 'fixup_lean_ring3'],
    ('sweep_x64_fused_kernel', (True, 3, True)): ['exact_grad_user_k3', 'fixup_lean_grad_user_k3'],
    ('sweep_x64_lean_kernel', (1, False, False, 0, False)): ['lean_chain2'],
    ('sweep_x64_lean_kernel', (1, False, False, 0, True)): ['lean_grad_user_k2'],
    ('sweep_x64_lean_kernel', (1, False, True, 0, False)): ['lean_groups_chain2'],
    ('sweep_x64_lean_kernel', (1, True, False, 0, False)): ['lean_small_chain2_x16'],
    ('sweep_x64_lean_kernel', (2, False, False, 0, False)): ['lean_chain3'],
    ('sweep_x64_lean_kernel', (2, False, False, 0, True)): ['lean_grad_user_p2'],
    ('sweep_x64_lean_kernel', (2, False, True, 0, False)): ['lean_groups_chain3'],
    ('sweep_x64_lean_kernel', (2, True, False, 0, False)): ['lean_small_chain3_x33'],
    ('sweep_x64_lean_kernel', (3, False, False, 0, False)): ['lean_ring3', 'lean_b1_ring3', 'fixup_lean_ring3'],
    ('sweep_x64_lean_kernel', (3, False, False, 0, True)): ['lean_grad_user_k3', 'fixup_lean_grad_user_k3'],
    ('sweep_x64_lean_kernel', (3, False, True, 0, False)): ['lean_groups_ring3'],
    ('sweep_x64_lean_kernel', (3, True, False, 0, False)): ['lean_small_ring3_x48'],
    ('sweep_x64_lean_kernel', (4, False, False, 0, False)): ['lean_ring4'],
    ('sweep_x64_lean_kernel', (4, False, True, 0, False)): ['lean_groups_ring4'],
    ('sweep_x64_lean_kernel', (4, True, False, 0, False)): ['lean_small_chain5_x17'],
    ('sweep_x64_lean_kernel', (6, False, False, 0, False)): ['lean_ring5'],
    ('sweep_x64_lean_kernel', (6, False, False, 1, False)): ['lean_ring7'],
    ('sweep_x64_lean_kernel', (6, False, True, 0, False)): ['lean_groups_ring5'],
    ('sweep_x64_lean_kernel', (6, False, True, 1, False)): ['lean_groups_ring7'],
    ('sweep_x64_lean_kernel', (8, False, False, 0, False)): ['lean_chain9'],
    ('sweep_x64_lean_kernel', (8, False, True, 0, False)): ['lean_groups_ring8'],
    ('sweep_x64_shared_kernel', (1, False, False, False, False, False, False)): ['shared_chain2_nou1'],
    ('sweep_x64_shared_kernel', (1, False, False, False, False, True, False)): ['shared_user_k2'],
    ('sweep_x64_shared_kernel', (1, False, False, False, True, False, False)): ['shared_grad_user_k2_nou1'],
    ('sweep_x64_shared_kernel', (1, False, False, False, True, True, False)): ['shared_grad_user_k2'],
    ('sweep_x64_shared_kernel', (1, False, False, True, False, False, False)): ['shared_groups_c2nou'],
    ('sweep_x64_shared_kernel', (1, False, False, True, False, True, False)): ['shared_groups_k2'],
    ('sweep_x64_shared_kernel', (1, False, False, True, True, False, False)): ['shared_groups_grad_uk2nou'],
    ('sweep_x64_shared_kernel', (1, False, False, True, True, True, False)): ['shared_groups_grad_k2'],
    ('sweep_x64_shared_kernel', (2, False, False, False, False, False, False)): ['shared_ring3_nou1'],
    ('sweep_x64_shared_kernel', (2, False, False, False, False, True, False)): ['shared_user_k3', 'shared_b1_user_k3'],
    ('sweep_x64_shared_kernel', (2, False, False, False, False, True, True)): ['shared_user_k4'],
    ('sweep_x64_shared_kernel', (2, False, False, False, True, False, False)): ['shared_grad_user_k3_nou4'],
    ('sweep_x64_shared_kernel', (2, False, False, False, True, True, False)): ['shared_grad_user_k3'],
    ('sweep_x64_shared_kernel', (2, False, False, False, True, True, True)): ['shared_grad_user_k4', 'fixup_shared_grad_user_k4'],
    ('sweep_x64_shared_kernel', (2, False, False, True, False, False, False)): ['shared_groups_r3nou'],
    ('sweep_x64_shared_kernel', (2, False, False, True, False, True, False)): ['shared_groups_k2_k3'],
    ('sweep_x64_shared_kernel', (2, False, False, True, False, True, True)): ['shared_groups_k2_k4'],
    ('sweep_x64_shared_kernel', (2, False, False, True, True, False, False)): ['shared_groups_grad_uk3nou'],
    ('sweep_x64_shared_kernel', (2, False, False, True, True, True, False)): ['shared_groups_grad_k2_k3'],
    ('sweep_x64_shared_kernel', (2, False, False, True, True, True, True)): ['shared_groups_grad_k2_k4'],
    ('sweep_x64_shared_kernel', (2, False, True, False, False, False, False)): ['shared_parallel3_nou1'],
    ('sweep_x64_shared_kernel', (2, False, True, True, False, False, False)): ['shared_groups_par3nou'],
    ('sweep_x64_shared_kernel', (2, True, False, False, False, False, False)): ['shared_ring8'],
    ('sweep_x64_shared_kernel', (2, True, False, True, False, False, False)): ['shared_groups_ring8', 'shared_groups_c2nou_ring8'],
    ('sweep_x64_shared_kernel', (2, True, True, False, False, False, False)): ['shared_user_k5'],
    ('sweep_x64_shared_kernel', (2, True, True, False, True, False, False)): ['shared_grad_user_k5'],
    ('sweep_x64_shared_kernel', (2, True, True, True, False, False, False)): ['shared_groups_k5'],
    ('sweep_x64_shared_kernel', (2, True, True, True, True, False, False)): ['shared_groups_grad_k2_k5'],
    ('table_frag_kernel', ('double', 2)): ['gemm_x256'],
    ('table_frag_kernel', ('float', 4)): ['gemm_f32_x256', 'gemm_f32_x512'],
}
FAST = ('sweep_x64_shared_kernel', 'sweep_x64_lean_kernel')

# kernels that run only inside a sweep or gradient call (no entry of their own) -> workloads above that launch them: the
# workload's outputs are compared with the oracle as for COVERED (tests/test_kernel_inventory.py checks this list too)
COMPOUND = {
    ('check_shared_claim_kernel', ()): ['gemm_x128'],
    ('fill_uniform_kernel', ()): ['gemm_x128'],
    ('unary_update_kernel', ()): ['gemm_x128'],
    ('variable_update_kernel', ()): ['gemm_x128'],
    ('pair_gradient_combine_kernel', ()): ['gemm_grad_x128', 'gradient_shared_x128'],
    ('unary_writeback_kernel', ()): ['shared_user_k3'],
    ('pair_weight_fragments_kernel', ()): ['gradient_shared_x64'],
    ('gradient_shared_pairs_kernel', ()): ['gradient_shared_x64'],
    ('gradient_x64_groups_kernel', ()): ['shared_groups_grad_k2_k3'],
    ('sweep_x64_fixup_groups_kernel', ()): ['shared_groups_k2_k3'],
}


@pytest.mark.parametrize('instance', sorted(COVERED, key=repr), ids=lambda i: '%s%s' % (i[0], i[1]))
def test_instance_matches_oracle(instance):
    for name in COVERED[instance]:
        launched, redo, err, _ = run_workload(name)
        if err is not None:
            raise err
        assert instance in launched, '%s did not launch %s (launched: %s)' % (name, instance, sorted(launched, key=repr))
        w = WORKLOADS[name]
        if w.get('zero') is not None:          # the degenerate graph went to the exact kernel, and only it
            assert sum(redo) == 1, '%s: %s graphs redone by the exact kernel, want 1' % (name, redo)
        elif instance[0] in FAST:              # the fast kernel's own results were compared, not the exact kernel's
            assert not any(redo), '%s: %s graphs redone by the exact kernel' % (name, redo)


@pytest.mark.parametrize('kernel', sorted(COMPOUND), ids=lambda k: k[0])
def test_compound_kernel_matches_oracle(kernel):
    """A kernel without an entry of its own ran inside each of its workloads, whose outputs match the oracle."""
    for name in COMPOUND[kernel]:
        _, _, err, everything = run_workload(name)
        if err is not None:
            raise err
        assert kernel in everything, '%s did not launch %s (launched: %s)' % (name, kernel, sorted(everything, key=repr))
