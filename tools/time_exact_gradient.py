#!/usr/bin/env python3
"""Times the exact gradient and the exact pair marginals by cutset conditioning next to exact inference and the lean sweep with
its gradient epilogue on the same inputs, by HIP events, in one process, alternating; and measures how far the BP gradient is
from the true one on the bench tables.

  k3   the default bench workload (user-shaped K3, 8192 graphs, X = 64, unique tables U(0,1) + 0.01, roots 1, 4, 7), features
       U(-1, 1) with F_ee = 3, F_ed = 6, the spec's own selectors and observed columns:
         exact_gradient        FactorGraphBatch.exact_gradient(): gradients and log_z only
         exact_pair_marginals  FactorGraphBatch.exact_pair_marginals(out=...)
         exact_inference       FactorGraphBatch.exact_inference(labels=..., marginals=...)
         sweep_gradient        FactorGraphBatch.sweep(3 roots, init=True, marginals=..., gradient=..., keep_messages=False)
       the two new calls are also reported against the byte model "each table and phi once in, outputs once out" as a share of
       the 8 TB/s HBM rate, and against the bytes the call really moves (the partials it writes and reads back).
  k4   the same on the user-shaped K4 (two cutset variables, 4096 configurations) at --batch-k4 graphs (256).
gradient_gap: the BP gradient of the sweep call against the exact one -- cosine and |bp - exact| / |exact| of the sums over the
batch, and the mean of the per-graph relative norms.
Prints one JSON line.  Options: --batch B (8192), --batch-k4 B (256), --launches L (per timed window: 20), --rounds R (5
alternations)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import numpy as np           # noqa: E402
import torch                 # noqa: E402
import cases as C            # noqa: E402
from macaronicusermodeling_amd.batch import FactorGraphBatch       # noqa: E402
from macaronicusermodeling_amd.topology import GraphTopology       # noqa: E402
from time_cutset import HBM_BYTES_PER_S, alternate                 # noqa: E402

F_EE, F_ED = 3, 6


def measure(spec, roots, B, launches, rounds, dev):
    from macaronicusermodeling_amd import exactgrad as K
    topo = GraphTopology.from_spec(spec)
    X, Vde = spec['X'], spec['Vde']
    by_id = {f['id']: f for f in spec['factors']}
    gen = torch.Generator(device=dev).manual_seed(1236)
    fb = FactorGraphBatch(topo, X, B, device=dev)
    fb.set_pair_tables(torch.rand(B * topo.P, X, X, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    fb.set_unary_tables(torch.rand(B * topo.U, X, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    rs = np.random.RandomState(7)
    pair_phi = [0 if by_id[topo.factor_ids[j]]['gap'] > 1 else 1 for j in topo.pair_factors]
    unary = [by_id[topo.factor_ids[j]] for j in topo.unary_factors]
    kinds = [2 if f['factor_type'] == 'en_de' else (0 if f['gap'] > 1 else 1) for f in unary]
    fb.set_features(rs.uniform(-1, 1, (X, X, F_EE)), rs.uniform(-1, 1, (X, X, F_EE)), rs.uniform(-1, 1, (X, Vde, F_ED)), pair_phi, kinds)
    labels = rs.randint(0, X, size=(B, topo.n_vars))
    fb.set_observations(labels, np.tile(np.array([f['observed_dim'] for f in unary]), (B, 1)))
    marg = torch.empty(B, topo.n_vars, X, dtype=torch.float64, device=dev)
    exact = torch.empty_like(marg)
    pm = torch.empty(B, topo.P, X, X, dtype=torch.float64, device=dev)
    g_ee, g_ed = (torch.empty(B, F, dtype=torch.float64, device=dev) for F in (F_EE, F_ED))
    b_ee, b_ed = torch.empty_like(g_ee), torch.empty_like(g_ed)
    fns = {'exact_gradient': lambda: fb.exact_gradient(out_ee=g_ee, out_ed=g_ed),
           'exact_pair_marginals': lambda: fb.exact_pair_marginals(out=pm),
           'exact_inference': lambda: fb.exact_inference(labels=fb._labels, marginals=exact),
           'sweep_gradient': lambda: fb.sweep(roots, init=True, marginals=marg, gradient=(b_ee, b_ed), keep_messages=False)}
    res = alternate(fns, launches, rounds)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    kernel = K.last_kernel()
    pl = K.plan(topo, None, X, dev)
    chunks = K.chunks(B, pl.n_configs, kernel)
    workspace = K.workspace_bytes(B, X, topo.n_vars, topo.P, topo.U, pl.n_forest, pl.n_cut)
    torch.cuda.synchronize()
    # the byte model: each table and phi once in, outputs once out
    inputs = B * (topo.P * X * X + topo.U * X) * 8 + (2 * X * X * F_EE + X * Vde * F_ED) * 8 + B * (topo.n_vars + topo.U) * 4
    model = dict(exact_gradient=inputs + B * (F_EE + F_ED + 1) * 8, exact_pair_marginals=inputs + B * (topo.P * X * X + 1) * 8)
    # what the call really moves beyond that: every partial written once and read back once
    moved = {k: v + 2 * workspace for k, v in model.items()}
    exact_sum = torch.cat([g_ee.sum(0), g_ed.sum(0)]).cpu().numpy()
    bp_sum = torch.cat([b_ee.sum(0), b_ed.sum(0)]).cpu().numpy()
    per_e, per_b = torch.cat([g_ee, g_ed], dim=1), torch.cat([b_ee, b_ed], dim=1)
    gap = dict(cosine=float(exact_sum.dot(bp_sum) / np.linalg.norm(exact_sum) / np.linalg.norm(bp_sum)),
               relative_norm=float(np.linalg.norm(bp_sum - exact_sum) / np.linalg.norm(exact_sum)),
               mean_per_graph_relative_norm=float(((per_b - per_e).norm(dim=1) / per_e.norm(dim=1)).mean()),
               mean_per_graph_cosine=float(torch.nn.functional.cosine_similarity(per_b, per_e, dim=1).mean()))
    return dict(batch=B, n_vars=topo.n_vars, cutset=pl.n_cut, configurations=pl.n_configs, chunks=chunks, kernel=kernel,
                workspace_bytes=workspace, ms_per_call=res, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in res.items()},
                over_exact_inference={k: med[k] / med['exact_inference'] for k in ('exact_gradient', 'exact_pair_marginals')},
                over_sweep_gradient={k: med[k] / med['sweep_gradient'] for k in ('exact_gradient', 'exact_pair_marginals')},
                model_bytes=model, hbm_fraction_of_8TBps={k: model[k] / (med[k] * 1e-3) / HBM_BYTES_PER_S for k in model},
                moved_bytes=moved, moved_fraction_of_8TBps={k: moved[k] / (med[k] * 1e-3) / HBM_BYTES_PER_S for k in moved},
                gradient_gap=gap)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--batch-k4', type=int, default=256)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda:0')
    out = dict(launches_per_window=a.launches,
               k3=measure(C.user_spec(10, [1, 4, 7], 64, 64, seed=1), [1, 4, 7], a.batch, a.launches, a.rounds, dev),
               k4=measure(C.user_spec(10, [1, 4, 6, 8], 64, 64, seed=1), [1, 4, 6], a.batch_k4, a.launches, a.rounds, dev))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
