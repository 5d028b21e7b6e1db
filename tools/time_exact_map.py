#!/usr/bin/env python3
"""Times exact MAP decoding by cutset conditioning next to the sum-product sweep, the max-product sweeps and exact inference of
the same inputs, by HIP events, in one process, alternating.

  k3   the default bench workload (user-shaped K3, 8192 graphs, X = 64, unique tables U(0,1) + 0.01, roots 1, 4, 7):
         sweep            FactorGraphBatch.sweep(3 roots, init=True, marginals=..., keep_messages=False) -- the lean call
         map_sweep        FactorGraphBatch.map_sweep(3 roots, init=True, keep_messages=False)
         exact_inference  FactorGraphBatch.exact_inference(marginals=...): one cutset variable, 64 configurations, two passes
         exact_map        FactorGraphBatch.exact_map(): the same configurations, one max pass, then the decode
         exact_map_mm     FactorGraphBatch.exact_map(max_marginals=...): both max passes
       Both exact_map calls are also reported against the byte model "each table and unary row once in, 4 n_vars + 8 bytes out
       (plus n_vars * 512 with max-marginals)" as a share of the 8 TB/s HBM rate.
  k4   the same tables on the user-shaped K4 (two cutset variables, 4096 configurations) at --batch-k4 graphs (256).
Prints one JSON line.  Options: --batch B (8192), --batch-k4 B (256), --launches L (per timed window: 20), --rounds R (5
alternations)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch                 # noqa: E402
import cases as C            # noqa: E402
from time_cutset import HBM_BYTES_PER_S, alternate                 # noqa: E402
from macaronicusermodeling_amd.batch import FactorGraphBatch       # noqa: E402
from macaronicusermodeling_amd.topology import GraphTopology       # noqa: E402


def model_bytes(topo, B, X, max_marginals):
    """Each table and unary row once in; the assignment and the score out, plus the max-marginals."""
    tables = B * (topo.P * X * X + topo.U * X) * 8
    return dict(tables=tables, total=tables + B * (4 * topo.n_vars + 8) + (B * topo.n_vars * X * 8 if max_marginals else 0))


def measure(spec, roots, B, launches, rounds, dev):
    from macaronicusermodeling_amd import exactmap as K
    topo = GraphTopology.from_spec(spec)
    X = spec['X']
    gen = torch.Generator(device=dev).manual_seed(1236)
    fb = FactorGraphBatch(topo, X, B, device=dev)
    fb.set_pair_tables(torch.rand(B * topo.P, X, X, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    fb.set_unary_tables(torch.rand(B * topo.U, X, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    marg = torch.empty(B, topo.n_vars, X, dtype=torch.float64, device=dev)
    exact = torch.empty_like(marg)
    mm = torch.empty_like(marg)
    fns = {'sweep': lambda: fb.sweep(roots, init=True, marginals=marg, keep_messages=False),
           'map_sweep': lambda: fb.map_sweep(roots, init=True, keep_messages=False),
           'exact_inference': lambda: fb.exact_inference(marginals=exact),
           'exact_map': lambda: fb.exact_map(),
           'exact_map_mm': lambda: fb.exact_map(max_marginals=mm)}
    res = alternate(fns, launches, rounds)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    bp_x, bp_score = fb.map_sweep(roots, init=True, keep_messages=False)
    x, score = fb.exact_map()
    kernel = K.last_kernel()
    torch.cuda.synchronize()
    agrees = (bp_x == x).all(dim=1)
    pl = K.plan(topo, None, X, dev)
    mb = {k: model_bytes(topo, B, X, k == 'exact_map_mm') for k in ('exact_map', 'exact_map_mm')}
    return dict(batch=B, n_vars=topo.n_vars, cutset=pl.n_cut, configurations=pl.n_configs, chunks=K.chunks(B, pl.n_configs), kernel=kernel,
                ms_per_call=res, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in res.items()},
                exact_map_over_exact_inference=med['exact_map'] / med['exact_inference'],
                exact_map_mm_over_exact_inference=med['exact_map_mm'] / med['exact_inference'],
                exact_map_over_map_sweep=med['exact_map'] / med['map_sweep'],
                model_bytes=mb, hbm_fraction_of_8TBps={k: mb[k]['total'] / (med[k] * 1e-3) / HBM_BYTES_PER_S for k in mb},
                map_sweep_agrees=float(agrees.double().mean()), mean_shortfall_nats=float((score - bp_score).clamp(min=0.0).mean()),
                max_shortfall_nats=float((score - bp_score).max()))


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
