#!/usr/bin/env python3
"""Times exact M-best decoding by cutset conditioning next to exact MAP decoding and the sum-product sweep of the same inputs,
by HIP events, in one process, alternating.

  k3   the default bench workload (user-shaped K3, 8192 graphs, X = 64, unique tables U(0,1) + 0.01, roots 1, 4, 7):
         sweep           FactorGraphBatch.sweep(3 roots, init=True, marginals=..., keep_messages=False) -- the lean call
         exact_map       FactorGraphBatch.exact_map(): one cutset variable, 64 configurations, one max pass, then the decode
         exact_mbest_1   FactorGraphBatch.exact_mbest(1): the same walk with every V_c kept, select, lists, merge
         exact_mbest_4   ... (4)
         exact_mbest_16  ... (16)
       Every exact_mbest call is also reported against the byte model "each table and unary row once in by the values pass and
       once more per selected configuration by the lists pass, M (4 n_vars + 8) + 4 bytes out" as a share of the 8 TB/s HBM rate.
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

MS = (1, 4, 16)


def model_bytes(topo, B, X, m, n_configs):
    """Each table and unary row once in by the values pass, once more per selected configuration by the lists pass; the rows,
    the scores and n_found out."""
    tables = B * (topo.P * X * X + topo.U * X) * 8
    return dict(tables=tables, total=tables * (1 + min(m, n_configs)) + B * (m * (4 * topo.n_vars + 8) + 4))


def measure(spec, roots, B, launches, rounds, dev):
    from macaronicusermodeling_amd import exactmbest as K
    topo = GraphTopology.from_spec(spec)
    X = spec['X']
    gen = torch.Generator(device=dev).manual_seed(1236)
    fb = FactorGraphBatch(topo, X, B, device=dev)
    fb.set_pair_tables(torch.rand(B * topo.P, X, X, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    fb.set_unary_tables(torch.rand(B * topo.U, X, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    marg = torch.empty(B, topo.n_vars, X, dtype=torch.float64, device=dev)
    fns = {'sweep': lambda: fb.sweep(roots, init=True, marginals=marg, keep_messages=False),
           'exact_map': lambda: fb.exact_map()}
    for m in MS:
        fns['exact_mbest_%d' % m] = lambda m=m: fb.exact_mbest(m)
    res = alternate(fns, launches, rounds)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    x, score = fb.exact_map()
    rows, scores, n_found = fb.exact_mbest(16)
    kernel = K.kernels(K.last_kernel())
    log_z = fb.exact_inference()[0]
    bp_x, _ = fb.map_sweep(roots, init=True, keep_messages=False)
    torch.cuda.synchronize()
    covered = (scores - log_z[:, None]).exp().cumsum(dim=1).mean(dim=0)
    bp_rank = (rows == bp_x[:, None, :]).all(dim=2)
    pl = K.plan(topo, None, X, dev)
    mb = {'exact_mbest_%d' % m: model_bytes(topo, B, X, m, pl.n_configs) for m in MS}
    return dict(batch=B, n_vars=topo.n_vars, cutset=pl.n_cut, configurations=pl.n_configs, chunks=K.chunks(B, pl.n_configs),
                values_kernel=kernel[0], lists_kernel=kernel[1],
                ms_per_call=res, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in res.items()},
                over_exact_map={k: med[k] / med['exact_map'] for k in mb}, over_sweep={k: med[k] / med['sweep'] for k in mb},
                model_bytes=mb, hbm_fraction_of_8TBps={k: mb[k]['total'] / (med[k] * 1e-3) / HBM_BYTES_PER_S for k in mb},
                first_row_is_exact_map=bool((rows[:, 0] == x).all() and (scores[:, 0] == score).all()),
                mean_mass_covered_by_rank=[float(v) for v in covered],
                map_sweep_set_in_top16=float(bp_rank.any(dim=1).double().mean()), map_sweep_set_is_first=float(bp_rank[:, 0].double().mean()))


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
