#!/usr/bin/env python3
"""Times exact inference by cutset conditioning next to the sum-product sweep call and log_partition of the same inputs, by
HIP events, in one process, alternating.

  k3   the default bench workload (user-shaped K3, 8192 graphs, X = 64, unique tables U(0,1) + 0.01, roots 1, 4, 7):
         sweep          FactorGraphBatch.sweep(3 roots, init=True, marginals=..., keep_messages=False) -- the lean call
         log_partition  FactorGraphBatch.log_partition(labels=...) on the messages a kept sweep left
         exact          FactorGraphBatch.exact_inference(labels=..., marginals=...): one cutset variable, 64 configurations
       exact is also reported against the byte model "each table once" -- every pairwise table and unary row read once, the
       marginals, log_z and joint_logp written -- as a share of the 8 TB/s HBM rate.
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
import torch                 # noqa: E402
import cases as C            # noqa: E402
from macaronicusermodeling_amd.batch import FactorGraphBatch       # noqa: E402
from macaronicusermodeling_amd.topology import GraphTopology       # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def window(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def alternate(fns, launches, rounds):
    """{name: [ms per call, one figure per round]}: every round times each function once, in turn."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(window(fn, launches))
    return out


def model_bytes(topo, B, X):
    """Each table once: pairwise tables, unary rows and labels in; marginals, log_z and joint_logp out."""
    tables = B * (topo.P * X * X + topo.U * X) * 8
    return dict(tables=tables, total=tables + B * topo.n_vars * 4 + B * (topo.n_vars * X + 2) * 8)


def measure(spec, roots, B, launches, rounds, dev):
    from macaronicusermodeling_amd import cutset as K
    topo = GraphTopology.from_spec(spec)
    X = spec['X']
    gen = torch.Generator(device=dev).manual_seed(1236)
    fb = FactorGraphBatch(topo, X, B, device=dev)
    fb.set_pair_tables(torch.rand(B * topo.P, X, X, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    fb.set_unary_tables(torch.rand(B * topo.U, X, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    labels = torch.randint(0, X, (B, topo.n_vars), generator=torch.Generator().manual_seed(5)).to(torch.int32).to(dev)
    marg = torch.empty(B, topo.n_vars, X, dtype=torch.float64, device=dev)
    exact = torch.empty_like(marg)
    fb.sweep(roots, init=True)                                   # the messages the log_partition windows read
    fns = {'sweep': lambda: fb.sweep(roots, init=True, marginals=marg, keep_messages=False),
           'log_partition': lambda: fb.log_partition(labels=labels),
           'exact': lambda: fb.exact_inference(labels=labels, marginals=exact)}
    res = alternate(fns, launches, rounds)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    fb.sweep(roots, init=True, marginals=marg)
    bethe = fb.log_partition()
    log_z, _, _ = fb.exact_inference(labels=labels, marginals=exact)
    kernel = K.last_kernel()
    torch.cuda.synchronize()
    pl = K.plan(topo, None, X, dev)
    mb = model_bytes(topo, B, X)
    return dict(batch=B, n_vars=topo.n_vars, cutset=pl.n_cut, configurations=pl.n_configs, chunks=K.chunks(B, pl.n_configs), kernel=kernel,
                ms_per_call=res, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in res.items()},
                exact_over_sweep=med['exact'] / med['sweep'], exact_over_log_partition=med['exact'] / med['log_partition'],
                model_bytes=mb, hbm_fraction_of_8TBps=mb['total'] / (med['exact'] * 1e-3) / HBM_BYTES_PER_S,
                mean_abs_bethe_gap=float((bethe - log_z).abs().mean()), max_marginal_gap=float((marg - exact).abs().max()))


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
