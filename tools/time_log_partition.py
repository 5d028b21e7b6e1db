#!/usr/bin/env python3
"""Times the log-partition read-out next to the sum-product call of the same inputs, by HIP events, in one process,
alternating.

  (default)        FactorGraphBatch.log_partition() -- the read-out alone, messages resident in HBM, log_z and joint_logp of
                   given labels out -- and FactorGraphBatch.sweep(roots, marginals=...) on the default bench
                   workload (K3, 8192 graphs, X = 64, unique tables, 3 sweeps) and on the training layout (two shared tables).
                   Prints both times, log_partition / sweep, the bytes the read-out has to move by the model below and the
                   fraction of the 8 TB/s HBM rate they amount to over the measured time.
  --only-logz N    N read-out launches on one workload (--layout unique|shared) and nothing else: the process to put under
                   `rocprofv3 --kernel-trace --stats`.
Options: --batch B (8192), --launches L (200 per timed window), --rounds R (5 alternations)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import torch                                   # noqa: E402
from time_map_decode import alternate, batches          # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def model_bytes(topo, B, shared_tables=0, X=64):
    """Compulsory HBM bytes of one read-out call: every pairwise table once (unique tables: one per graph and factor;
    shared: `shared_tables` tables in all), the 2P + U in-slot messages and the U unary rows of every graph, the table-index
    rows and labels, log_z and joint_logp out."""
    parts = dict(pair_tables=(shared_tables if shared_tables else B * topo.P) * X * X * 8,
                 messages=B * (2 * topo.P + topo.U) * X * 8, unary_rows=B * topo.U * X * 8,
                 index_arrays=B * (topo.P + topo.U + topo.n_vars) * 4, outputs=B * 16)
    parts['total'] = sum(parts.values())
    return parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--only-logz', type=int, default=0)
    ap.add_argument('--layout', choices=('unique', 'shared'), default='unique')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    from macaronicusermodeling_amd import logz as L
    topo, roots, unique, layout = batches(a.batch)
    labels = torch.randint(0, 64, (a.batch, topo.n_vars), generator=torch.Generator().manual_seed(5)).to(torch.int32).to(unique.device)
    if a.only_logz:
        fb = unique if a.layout == 'unique' else layout
        fb.sweep(roots, init=True)
        for _ in range(a.only_logz):
            fb.log_partition(labels=labels)
        torch.cuda.synchronize()
        print(json.dumps(dict(launches=a.only_logz, batch=a.batch, layout=a.layout, kernel=L.last_kernel(),
                              model_bytes=model_bytes(topo, a.batch, 2 if a.layout == 'shared' else 0))))
        return
    marg = torch.empty(a.batch, topo.n_vars, 64, dtype=torch.float64, device=unique.device)
    out = {}
    for name, fb, shared in (('unique_tables', unique, 0), ('training_layout', layout, 2)):
        fb.sweep(roots, init=True)                               # the messages the read-out windows read

        def sweep(fb=fb):
            fb.sweep(roots, init=True, marginals=marg)           # (messages kept: every window leaves the same ones behind)
        res = alternate({'log_partition': lambda fb=fb: fb.log_partition(labels=labels), 'sweep': sweep}, a.launches, a.rounds)
        log_z, joint = fb.log_partition(labels=labels)
        kernel = L.last_kernel()
        torch.cuda.synchronize()
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        mb = model_bytes(topo, a.batch, shared)
        out[name] = dict(ms_per_call=res, median_ms=med, log_partition_over_sweep=med['log_partition'] / med['sweep'],
                         kernel=kernel, model_bytes=mb,
                         hbm_fraction_of_8TBps=mb['total'] / (med['log_partition'] * 1e-3) / HBM_BYTES_PER_S,
                         mean_log_z=float(log_z.mean()), mean_joint_logp=float(joint.mean()))
    out['batch'], out['launches_per_window'] = a.batch, a.launches
    print(json.dumps(out))


if __name__ == '__main__':
    main()
