#!/usr/bin/env python3
"""Times posterior sampling next to the sum-product and max-product calls of the same inputs, by HIP events, in one process,
alternating.

FactorGraphBatch.sample for S in {1, 8, 32} samples per graph, FactorGraphBatch.sweep(..., marginals=...) and
FactorGraphBatch.map_sweep on the default bench workload (K3, 8192 graphs, X = 64, unique tables, 3 sweeps,
keep_messages=False).  The uniforms are drawn once outside the timed windows: a sample() call is then one launch.  Prints
the times, sample / sweep per S, the compulsory-byte model of each sample call (every table and unary row once, uniforms
in, samples and log q out) and the share of the HBM rate that model achieves at S = 1 (--hbm-gbs: the rate to hold it
against, default the 8 TB/s of the data sheet).
Options: --batch B (8192), --launches L (50 per timed window), --rounds R (5 alternations), --samples 1,8,32."""
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


def model_bytes(topo, B, S, X=64):
    """Compulsory HBM bytes of one unique-table sample call: every table and unary row once (the chunk rule gives a graph one
    workgroup at this batch size), the index arrays, uniforms in, samples and log q out."""
    parts = dict(pair_tables=B * topo.P * X * X * 8, unary_rows=B * topo.U * X * 8, index_arrays=B * (topo.P + topo.U) * 4,
                 uniforms=S * B * topo.n_vars * 8, samples=S * B * topo.n_vars * 4, logq=S * B * 8)
    parts['total'] = sum(parts.values())
    return parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--samples', default='1,8,32')
    ap.add_argument('--hbm-gbs', type=float, default=8000.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    from macaronicusermodeling_amd import sample as S_
    spec, roots = C.user_spec(10, [1, 4, 7], 64, 64, seed=1), [1, 4, 7]
    topo = GraphTopology.from_spec(spec)
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1236)
    B = a.batch
    fb = FactorGraphBatch(topo, 64, B, device=dev)
    fb.set_pair_tables(torch.rand(B * topo.P, 64, 64, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    fb.set_unary_tables(torch.rand(B * topo.U, 64, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    marg = torch.empty(B, topo.n_vars, 64, dtype=torch.float64, device=dev)
    counts = [int(s) for s in a.samples.split(',')]
    uniforms = {s: torch.rand((s, B, topo.n_vars), dtype=torch.float64, device=dev, generator=gen) for s in counts}
    fns = {'sweep': lambda: fb.sweep(roots, init=True, marginals=marg, keep_messages=False),
           'map_sweep': lambda: fb.map_sweep(roots, init=True, keep_messages=False)}
    for s in counts:
        fns['sample_S%d' % s] = lambda s=s: fb.sample(roots, n_samples=s, uniforms=uniforms[s])
    res = alternate(fns, a.launches, a.rounds)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    out = dict(batch=B, launches_per_window=a.launches, ms_per_call=res, median_ms=med,
               sample_over_sweep={'S%d' % s: med['sample_S%d' % s] / med['sweep'] for s in counts},
               chunks={'S%d' % s: S_.chunks(B, s) for s in counts},
               model_bytes={'S%d' % s: model_bytes(topo, B, s) for s in counts})
    if 1 in counts:
        gbs = out['model_bytes']['S1']['total'] / (med['sample_S1'] * 1e-3) / 1e9
        out['S1_model_gbs'] = gbs
        out['S1_share_of_hbm_rate'] = gbs / a.hbm_gbs
        out['hbm_gbs_held_against'] = a.hbm_gbs
    print(json.dumps(out))


if __name__ == '__main__':
    main()
