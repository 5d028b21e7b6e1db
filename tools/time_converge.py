#!/usr/bin/env python3
"""Times sweeps to convergence next to the sum-product and sampling calls of the same inputs, by HIP events, in one process,
alternating.

On the default bench workload (K3, 8192 graphs, X = 64, unique tables U(0,1) + 0.01, roots 1, 4, 7):
  sweep            FactorGraphBatch.sweep(3 roots, init=True, marginals=...)
  sample_S1        FactorGraphBatch.sample(3 roots, n_samples=1): n_vars = 3 steps of the same 3-sweep program in the layout
                   converge_x64_kernel shares -- sample_S1 / 3 is the yardstick for one round
  converge_r1      converge(3 roots, tol=0, max_rounds=1)
  converge_r8      converge(3 roots, tol=0, max_rounds=8): (converge_r8 - converge_r1) / 7 is the time of a round (/ (mean rounds
                   run - 1) should graphs reach an exact fixed point sooner; the rounds run are reported)
  converge_tol     converge(tol=1e-6, max_rounds=50), with the histogram of `rounds` and the count still above tol
Prints one JSON line.  Options: --batch B (8192), --launches L (20 per timed window), --rounds R (5 alternations),
--scale s (0: the bench tables; s > 0: tables exp(s * N(0,1)), the coupling of tests/test_converge_cpu.py)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--scale', type=float, default=0.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    from macaronicusermodeling_amd import converge as V
    spec, roots = C.user_spec(10, [1, 4, 7], 64, 64, seed=1), [1, 4, 7]
    topo = GraphTopology.from_spec(spec)
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1236)
    B = a.batch
    fb = FactorGraphBatch(topo, 64, B, device=dev)
    if a.scale > 0:
        fb.set_pair_tables(torch.exp(a.scale * torch.randn(B * topo.P, 64, 64, dtype=torch.float64, device=dev, generator=gen)))
        fb.set_unary_tables(torch.exp(a.scale * torch.randn(B * topo.U, 64, dtype=torch.float64, device=dev, generator=gen)))
    else:
        fb.set_pair_tables(torch.rand(B * topo.P, 64, 64, dtype=torch.float64, device=dev, generator=gen) + 0.01)
        fb.set_unary_tables(torch.rand(B * topo.U, 64, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    marg = torch.empty(B, topo.n_vars, 64, dtype=torch.float64, device=dev)
    uniforms = torch.rand((1, B, topo.n_vars), dtype=torch.float64, device=dev, generator=gen)
    fns = {'sweep': lambda: fb.sweep(roots, init=True, marginals=marg),
           'sample_S1': lambda: fb.sample(roots, n_samples=1, uniforms=uniforms),
           'converge_r1': lambda: fb.converge(roots, tol=0.0, max_rounds=1),
           'converge_r8': lambda: fb.converge(roots, tol=0.0, max_rounds=8),
           'converge_tol': lambda: fb.converge(tol=1e-6, max_rounds=50)}
    res = alternate(fns, a.launches, a.rounds)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    rounds, residual = fb.converge(tol=1e-6, max_rounds=50)
    r8, _ = fb.converge(roots, tol=0.0, max_rounds=8)
    torch.cuda.synchronize()
    rounds_h = rounds.cpu().numpy()
    hist = {str(int(r)): int((rounds_h == r).sum()) for r in sorted(set(rounds_h.tolist()))}
    # tol = 0 stops a graph that reaches an exact fixed point before round 8: the launch is throughput-bound at this batch size
    # (32 graphs per CU), so the difference is divided by the MEAN rounds run beyond the first; the rounds run are reported
    r8_h = r8.cpu().numpy()
    per_round = (med['converge_r8'] - med['converge_r1']) / max(float(r8_h.mean()) - 1.0, 1.0)
    out = dict(batch=B, scale=a.scale, launches_per_window=a.launches, kernel=V.last_kernel(), ms_per_call=res, median_ms=med,
               spread_ms=spread, ms_per_round=per_round, sample_S1_ms_per_step=med['sample_S1'] / topo.n_vars,
               round_over_sample_step=per_round / (med['sample_S1'] / topo.n_vars),
               rounds_run_at_tol0_max8=dict(min=int(r8_h.min()), max=int(r8_h.max()), mean=float(r8_h.mean())),
               rounds_histogram=hist, mean_rounds=float(rounds_h.mean()),
               not_converged=int((~(residual <= 1e-6)).sum().item()))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
