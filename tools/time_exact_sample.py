#!/usr/bin/env python3
"""Times exact posterior sampling by cutset conditioning next to the loopy sampler, exact inference and the sum-product sweep
of the same inputs, by HIP events, in one process, alternating.

  k3   the default bench workload (user-shaped K3, 8192 graphs, X = 64, unique tables U(0,1) + 0.01, roots 1, 4, 7), for
       S = 1, 8 and 32 samples per graph:
         sweep            FactorGraphBatch.sweep(3 roots, init=True, marginals=..., keep_messages=False) -- the lean call
         exact_inference  FactorGraphBatch.exact_inference(marginals=...): one cutset variable, 64 configurations, two passes
         sample_S         FactorGraphBatch.sample(3 roots, n_samples=S, uniforms=...): sequential conditioning on loopy sweeps
         exact_sample_S   FactorGraphBatch.exact_sample(n_samples=S, uniforms=...): the weights pass, the scan, the draw pass
       exact_sample_S is also reported against the byte model "each table and unary row twice in (once per pass), every Z_c
       written as a pair, read and scanned, the uniforms in, 4 n_vars + 8 bytes per sample out" as a share of the 8 TB/s HBM rate.
  k4   the same tables on the user-shaped K4 (two cutset variables, 4096 configurations) at --batch-k4 graphs (256).
Prints one JSON line.  Options: --batch B (8192), --batch-k4 B (256), --launches L (per timed window: 20), --rounds R (5
alternations), --samples S,S,... (1,8,32)."""
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


def model_bytes(topo, B, X, S, n_configs):
    """Each table and unary row once per pass; the Z_c pairs out, in, and the scanned weights out; uniforms in, samples and logp out."""
    tables = 2 * B * (topo.P * X * X + topo.U * X) * 8
    weights = B * n_configs * (2 + 2 + 1) * 8
    return dict(tables=tables, weights=weights, total=tables + weights + S * B * (topo.n_vars * 8 + 4 * topo.n_vars + 8))


def measure(spec, roots, B, samples, launches, rounds, dev):
    from macaronicusermodeling_amd import exactsample as K
    topo = GraphTopology.from_spec(spec)
    X = spec['X']
    gen = torch.Generator(device=dev).manual_seed(1236)
    fb = FactorGraphBatch(topo, X, B, device=dev)
    fb.set_pair_tables(torch.rand(B * topo.P, X, X, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    fb.set_unary_tables(torch.rand(B * topo.U, X, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    marg = torch.empty(B, topo.n_vars, X, dtype=torch.float64, device=dev)
    exact = torch.empty_like(marg)
    u = {S: torch.rand(S, B, topo.n_vars, dtype=torch.float64, device=dev, generator=gen) for S in samples}
    fns = {'sweep': lambda: fb.sweep(roots, init=True, marginals=marg, keep_messages=False),
           'exact_inference': lambda: fb.exact_inference(marginals=exact)}
    for S in samples:
        fns['sample_%d' % S] = lambda S=S: fb.sample(roots, n_samples=S, uniforms=u[S])
        fns['exact_sample_%d' % S] = lambda S=S: fb.exact_sample(n_samples=S, uniforms=u[S])
    res = alternate(fns, launches, rounds)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    S = samples[-1]
    x, logp, log_z = fb.exact_sample(n_samples=S, uniforms=u[S], log_z=True)
    kernel = K.last_kernel()
    joint = torch.stack([fb.exact_inference(labels=x[s])[2] for s in range(min(S, 2))])
    _, logq = fb.sample(roots, n_samples=S, uniforms=u[S])
    torch.cuda.synchronize()
    pl = K.plan(topo, None, X, dev)
    mb = {S: model_bytes(topo, B, X, S, pl.n_configs) for S in samples}
    return dict(batch=B, n_vars=topo.n_vars, cutset=pl.n_cut, configurations=pl.n_configs, kernel=kernel,
                weights_chunks=K.chunks(B, pl.n_configs),
                draw_chunks={S: K.chunks(B, -(-S // 4) if kernel == K.KERNEL_X64 else S) for S in samples},
                ms_per_call=res, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in res.items()},
                exact_sample_over_sample={S: med['exact_sample_%d' % S] / med['sample_%d' % S] for S in samples},
                exact_sample_over_exact_inference={S: med['exact_sample_%d' % S] / med['exact_inference'] for S in samples},
                exact_sample_over_sweep={S: med['exact_sample_%d' % S] / med['sweep'] for S in samples},
                model_bytes=mb,
                hbm_fraction_of_8TBps={S: mb[S]['total'] / (med['exact_sample_%d' % S] * 1e-3) / HBM_BYTES_PER_S for S in samples},
                max_abs_logp_minus_joint_logp=float((logp[:joint.shape[0]] - joint).abs().max()),
                mean_logp=float(logp.mean()), mean_logq_of_sample=float(logq.mean()), mean_log_z=float(log_z.mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--batch-k4', type=int, default=256)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--samples', default='1,8,32')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda:0')
    samples = [int(s) for s in a.samples.split(',')]
    out = dict(launches_per_window=a.launches,
               k3=measure(C.user_spec(10, [1, 4, 7], 64, 64, seed=1), [1, 4, 7], a.batch, samples, a.launches, a.rounds, dev),
               k4=measure(C.user_spec(10, [1, 4, 6, 8], 64, 64, seed=1), [1, 4, 6], a.batch_k4, samples, a.launches, a.rounds, dev))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
