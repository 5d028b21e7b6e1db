#!/usr/bin/env python3
"""Times the draws beyond the exact limit (FactorGraphBatch.cutset_resample, the listed mode of libmlbp_exactsample.so) and
records their quality where the truth exists, by HIP events; every step runs in a child process of its own under its own time
limit, and a step that fails ends the run.

  time_k5     user-shaped K5, 8192 graphs, X = 64, unique tables U(0,1) + 0.01: cutset_resample(configs, log_q, n_samples=S) at
              N = 64, 256 and 1024 entries per graph and S = 1, 8 and 32 draws -- the list drawn once by cutset_draw() on the
              messages of one sweep, outside the timed windows -- and beside it, alternating in the same process:
              cutset_estimate(configs, log_q) on the same list, cutset_draw() at the same N, and sample() at the same S (windows
              of 2 launches: it sweeps again for every variable of every draw).
  time_k8     the same at user-shaped K8, 1024 graphs (six cutset variables).
  quality_k3  the bench tables at K3 (8192 graphs), where exact_inference() and exact_sample() give the truth: for the default
              proposal and proposal='messages' at N = 256 and S = 32, log_z - log_z_hat (the error of logp_hat, the same for every
              draw of a graph), the median ess / N, and the largest gap between the single-variable frequencies of the S B draws
              and the batch mean of the exact marginals -- beside the same figure for exact_sample() at equal S, which is
              Monte-Carlo noise alone.
  quality_k4  the same at K4 (256 graphs).
  trace_k5    (not among the default steps) ten cutset_resample calls at N = 256, S = 8 on the K5 batch, for `rocprofv3
              --kernel-trace --stats --output-format csv -- python3 tools/time_cutset_resample.py --child trace_k5`, a run of its own:
              the rows of exactsample_* are the call's split by kernel.
Writes profiles/r31a_time_cutset_resample_<step>.json and prints each.  Options: --steps a,b (all four), --launches L (per timed
window: 20), --rounds R (5 alternations), --limit S (seconds per step: 420), --out DIR (profiles)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

STEPS = ('time_k5', 'time_k8', 'quality_k3', 'quality_k4')
SIZES = (64, 256, 1024)
DRAWS = (1, 8, 32)
PREDICTED = {3: [1, 4, 7], 4: [1, 4, 6, 8], 5: [1, 3, 4, 6, 8], 8: [0, 1, 3, 4, 6, 7, 8, 9]}


def _batch(n, B, dev):
    import torch
    import cases as C
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    spec = C.user_spec(10, PREDICTED[n], 64, 64, seed=1)
    topo = GraphTopology.from_spec(spec)
    gen = torch.Generator(device=dev).manual_seed(1236)
    fb = FactorGraphBatch(topo, 64, B, device=dev)
    fb.set_pair_tables(torch.rand(B * topo.P, 64, 64, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    fb.set_unary_tables(torch.rand(B * topo.U, 64, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    fb.initialize()
    return fb, PREDICTED[n][:3]


def time_step(n, B, launches, rounds):
    import torch
    from time_cutset import alternate
    from macaronicusermodeling_amd import exactsample as K
    dev = torch.device('cuda:0')
    fb, roots = _batch(n, B, dev)
    topo = fb.topo
    fb.sweep(roots, init=True)                                  # the messages cutset_draw() reads
    lists = {N: fb.cutset_draw(N, seed=7) for N in SIZES}
    gen = torch.Generator(device=dev).manual_seed(99)
    u = {S: torch.rand(S, B, topo.n_vars, dtype=torch.float64, device=dev, generator=gen) for S in DRAWS}
    marg = torch.empty(B, topo.n_vars, 64, dtype=torch.float64, device=dev)
    fns = {}
    for N, (c, q) in lists.items():
        for S in DRAWS:
            fns['resample_n%d_s%d' % (N, S)] = lambda c=c, q=q, S=S: fb.cutset_resample(c, q, n_samples=S, uniforms=u[S])
        fns['estimate_n%d' % N] = lambda c=c, q=q: fb.cutset_estimate(configs=c, log_q=q, marginals=marg)
        fns['draw_n%d' % N] = lambda N=N: fb.cutset_draw(N, seed=7)
    res = alternate(fns, launches, rounds)
    res.update(alternate({'sample_s%d' % S: (lambda S=S: fb.sample(roots, n_samples=S, uniforms=u[S])) for S in DRAWS}, 2, rounds))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    c, q = lists[256]
    _, _, log_z_hat, ess = fb.cutset_resample(c, q, n_samples=8, uniforms=u[8], log_z=True, ess=True)
    kernel = K.last_kernel()
    ref_lz, _, ref_ess = fb.cutset_estimate(configs=c, log_q=q, marginals=marg)
    torch.cuda.synchronize()
    return dict(batch=B, n_vars=topo.n_vars, kernel=kernel, launches_per_window=launches, ms_per_call=res, median_ms=med,
                spread_ms={k: max(v) - min(v) for k, v in res.items()},
                weights_chunks={N: K.chunks(B, N) for N in SIZES}, draw_chunks={S: K.chunks(B, -(-S // 4) if kernel == K.KERNEL_X64 else S) for S in DRAWS},
                resample_over_estimate={'n%d_s%d' % (N, S): med['resample_n%d_s%d' % (N, S)] / med['estimate_n%d' % N] for N in SIZES for S in DRAWS},
                resample_over_draw={'n%d_s%d' % (N, S): med['resample_n%d_s%d' % (N, S)] / med['draw_n%d' % N] for N in SIZES for S in DRAWS},
                sample_over_list_and_resample={'n%d_s%d' % (N, S): med['sample_s%d' % S] / (med['draw_n%d' % N] + med['resample_n%d_s%d' % (N, S)])
                                               for N in SIZES for S in DRAWS},
                ns_per_entry={N: med['resample_n%d_s1' % N] * 1e6 / (B * N) for N in SIZES},
                max_abs_log_z_hat_minus_estimate=float((log_z_hat - ref_lz).abs().max()), max_rel_ess_minus_estimate=float(((ess - ref_ess) / ref_ess).abs().max()),
                median_ess_over_n_at_256=float(ess.median()) / 256)


def _frequency_gap(x, exact):
    """The largest |frequency of (variable, state) over the S B draws - batch mean of the exact marginal|."""
    import torch
    S, B, n = x.shape
    want = exact.mean(dim=0)
    worst = 0.0
    for v in range(n):
        freq = torch.bincount(x[:, :, v].reshape(-1).long(), minlength=64).double() / (S * B)
        worst = max(worst, float((freq - want[v]).abs().max()))
    return worst


def quality_step(n, B, N=256, S=32):
    import torch
    dev = torch.device('cuda:0')
    fb, roots = _batch(n, B, dev)
    log_z, exact = fb.exact_inference()
    x, _ = fb.exact_sample(n_samples=S, seed=12)
    out = dict(batch=B, n_vars=fb.topo.n_vars, N=N, S=S, exact_sample_frequency_gap=_frequency_gap(x, exact), proposals={})
    for proposal in ('sample', 'messages'):
        x, logp_hat, log_z_hat, ess = fb.estimate_sample(roots, n_samples=S, n_list=N, seed=11, proposal=proposal)
        err = log_z - log_z_hat
        out['proposals'][proposal] = dict(mean_log_z_minus_log_z_hat=float(err.mean()), mean_abs_log_z_error=float(err.abs().mean()),
                                          max_abs_log_z_error=float(err.abs().max()), median_ess_over_n=float(ess.median()) / N,
                                          min_ess_over_n=float(ess.min()) / N, frequency_gap=_frequency_gap(x, exact))
    torch.cuda.synchronize()
    return out


def trace_step(n, B, N=256, S=8, calls=10):
    import torch
    dev = torch.device('cuda:0')
    fb, roots = _batch(n, B, dev)
    fb.sweep(roots, init=True)
    configs, log_q = fb.cutset_draw(N, seed=7)
    u = torch.rand(S, B, fb.topo.n_vars, dtype=torch.float64, device=dev)
    for _ in range(calls):
        fb.cutset_resample(configs, log_q, n_samples=S, uniforms=u)
    torch.cuda.synchronize()
    return dict(batch=B, n_vars=fb.topo.n_vars, N=N, S=S, calls=calls)


def run_step(name, launches, rounds):
    if name == 'trace_k5':
        return trace_step(5, 8192)
    if name == 'time_k5':
        return time_step(5, 8192, launches, rounds)
    if name == 'time_k8':
        return time_step(8, 1024, launches, rounds)
    if name == 'quality_k3':
        return quality_step(3, 8192)
    if name == 'quality_k4':
        return quality_step(4, 256)
    raise SystemExit('unknown step %r' % name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', default=','.join(STEPS))
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--limit', type=int, default=420)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    ap.add_argument('--child', default=None, help='run this one step in this process and print its JSON line')
    a = ap.parse_args()
    if a.child:
        import torch
        assert torch.cuda.is_available(), 'needs an MI355X'
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
        print(json.dumps(run_step(a.child, a.launches, a.rounds)))
        return
    os.makedirs(a.out, exist_ok=True)
    for name in a.steps.split(','):
        cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', name, '--launches', str(a.launches),
               '--rounds', str(a.rounds)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if done.returncode != 0:                                # a fault, an abort or the time limit: nothing more is started
            raise SystemExit('step %s ended with status %d' % (name, done.returncode))
        line = done.stdout.strip().splitlines()[-1]
        json.loads(line)
        path = os.path.join(a.out, 'r31a_time_cutset_resample_%s.json' % name)
        open(path, 'w').write(line + '\n')
        print(name, line, flush=True)


if __name__ == '__main__':
    main()
