#!/usr/bin/env python3
"""Times the cutset proposal drawn from held messages (FactorGraphBatch.cutset_draw) beside the estimate it feeds and the
re-sweeping proposal it replaces, and records what the cheaper proposal costs in effective sample size, by HIP events; every
step runs in a child process of its own under its own time limit, and a step that fails ends the run.

  time_k5      user-shaped K5, 8192 graphs, X = 64, unique tables U(0,1) + 0.01 (the bench tables): cutset_draw at N = 64, 256
               and 1024 entries per graph from the messages of one sweep call -- the uniforms made once, outside the timed
               windows -- and beside it, alternating in the same process: cutset_estimate(configs, log_q) on the drawn list at
               each N, and cutset_proposal() alone at N = 64.  Records the ratios draw / estimate at N = 256 and
               cutset_proposal / draw at N = 64, and the median ess / N of the drawn lists.
  time_k8      the same at user-shaped K8, 1024 graphs (six cutset variables).
  accuracy_k3  the bench tables at K3 (8192 graphs): for each proposal ('sample', 'messages') at N = 64, 256, 1024 the mean
               and maximum of |log_z_hat - log_z| against exact_inference and the median ess / N.
  accuracy_k4  the same at K4 (256 graphs).
  ess_k5, ess_k8   where no truth exists: the median ess / N of each proposal at N = 64 (both) and 256, 1024 ('messages').
Writes profiles/r25a_time_cutset_draw_<step>.json and prints each.  Options: --steps a,b (all six), --launches L (per timed
window: 20), --rounds R (5 alternations), --limit S (seconds per step: 420), --out DIR (profiles)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

STEPS = ('time_k5', 'time_k8', 'accuracy_k3', 'accuracy_k4', 'ess_k5', 'ess_k8')
SIZES = (64, 256, 1024)


def time_step(n, B, launches, rounds):
    import torch
    from time_cutset import alternate
    from time_cutset_estimate import _batch
    from macaronicusermodeling_amd import cutdraw as K
    dev = torch.device('cuda:0')
    fb, roots = _batch(n, B, dev)
    topo = fb.topo
    pl = K.plan(topo, None, 64, dev)
    fb.sweep(roots, init=True)                                  # the messages every draw reads
    gen = torch.Generator(device=dev).manual_seed(7)
    uniforms = {N: torch.rand((B, N, pl.n_cut), dtype=torch.float64, device=dev, generator=gen) for N in SIZES}
    lists = {N: fb.cutset_draw(N, uniforms=uniforms[N]) for N in SIZES}
    kernel = K.last_kernel()
    marg = torch.empty(B, topo.n_vars, 64, dtype=torch.float64, device=dev)
    fns = {}
    for N in SIZES:
        fns['draw_n%d' % N] = lambda N=N: fb.cutset_draw(N, uniforms=uniforms[N])
        fns['estimate_n%d' % N] = lambda c=lists[N][0], q=lists[N][1]: fb.cutset_estimate(configs=c, log_q=q, marginals=marg)
    res = alternate(fns, launches, rounds)
    res.update(alternate({'proposal_n64': lambda: fb.cutset_proposal(roots, 64, seed=7)}, 2, rounds))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    ess = {N: float(fb.cutset_estimate(configs=lists[N][0], log_q=lists[N][1], marginals=marg)[2].median()) / N for N in SIZES}
    torch.cuda.synchronize()
    return dict(batch=B, n_vars=topo.n_vars, cutset=pl.n_cut, kernel=kernel, chunks={N: K.chunks(B, N) for N in SIZES},
                launches_per_window=launches, ms_per_call=res, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in res.items()},
                ns_per_entry={N: med['draw_n%d' % N] * 1e6 / (B * N) for N in SIZES},
                draw_over_estimate={N: med['draw_n%d' % N] / med['estimate_n%d' % N] for N in SIZES},
                proposal_over_draw_n64=med['proposal_n64'] / med['draw_n64'],
                draw_share_n64=med['draw_n64'] / (med['draw_n64'] + med['estimate_n64']),
                median_ess_over_n=ess)


def _both(fb, roots, sizes_sample, log_z=None):
    """Per proposal and N: the median ess / N and, where log_z is given, the error of log_z_hat."""
    out = {}
    for proposal, sizes in (('sample', sizes_sample), ('messages', SIZES)):
        out[proposal] = {}
        for N in sizes:
            log_z_hat, _, ess = fb.cutset_estimate(roots, n_samples=N, seed=11, proposal=proposal)
            row = dict(median_ess_over_n=float(ess.median()) / N, min_ess_over_n=float(ess.min()) / N)
            if log_z is not None:
                err = (log_z_hat - log_z).abs()
                row.update(mean_abs_log_z_error=float(err.mean()), max_abs_log_z_error=float(err.max()))
            out[proposal][N] = row
    return out


def accuracy_step(n, B):
    import torch
    from time_cutset_estimate import _batch
    fb, roots = _batch(n, B, torch.device('cuda:0'))
    log_z, _ = fb.exact_inference()
    out = dict(batch=B, n_vars=fb.topo.n_vars, proposals=_both(fb, roots, SIZES, log_z))
    torch.cuda.synchronize()
    return out


def ess_step(n, B):
    import torch
    from time_cutset_estimate import _batch
    fb, roots = _batch(n, B, torch.device('cuda:0'))
    out = dict(batch=B, n_vars=fb.topo.n_vars, proposals=_both(fb, roots, SIZES[:1]))
    torch.cuda.synchronize()
    return out


def run_step(name, launches, rounds):
    if name == 'time_k5':
        return time_step(5, 8192, launches, rounds)
    if name == 'time_k8':
        return time_step(8, 1024, launches, rounds)
    if name == 'accuracy_k3':
        return accuracy_step(3, 8192)
    if name == 'accuracy_k4':
        return accuracy_step(4, 256)
    if name == 'ess_k5':
        return ess_step(5, 8192)
    if name == 'ess_k8':
        return ess_step(8, 1024)
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
        path = os.path.join(a.out, 'r25a_time_cutset_draw_%s.json' % name)
        open(path, 'w').write(line + '\n')
        print(name, line, flush=True)


if __name__ == '__main__':
    main()
