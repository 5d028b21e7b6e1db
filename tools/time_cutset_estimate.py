#!/usr/bin/env python3
"""Times log Z by cutset importance sampling (FactorGraphBatch.cutset_estimate) and records its accuracy where the truth
exists, by HIP events; every step runs in a child process of its own under its own time limit, and a step that fails ends
the run.

  time_k5      user-shaped K5, 8192 graphs, X = 64, unique tables U(0,1) + 0.01: cutset_estimate(configs, log_q) at N = 64,
               256 and 1024 entries per graph -- the list drawn once by cutset_proposal, outside the timed windows -- and beside
               it, alternating in the same process: the lean sweep call on the bench's K3, exact_inference at K4 (256 graphs)
               and cutset_proposal alone at N = 64, so that sample()'s share of a whole estimate is known.
  time_k8      the same at user-shaped K8, 1024 graphs (six cutset variables).
  accuracy_k3  the bench tables at K3 (8192 graphs), the default proposal at N = 64, 256, 1024: mean and maximum of
               |log_z_hat - log_z| against exact_inference, the largest marginal gap, the median ess / N -- beside the Bethe
               gap and the BP marginal gap of the same graphs.
  accuracy_k4  the same at K4 (256 graphs).
  trace_k5, trace_k8   (not among the default steps) ten cutset_estimate(configs, log_q) calls at N = 256 on the K5 / K8 batch, for
               `rocprofv3 --kernel-trace --stats --output-format csv -- python3 tools/time_cutset_estimate.py --child trace_k5`, a
               run of its own: the rows of cutsetis_* are the call's split by kernel.
Writes profiles/r24a_time_cutset_estimate_<step>.json and prints each.  Options: --steps a,b (all four), --launches L (per timed
window: 20), --rounds R (5 alternations), --limit S (seconds per step: 420), --out DIR (profiles)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

STEPS = ('time_k5', 'time_k8', 'accuracy_k3', 'accuracy_k4')
SIZES = (64, 256, 1024)
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
    return fb, PREDICTED[n][:3]


def time_step(n, B, launches, rounds):
    import torch
    from time_cutset import alternate
    from macaronicusermodeling_amd import cutsetis as K
    dev = torch.device('cuda:0')
    fb, roots = _batch(n, B, dev)
    topo = fb.topo
    lists = {N: fb.cutset_proposal(roots, N, seed=7) for N in SIZES}
    marg = torch.empty(B, topo.n_vars, 64, dtype=torch.float64, device=dev)
    k3, roots3 = _batch(3, 8192, dev)
    marg3 = torch.empty(8192, 3, 64, dtype=torch.float64, device=dev)
    k4, _ = _batch(4, 256, dev)
    marg4 = torch.empty(256, 4, 64, dtype=torch.float64, device=dev)
    fns = {'estimate_n%d' % N: (lambda c=c, q=q: fb.cutset_estimate(configs=c, log_q=q, marginals=marg)) for N, (c, q) in lists.items()}
    fns['sweep_k3'] = lambda: k3.sweep(roots3, init=True, marginals=marg3, keep_messages=False)
    fns['exact_k4'] = lambda: k4.exact_inference(marginals=marg4)
    res = alternate(fns, launches, rounds)
    res.update(alternate({'proposal_n64': lambda: fb.cutset_proposal(roots, 64, seed=7)}, 2, rounds))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    _, _, ess = fb.cutset_estimate(configs=lists[64][0], log_q=lists[64][1], marginals=marg)
    kernel = K.last_kernel()
    torch.cuda.synchronize()
    pl = K.plan(topo, None, 64, dev)
    return dict(batch=B, n_vars=topo.n_vars, cutset=pl.n_cut, kernel=kernel, chunks={N: K.chunks(B, N) for N in SIZES},
                launches_per_window=launches, ms_per_call=res, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in res.items()},
                ns_per_entry={N: med['estimate_n%d' % N] * 1e6 / (B * N) for N in SIZES},
                proposal_share_n64=med['proposal_n64'] / (med['proposal_n64'] + med['estimate_n64']),
                median_ess_over_n_at_64=float(ess.median()) / 64)


def accuracy_step(n, B):
    import torch
    dev = torch.device('cuda:0')
    fb, roots = _batch(n, B, dev)
    log_z, exact = fb.exact_inference()
    bp = torch.empty_like(exact)
    fb.sweep(roots, init=True, marginals=bp)
    bethe = fb.log_partition()
    out = dict(batch=B, n_vars=fb.topo.n_vars, mean_abs_bethe_gap=float((bethe - log_z).abs().mean()), max_abs_bethe_gap=float((bethe - log_z).abs().max()),
               max_bp_marginal_gap=float((bp - exact).abs().max()), estimates={})
    for N in SIZES:
        log_z_hat, marg, ess = fb.cutset_estimate(roots, n_samples=N, seed=11)
        err = (log_z_hat - log_z).abs()
        out['estimates'][N] = dict(mean_abs_log_z_error=float(err.mean()), max_abs_log_z_error=float(err.max()),
                                   max_marginal_gap=float((marg - exact).abs().max()), mean_marginal_gap=float((marg - exact).abs().mean()),
                                   median_ess_over_n=float(ess.median()) / N, min_ess_over_n=float(ess.min()) / N)
    torch.cuda.synchronize()
    return out


def trace_step(n, B, N=256, calls=10):
    import torch
    dev = torch.device('cuda:0')
    fb, roots = _batch(n, B, dev)
    configs, log_q = fb.cutset_proposal(roots, N, seed=7)
    marg = torch.empty(B, fb.topo.n_vars, 64, dtype=torch.float64, device=dev)
    for _ in range(calls):
        fb.cutset_estimate(configs=configs, log_q=log_q, marginals=marg)
    torch.cuda.synchronize()
    return dict(batch=B, n_vars=fb.topo.n_vars, N=N, calls=calls)


def run_step(name, launches, rounds):
    if name == 'trace_k5':
        return trace_step(5, 8192)
    if name == 'trace_k8':
        return trace_step(8, 1024)
    if name == 'time_k5':
        return time_step(5, 8192, launches, rounds)
    if name == 'time_k8':
        return time_step(8, 1024, launches, rounds)
    if name == 'accuracy_k3':
        return accuracy_step(3, 8192)
    if name == 'accuracy_k4':
        return accuracy_step(4, 256)
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
        path = os.path.join(a.out, 'r24a_time_cutset_estimate_%s.json' % name)
        open(path, 'w').write(line + '\n')
        print(name, line, flush=True)


if __name__ == '__main__':
    main()
