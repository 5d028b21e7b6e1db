#!/usr/bin/env python3
"""Times search decoding beyond the exact limit (FactorGraphBatch.cutset_map and search_map) and records its quality, by HIP
events; every step runs in a child process of its own under its own time limit, and a step that fails ends the run.

  time_k5     user-shaped K5, 8192 graphs, X = 64, unique tables U(0,1) + 0.01: cutset_map(configs) at N = 64, 256 and 1024
              entries per graph -- the list made once by sweep() and cutset_draw(), outside the timed windows -- and beside it,
              alternating in the same process: cutset_estimate(configs, log_q) on the SAME list (the sum walk, with its pass back:
              the yardstick), map_sweep over three roots, and the whole search_map at N = 64, 256 and 1024.
  time_k8     the same at user-shaped K8, 1024 graphs (six cutset variables).
  quality_k3  the bench tables at K3 (8192 graphs), where exact_map() is the truth: the share of graphs on which search_map at
              N = 64, 256, 1024 returns exact_map()'s assignment, the mean and the worst shortfall in nats -- beside
              map_sweep's own share and shortfall.
  quality_k4  the same at K4 (256 graphs).
  quality_k5, quality_k8   beyond the truth (8192 and 1024 graphs): the share of graphs whose score rose above map_sweep's, the
              mean gain in nats, the share where entry 0 -- the max-product cutset state -- already wins.
Writes profiles/r29a_time_search_map_<step>.json and prints each.  Options: --steps a,b (all six), --launches L (per timed
window: 20), --rounds R (5 alternations), --limit S (seconds per step: 420), --out DIR (profiles)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

STEPS = ('time_k5', 'time_k8', 'quality_k3', 'quality_k4', 'quality_k5', 'quality_k8')
SIZES = (64, 256, 1024)
PREDICTED = {3: [1, 4, 7], 4: [1, 4, 6, 8], 5: [1, 3, 4, 6, 8], 8: [0, 1, 3, 4, 6, 7, 8, 9]}
BATCH = {3: 8192, 4: 256, 5: 8192, 8: 1024}
ROSE = 1e-9                     # a score counts as risen beyond this, relative to max(1, |score|): train.SEARCH_ROSE


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


def time_step(n, launches, rounds):
    import torch
    from time_cutset import alternate
    from macaronicusermodeling_amd import exactmap as K
    dev = torch.device('cuda:0')
    B = BATCH[n]
    fb, roots = _batch(n, B, dev)
    topo = fb.topo
    fb.sweep(roots, init=True)
    lists = {N: fb.cutset_draw(N, seed=7) for N in SIZES}
    marg = torch.empty(B, topo.n_vars, 64, dtype=torch.float64, device=dev)
    fns = {}
    for N, (c, q) in lists.items():
        fns['cutset_map_n%d' % N] = lambda c=c: fb.cutset_map(c)
        fns['cutset_estimate_n%d' % N] = lambda c=c, q=q: fb.cutset_estimate(configs=c, log_q=q, marginals=marg)
    fns['map_sweep'] = lambda: fb.map_sweep(roots, init=True, keep_messages=False)
    res = alternate(fns, launches, rounds)
    res.update(alternate({'search_map_n%d' % N: (lambda N=N: fb.search_map(roots, n_samples=N, seed=7)) for N in SIZES}, max(1, launches // 4), rounds))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    fb.cutset_map(lists[64][0])
    kernel = K.last_kernel()
    torch.cuda.synchronize()
    return dict(batch=B, n_vars=topo.n_vars, cutset=int(lists[64][0].shape[2]), kernel=kernel, chunks={N: K.chunks(B, N) for N in SIZES},
                launches_per_window=launches, ms_per_call=res, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in res.items()},
                ns_per_entry={N: med['cutset_map_n%d' % N] * 1e6 / (B * N) for N in SIZES},
                cutset_map_over_cutset_estimate={N: med['cutset_map_n%d' % N] / med['cutset_estimate_n%d' % N] for N in SIZES},
                search_map_over_map_sweep={N: med['search_map_n%d' % N] / med['map_sweep'] for N in SIZES})


def quality_step(n):
    import torch
    dev = torch.device('cuda:0')
    B = BATCH[n]
    fb, roots = _batch(n, B, dev)
    out = dict(batch=B, n_vars=fb.topo.n_vars, sizes={})
    truth = None
    if n <= 4:
        truth = fb.exact_map()
        bp_x, bp_score = fb.map_sweep(roots, init=True)
        short = (truth[1] - bp_score).clamp(min=0.0)
        out['map_sweep'] = dict(share_exact=float((bp_x == truth[0]).all(dim=1).double().mean()), mean_shortfall_nats=float(short.mean()),
                                worst_shortfall_nats=float(short.max()))
    for N in SIZES:
        configs, bp_x, bp_score = fb._search_list(roots, N, 11, None, None)
        x, score, entry = fb.cutset_map(configs, entry=True)
        gain = score - bp_score
        rose = gain > ROSE * score.abs().clamp(min=1.0)
        rec = dict(share_improved=float(rose.double().mean()), mean_gain_nats=float(gain.mean()), worst_loss_nats=float((-gain).max()),
                   share_entry0_wins=float((entry == 0).double().mean()), share_words_changed=float((x != bp_x).any(dim=1).double().mean()))
        if truth is not None:
            short = (truth[1] - score).clamp(min=0.0)
            rec.update(share_exact=float((x == truth[0]).all(dim=1).double().mean()), mean_shortfall_nats=float(short.mean()),
                       worst_shortfall_nats=float(short.max()), above_truth_nats=float((score - truth[1]).max()))
        out['sizes'][N] = rec
    torch.cuda.synchronize()
    return out


def run_step(name, launches, rounds):
    kind, n = name.split('_k')
    if kind == 'time' and int(n) in (5, 8):
        return time_step(int(n), launches, rounds)
    if kind == 'quality' and int(n) in BATCH:
        return quality_step(int(n))
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
        path = os.path.join(a.out, 'r29a_time_search_map_%s.json' % name)
        open(path, 'w').write(line + '\n')
        print(name, line, flush=True)


if __name__ == '__main__':
    main()
