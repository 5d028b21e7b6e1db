#!/usr/bin/env python3
"""Times max-product sweeps to convergence (FactorGraphBatch.map_converge) next to map_sweep, converge and the lean sweep call of
the same inputs, and records what settling buys, by HIP events; every step runs in a child process of its own under its own
time limit, and a step that fails ends the run.

  time_k3      user-shaped K3, 8192 graphs, X = 64, unique tables U(0,1) + 0.01, roots 1, 4, 7; alternating in one process:
                 sweep              FactorGraphBatch.sweep(3 roots, init=True, marginals=...): the lean sweep call
                 map_sweep          map_sweep(3 roots)
                 converge_tol       converge(tol=1e-6, max_rounds=50)
                 map_converge_r1    map_converge(3 roots, tol=0, max_rounds=1): map_sweep's work in the converge kernel
                 map_converge_r8    map_converge(3 roots, tol=0, max_rounds=8): (r8 - r1) / (mean rounds run - 1) is a round
                 map_converge_tol   map_converge(tol=1e-6, max_rounds=50), with the histogram of `rounds` and the count of
                                    graphs still moving at max_rounds
  time_k3s2    the same with tables exp(2 N(0,1))
  time_k4, time_k5, time_k8   the same at K4 (256 graphs), K5 (8192) and K8 (1024)
  quality_k3, quality_k4      the bench tables where exact_map() is the truth: the share of graphs on which map_sweep and
               map_converge return exact_map()'s assignment, the mean and the worst shortfall in nats, and the same over the
               graphs that settled and over those that did not
  quality_k5, quality_k8      beyond the truth: search_map(entry0='settled') against search_map() at N = 64 and 256 on the same
               draws -- the share of graphs where it scores above, below, and the mean difference in nats
  sum_k3, sum_k4   the sum mode, parent against change (needs --parent-lib, a libmlbp_converge.so built from the commit before the
               max-product mode, bound under the args struct it had): converge(tol=1e-6) through both libraries on the same
               tensors, alternating, and the parent's run-to-run spread
Writes profiles/r38a_time_map_converge_<step>.json and prints each.  Options: --steps a,b, --launches L (per timed window: 20),
--rounds R (5 alternations), --limit S (seconds per step: 420), --out DIR (profiles), --parent-lib PATH."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

STEPS = ('time_k3', 'time_k3s2', 'time_k4', 'time_k5', 'time_k8', 'quality_k3', 'quality_k4', 'quality_k5', 'quality_k8')
PREDICTED = {3: [1, 4, 7], 4: [1, 4, 6, 8], 5: [1, 3, 4, 6, 8], 8: [0, 1, 3, 4, 6, 7, 8, 9]}
BATCH = {3: 8192, 4: 256, 5: 8192, 8: 1024}
ROSE = 1e-9                     # a score counts as risen beyond this, relative to max(1, |score|): train.SEARCH_ROSE
TOL, MAX_ROUNDS = 1e-6, 50


def _batch(n, B, dev, scale=0.0):
    import torch
    import cases as C
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    spec = C.user_spec(10, PREDICTED[n], 64, 64, seed=1)
    topo = GraphTopology.from_spec(spec)
    gen = torch.Generator(device=dev).manual_seed(1236)
    fb = FactorGraphBatch(topo, 64, B, device=dev)
    if scale > 0:
        fb.set_pair_tables(torch.exp(scale * torch.randn(B * topo.P, 64, 64, dtype=torch.float64, device=dev, generator=gen)))
        fb.set_unary_tables(torch.exp(scale * torch.randn(B * topo.U, 64, dtype=torch.float64, device=dev, generator=gen)))
    else:
        fb.set_pair_tables(torch.rand(B * topo.P, 64, 64, dtype=torch.float64, device=dev, generator=gen) + 0.01)
        fb.set_unary_tables(torch.rand(B * topo.U, 64, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    return fb, PREDICTED[n][:3]


def _median(v):
    return sorted(v)[len(v) // 2]


def _histogram(rounds):
    h = rounds.cpu().numpy()
    return {str(int(r)): int((h == r).sum()) for r in sorted(set(h.tolist()))}


def time_step(n, scale, launches, rounds):
    import torch
    from time_converge import alternate
    from macaronicusermodeling_amd import converge as V
    dev = torch.device('cuda:0')
    B = BATCH[n]
    fb, roots = _batch(n, B, dev, scale)
    marg = torch.empty(B, fb.topo.n_vars, 64, dtype=torch.float64, device=dev)
    fns = {'sweep': lambda: fb.sweep(roots, init=True, marginals=marg),
           'map_sweep': lambda: fb.map_sweep(roots, init=True),
           'converge_tol': lambda: fb.converge(tol=TOL, max_rounds=MAX_ROUNDS),
           'map_converge_r1': lambda: fb.map_converge(roots, tol=0.0, max_rounds=1),
           'map_converge_r8': lambda: fb.map_converge(roots, tol=0.0, max_rounds=8),
           'map_converge_tol': lambda: fb.map_converge(tol=TOL, max_rounds=MAX_ROUNDS)}
    res = alternate(fns, launches, rounds)
    med = {k: _median(v) for k, v in res.items()}
    _, _, rounds_t, residual = fb.map_converge(tol=TOL, max_rounds=MAX_ROUNDS)
    kernel = V.last_kernel()
    r8 = fb.map_converge(roots, tol=0.0, max_rounds=8)[2].double()
    sum_rounds, sum_residual = fb.converge(tol=TOL, max_rounds=MAX_ROUNDS)
    torch.cuda.synchronize()
    return dict(batch=B, n_vars=fb.topo.n_vars, n_msgs=fb.topo.n_msgs, scale=scale, kernel=kernel, launches_per_window=launches,
                ms_per_call=res, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in res.items()},
                ms_per_round=(med['map_converge_r8'] - med['map_converge_r1']) / max(float(r8.mean()) - 1.0, 1.0),
                rounds_run_at_tol0_max8=dict(min=int(r8.min()), max=int(r8.max()), mean=float(r8.mean())),
                rounds_histogram=_histogram(rounds_t), mean_rounds=float(rounds_t.double().mean()),
                still_moving=int((~(residual <= TOL)).sum()),
                converge_rounds_histogram=_histogram(sum_rounds), converge_still_moving=int((~(sum_residual <= TOL)).sum()))


def _against(truth, x, score, rows=None):
    import torch
    if rows is not None:
        if int(rows.sum()) == 0:
            return dict(graphs=0)
        truth, x, score = (truth[0][rows], truth[1][rows]), x[rows], score[rows]
    same = (x == truth[0]).all(dim=1)
    short = torch.where(same, torch.zeros_like(score), (truth[1] - score).clamp(min=0.0))
    return dict(graphs=int(same.numel()), share_exact=float(same.double().mean()), mean_shortfall_nats=float(short.mean()),
                worst_shortfall_nats=float(short.max()))


def quality_step(n):
    import torch
    dev = torch.device('cuda:0')
    B = BATCH[n]
    fb, roots = _batch(n, B, dev)
    out = dict(batch=B, n_vars=fb.topo.n_vars, tol=TOL, max_rounds=MAX_ROUNDS)
    if n <= 4:
        truth = fb.exact_map()
        bp_x, bp_score = fb.map_sweep(roots, init=True)
        x, score, rounds, residual = fb.map_converge(roots, tol=TOL, max_rounds=MAX_ROUNDS)
        settled = residual <= TOL
        gain = score - bp_score
        bar = ROSE * score.abs().clamp(min=1.0)
        out.update(map_sweep=_against(truth, bp_x, bp_score), map_converge=_against(truth, x, score),
                   map_converge_settled=_against(truth, x, score, settled), map_converge_still_moving=_against(truth, x, score, ~settled),
                   map_sweep_on_the_settled=_against(truth, bp_x, bp_score, settled),
                   rounds_histogram=_histogram(rounds), still_moving=int((~settled).sum()),
                   share_rose=float((gain > bar).double().mean()), share_fell=float((gain < -bar).double().mean()),
                   share_words_changed=float((x != bp_x).any(dim=1).double().mean()))
    else:
        out['sizes'] = {}
        for N in (64, 256):
            _, plain, _ = fb.search_map(roots, n_samples=N, seed=11)
            _, score, score_settled, score_bp = fb.search_map(roots, n_samples=N, seed=11, entry0='settled', tol=TOL, max_rounds=MAX_ROUNDS)
            diff = score - plain
            bar = ROSE * score.abs().clamp(min=1.0)
            out['sizes'][N] = dict(share_above=float((diff > bar).double().mean()), share_below=float((diff < -bar).double().mean()),
                                   mean_difference_nats=float(diff.mean()), worst_loss_nats=float((-diff).max()),
                                   share_entry0_settled_above_sweeps=float((score_settled - score_bp > bar).double().mean()),
                                   share_entry0_settled_below_sweeps=float((score_settled - score_bp < -bar).double().mean()))
        residual = fb.map_converge(roots, tol=TOL, max_rounds=MAX_ROUNDS)[3]
        out['still_moving'] = int((~(residual <= TOL)).sum())
    torch.cuda.synchronize()
    return out


def sum_step(n, launches, rounds, parent_lib):
    """converge(tol=1e-6) through the parent's library and through this one, on the same tensors, alternating."""
    import torch
    import make_converge_bits as G
    from time_converge import alternate
    dev = torch.device('cuda:0')
    B = BATCH[n]
    fb, _ = _batch(n, B, dev)
    bound = G.bind_old(os.path.abspath(parent_lib))

    def parent():
        with G.old_library(bound):
            return fb.converge(tol=TOL, max_rounds=MAX_ROUNDS)

    def change():
        return fb.converge(tol=TOL, max_rounds=MAX_ROUNDS)
    want = [t.clone() for t in parent()] + [fb.msgs.clone()]
    got = [t.clone() for t in change()] + [fb.msgs.clone()]
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(want, got))
    res = alternate({'parent': parent, 'change': change}, launches, rounds)
    med = {k: _median(v) for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    bound_ms = med['parent'] + spread['parent'] + 0.015 * med['parent']
    return dict(batch=B, n_vars=fb.topo.n_vars, launches_per_window=launches, ms_per_call=res, median_ms=med, spread_ms=spread,
                change_over_parent=med['change'] / med['parent'], bound_ms=bound_ms, within_bound=bool(med['change'] <= bound_ms),
                same_bits=bool(same))


def run_step(name, launches, rounds, parent_lib):
    kind, n = name.split('_k')
    scale = 0.0
    if n.endswith('s2'):
        n, scale = n[:-2], 2.0
    if int(n) not in BATCH:
        raise SystemExit('unknown step %r' % name)
    if kind == 'time':
        return time_step(int(n), scale, launches, rounds)
    if kind == 'quality':
        return quality_step(int(n))
    if kind == 'sum' and parent_lib:
        return sum_step(int(n), launches, rounds, parent_lib)
    raise SystemExit('unknown step %r (sum_* needs --parent-lib)' % name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', default=','.join(STEPS))
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--limit', type=int, default=420)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--child', default=None, help='run this one step in this process and print its JSON line')
    a = ap.parse_args()
    if a.child:
        import torch
        assert torch.cuda.is_available(), 'needs an MI355X'
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
        print(json.dumps(run_step(a.child, a.launches, a.rounds, a.parent_lib)))
        return
    os.makedirs(a.out, exist_ok=True)
    for name in a.steps.split(','):
        cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', name, '--launches', str(a.launches),
               '--rounds', str(a.rounds)] + (['--parent-lib', a.parent_lib] if a.parent_lib else [])
        done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if done.returncode != 0:                                # a fault, an abort or the time limit: nothing more is started
            raise SystemExit('step %s ended with status %d' % (name, done.returncode))
        line = done.stdout.strip().splitlines()[-1]
        json.loads(line)
        path = os.path.join(a.out, 'r38a_time_map_converge_%s.json' % name)
        open(path, 'w').write(line + '\n')
        print(name, line, flush=True)


if __name__ == '__main__':
    main()
