#!/usr/bin/env python3
"""Times M-best decoding beyond the exact limit (FactorGraphBatch.cutset_mbest and search_mbest), records its quality, and holds
the exact call against the library as it was, by HIP events; every step runs in a child process of its own under its own time
limit, and a step that fails ends the run.

  time_k5     user-shaped K5, 8192 graphs, X = 64, unique tables U(0,1) + 0.01: cutset_mbest(configs, m) at N = 64, 256 and
              1024 entries per graph and m = 1, 4, 16 -- the list made once by sweep() and cutset_draw(), outside the timed
              windows -- and beside it, alternating in the same process, cutset_map(configs) on the SAME list (the yardstick:
              the max walk and one re-solve); then the whole search_mbest at m = 4.
  time_k8     the same at user-shaped K8, 1024 graphs (six cutset variables).
  quality_k3  the bench tables at K3 (8192 graphs), where exact_mbest() is the truth: the share of graphs on which
              search_mbest's rows at m = 4 equal exact_mbest()'s, and the share of rows, at N = 64, 256, 1024.
  quality_k4  the same at K4 (256 graphs).
  quality_k5, quality_k8   beyond the truth: the share of graphs whose row 0 scores above map_sweep's assignment, the mean gain
              in nats, the mean score span of the four rows.
  ab_exact    exact_mbest() at K3 B = 8192 and K4 B = 256, m = 1, 4, 16, the library at --parent (built from the commit before
              the listed mode, bound under the args struct it had: tests/golden/make_exactmbest_bits.old_library) against this
              tree's, through ONE FactorGraphBatch on the same tensors, every library timed twice per round; and whether every
              output bit is equal.  Writes profiles/r35a_ab_exact_mbest_parent_change.json.
Writes profiles/r35a_time_search_mbest_<step>.json and prints each.  Options: --steps a,b (all but ab_exact), --launches L (per
timed window: 20), --rounds R (5 alternations), --limit S (seconds per step: 420), --out DIR (profiles), --parent LIB."""
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
ROWS = (1, 4, 16)
ROSE = 1e-9                     # a score counts as risen beyond this, relative to max(1, |score|): train.SEARCH_ROSE


def time_step(n, launches, rounds):
    import torch
    from time_cutset import alternate
    from time_search_map import BATCH, _batch
    from macaronicusermodeling_amd import exactmbest as K
    dev = torch.device('cuda:0')
    B = BATCH[n]
    fb, roots = _batch(n, B, dev)
    topo = fb.topo
    fb.sweep(roots, init=True)
    lists = {N: fb.cutset_draw(N, seed=7)[0] for N in SIZES}
    fns, kernels = {}, {}
    for N, c in lists.items():
        fns['cutset_map_n%d' % N] = lambda c=c: fb.cutset_map(c)
        for m in ROWS:
            fns['cutset_mbest_n%d_m%d' % (N, m)] = lambda c=c, m=m: fb.cutset_mbest(c, m)
    res = alternate(fns, launches, rounds)
    res.update(alternate({'search_mbest_n%d_m4' % N: (lambda N=N: fb.search_mbest(roots, 4, n_samples=N, seed=7)) for N in SIZES},
                         max(1, launches // 4), rounds))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    for m in ROWS:
        fb.cutset_mbest(lists[64], m)
        kernels[m] = K.kernels(K.last_kernel())
    torch.cuda.synchronize()
    return dict(batch=B, n_vars=topo.n_vars, cutset=int(lists[64].shape[2]), kernels=kernels, chunks={N: K.chunks(B, N) for N in SIZES},
                launches_per_window=launches, ms_per_call=res, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in res.items()},
                cutset_mbest_over_cutset_map={'n%d_m%d' % (N, m): med['cutset_mbest_n%d_m%d' % (N, m)] / med['cutset_map_n%d' % N]
                                              for N in SIZES for m in ROWS})


def quality_step(n):
    import torch
    from time_search_map import BATCH, _batch
    dev = torch.device('cuda:0')
    B, m = BATCH[n], 4
    fb, roots = _batch(n, B, dev)
    out = dict(batch=B, n_vars=fb.topo.n_vars, m=m, sizes={})
    truth = fb.exact_mbest(m) if n <= 4 else None
    for N in SIZES:
        x, score, found, score_bp = fb.search_mbest(roots, m, n_samples=N, seed=11)
        gain = score[:, 0] - score_bp
        rec = dict(share_row0_above_map_sweep=float((gain > ROSE * score[:, 0].abs().clamp(min=1.0)).double().mean()),
                   mean_gain_nats=float(gain.mean()), worst_loss_nats=float((-gain).max()),
                   mean_span_nats=float((score[:, 0] - score[:, m - 1]).mean()), share_full_lists=float((found == m).double().mean()))
        if truth is not None:
            same = (x == truth[0]).all(dim=2)
            rec.update(share_graphs_every_row_exact=float(same.all(dim=1).double().mean()), share_rows_exact=float(same.double().mean()),
                       share_row0_exact=float(same[:, 0].double().mean()), above_truth_nats=float((score - truth[1]).max()))
        out['sizes'][N] = rec
    torch.cuda.synchronize()
    return out


def ab_step(parent, launches, rounds):
    import torch
    from make_exactmbest_bits import bind_old, old_library
    from time_cutset import alternate
    from time_search_map import BATCH, _batch
    from macaronicusermodeling_amd import exactmbest as K
    dev = torch.device('cuda:0')
    out, bound = {}, bind_old(parent)
    for n in (3, 4):
        fb, _ = _batch(n, BATCH[n], dev)
        for m in ROWS:
            def old(m=m):
                with old_library(bound):
                    return fb.exact_mbest(m)
            new = lambda m=m: fb.exact_mbest(m)                  # noqa: E731
            a, b = old(), new()
            kernels = K.kernels(K.last_kernel())
            torch.cuda.synchronize()
            bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t          # noqa: E731
            equal = all(bool(torch.equal(bits(u), bits(v))) for u, v in zip(a, b))
            res = alternate({'parent': old, 'change': new, 'parent2': old, 'change2': new}, launches, rounds)
            med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
            spread = max(max(res[k]) - min(res[k]) for k in ('parent', 'parent2')) / med['parent']
            worst = max(med['change'], med['change2']) / min(med['parent'], med['parent2'])
            out['k%d_b%d_m%d' % (n, BATCH[n], m)] = dict(kernels=kernels, every_bit_equal=equal, ms=res, median_ms=med,
                                                          over_parent={k: med[k] / med['parent'] for k in med}, parent_spread_rel=spread,
                                                          worst_change_over_parent=worst, bar=1.0 + spread + 0.015, within_bar=worst <= 1.0 + spread + 0.015)
    return out


def run_step(name, launches, rounds, parent):
    if name == 'ab_exact':
        if not parent:
            raise SystemExit('ab_exact needs --parent')
        return ab_step(os.path.abspath(parent), launches, rounds)
    kind, n = name.split('_k')
    if kind == 'time' and int(n) in (5, 8):
        return time_step(int(n), launches, rounds)
    if kind == 'quality' and int(n) in (3, 4, 5, 8):
        return quality_step(int(n))
    raise SystemExit('unknown step %r' % name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', default=','.join(STEPS))
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--limit', type=int, default=420)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    ap.add_argument('--parent', default=None, help='ab_exact: libmlbp_exactmbest.so built from the commit before the listed mode')
    ap.add_argument('--child', default=None, help='run this one step in this process and print its JSON line')
    a = ap.parse_args()
    if a.child:
        import torch
        assert torch.cuda.is_available(), 'needs an MI355X'
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        print(json.dumps(run_step(a.child, a.launches, a.rounds, a.parent)))
        return
    os.makedirs(a.out, exist_ok=True)
    for name in a.steps.split(','):
        cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', name, '--launches', str(a.launches),
               '--rounds', str(a.rounds)] + (['--parent', a.parent] if a.parent else [])
        done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if done.returncode != 0:                                # a fault, an abort or the time limit: nothing more is started
            raise SystemExit('step %s ended with status %d' % (name, done.returncode))
        line = done.stdout.strip().splitlines()[-1]
        json.loads(line)
        path = os.path.join(a.out, 'r35a_ab_exact_mbest_parent_change.json' if name == 'ab_exact' else 'r35a_time_search_mbest_%s.json' % name)
        open(path, 'w').write(line + '\n')
        print(name, line, flush=True)


if __name__ == '__main__':
    main()
