#!/usr/bin/env python3
"""Times the gradient beyond the exact limit (FactorGraphBatch.cutset_gradient, the listed mode of libmlbp_exactgrad.so) and
records its quality where the truth exists, by HIP events; every step runs in a child process of its own under its own time
limit, and a step that fails ends the run.

  time_k5     user-shaped K5, X = 64, unique tables U(0,1) + 0.01, features U(-1, 1) with F_ee = 3, F_ed = 6:
              cutset_gradient(configs, log_q) at N = 64, 256 and 1024 entries per graph -- the list drawn once by cutset_draw() on
              the messages of one sweep, outside the timed windows -- and beside it, alternating in the same process:
              cutset_estimate(configs, log_q) on the same list and cutset_draw() at the same N.  The batch is 8192 graphs when the
              listed workspace (four partials of 330 256 bytes per graph: 10.8 GB) and the tables fit the device's free memory,
              else the largest power of two that does; the record says which.
  time_k8     the same at user-shaped K8, 1024 graphs (six cutset variables, 28 pairwise factors).
  quality_k3  the bench tables at K3 (8192 graphs), where exact_gradient() gives the truth: estimate_gradient() at n_list = 256
              for both proposals -- cosine and |estimate - exact| / |exact| of the sums over the batch and the means of the same
              per graph, log_z - log_z_hat -- beside the same figures of the BP gradient of the sweep call.  Recorded, not asserted.
  quality_k4  the same at K4 (256 graphs).
Writes profiles/r34a_time_cutset_gradient_<step>.json and prints each.  Options: --steps a,b (all four), --launches L (per timed
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
PREDICTED = {3: [1, 4, 7], 4: [1, 4, 6, 8], 5: [1, 3, 4, 6, 8], 8: [0, 1, 3, 4, 6, 7, 8, 9]}
F_EE, F_ED = 3, 6


def feature_batch(spec, B, dev):
    """A batch of `spec` with unique tables U(0,1) + 0.01, features U(-1, 1), the spec's selectors and observed columns where it
    has them (user-shaped graphs) and random ones elsewhere, random labels."""
    import numpy as np
    import torch
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(spec)
    X, Vde = spec['X'], spec.get('Vde', spec['X'])
    by_id = {f['id']: f for f in spec['factors']}
    gen = torch.Generator(device=dev).manual_seed(1236)
    fb = FactorGraphBatch(topo, X, B, device=dev)
    fb.set_pair_tables(torch.rand(B * topo.P, X, X, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    fb.set_unary_tables(torch.rand(B * topo.U, X, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    rs = np.random.RandomState(7)
    unary = [by_id[topo.factor_ids[j]] for j in topo.unary_factors]
    if all('gap' in f for f in by_id.values()):
        pair_phi = [0 if by_id[topo.factor_ids[j]]['gap'] > 1 else 1 for j in topo.pair_factors]
        kinds = [2 if f['factor_type'] == 'en_de' else (0 if f['gap'] > 1 else 1) for f in unary]
        obs = np.tile(np.array([f['observed_dim'] for f in unary]), (B, 1))
    else:
        pair_phi = [int(x) for x in rs.randint(0, 2, size=topo.P)]
        kinds = [int(x) for x in rs.randint(0, 3, size=topo.U)]
        obs = np.stack([rs.randint(0, Vde if k == 2 else X, size=B) for k in kinds], axis=1).reshape(B, topo.U)
    fb.set_features(rs.uniform(-1, 1, (X, X, F_EE)), rs.uniform(-1, 1, (X, X, F_EE)), rs.uniform(-1, 1, (X, Vde, F_ED)), pair_phi, kinds)
    fb.set_observations(rs.randint(0, X, size=(B, topo.n_vars)), obs)
    fb.initialize()
    return fb


def _user_spec(n):
    import cases as C
    return C.user_spec(10, PREDICTED[n], 64, 64, seed=1)


def _fitting_batch(n, B):
    """The largest B' = B / 2^k whose listed workspace, tables and lists fit the device's free memory (with a tenth to spare)."""
    import torch
    from macaronicusermodeling_amd import cutsetis as KP, exactgrad as K
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(_user_spec(n))
    pl = KP.plan(topo, None, 64, torch.device('cuda:0'))
    free = torch.cuda.mem_get_info()[0]
    while B > 1:
        need = K.listed_workspace_bytes(B, 64, topo.n_vars, topo.P, topo.U, pl.n_forest, max(SIZES))
        need += B * (topo.P * 64 * 64 + topo.U * 64 + 2 * topo.n_msgs * 64) * 8 + B * max(SIZES) * (pl.n_cut * 4 + 8) * 2
        if need <= 0.9 * free:
            break
        B //= 2
    return B


def time_step(n, B_asked, launches, rounds):
    import torch
    from time_cutset import alternate
    from macaronicusermodeling_amd import cutsetis as KP, exactgrad as K
    dev = torch.device('cuda:0')
    B = _fitting_batch(n, B_asked)
    fb = feature_batch(_user_spec(n), B, dev)
    topo, roots = fb.topo, PREDICTED[n][:3]
    fb.sweep(roots, init=True)                                  # the messages cutset_draw() reads
    lists = {N: fb.cutset_draw(N, seed=7) for N in SIZES}
    marg = torch.empty(B, topo.n_vars, 64, dtype=torch.float64, device=dev)
    g_ee, g_ed = (torch.empty(B, F, dtype=torch.float64, device=dev) for F in (F_EE, F_ED))
    fns = {}
    for N, (c, q) in lists.items():
        fns['gradient_n%d' % N] = lambda c=c, q=q: fb.cutset_gradient(c, q, out_ee=g_ee, out_ed=g_ed)
        fns['estimate_n%d' % N] = lambda c=c, q=q: fb.cutset_estimate(configs=c, log_q=q, marginals=marg)
        fns['draw_n%d' % N] = lambda N=N: fb.cutset_draw(N, seed=7)
    res = alternate(fns, launches, rounds)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    c, q = lists[256]
    _, _, log_z_hat = fb.cutset_gradient(c, q, out_ee=g_ee, out_ed=g_ed)
    kernel = K.last_kernel()
    ref_lz = fb.cutset_estimate(configs=c, log_q=q, marginals=marg)[0]
    torch.cuda.synchronize()
    pl = KP.plan(topo, None, 64, dev)
    return dict(batch=B, batch_asked=B_asked, n_vars=topo.n_vars, cutset=pl.n_cut, kernel=kernel, launches_per_window=launches, ms_per_call=res,
                median_ms=med, spread_ms={k: max(v) - min(v) for k, v in res.items()},
                chunks={N: K.chunks(B, N, kernel) for N in SIZES},
                workspace_bytes={N: K.listed_workspace_bytes(B, 64, topo.n_vars, topo.P, topo.U, pl.n_forest, N) for N in SIZES},
                gradient_over_estimate={N: med['gradient_n%d' % N] / med['estimate_n%d' % N] for N in SIZES},
                gradient_over_draw={N: med['gradient_n%d' % N] / med['draw_n%d' % N] for N in SIZES},
                ns_per_entry={N: med['gradient_n%d' % N] * 1e6 / (B * N) for N in SIZES},
                max_abs_log_z_hat_minus_estimate=float((log_z_hat - ref_lz).abs().max()))


def _gap(est_ee, est_ed, ref_ee, ref_ed):
    import numpy as np
    import torch
    per_e, per_r = torch.cat([est_ee, est_ed], dim=1), torch.cat([ref_ee, ref_ed], dim=1)
    e, r = per_e.sum(0).cpu().numpy(), per_r.sum(0).cpu().numpy()
    return dict(cosine=float(e.dot(r) / np.linalg.norm(e) / np.linalg.norm(r)), relative_norm=float(np.linalg.norm(e - r) / np.linalg.norm(r)),
                mean_per_graph_relative_norm=float(((per_e - per_r).norm(dim=1) / per_r.norm(dim=1)).mean()),
                mean_per_graph_cosine=float(torch.nn.functional.cosine_similarity(per_e, per_r, dim=1).mean()))


def quality_step(n, B, N=256):
    import torch
    dev = torch.device('cuda:0')
    fb = feature_batch(_user_spec(n), B, dev)
    roots = PREDICTED[n][:3]
    x_ee, x_ed, log_z = fb.exact_gradient()
    b_ee, b_ed = torch.empty_like(x_ee), torch.empty_like(x_ed)
    marg = torch.empty(B, fb.topo.n_vars, 64, dtype=torch.float64, device=dev)
    fb.sweep(roots, init=True, marginals=marg, gradient=(b_ee, b_ed))
    out = dict(batch=B, n_vars=fb.topo.n_vars, N=N, bp=_gap(b_ee, b_ed, x_ee, x_ed), proposals={})
    for proposal in ('messages', 'sample'):
        e_ee, e_ed, log_z_hat = fb.estimate_gradient(roots, n_list=N, seed=11, proposal=proposal)
        err = log_z - log_z_hat
        out['proposals'][proposal] = dict(_gap(e_ee, e_ed, x_ee, x_ed), mean_log_z_minus_log_z_hat=float(err.mean()),
                                          mean_abs_log_z_error=float(err.abs().mean()), max_abs_log_z_error=float(err.abs().max()))
    torch.cuda.synchronize()
    return out


def run_step(name, launches, rounds):
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
        path = os.path.join(a.out, 'r34a_time_cutset_gradient_%s.json' % name)
        open(path, 'w').write(line + '\n')
        print(name, line, flush=True)


if __name__ == '__main__':
    main()
