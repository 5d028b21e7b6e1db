#!/usr/bin/env python3
"""Times max-product decoding next to the sum-product call of the same inputs, by HIP events, in one process, alternating.

  (default)        FactorGraphBatch.map_sweep and FactorGraphBatch.sweep(..., marginals=...) on the default bench workload
                   (K3, 8192 graphs, X = 64, unique tables, 3 sweeps, keep_messages=False) and on the training layout (two
                   shared tables); prints both times and map_sweep / sweep, and the compulsory-byte model of the unique-table
                   call.
  --trainer        TiDirTrainer.decode() next to TiDirTrainer.predict() on the 8192-instance synthetic TI_DIR of bench.py's
                   train_epoch leg (host work included: both return host results).
  --only-map N     N map_sweep launches on the unique-table workload and nothing else: the process to put under
                   `rocprofv3 --kernel-trace --stats` or, in runs of their own, `--kernel-trace --pmc FETCH_SIZE` /
                   `--pmc WRITE_SIZE` (summarised by tools/pmc_traffic.py: 2 x FETCH_SIZE + WRITE_SIZE).
Options: --batch B (8192), --launches L (200 per timed window), --rounds R (5 alternations)."""
import argparse
import json
import os
import sys
import tempfile

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
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(window(fn, launches))
    return out


def model_bytes(topo, B, X=64):
    """Compulsory HBM bytes of one unique-table map_sweep call without write-back: every table and unary row once, the index
    arrays, assignment and score out."""
    parts = dict(pair_tables=B * topo.P * X * X * 8, unary_rows=B * topo.U * X * 8, index_arrays=B * (topo.P + topo.U) * 4,
                 assignment=B * topo.n_vars * 4, score=B * 8)
    parts['total'] = sum(parts.values())
    return parts


def batches(B):
    spec, roots = C.user_spec(10, [1, 4, 7], 64, 64, seed=1), [1, 4, 7]
    topo = GraphTopology.from_spec(spec)
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1236)
    unique = FactorGraphBatch(topo, 64, B, device=dev)
    unique.set_pair_tables(torch.rand(B * topo.P, 64, 64, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    unique.set_unary_tables(torch.rand(B * topo.U, 64, dtype=torch.float64, device=dev, generator=gen) + 0.01)
    layout = FactorGraphBatch(topo, 64, B, device=dev)         # the training layout: two pots behind every graph, unary rows out of 192
    layout.set_pair_tables(torch.rand(2, 64, 64, dtype=torch.float64, device=dev, generator=gen) + 0.01,
                           pair_tab=[[0, 0, 0]] * B)
    layout.set_unary_tables(torch.rand(192, 64, dtype=torch.float64, device=dev, generator=gen) + 0.01,
                            unary_tab=torch.randint(0, 192, (B, topo.U), generator=torch.Generator().manual_seed(7)).numpy())
    return topo, roots, unique, layout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--trainer', action='store_true')
    ap.add_argument('--only-map', type=int, default=0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    if a.trainer:
        from bench import TRAIN_EPOCH_TIDIR
        from macaronicusermodeling_amd import tidir
        from macaronicusermodeling_amd.train import TiDirTrainer
        with tempfile.TemporaryDirectory() as d:
            p = tidir.synthesize(d, **TRAIN_EPOCH_TIDIR)
            tt = TiDirTrainer(p['ti'], p['end'], p['ded'], p['phi_pmi'], p['phi_pmi_w1'], p['phi_ed'], p['phi_ped'], sweeps=3)
        gen = torch.Generator().manual_seed(3)
        tt.theta_en_en.copy_(torch.randn(3, generator=gen, dtype=torch.float64) * 0.3)
        tt.theta_en_de.copy_(torch.randn(6, generator=gen, dtype=torch.float64) * 0.3)
        res = alternate(dict(decode=tt.decode, predict=tt.predict), max(a.launches // 40, 3), a.rounds)
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        print(json.dumps(dict(workload='TiDirTrainer, %d instances, %d sentence shapes' % (tt.n_total, len(tt.trainers)),
                              ms_per_call=res, median_ms=med, decode_over_predict=med['decode'] / med['predict'])))
        return
    topo, roots, unique, layout = batches(a.batch)
    if a.only_map:
        for _ in range(a.only_map):
            unique.map_sweep(roots, init=True, keep_messages=False)
        torch.cuda.synchronize()
        print(json.dumps(dict(launches=a.only_map, batch=a.batch, model_bytes=model_bytes(topo, a.batch))))
        return
    marg = torch.empty(a.batch, topo.n_vars, 64, dtype=torch.float64, device=unique.device)
    out = {}
    for name, fb in (('unique_tables', unique), ('training_layout', layout)):
        res = alternate({'map_sweep': lambda fb=fb: fb.map_sweep(roots, init=True, keep_messages=False),
                         'sweep': lambda fb=fb: fb.sweep(roots, init=True, marginals=marg, keep_messages=False)}, a.launches, a.rounds)
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        out[name] = dict(ms_per_call=res, median_ms=med, map_over_sweep=med['map_sweep'] / med['sweep'])
    out['model_bytes_unique_tables'] = model_bytes(topo, a.batch)
    out['batch'], out['launches_per_window'] = a.batch, a.launches
    print(json.dumps(out))


if __name__ == '__main__':
    main()
