"""Two builds of libmlbp.so in one process: the shared-table sweep call with its DIRECT gradient epilogue (user K3 through
UserGraphTrainer, B = 8192, random and reference feature planes), medians of 5 alternations of windows of 20 launches, HIP
events, each library timed twice per round; every output bit of the two is compared.

  python tools/ab_shared_gradient.py --parent LIB [--out DIR]

LIB is a libmlbp.so built from the commit to compare with (the package is copied under a second name beside it, so both
libraries and both sets of Python wrappers live in this process).  Writes DIR/ab_shared_direct_gradient.json (default: profiles)."""
import argparse, json, os, shutil, sys, tempfile
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import cases as C
ap = argparse.ArgumentParser()
ap.add_argument('--parent', required=True, help='libmlbp.so of the commit to compare with')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
args = ap.parse_args()
tmp = tempfile.mkdtemp()
shutil.copytree(os.path.join(ROOT, 'macaronicusermodeling_amd'), os.path.join(tmp, 'mlbp_parent_pkg'), ignore=shutil.ignore_patterns('__pycache__', 'csrc*'))
shutil.copy(args.parent, os.path.join(tmp, 'mlbp_parent_pkg', 'libmlbp.so'))
sys.path.insert(0, tmp)
import macaronicusermodeling_amd.train as T_change
import mlbp_parent_pkg.train as T_parent
from macaronicusermodeling_amd import _ffi as F_change
from mlbp_parent_pkg import _ffi as F_parent
assert F_change.LIB_PATH != F_parent.LIB_PATH

def build(T, F, pred, planes, B):
    spec = C.user_spec(10, pred, 64, 48, seed=1)
    inputs = C.make_inputs(spec, 77)
    if planes == 'reference':
        inputs = C.reference_planes(inputs)
    topo = T.GraphTopology.from_spec(spec)
    rs = np.random.RandomState(5)
    by_id = {f['id']: f for f in spec['factors']}
    labels = rs.randint(0, 64, size=(B, topo.n_vars))
    obs = np.zeros((B, topo.U), dtype=np.int64)
    for u, j in enumerate(topo.unary_factors):
        f = by_id[topo.factor_ids[j]]
        obs[:, u] = rs.randint(0, 48 if f['factor_type'] == 'en_de' else 64, size=B)
    roots = list(spec['var_ids'])[1:] + list(spec['var_ids'])[:1]
    tr = T.UserGraphTrainer(spec, labels, obs, inputs['phi_en_en'], inputs['phi_en_en_w1'], inputs['phi_en_de'],
                            inputs['theta_en_en'], inputs['theta_en_de'], roots=roots)
    tr.build_potentials()
    g = (torch.full_like(tr._g_ee, float('nan')), torch.full_like(tr._g_ed, float('nan')))
    marg = torch.full_like(tr._marg, float('nan'))
    def call():
        tr.batch.sweep(roots, init=True, marginals=marg, gradient=g, keep_messages=False)
    call(); torch.cuda.synchronize()
    assert F.lib.mlbp_last_sweep_kernel() == 3 and F.lib.mlbp_last_sweep_fused_gradient() == 1
    assert topo.plan(roots)['shared_gradient_from_tiles'] == 1
    assert tr.batch.program(roots).exact_count(B) == 0
    return call, g, marg, tr

def window(call, n=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        call()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n

out = {}
for name, pred, planes in (('k3_random_planes', [1, 4, 7], 'random'), ('k3_reference_planes', [1, 2, 7], 'reference')):
    B = 8192
    cp, gp, mp, trp = build(T_parent, F_parent, pred, planes, B)
    cc, gc, mc, trc = build(T_change, F_change, pred, planes, B)
    same = bool(torch.equal(gp[0], gc[0]) and torch.equal(gp[1], gc[1]) and torch.equal(mp, mc))
    for _ in range(3):
        window(cp); window(cc)
    tp, tc = [[], []], [[], []]
    for r in range(5):
        for k in range(2):
            tp[k].append(window(cp)); tc[k].append(window(cc))
    allp = tp[0] + tp[1]
    med = lambda v: float(np.median(v))
    res = dict(parent_ms=med(allp), change_ms=med(tc[0] + tc[1]), ratios=[med(tc[k]) / med(tp[k]) for k in range(2)],
               parent_spread=(max(allp) - min(allp)) / med(allp), same_bits=same, parent_windows=tp, change_windows=tc, B=B)
    res['bar'] = 1.0 + res['parent_spread'] + 0.015
    out[name] = res
    print(name, {k: res[k] for k in ('parent_ms', 'change_ms', 'ratios', 'parent_spread', 'bar', 'same_bits')}, flush=True)
os.makedirs(args.out, exist_ok=True)
json.dump(out, open(os.path.join(args.out, 'ab_shared_direct_gradient.json'), 'w'), indent=1)
shutil.rmtree(tmp, ignore_errors=True)
