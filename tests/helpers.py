"""Test helpers: turn case specs + seeded inputs into FactorGraphBatch device tensors."""
import numpy as np

import cases as C
from oracle import lbp_oracle as O


def batch_tables(spec, topo, inputs_list):
    """pair tables [B*P][X][X] and unary tables [B*U][X] in (graph, slot) order."""
    g = O.Graph(spec)
    X = spec['X']
    pair, unary = [], []
    for inputs in inputs_list:
        for j in topo.pair_factors:
            pair.append(O.factor_table(g, inputs, g.by_id[topo.factor_ids[j]]).reshape(X, X))
        for j in topo.unary_factors:
            unary.append(O.factor_table(g, inputs, g.by_id[topo.factor_ids[j]]).reshape(X))
    pair = np.stack(pair) if pair else np.zeros((0, X, X))
    unary = np.stack(unary) if unary else np.zeros((0, X))
    return pair, unary


def case_inputs(case, n_graphs):
    """Graph 0 = the fixture's inputs; further graphs use other seeds."""
    kind = case['kind'] or 'uniform'
    return [C.make_inputs(case['spec'], case['seed'] + 1000 * i, kind) for i in range(n_graphs)]


def oracle_msgs(spec, inputs, roots, force_loopy=True):
    g = O.Graph(spec)
    msgs = O.init_messages(g)
    for r in roots:
        O.sweep(g, inputs, msgs, r)
    keys = C.msg_keys(spec)
    return g, msgs, np.stack([msgs[k] for k in keys])


def random_spec(rs, name, X=4):
    """A connected random graph: a random tree over 3-9 variables with shuffled, non-contiguous ids, up to three extra
    pairwise factors (loops, also parallel ones), unary factors on a random subset, factor ids in random creation
    order, table axes either way round."""
    n = int(rs.randint(3, 10))
    vids = sorted(rs.choice(40, size=n, replace=False).tolist())
    rs.shuffle(vids)
    edges = [(vids[i], vids[int(rs.randint(0, i))]) for i in range(1, n)]
    for _ in range(int(rs.randint(0, 4))):
        a, b = rs.choice(n, size=2, replace=False)
        edges.append((vids[a], vids[b]))
    facs = [[v] for v in vids if rs.rand() < 0.7] + [[a, b] if rs.rand() < 0.5 else [b, a] for a, b in edges]
    order = rs.permutation(len(facs))
    ids = sorted(rs.choice(200, size=len(facs), replace=False).tolist())
    factors = []
    for k, j in enumerate(order):
        vs = facs[j]
        dims = [0] if len(vs) == 1 else ([0, 1] if rs.rand() < 0.5 else [1, 0])
        factors.append(dict(id=int(ids[k]), vars=[int(v) for v in vs], dims=dims, table=k))
    rs.shuffle(factors)                                  # creation order != id order
    seen = []
    for f in factors:
        for v in f['vars']:
            if v not in seen:
                seen.append(v)
    return dict(name=name, style='explicit', X=X, var_ids=seen, labels=[0] * len(seen), factors=factors)




def posterior_buffers(fb, seed):
    """(labels, out, sum_out) for FactorGraphBatch.sweep(posterior=...): random int32 labels [B][n_vars] in [0, X) on fb's
    device, NaN-filled outputs."""
    import torch
    labels = np.random.RandomState(seed).randint(0, fb.X, size=(fb.B, fb.topo.n_vars)).astype(np.int32)
    nan = float('nan')
    return (torch.from_numpy(labels).to(fb.device), torch.full((fb.B,), nan, dtype=torch.float64, device=fb.device),
            torch.full((1,), nan, dtype=torch.float64, device=fb.device))


PLANE_COLUMNS = {'correct': 2, 'full_history': 3, 'hit_history': 4}       # the per-instance planes of phi_en_de (train_mp.py:178-217)


def tidir_oracle_graph(key, b, i, phi_ee, phi_w1, phi_ed, th_ee, th_ed):
    """The oracle's form of instance i of a tidir.bucket_instances bucket, as create_factor_graph builds it
    (train_mp.py:105-306): (graph, inputs, roots, plane cells).  Labels and observed columns are the instance's, the three
    planes are written into phi_en_de, the potentials are exp(phi . theta), and the roots are the batched trainer's rule
    (predicted positions in order, cyclic, three sweeps)."""
    import copy
    X = phi_ee.shape[0]
    unary = [f for f in sorted(b['spec']['factors'], key=lambda f: f['id']) if len(f['vars']) == 1]
    s = copy.deepcopy(b['spec'])
    s['labels'] = [int(v) for v in b['var_labels'][i]]
    for u, f in enumerate(unary):
        s['factors'][f['id']]['observed_dim'] = int(b['unary_obs'][i, u])
    phi_i = phi_ed.copy()
    n_cells = 0
    for name, k in PLANE_COLUMNS.items():
        plane = np.zeros(phi_ed.shape[:2])
        for ci, cj, cv in b['rows'][i]['planes'][name]:
            plane[ci, cj] += cv
            n_cells += 1
        phi_i[:, :, k] = plane
    inputs = dict(phi_en_en=phi_ee, phi_en_en_w1=phi_w1, phi_en_de=phi_i, theta_en_en=th_ee, theta_en_de=th_ed,
                  pot_en_en=np.exp(phi_ee.dot(th_ee.T).reshape(X, X)), pot_en_en_w1=np.exp(phi_w1.dot(th_ee.T).reshape(X, X)),
                  pot_en_de=np.exp(phi_i.dot(th_ed.T).reshape(phi_ed.shape[:2])))
    roots = [key[1][j % len(key[1])] for j in range(3)]
    return O.Graph(s), inputs, roots, n_cells


def tidir_gold(name):
    """A TI_DIR fixture written by the generators under tests/golden: <name>.json, or <name>.json.gz."""
    import gzip
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', name + '.json')
    if os.path.exists(path + '.gz'):
        return json.loads(gzip.open(path + '.gz').read().decode('utf8'))
    return json.load(open(path, encoding='utf8'))


def write_tidir(gold, d):
    """A fixture's TI_DIR as the files TiDirTrainer reads; returns their paths."""
    import os
    paths = {k: os.path.join(d, k) for k in ('ti', 'vocab.en', 'vocab.de', 'phi.pmi', 'phi.pmi_w1', 'phi.ed', 'phi.ped')}
    open(paths['ti'], 'w', encoding='utf8').write('\n'.join(gold['instances']) + '\n')
    open(paths['vocab.en'], 'w', encoding='utf8').write('\n'.join(gold['vocab_en']) + '\n')
    open(paths['vocab.de'], 'w', encoding='utf8').write('\n'.join(gold['vocab_de']) + '\n')
    for k, name in (('phi.pmi', 'phi_pmi'), ('phi.pmi_w1', 'phi_pmi_w1'), ('phi.ed', 'phi_ed'), ('phi.ped', 'phi_ped')):
        np.savetxt(paths[k], np.array(gold[name]))
    return paths
