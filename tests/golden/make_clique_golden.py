#!/usr/bin/env python3
"""Pin sentences with 4 to 12 predicted words (K4 ... K12 cliques of pairwise factors) on the reference's own code.

    python tests/golden/make_clique_golden.py [--reference /root/reference]

create_factor_graph (train_mp.py:257-299) joins every pair of predicted words of a sentence: k predicted words give k(k-1)/2
pairwise factors.  At X = 64 the clique size picks the sweep kernel (shared-table matrix cores up to 16 pairwise factors,
the exact kernel streaming its tables beyond, the generic kernel with messages in global memory once the exact kernel's
LDS image no longer fits), so the fixture holds one sentence of each of K1 to K10 and K12 (K8: 28 pairwise factors, not a
multiple of the three the shared-table pair gradient takes per pass).

Same mechanism as make_tidir_golden.py / make_batch_golden.py: the named definitions of training_classes.py / train_mp.py are
taken out of the files' syntax trees (lib2to3 in memory) and executed against the reference's own LBP.py; nothing derived
from the reference's text is written to the repository.  Inputs: the first sentence of each clique size in a synthetic
TI_DIR from tidir.synthesize (24 instances, X = 64, V_de = 12, sentences of 3 to 14 words with 1 to 12 predicted; the seed is
the first that covers the cliques above), its feature matrices rounded to three decimals, seeded non-zero theta, all three
feature planes on.

Saved in tidir_cliques_reference.json.gz (gzip, no timestamp: a rerun gives the same bytes), in the field names of the other two TI_DIR fixtures:
  * the TI_DIR (instances, vocabularies, the four feature matrices) and theta;
  * `reference`: per instance normalised guesses and nodes, variables, factors in creation order, the roots, marginals after
    initialize + three sweeps, get_posterior_probs and the step `return_gradient()` (as tidir_reference.json);
  * `user_adapt`: every instance through batch_sgd with --user_adapt and seeded per-user thetas (as tidir_reference.json);
  * `minibatch`: a shuffled order cut into minibatches of 4, theta after each (as tidir_batch_reference.json);
  * `predictions`: every instance through batch_predictions: block, .dist lines, log-posterior, precision counts.
Needs the reference checkout (--reference); never run on the GPU box."""
import argparse
import gzip
import hashlib
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden as G  # noqa: E402
from make_tidir_golden import definitions  # noqa: E402

CLIQUES = tuple(range(1, 11)) + (12,)  # predicted words per sentence, one sentence each (P = 0 to 45, and 66)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    a = ap.parse_args()
    from macaronicusermodeling_amd import tidir
    L, au, cleanup = G.load_reference(a.reference)
    tmp = tempfile.mkdtemp(prefix='mlbp_cliques_')
    try:
        roots = G.Roots(L)
        L.FactorNode.__lt__ = lambda self, other: self.id < other.id       # Python 2 ordered any two objects (make_text_golden.py)
        tc = {'sys': sys}
        exec(definitions(os.path.join(a.reference, 'training_classes.py'), ['TrainingInstance', 'Guess', 'SimpleNode']), tc)
        X, Vde, n_inst, seed = 64, 12, 24, 21
        paths = tidir.synthesize(tmp, n_instances=n_inst, X=X, Vde=Vde, sent_len=(3, 14), n_predicted=(1, 12), seed=seed)
        lines = [l for l in open(paths['ti'], encoding='utf8').read().split('\n') if l.strip()]
        first = {}                                  # the first sentence of each clique size, in file order
        for l in lines:
            first.setdefault(len(json.loads(l)['current_guesses']), l)
        assert set(CLIQUES) <= set(first), sorted(first)
        lines = [l for l in lines if first[len(json.loads(l)['current_guesses'])] is l]
        ks = [len(json.loads(l)['current_guesses']) for l in lines]
        for k in ('phi_pmi', 'phi_pmi_w1', 'phi_ed', 'phi_ped'):    # short inputs: three decimals keep the fixture small
            np.savetxt(paths[k], np.round(np.loadtxt(paths[k]), 3))
        en, de = tidir.read_vocab(paths['end']), tidir.read_vocab(paths['ded'])
        phi_ee, phi_w1, phi_ed = tidir.load_features(paths['phi_pmi'], paths['phi_pmi_w1'], paths['phi_ed'], paths['phi_ped'])
        rs = np.random.RandomState(13)
        ee_names, ed_names = ['pmi', 'pmi_w1', 'bias'], ['ed', 'ped', 'correct', 'full_history', 'hit_history', 'bias']     # train_mp.py:520-522
        theta_ee, theta_ed = rs.randn(1, 3) * 0.5, rs.randn(1, 6) * 0.5
        reg_param, lr = 0.1, 0.1
        ns = {'np': np, 'sys': sys, 'json': json, 'DTYPE': np.float64, 'PRED2GIVEN': 'pred2given', 'PRED2PRED': 'pred2pred',
              'VariableNode': L.VariableNode, 'FactorNode': L.FactorNode, 'FactorGraph': L.FactorGraph, 'PotentialTable': L.PotentialTable,
              'VAR_TYPE_GIVEN': L.VAR_TYPE_GIVEN, 'VAR_TYPE_PREDICTED': L.VAR_TYPE_PREDICTED, 'TrainingInstance': tc['TrainingInstance'],
              'options': types.SimpleNamespace(user_adapt=False, experience_adapt=False, use_correct_feat=True, history=True,
                                               session_history=True, use_approx_beliefs=False, use_approx_inference=False,
                                               report_times=False, reg_param=reg_param, reg_param_ua_scale='1.0'),
              'N': len(lines), 'de_domain': de, 'domain2theta': {}}
        exec(definitions(os.path.join(a.reference, 'train_mp.py'),
                         ['find_guess', 'get_var_node_pair', 'create_factor_graph', 'apply_regularization', 'batch_sgd', 'batch_predictions']), ns)
        en2id = {w: i for i, w in enumerate(en)}
        de2id = {w: i for i, w in enumerate(de)}

        def phi():
            return L.PhiWrapper(phi_ee.copy(), phi_w1.copy(), phi_ed.copy())

        def root_queue(line):
            """has_loops' start, then one root per sweep the reference will run: the predicted positions in order, cyclic
            (the batched trainer's rule); a tree (K1, K2) runs one sweep (LBP.py:219)."""
            rec = json.loads(line)
            sent = sorted(rec['current_sent'], key=lambda n: n['position'])
            guessed = {tuple(g['id']) for g in rec['current_guesses']}
            vids = [i for i, n in enumerate(sent) if n['lang'] != 'en' and tuple(n['id']) in guessed]
            return [vids[0]] + [vids[i % len(vids)] for i in range(3 if len(vids) >= 3 else 1)]

        err = sys.stderr
        sys.stderr = open(os.devnull, 'w')          # create_factor_graph writes a progress dot per instance
        try:
            # ---- per instance: what create_factor_graph built, three sweeps, posterior, step (as make_tidir_golden.py) ----
            out_inst = []
            for line in lines:
                ti = tc['TrainingInstance'].from_dict(json.loads(line))
                fg = ns['create_factor_graph'](ti=ti, learning_rate=lr, theta_en_en_names=ee_names, theta_en_de_names=ed_names,
                                               theta_en_en=theta_ee.copy(), theta_en_de=theta_ed.copy(), phi_wrapper=phi(), en_domain=en,
                                               de2id=de2id, en2id=en2id, d2t={})
                vids = sorted(fg.variables.keys())
                seq = [vids[i % len(vids)] for i in range(3)]
                roots.queue = [vids[0]]
                fg.initialize()
                fg.isLoopy = True                   # run the three sweeps also on a tree (the batched trainer always does)
                roots.queue = list(seq)
                fg.treelike_inference(3)
                assert not roots.queue
                out_inst.append(dict(
                    guesses={fld: [[list(g.id), g.guess, bool(g.revealed), g.l2_word, g.reference] for g in getattr(ti, fld)]
                             for fld in ('current_guesses', 'current_revealed_guesses', 'past_correct_guesses', 'past_guesses_for_current_sent')},
                    nodes=[[n.sent_id, list(n.id), n.l2_word, n.l1_parent, n.position, n.lang] for n in ti.current_sent],
                    variables=[[v, fg.variables[v].var_type, fg.variables[v].supervised_label, fg.variables[v].truth_label] for v in vids],
                    factors=[[f.id, f.factor_type, [v.id for v in f.varset], f.potential_table.observed_dim, f.gap, f.position, f.word_label]
                             for f in sorted(fg.factors, key=lambda f: f.id)],
                    roots=seq,
                    marginals=[fg.variables[v].get_marginal().m.reshape(-1).tolist() for v in vids],
                    step=[np.asarray(g, dtype=np.float64).reshape(-1).tolist() for g in fg.return_gradient()],
                    log_posterior=float(np.sum(fg.get_posterior_probs())),
                    log_posterior_terms=np.asarray(fg.get_posterior_probs(), dtype=np.float64).reshape(-1).tolist()))
            # ---- --user_adapt (train_mp.py:162-171, 226-247, 382-394), as make_tidir_golden.py ----
            users = sorted({json.loads(l)['user_id'] for l in lines})
            d2t = {}
            for u in users:
                d2t['en_en', u] = rs.randn(1, 3) * 0.5
                d2t['en_de', u] = rs.randn(1, 6) * 0.5
            ns['options'].user_adapt = True
            ns['options'].reg_param_ua_scale = '0.5'
            ns['domain2theta'] = d2t
            theta_dom0 = {u: [d2t['en_en', u].reshape(-1).tolist(), d2t['en_de', u].reshape(-1).tolist()] for u in users}
            adapt_inst = []
            for line in lines:
                roots.queue = root_queue(line)
                sent_id, p, g_ee, g_ed, ag = ns['batch_sgd'](line, ee_names, ed_names, theta_ee.copy(), theta_ed.copy(), phi(), lr, en, de2id, en2id,
                                                              {k: v.copy() for k, v in d2t.items()})
                assert not roots.queue
                (u,) = {d for _, d in ag}
                adapt_inst.append(dict(sent_id=sent_id, user=u, log_posterior=float(np.sum(p)),
                                       step=[np.asarray(g_ee).reshape(-1).tolist(), np.asarray(g_ed).reshape(-1).tolist()],
                                       step_domain=[np.asarray(ag['en_en', u]).reshape(-1).tolist(), np.asarray(ag['en_de', u]).reshape(-1).tolist()]))
            ns['options'].user_adapt = False
            ns['options'].reg_param_ua_scale = '1.0'
            ns['domain2theta'] = {}
            # ---- minibatched shuffled epoch (train_mp.py:631-649 + 405-424), as make_batch_golden.py ----
            order = [int(v) for v in np.random.RandomState(17).permutation(len(lines))]
            k = 4
            th_ee, th_ed = theta_ee.copy(), theta_ed.copy()
            mini = []
            for m0 in range(0, len(order), k):
                idx = order[m0:m0 + k]
                acc_ee, acc_ed, logps = np.zeros_like(th_ee), np.zeros_like(th_ed), []
                for i in idx:
                    roots.queue = root_queue(lines[i])
                    sent_id, p, g_ee, g_ed, ag = ns['batch_sgd'](lines[i], ee_names, ed_names, th_ee.copy(), th_ed.copy(), phi(), lr, en, de2id, en2id, {})
                    assert not roots.queue
                    acc_ee += g_ee; acc_ed += g_ed                       # batch_sgd_accumulate, train_mp.py:419-424
                    logps.append(float(np.sum(p)))
                th_ee, th_ed = th_ee + acc_ee, th_ed + acc_ed
                mini.append(dict(instances=idx, log_posteriors=logps, theta_en_en=th_ee.reshape(-1).tolist(), theta_en_de=th_ed.reshape(-1).tolist()))
            # ---- prediction pass (train_mp.py:310-343, qp=False) ----
            preds = []
            for line in lines:
                roots.queue = root_queue(line)
                p, fgs, dist, prec = ns['batch_predictions'](line, ee_names, ed_names, theta_ee.copy(), theta_ed.copy(), phi(), lr, en, de2id, en2id, {})
                assert not roots.queue
                preds.append(dict(log_posterior=float(np.sum(p)), block=fgs, dist=dist, precision=[int(v) for v in prec]))
        finally:
            sys.stderr = err
            roots.queue = []
        out = dict(X=X, Vde=Vde, vocab_en=en, vocab_de=de, instances=lines,
                   phi_pmi=np.loadtxt(paths['phi_pmi']).tolist(), phi_pmi_w1=np.loadtxt(paths['phi_pmi_w1']).tolist(),
                   phi_ed=np.loadtxt(paths['phi_ed']).tolist(), phi_ped=np.loadtxt(paths['phi_ped']).tolist(),
                   theta_en_en=theta_ee.tolist(), theta_en_de=theta_ed.tolist(), ee_names=ee_names, ed_names=ed_names,
                   options=dict(use_correct_feat=True, history=True, session_history=True, sweeps=3, learning_rate=lr, reg_param=reg_param),
                   reference=out_inst,
                   user_adapt=dict(users=users, theta_dom=theta_dom0, reg_param_ua_scale=0.5, instances=adapt_inst),
                   minibatch=dict(order=order, size=k, learning_rate=lr, steps=mini),
                   predictions=preds)
        with open(os.path.join(HERE, 'tidir_cliques_reference.json.gz'), 'wb') as f, gzip.GzipFile('', 'wb', 9, f, mtime=0) as z:
            z.write(json.dumps(out, ensure_ascii=False).encode('utf8'))
        man_path = os.path.join(HERE, 'MANIFEST.json')
        man = json.load(open(man_path)) if os.path.exists(man_path) else {}
        man['tidir_cliques_reference'] = {'generator': 'tests/golden/make_clique_golden.py',
                                          'reference_files': {f: hashlib.sha256(open(os.path.join(a.reference, f), 'rb').read()).hexdigest()
                                                              for f in ('training_classes.py', 'train_mp.py', 'LBP.py')}}
        json.dump(man, open(man_path, 'w'), indent=1, sort_keys=True)
        print('wrote tidir_cliques_reference.json.gz: %d instances, predicted words per sentence %s; %d minibatches'
              % (len(out_inst), sorted(ks), len(mini)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        cleanup()


if __name__ == '__main__':
    main()
