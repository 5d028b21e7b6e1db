"""Sentences with 4 to 12 predicted words through TiDirTrainer, pinned on the reference pipeline.

create_factor_graph (train_mp.py:257-299) joins every pair of predicted words: k words give a K_k clique of k(k-1)/2
pairwise factors.  At X = 64 the clique size picks the path: the shared-table matrix-core kernels up to 16 pairwise factors
(K2 to K6), the exact kernel streaming its tables for K7 to K9 (gradient from the per-graph kernels), and the generic
kernel with its messages in global memory for K10 and K12: their 220 and 288 message slots, with the program image, put the
exact kernel's LDS image past 160 KiB (the 180 of the K9 still fit).
tests/golden/tidir_cliques_reference.json.gz (make_clique_golden.py) holds what the reference computes on one sentence of each of
K1 to K10 and K12: marginals, posteriors, steps, a --user_adapt pass, a minibatched shuffled epoch and the prediction
text."""
import json

import numpy as np
import pytest

import kernel_inventory as K
from helpers import tidir_gold, write_tidir

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

KERNEL_EXACT, KERNEL_GENERIC = 2, 5          # mlbp.h MLBP_KERNEL_*
LARGE = {7: KERNEL_EXACT, 8: KERNEL_EXACT, 9: KERNEL_EXACT, 10: KERNEL_GENERIC, 12: KERNEL_GENERIC}     # predicted words -> sweep kernel at X = 64


def _gold():
    return tidir_gold('tidir_cliques_reference')


def _trainer(paths, gold, **kw):
    from macaronicusermodeling_amd.train import TiDirTrainer
    tt = TiDirTrainer(paths['ti'], paths['vocab.en'], paths['vocab.de'], paths['phi.pmi'], paths['phi.pmi_w1'], paths['phi.ed'],
                      paths['phi.ped'], sweeps=3, use_correct_feat=True, history=True, session_history=True, **kw)
    tt.theta_en_en.copy_(torch.tensor(gold['theta_en_en'], dtype=torch.float64).reshape(-1))
    tt.theta_en_de.copy_(torch.tensor(gold['theta_en_de'], dtype=torch.float64).reshape(-1))
    return tt


def _sent_id(line):
    return json.loads(line)['current_sent'][0]['sent_id']


def _check_buckets(tt, by_sent):
    """Every bucket's marginals and log-posteriors (as the last statistics call left them) against the reference's."""
    seen = 0
    for key, tr in tt.trainers.items():
        marg, lp = tr._marg.cpu().numpy(), tr._lp.cpu().numpy()
        for i, row in enumerate(tt.buckets[key]['rows']):
            ref = by_sent[row['sent_id']]
            assert list(tr.roots) == ref['roots']
            np.testing.assert_allclose(marg[i], np.array(ref['marginals']), rtol=1e-9, atol=1e-300)
            np.testing.assert_allclose(lp[i], ref['log_posterior'], rtol=1e-9)
            seen += 1
    return seen


def _check_grouped_then_large(log, words):
    """A grouped statistics call's launch log (words: predicted words per bucket, in bucket order): the shared-table kernels
    ran as grouped launches only, and every K7+ bucket's sweep kernel followed them -- the exact kernel streaming its tables
    for K7 to K9, the generic kernel for K10 and K12 -- the last of them reported as the call's kernel."""
    from macaronicusermodeling_amd import _ffi
    shared = [e for e in log if e[0] in ('shared_prepare_kernel', 'sweep_x64_shared_kernel')]
    assert ('shared_prepare_kernel', (True,)) in shared and ('shared_prepare_kernel', (False,)) not in shared
    assert all(e[1][3] for e in shared if e[0] == 'sweep_x64_shared_kernel')           # (MULTI: the grouped instances)
    behind = log[max(i for i, e in enumerate(log) if e[0] == 'sweep_x64_shared_kernel'):]
    large = [k for k in words if k in LARGE]
    assert large
    if any(k <= 9 for k in large):
        assert ('sweep_x64_fused_kernel', (True, 0, False)) in behind
    if any(k >= 10 for k in large):
        assert ('sweep_generic_kernel', (True, False)) in behind
    assert _ffi.lib.mlbp_last_sweep_kernel() == LARGE[large[-1]]


@pytest.mark.parametrize('grouped', [True, False], ids=['grouped', 'per_bucket'])
def test_large_cliques_equal_the_reference_pipeline(tmp_path, grouped):
    """TiDirTrainer on the fixture's files, with and without grouped sweeps: per-bucket marginals and log-posteriors of K1 to
    K12 equal the reference's, and one epoch moves theta by the sum of the reference's steps."""
    gold = _gold()
    tt = _trainer(write_tidir(gold, str(tmp_path)), gold, grouped_sweeps=grouped)
    assert {len(k[1]) for k in tt.trainers} >= {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12}
    K.reset()
    tt.local_statistics()
    if grouped:          # the K2 to K6 buckets ran in the grouped launches on the matrix cores, the K7+ buckets' own launches behind them
        _check_grouped_then_large(K.launched(), [len(key[1]) for key in tt.trainers])
    by_sent = {_sent_id(l): r for l, r in zip(gold['instances'], gold['reference'])}
    assert _check_buckets(tt, by_sent) == len(gold['reference']) == 11
    o = gold['options']
    mean_lp = tt.epoch(o['learning_rate'], o['reg_param'] / len(gold['reference']))
    want_ee = np.array(gold['theta_en_en']).reshape(-1) + sum(np.array(r['step'][0]) for r in gold['reference'])
    want_ed = np.array(gold['theta_en_de']).reshape(-1) + sum(np.array(r['step'][1]) for r in gold['reference'])
    np.testing.assert_allclose(tt.theta_en_en.cpu().numpy(), want_ee, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(tt.theta_en_de.cpu().numpy(), want_ed, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(mean_lp, np.mean([r['log_posterior'] for r in gold['reference']]), rtol=1e-9)


@pytest.mark.parametrize('shared_gradient', [True, False], ids=['shared_pairs_gradient', 'per_graph_gradient'])
def test_each_large_clique_takes_its_kernel_and_equals_the_reference(tmp_path, shared_gradient):
    """Each K7 to K10 and K12 sentence as a file of its own (one bucket, no grouping): the sweep kernel it took (the exact
    kernel streaming its tables for K7 to K9; the generic kernel, messages in global memory, for K10 and K12), no gradient
    fused into the sweep, marginals and log-posterior equal to the reference's, and one epoch moves theta by the reference's step.  The gradient comes from the shared-table
    pair kernel (P in chunks of three; K8's 28 leave a partial last chunk) or, with the batch's use_shared_gradient off, from the
    per-graph X = 64 kernel."""
    from macaronicusermodeling_amd import _ffi
    gold = _gold()
    o = gold['options']
    done = set()
    for j, (line, ref) in enumerate(zip(gold['instances'], gold['reference'])):
        k = len(ref['variables'])
        if k not in LARGE:
            continue
        d = tmp_path / ('instance%d' % j)
        d.mkdir()
        tt = _trainer(write_tidir(dict(gold, instances=[line]), str(d)), gold)
        (tr,) = tt.trainers.values()
        assert tr.topo.P == k * (k - 1) // 2 and tr.topo.plan(tr.roots[:tr.n_sweeps_run])['shared_ok'] == 0
        tr.batch.use_shared_gradient = shared_gradient
        tt.local_statistics()
        assert (_ffi.lib.mlbp_last_sweep_kernel(), _ffi.lib.mlbp_last_sweep_fused_gradient()) == (LARGE[k], 0), k
        assert _check_buckets(tt, {_sent_id(line): ref}) == 1
        tt.epoch(o['learning_rate'], o['reg_param'] / len(gold['instances']))      # the reference's regularisation: reg_param / N
        np.testing.assert_allclose(tt.theta_en_en.cpu().numpy(), np.array(gold['theta_en_en']).reshape(-1) + ref['step'][0],
                                   rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(tt.theta_en_de.cpu().numpy(), np.array(gold['theta_en_de']).reshape(-1) + ref['step'][1],
                                   rtol=1e-9, atol=1e-12)
        done.add(k)
    assert done == set(LARGE)


def test_user_adapt_epoch_on_large_cliques_equals_the_reference_batch_sgd(tmp_path):
    """--user_adapt on the fixture (batch_sgd with seeded per-user thetas, make_clique_golden.py): one epoch of
    TiDirTrainer(adapt='user') adds exactly the sums of the reference's global and per-user steps."""
    gold = _gold()
    ua = gold['user_adapt']
    names = ua['users']
    tt = _trainer(write_tidir(gold, str(tmp_path)), gold, adapt='user', domains=names, reg_param_ua_scale=ua['reg_param_ua_scale'])
    for i, u in enumerate(names):
        tt.theta_dom_en_en[i].copy_(torch.tensor(ua['theta_dom'][u][0], dtype=torch.float64))
        tt.theta_dom_en_de[i].copy_(torch.tensor(ua['theta_dom'][u][1], dtype=torch.float64))
    o = gold['options']
    mean_lp = tt.epoch(o['learning_rate'], o['reg_param'] / len(gold['instances']))
    inst = ua['instances']
    np.testing.assert_allclose(mean_lp, np.mean([r['log_posterior'] for r in inst]), rtol=1e-9)
    np.testing.assert_allclose(tt.theta_en_en.cpu().numpy(), np.array(gold['theta_en_en']).reshape(-1) + sum(np.array(r['step'][0]) for r in inst),
                               rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(tt.theta_en_de.cpu().numpy(), np.array(gold['theta_en_de']).reshape(-1) + sum(np.array(r['step'][1]) for r in inst),
                               rtol=1e-9, atol=1e-12)
    for i, u in enumerate(names):
        mine = [r for r in inst if r['user'] == u]
        assert mine
        np.testing.assert_allclose(tt.theta_dom_en_en[i].cpu().numpy(), np.array(ua['theta_dom'][u][0]) + sum(np.array(r['step_domain'][0]) for r in mine),
                                   rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(tt.theta_dom_en_de[i].cpu().numpy(), np.array(ua['theta_dom'][u][1]) + sum(np.array(r['step_domain'][1]) for r in mine),
                                   rtol=1e-9, atol=1e-12)


def test_minibatched_shuffled_epoch_on_large_cliques_equals_the_reference_sequence(tmp_path):
    """The fixture's minibatched epoch (a fixed shuffled order, minibatches of 4, every instance at the theta its minibatch
    starts from): TiDirTrainer(minibatch=4) must land on the reference's theta after every minibatch, grouped and per-bucket,
    'rebuild' and 'masked' (eager and replayed from a HIP graph)."""
    gold = _gold()
    mb = gold['minibatch']
    paths = write_tidir(gold, str(tmp_path))
    for grouped, mode, graph in ((True, 'rebuild', False), (False, 'rebuild', False), (True, 'masked', False), (False, 'masked', False),
                                 (True, 'masked', True)):
        tt = _trainer(paths, gold, minibatch=mb['size'], shuffle_seed=3, grouped_sweeps=grouped, minibatch_mode=mode)
        tt.epoch_order = lambda epoch: np.array(mb['order'])
        seen = []
        if mode == 'rebuild':
            update = tt._update

            def recording(lr, reg):
                out = update(lr, reg)
                seen.append((tt.theta_en_en.cpu().numpy().copy(), tt.theta_en_de.cpu().numpy().copy(), out))
                return out
            tt._update = recording
        else:
            update = tt._update_on_device

            def recording(lr, reg):
                update(lr, reg)
                n = tt.n_stat
                seen.append((tt.theta_en_en.cpu().numpy().copy(), tt.theta_en_de.cpu().numpy().copy(),
                             (float(tt.stats[n - 2].item()), float(tt.stats[n - 1].item()))))
            tt._update_on_device = recording
            if graph:
                tt.capture_masked()
        mean_lp = tt.epoch(mb['learning_rate'], gold['options']['reg_param'] / len(gold['instances']))
        assert len(seen) == len(mb['steps']) == 3, (grouped, mode, graph)
        for (ee, ed, (lp, n)), step in zip(seen, mb['steps']):
            np.testing.assert_allclose(ee, step['theta_en_en'], rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(ed, step['theta_en_de'], rtol=1e-9, atol=1e-12)
            assert n == len(step['instances'])
            np.testing.assert_allclose(lp, sum(step['log_posteriors']), rtol=1e-9)
        np.testing.assert_allclose(mean_lp, np.mean([l for s in mb['steps'] for l in s['log_posteriors']]), rtol=1e-9)


def test_prediction_files_on_large_cliques_equal_the_reference_text(tmp_path):
    """predict(save_predictions=...) on the fixture: the '*SENT_ID:' blocks and .dist lines equal, character for character,
    what the reference's batch_predictions returned; precision counts and mean log-posterior are its sums."""
    gold = _gold()
    tt = _trainer(write_tidir(gold, str(tmp_path)), gold)
    out = str(tmp_path / 'pred')
    mean_lp, counts = tt.predict(save_predictions=out)
    want = gold['predictions']
    assert open(out, encoding='utf8').read() == ''.join(p['block'] + '\n' for p in want)
    assert open(out + '.dist', encoding='utf8').read() == ''.join(p['dist'] + '\n' for p in want)
    assert counts == tuple(int(sum(p['precision'][k] for p in want)) for k in range(4))
    np.testing.assert_allclose(mean_lp, np.mean([p['log_posterior'] for p in want]), rtol=1e-9)


def test_large_cliques_with_theta_far_out_agree_grouped_and_per_bucket(tmp_path):
    """The bias plane of the en_en features at 200 (every en_en entry e^200): constant products overflow, the matrix-core
    kernels flag their graphs and the exact kernel redoes them.  Grouped and per-bucket statistics are finite and agree.  (No
    reference pin: the reference's own overflow behaviour is not what is tested here.)"""
    gold = _gold()
    paths = write_tidir(gold, str(tmp_path))
    a, b = _trainer(paths, gold, grouped_sweeps=True), _trainer(paths, gold, grouped_sweeps=False)
    for t in (a, b):
        t.theta_en_en.copy_(torch.tensor([0.3, -0.2, 200.0], dtype=torch.float64, device=t.theta_en_en.device))
    sa, sb = a.local_statistics().cpu().numpy(), b.local_statistics().cpu().numpy()
    assert np.isfinite(sa).all() and np.isfinite(sb).all()
    np.testing.assert_allclose(sa, sb, rtol=1e-9, atol=1e-9)


def test_one_large_clique_leaves_the_other_shapes_on_the_matrix_cores(tmp_path):
    """A file of K2 to K4 sentences and one K7 sentence: the K7 bucket does not qualify for the shared-table kernels, and the
    library leaves it out of the grouped launches, not the call: K2 to K4 stay on the matrix cores and the K7 bucket's exact
    kernel runs behind them.  Statistics equal the per-bucket run's."""
    gold = _gold()
    k = [len(r['variables']) for r in gold['reference']]
    k7 = k.index(7)
    lines = [l for l, n in zip(gold['instances'], k) if 2 <= n <= 4] + [gold['instances'][k7]]
    paths = write_tidir(dict(gold, instances=lines), str(tmp_path))
    a, b = _trainer(paths, gold, grouped_sweeps=True), _trainer(paths, gold, grouped_sweeps=False)
    assert sorted({tr.topo.P for tr in a.trainers.values()}) == [1, 3, 6, 21]
    assert [tr.topo.plan(tr.roots[:tr.n_sweeps_run])['shared_ok'] for tr in a.trainers.values()].count(0) == 1
    K.reset()
    sa = a.local_statistics().cpu().numpy()
    _check_grouped_then_large(K.launched(), [len(key[1]) for key in a.trainers])
    np.testing.assert_allclose(sa, b.local_statistics().cpu().numpy(), rtol=1e-9, atol=1e-12)
