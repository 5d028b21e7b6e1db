"""Max-product sweeps and MAP decoding on the GPU (libmlbp_map.so) against the float64 NumPy walk of tests/test_map_cpu.py.

Tolerances: messages, max-marginals and scores rtol 1e-10 (products and maxima are exact; only the normalising sum is ordered
differently).  Assignments are compared exactly, except that a variable whose two largest max-marginal entries in the NumPy
walk differ by less than 1e-6 relative is left out (a last-bit difference may flip that argmax); how many graphs may hold such
a variable is capped per case, and the inputs were chosen so that the walk stays inside the cap.  The device score is compared
with the walk's score function evaluated at the DEVICE assignment, so a left-out variable does not loosen it.

Mutations these cases are built to catch: `fmax` turned into a sum in pair_mt_partial or pair_tm_rows (every parity case of the
X = 64 kernel compares messages at 1e-10) or in either orientation of the generic kernel (test_x128, test_x512,
test_small_x_equals_brute_force); the lowest index at the maximum turned into the highest (test_tie_rule_and_zero_table,
test_trainer_at_zero_thetas_decodes_word_zero); the two axes swapped in the score (every parity case with a pairwise factor:
the score is compared with the walk's at the device's own assignment)."""
import threading

import numpy as np
import pytest

import cases as C
import test_map_cpu as W
from helpers import batch_tables, tidir_gold, tidir_oracle_graph, write_tidir
from oracle import lbp_oracle as O

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

X64_RESIDENT = ('map_sweep_x64_kernel', (True,))       # P <= 3: tables in registers
X64_STREAMED = ('map_sweep_x64_kernel', (False,))
GENERIC = ('map_sweep_generic_kernel', ())
# kernel instance -> the tests that launch it (tests/test_map_cpu.py holds this against the library's symbol table)
CASES = {
    X64_RESIDENT: ['test_k3_unique_tables', 'test_k1', 'test_shared_tables_give_the_bits_of_unique_copies', 'test_batch_sizes',
                   'test_tie_rule_and_zero_table', 'test_capture_and_replay', 'test_tidir_decode_on_synthetic_sentences'],
    X64_STREAMED: ['test_k4', 'test_chain_equals_viterbi', 'test_ring', 'test_k7', 'test_tidir_decode_on_the_clique_fixture'],
    GENERIC: ['test_x128', 'test_x512', 'test_small_x_equals_brute_force', 'test_tidir_decode_on_the_clique_fixture'],
}
KERNEL_OF = {X64_RESIDENT: 1, X64_STREAMED: 1, GENERIC: 2}     # mlbp_map.h MLBP_MAP_KERNEL_*
NEAR_TIE = 1e-6


def _M():
    from macaronicusermodeling_amd import mapdecode
    return mapdecode


def _batch(spec, inputs_list, normalize=True, tables=None, pair_tab=None):
    from macaronicusermodeling_amd.batch import FactorGraphBatch
    from macaronicusermodeling_amd.topology import GraphTopology
    topo = GraphTopology.from_spec(spec)
    fb = FactorGraphBatch(topo, spec['X'], len(inputs_list), normalize_messages=normalize)
    pair, unary = batch_tables(spec, topo, inputs_list) if tables is None else tables
    if topo.P:
        fb.set_pair_tables(pair, pair_tab)
    if topo.U:
        fb.set_unary_tables(unary)
    return fb


def _run(fb, roots, init=True, keep_messages=True):
    mm = torch.full((fb.B, fb.topo.n_vars, fb.X), float('nan'), dtype=torch.float64, device=fb.device)
    x, score = fb.map_sweep(roots, init=init, max_marginals=mm, keep_messages=keep_messages)
    kernel = _M().last_kernel()
    torch.cuda.synchronize()
    return dict(x=x.cpu().numpy(), score=score.cpu().numpy(), mm=mm.cpu().numpy(), msgs=fb.msgs.cpu().numpy(), kernel=kernel)


def _compare(name, spec, topo, inputs_list, roots, got, graphs=None, may_omit=0, normalize=True, messages=True, ref=None):
    """Device results against the walk, graph by graph; returns the walks.  Prints the figures before it asserts.
    ref: {graph: walk} computed beforehand on the same inputs, roots and `normalize` (read, never written)."""
    keys = C.msg_keys(spec)
    omitted, min_gap, wrong, walks = 0, np.inf, [], {}
    for b in (range(len(inputs_list)) if graphs is None else graphs):
        w = walks[b] = W.walk(spec, inputs_list[b], roots, normalize=normalize) if ref is None else ref[b]
        if messages:
            np.testing.assert_allclose(got['msgs'][b], np.stack([w['msgs'][k] for k in keys]), rtol=1e-10, atol=1e-300, err_msg='%s graph %d' % (name, b))
        np.testing.assert_allclose(got['mm'][b], np.stack([w['mm'][v] for v in topo.var_ids]), rtol=1e-10, atol=1e-300, err_msg='%s graph %d' % (name, b))
        near = [v for v in topo.var_ids if w['gap'][v] < NEAR_TIE]
        omitted += bool(near)
        min_gap = min([min_gap] + [w['gap'][v] for v in topo.var_ids if v not in near])
        x_dev = {v: int(got['x'][b, i]) for i, v in enumerate(topo.var_ids)}
        wrong += [(b, v, x_dev[v], w['x'][v]) for v in topo.var_ids if v not in near and x_dev[v] != w['x'][v]]
        np.testing.assert_allclose(got['score'][b], W.score_of(w['g'], inputs_list[b], x_dev), rtol=1e-10, err_msg='%s graph %d' % (name, b))
    print('%s: %d graphs, %d with a left-out variable (cap %d), smallest compared gap %.2e, %d assignments differ'
          % (name, len(walks), omitted, may_omit, min_gap, len(wrong)))
    assert omitted <= may_omit, (name, omitted)
    assert not wrong, (name, wrong[:8])
    return walks


def _case(name, spec, seeds, roots, instance, may_omit=0, kind='uniform'):
    inputs = [C.make_inputs(spec, s, kind) for s in seeds]
    fb = _batch(spec, inputs)
    got = _run(fb, roots)
    assert got['kernel'] == KERNEL_OF[instance] == _M().pick_kernel(spec['X'], fb.topo.n_msgs, fb.topo.n_vars), name
    assert (fb.topo.P <= 3) == (instance != X64_STREAMED) or instance == GENERIC
    walks = _compare(name, spec, fb.topo, inputs, roots, got, may_omit=may_omit)
    return fb, inputs, got, walks


K3 = dict(spec=lambda: C.user_spec(10, [1, 4, 7], 64, 64, seed=1), seeds=range(500, 564), roots=[1, 4, 7])


def test_k3_unique_tables():
    _case('K3', K3['spec'](), K3['seeds'], K3['roots'], X64_RESIDENT)


def test_k1():
    fb, _, _, _ = _case('K1', C.user_spec(10, [4], 64, 64, seed=3), range(16), [4], X64_RESIDENT)
    assert fb.topo.P == 0


def test_k4():
    fb, _, _, _ = _case('K4', C.user_spec(10, [0, 2, 5, 8], 64, 64, seed=4), range(700, 732), [0, 2, 5], X64_STREAMED)
    assert fb.topo.P == 6


def _viterbi(spec, inputs):
    """Exact MAP of a chain by dynamic programming over the tables (products, as the potentials are)."""
    g = O.Graph(spec)
    n = len(spec['var_ids'])
    unary = [O.factor_table(g, inputs, g.by_id[i]).reshape(-1) for i in range(n)]
    pair = [O.factor_table(g, inputs, g.by_id[n + i]) for i in range(n - 1)]
    delta, back = unary[0], []
    for i in range(n - 1):
        cand = delta[:, None] * pair[i]
        back.append(cand.argmax(0))
        delta = cand.max(0) * unary[i + 1]
        delta = delta / delta.sum()
    x = [int(delta.argmax())]
    for bp in reversed(back):
        x.append(int(bp[x[-1]]))
    return x[::-1]


def test_chain_equals_viterbi():
    spec = C.chain_spec(8, 64)
    fb, inputs, got, _ = _case('chain8', spec, range(1, 33), [0], X64_STREAMED)
    for b, inp in enumerate(inputs):
        assert list(got['x'][b]) == _viterbi(spec, inp), b


@pytest.mark.parametrize('roots,may_omit', [([0, 3, 5], 2), ([0, 3, 5, 0, 3, 5, 0, 3, 5, 0], 4)], ids=['3_sweeps', '10_sweeps'])
def test_ring(roots, may_omit):
    """Max-product on a ring produces exact ties in some graphs: those variables are left out (capped), messages and
    max-marginals are compared on every graph."""
    _case('ring8/%d sweeps' % len(roots), C.ring_spec(8, 64), range(1, 33), roots, X64_STREAMED, may_omit=may_omit)


def test_k7():
    """126 message slots = 63 KB: inside the X = 64 kernel's LDS budget of mlbp_map.h (126 * 512 + 4608 + 4 * 8 <= 81920), with
    its 21 tables streamed per update."""
    M = _M()
    spec = C.user_spec(12, [0, 1, 3, 5, 7, 9, 11], 64, 64, seed=5)
    fb, _, _, _ = _case('K7', spec, range(800, 816), [0, 1, 3], X64_STREAMED)
    assert (fb.topo.n_msgs, fb.topo.P) == (126, 21) and 126 * 512 + 4608 + 4 * 8 <= M.X64_LDS_BYTES


def test_x128():
    _case('X128', C.user_spec(10, [1, 4, 7], 128, 128, seed=1), range(500, 516), [1, 4, 7], GENERIC)


def test_x512():
    _case('X512', C.ring_spec(8, 512), range(1, 5), [0, 3, 5], GENERIC)


def test_small_x_equals_brute_force():
    """The CPU module's tree cases on the device: the assignment is the brute-force MAP."""
    todo = [(name, make(), [C.make_inputs(make(), s, kind) for s in range(40)], roots) for name, make, roots, kind in W.TREE_CASES]
    todo += [(s['name'], s, [C.make_inputs(s, i)], [s['var_ids'][0]]) for i, s in enumerate(W.random_trees())]
    for name, spec, inputs, roots in todo:
        fb = _batch(spec, inputs)
        got = _run(fb, roots)
        assert got['kernel'] == KERNEL_OF[GENERIC]
        _compare(name, spec, fb.topo, inputs, roots, got)
        for b, inp in enumerate(inputs):
            x, best, _ = W.brute_force(O.Graph(spec), inp)
            assert [int(v) for v in got['x'][b]] == [x[v] for v in fb.topo.var_ids], (name, b)
            np.testing.assert_allclose(got['score'][b], best, rtol=1e-10)


def test_shared_tables_give_the_bits_of_unique_copies():
    """The K3 case with two tables behind every graph through pair_tab == the same tables passed as unique copies, bit for bit."""
    spec = K3['spec']()
    inputs = [C.make_inputs(spec, s) for s in K3['seeds']]
    B = len(inputs)
    fb_u = _batch(spec, inputs)
    two = fb_u.pair_tables[:2].clone()
    tab = np.tile(np.array([[0, 1, 0]]), (B, 1))
    tab[1::2] = [1, 1, 0]
    unary = fb_u.unary_tables
    fb_s = _batch(spec, inputs, tables=(two, unary), pair_tab=tab)
    fb_c = _batch(spec, inputs, tables=(two[torch.from_numpy(tab.reshape(-1)).to(two.device)], unary))
    a, b = _run(fb_s, K3['roots']), _run(fb_c, K3['roots'])
    assert a['kernel'] == b['kernel'] == 1
    for k in ('x', 'score', 'mm', 'msgs'):
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a['x'], _run(fb_u, K3['roots'])['x'])          # (other tables, other answers)


def test_tie_rule_and_zero_table():
    """All-ones tables tie everywhere: assignment 0 for every variable (X = 64 and generic).  An all-zero pairwise table gives the
    uniform message, as the walk says."""
    for spec in (K3['spec'](), C.user_spec(10, [1, 4, 7], 128, 128, seed=1), C.chain_spec(5, 8)):
        X = spec['X']
        inputs = [C.make_inputs(spec, 1)] * 3
        fb = _batch(spec, inputs)
        fb.pair_tables.fill_(1.0)
        fb.unary_tables.fill_(1.0)
        got = _run(fb, [spec['var_ids'][0]] * 2)
        assert (got['x'] == 0).all() and np.allclose(got['mm'], 1.0 / X, rtol=1e-12) and np.array_equal(got['score'], np.zeros(3))
    spec = K3['spec']()
    inputs = [C.make_inputs(spec, s) for s in (500, 501)]
    for inp in inputs:
        inp['pot_en_en'] = np.zeros_like(inp['pot_en_en'])         # the gap > 1 table: all three pairwise factors of (1, 4, 7)
    fb = _batch(spec, inputs)
    got = _run(fb, K3['roots'])
    topo = fb.topo
    _compare('K3 zero table', spec, topo, inputs, K3['roots'], got)
    for j in topo.pair_factors:
        for k in range(2):
            assert np.array_equal(got['msgs'][:, topo.f2v[2 * j + k]], np.full((2, 64), 1.0 / 64))
    assert np.isneginf(got['score']).all()


def test_init_false_keep_messages_and_unnormalised():
    spec = K3['spec']()
    inputs = [C.make_inputs(spec, s) for s in range(500, 508)]
    fb = _batch(spec, inputs)
    whole = _run(fb, [1, 4, 7])
    _run(fb, [1], init=True)
    rest = _run(fb, [4, 7], init=False)
    for k in ('x', 'score', 'mm', 'msgs'):
        assert np.array_equal(whole[k], rest[k]), k
    fb.msgs.fill_(float('nan'))
    dropped = _run(fb, [1, 4, 7], keep_messages=False)
    for k in ('x', 'score', 'mm'):
        assert np.array_equal(whole[k], dropped[k]), k
    # X = 128: the generic kernel keeps its messages in self.msgs either way
    spec_g = C.user_spec(10, [1, 4, 7], 128, 128, seed=1)
    inputs_g = [C.make_inputs(spec_g, s) for s in (500, 501)]
    fb_g = _batch(spec_g, inputs_g)
    whole_g = _run(fb_g, [1, 4, 7])
    _run(fb_g, [1, 4], init=True)
    rest_g = _run(fb_g, [7], init=False, keep_messages=False)
    for k in ('x', 'score', 'mm'):
        assert np.array_equal(whole_g[k], rest_g[k]), k
    # normalize_messages=False: the walk run without normalisation
    for sp, inp in ((spec, inputs), (spec_g, inputs_g)):
        fb_n = _batch(sp, inp, normalize=False)
        got = _run(fb_n, [1, 4, 7])
        _compare('unnormalised X=%d' % sp['X'], sp, fb_n.topo, inp, [1, 4, 7], got, normalize=False)


@pytest.mark.parametrize('B', [1, 333, 8192 + 19])
def test_batch_sizes(B):
    """Grid tails: every graph of the batch is computed (the large one is checked on 16 sampled graphs, the last included)."""
    spec = K3['spec']()
    distinct = [C.make_inputs(spec, s) for s in K3['seeds']]
    inputs = [distinct[b % len(distinct)] for b in range(B)]
    fb = _batch(spec, inputs)
    got = _run(fb, K3['roots'])
    graphs = None if B <= 333 else sorted(set(np.random.RandomState(B).randint(0, B, size=14).tolist()) | {0, B - 1})
    _compare('K3 B=%d' % B, spec, fb.topo, inputs, K3['roots'], got, graphs=graphs if B > 64 else None)
    n = len(distinct)
    for k in ('x', 'score', 'mm'):                    # every graph: equal inputs give equal bits
        assert np.array_equal(got[k][n:], got[k][np.arange(n, B) % n]), k
    assert (got['x'] >= 0).all() and np.isfinite(got['score']).all()


def test_out_of_range_table_index_is_refused_by_python():
    spec = K3['spec']()
    inputs = [C.make_inputs(spec, 500)]
    fb = _batch(spec, inputs)
    with pytest.raises(IndexError):
        fb.set_pair_tables(fb.pair_tables, np.array([[0, 1, 3]]))
    fb32 = _batch(C.user_spec(10, [1, 4, 7], 256, 64, seed=1), [C.make_inputs(C.user_spec(10, [1, 4, 7], 256, 64, seed=1), 1)])
    fb32.set_pair_tables(fb32.pair_tables, dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        fb32.map_sweep([1])
    fb.use_approx_inference = True
    with pytest.raises(NotImplementedError):
        fb.map_sweep([1])


def test_capture_and_replay():
    """map_sweep recorded in a HIP graph on one stream after an eager warm-up, replayed twice with the tables overwritten in
    place between the replays: the outputs follow the tables."""
    spec = K3['spec']()
    first = [C.make_inputs(spec, s) for s in range(500, 508)]
    second = [C.make_inputs(spec, s) for s in range(540, 548)]
    fb = _batch(spec, first)
    other = _batch(spec, second)
    mm = torch.empty(fb.B, fb.topo.n_vars, 64, dtype=torch.float64, device=fb.device)
    fb.map_sweep(K3['roots'], max_marginals=mm)                                   # eager warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x, score = fb.map_sweep(K3['roots'], max_marginals=mm)
    for inputs, src in ((first, fb), (second, other), (first, None)):
        if src is other:
            fb.pair_tables.copy_(other.pair_tables)
            fb.unary_tables.copy_(other.unary_tables)
        elif src is None:
            pair, unary = batch_tables(spec, fb.topo, first)
            fb.pair_tables.copy_(torch.from_numpy(pair))
            fb.unary_tables.copy_(torch.from_numpy(unary))
        x.fill_(-7); score.fill_(float('nan')); mm.fill_(float('nan')); fb.msgs.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        got = dict(x=x.cpu().numpy(), score=score.cpu().numpy(), mm=mm.cpu().numpy(), msgs=fb.msgs.cpu().numpy())
        _compare('K3 replay', spec, fb.topo, inputs, K3['roots'], got)


def test_two_threads_on_two_streams():
    """Two threads, each on a stream of its own with its own inputs and shape, each get their own results and their own record
    of the kernel that ran."""
    M = _M()
    jobs = [(K3['spec'](), range(500, 516), K3['roots'], 1), (C.user_spec(10, [1, 4, 7], 128, 128, seed=1), range(500, 504), [1, 4, 7], 2)]
    out, errors = {}, []

    def work(i):
        try:
            spec, seeds, roots, kernel = jobs[i]
            inputs = [C.make_inputs(spec, s) for s in seeds]
            with torch.cuda.stream(torch.cuda.Stream()):
                fb = _batch(spec, inputs)
                runs = []
                for _ in range(5):
                    runs.append(_run(fb, roots))
                    assert M.last_kernel() == kernel
            out[i] = (spec, fb.topo, inputs, roots, runs)
        except Exception as e:              # noqa: BLE001  (re-raised on the main thread)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    for i in range(2):
        spec, topo, inputs, roots, runs = out[i]
        _compare('thread %d' % i, spec, topo, inputs, roots, runs[0])
        for r in runs[1:]:
            for k in ('x', 'score', 'mm', 'msgs'):
                assert np.array_equal(r[k], runs[0][k]), (i, k)


# ---- trainers -------------------------------------------------------------------------------------
def _check_decode(name, tt, phi, th_ee, th_ed, guesses, counts):
    """TiDirTrainer.decode() against the walk on every instance's own graph (three sweeps when it is loopy, one when it is a
    tree, as the trainer runs them); counts recomputed from the instances' labels.  No word may be left out."""
    phi_ee, phi_w1, phi_ed = phi
    want_counts, min_gap, seen, kernels = np.zeros(4, dtype=np.int64), np.inf, 0, set()
    for key, b in sorted(tt.buckets.items()):
        for i, row in enumerate(b['rows']):
            g, inputs, roots, _ = tidir_oracle_graph(key, b, i, phi_ee, phi_w1, phi_ed, th_ee, th_ed)
            n = 3 if O.has_loops(g, roots[0]) else 1
            w = W.walk(g.spec, inputs, roots[:n])
            positions, words, score = guesses[row['index']]
            assert positions == tuple(key[1]) == tuple(g.var_order)
            min_gap = min([min_gap] + list(w['gap'].values()))
            assert words == [tt.en[w['x'][v]] for v in key[1]], (name, row['index'], w['gap'])
            np.testing.assert_allclose(score, w['score'], rtol=1e-10)
            hit = [w['x'][v] == int(b['var_labels'][i][k]) for k, v in enumerate(key[1])]
            want_counts += np.array([all(hit), 1, sum(hit), len(hit)])
            seen += 1
    print('%s: %d sentences, %d predicted words, smallest gap of the walk %.2e, counts %s' % (name, seen, want_counts[3], min_gap, counts))
    assert min_gap >= NEAR_TIE                                  # no word may be left out
    assert tuple(int(v) for v in want_counts) == tuple(counts)
    return seen, want_counts


def test_tidir_decode_on_the_clique_fixture(tmp_path):
    """K1 to K12 at X = 64 at the fixture's own thetas.  Every bucket runs the kernel the header's rule names: the X = 64 kernel
    with its tables in registers (K1 to K3) or streamed (K4 and up, while the message slots fit its LDS budget), the generic
    kernel beyond that."""
    from macaronicusermodeling_amd import tidir
    from test_gpu_cliques import _trainer
    M = _M()
    gold = tidir_gold('tidir_cliques_reference')
    paths = write_tidir(gold, str(tmp_path))
    tt = _trainer(paths, gold)
    guesses, counts = tt.decode()
    phi = tidir.load_features(paths['phi.pmi'], paths['phi.pmi_w1'], paths['phi.ed'], paths['phi.ped'])
    seen, want = _check_decode('clique fixture', tt, phi, np.array(gold['theta_en_en']).reshape(1, -1),
                               np.array(gold['theta_en_de']).reshape(1, -1), guesses, counts)
    assert (seen, int(want[3])) == (11, 67)
    ran = set()
    for key, tr in tt.trainers.items():
        tr.decode()
        assert M.last_kernel() == M.pick_kernel(64, tr.topo.n_msgs, tr.topo.n_vars)
        ran.add((M.last_kernel(), tr.topo.P <= 3))
    assert ran == {(1, True), (1, False), (2, False)}
    x, score = tt.trainers[next(iter(tt.trainers))].decode()
    assert x.dtype == np.int64 and score.dtype == np.float64 and x.shape[0] == score.shape[0]


def _synthetic(tmp_path):
    from macaronicusermodeling_amd import tidir
    from macaronicusermodeling_amd.train import TiDirTrainer
    paths = tidir.synthesize(str(tmp_path), n_instances=60, X=64, Vde=64, sent_len=(5, 7), n_predicted=(1, 4), seed=5)
    tt = TiDirTrainer(paths['ti'], paths['end'], paths['ded'], paths['phi_pmi'], paths['phi_pmi_w1'], paths['phi_ed'], paths['phi_ped'], sweeps=3)
    phi = tidir.load_features(paths['phi_pmi'], paths['phi_pmi_w1'], paths['phi_ed'], paths['phi_ped'])
    return tt, phi


def test_tidir_decode_on_synthetic_sentences(tmp_path):
    tt, phi = _synthetic(tmp_path)
    rs = np.random.RandomState(1)
    th_ee, th_ed = rs.randn(1, 3) * 0.3, rs.randn(1, 6) * 0.3
    tt.theta_en_en.copy_(torch.from_numpy(th_ee.reshape(-1)))
    tt.theta_en_de.copy_(torch.from_numpy(th_ed.reshape(-1)))
    guesses, counts = tt.decode()
    seen, want = _check_decode('synthetic', tt, phi, th_ee, th_ed, guesses, counts)
    assert (len(tt.buckets), int(want[3])) == (52, 162) and seen == len(guesses) == 60
    # predict() still ranks every word on its own; decode() answers the joint question and leaves predict() as it was
    lp, c = tt.predict()
    assert c[3] == 162 and np.isfinite(lp)


def test_trainer_at_zero_thetas_decodes_word_zero(tmp_path):
    """Zero thetas: every potential is 1, every max-marginal exactly uniform, so every predicted word ties over the whole
    vocabulary and the tie rule gives word index 0 -- at trainer level."""
    tt, _ = _synthetic(tmp_path)
    guesses, counts = tt.decode()
    n_words = 0
    for key, b in tt.buckets.items():
        for row in b['rows']:
            positions, words, score = guesses[row['index']]
            assert words == [tt.en[0]] * len(key[1]) and score == 0.0
            n_words += len(words)
    assert n_words == 162
    labels = np.concatenate([b['var_labels'].reshape(-1) for b in tt.buckets.values()])
    assert counts[3] == 162 and counts[2] == int((labels == 0).sum()) and counts[1] == 60
