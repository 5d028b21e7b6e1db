"""bench.py --dump-outputs on host tensors: the byte budget, the seeded graph sample shared by every per-graph array, and
the same files from run to run.  Runs without a GPU."""
import os

import numpy as np
import torch

import bench


def _outputs(B, n_msgs=36, n_vars=3, X=64):
    g = torch.Generator().manual_seed(3)
    per_graph = {'marginals': torch.rand(B, n_vars, X, dtype=torch.float64, generator=g),
                 'log_posterior': torch.rand(B, dtype=torch.float64, generator=g),
                 'messages': torch.rand(B, n_msgs, X, dtype=torch.float64, generator=g)}
    return per_graph, {'log_posterior_total': torch.rand(1, dtype=torch.float64, generator=g)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_a_large_batch_is_sampled_under_the_budget_and_the_same_every_run(tmp_path):
    per_graph, whole = _outputs(8192)
    bench.dump_outputs(str(tmp_path / 'a'), per_graph, whole)
    bench.dump_outputs(str(tmp_path / 'b'), per_graph, whole)
    a, b = _load(str(tmp_path / 'a')), _load(str(tmp_path / 'b'))
    assert sorted(a) == ['log_posterior', 'log_posterior_total', 'marginals', 'messages']
    assert sum(os.path.getsize(str(tmp_path / 'a' / f)) for f in os.listdir(str(tmp_path / 'a'))) <= bench.DUMP_BYTES
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k])
    n = a['marginals'].shape[0]
    assert 1000 < n < 8192
    idx = np.sort(np.random.RandomState(bench.DUMP_SAMPLE_SEED).choice(8192, n, replace=False))
    for k, t in per_graph.items():
        np.testing.assert_array_equal(a[k], t.numpy()[idx])
    np.testing.assert_array_equal(a['log_posterior_total'], whole['log_posterior_total'].numpy())


def test_a_small_batch_is_written_whole(tmp_path):
    per_graph, whole = _outputs(64)
    bench.dump_outputs(str(tmp_path), per_graph, whole)
    got = _load(str(tmp_path))
    for k, t in per_graph.items():
        np.testing.assert_array_equal(got[k], t.numpy())
