"""tests/knn_host.py against the existing oracles: the same edges on random inputs (no ties: the tie rule is idle), different
edges on the tied lattice inputs of the GPU tests -- cdist(...).topk(...) does not order equal distances by index, which is
why a tied input needs the stable reference."""
import numpy as np
import pytest
import torch

import knn_host as K
from gnnmp import graph_build
from oracle import ref_cpu

# (N, C, k1): the shapes of tests/test_graph_build_edges_gpu.py at which the two orders were seen to differ
TIED = [(100, 2, 6), (1100, 2, 5), (2100, 2, 4), (2300, 3, 19)]


@pytest.mark.parametrize('n,C,k1,n_free', [(500, 2, 6, 250), (333, 3, 9, 150), (90, 7, 16, 45), (12, 2, 6, 4), (3, 2, 8, 3),
                                           (1100, 14, 5, 1100)])
def test_equals_the_oracles_on_random_inputs(n, C, k1, n_free):
    v = torch.rand(n, C, generator=torch.Generator().manual_seed(n + C)) * 2 - 1
    mine = K.build_edges_stable(v, n_free, k1)
    assert torch.equal(mine, ref_cpu.build_edges(v, n_free, k1))
    assert torch.equal(mine, graph_build.build_edges(v, n_free, k1))
    assert not K.has_tie_at_kth(v, k1).any()


@pytest.mark.parametrize('n,C,k1', TIED)
def test_differs_from_the_oracles_on_tied_inputs(n, C, k1):
    v = K.tied(n, C, seed=n)
    assert K.has_tie_at_kth(v, k1).any()
    mine = K.build_edges_stable(v, n // 2, k1)
    for other in (ref_cpu.build_edges(v, n // 2, k1), graph_build.build_edges(v, n // 2, k1)):
        assert mine.shape != other.shape or not torch.equal(mine, other)


def test_knn_stable_is_the_lower_index_rule():
    # three points in a line: 1 and 2 are equidistant from 0; two copies of one point: the lower index first, itself or not
    x = torch.tensor([[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [1.0, 0.0]])
    assert K.knn_stable(x, 3).tolist() == [[0, 1, 2], [1, 3, 0], [2, 0, 1], [1, 3, 0]]
    assert K.argmin_stable32(x, torch.tensor([0.5, 7.0])) == 0           # rows 0, 1 and 3 at the same distance
    assert K.argmin_stable32(x[1:], torch.tensor([1.0, 1.0])) == 0


def test_bucket_sizes_count_the_columns_before_coalescing():
    v = K.tied(100, 2, seed=3)
    for n_free, k1 in [(50, 6), (0, 3), (100, 1), (130, 200)]:
        f, k = min(n_free, 100), min(k1, 100)
        b = K.bucket_sizes(v, n_free, k1)
        assert b.sum() == 2 * (100 * k + f * min(k1, f))
        # every source keeps at most its bucket and at least one column (its self loop)
        src = K.build_edges_stable(v, n_free, k1)[0].numpy()
        u = np.bincount(src, minlength=100)
        assert (u <= b).all() and (u >= 1).all()


def test_lattice_is_exact_and_duplicated():
    x = K.lattice(300, 3, 0.125, 1, 4)
    assert x.dtype == torch.float32 and tuple(x.shape) == (300, 3)
    assert torch.equal(x * 8, (x * 8).round()) and x.abs().max() <= 8
    assert len({tuple(r) for r in x.tolist()}) in range(296, 300)          # up to 4 rows are copies
    d = K.sqdist64(x, x)
    assert np.array_equal(d, d.astype(np.float32).astype(np.float64))
    assert torch.equal(x, K.lattice(300, 3, 0.125, 1, 4))
    dense = K.lattice(500, 2, 0.25, 2, 0, side=4)
    assert len({tuple(r) for r in dense.tolist()}) == 16
    assert tuple(K.lattice(0, 2, 0.125, 1, 0).shape) == (0, 2) and tuple(K.tied(1, 2, 5).shape) == (1, 2)
