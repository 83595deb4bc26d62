"""The graph builder (csrc/graph_kernels.hip) at every size at which it changes form, on TIED inputs as well as random ones.

Reference: tests/knn_host.py -- float64 squared distances from the float32 coordinates, stable (distance, index) order -- so
the documented tie rule (the lower index wins on equal distance) is part of what is compared: columns and edge_ptr must be
identical (integer results, bit-exact bar).  The tied inputs are dyadic lattice points with duplicated rows, on which the
oracle's cdist(...).topk(...) picks other neighbours (tests/test_knn_host.py); every tied case first asserts on the host
that some node really has a tie at its k-th neighbour.

Forms of gb_knn, by candidate count M (N in the pass over all nodes, min(n_free, N) in the pass over the free ones):
  graph of N <= 1024 nodes   first launch, 16 distances per lane in registers, both passes from one set of distances
  N > 1024                   node listed for the second launch; per pass: M <= 2048 32 distances per lane in registers,
                             M > 2048 and k <= 16 streamed per-lane top-16, M > 2048 and k > 16 recompute per round
gb_unique: a source's bucket of up to cap = max(256, 8 k1_max) entries is rank-sorted in LDS, a larger one in place.
"""
import numpy as np
import pytest
import torch

import knn_host as K
from gnnmp import graph_build

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ['tied', 'random']


def _points(kind, n, C, seed):
    if kind == 'tied':
        return K.tied(n, C, seed)
    return torch.rand(n, C, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _check(vs, nf, k1, tied=False):
    """build_edges_gpu on the ragged batch against build_edges_stable per graph: same columns, same edge_ptr."""
    if tied:
        for v, k in zip(vs, k1):
            if 1 < k < v.shape[0] and v.shape[0] >= 16:
                assert K.has_tie_at_kth(v, k).any()            # the tie rule decides a neighbour in this graph
    ptr = torch.zeros(len(vs) + 1, dtype=torch.int32)
    ptr[1:] = torch.tensor([v.shape[0] for v in vs]).cumsum(0).to(torch.int32)
    ei, eptr = graph_build.build_edges_gpu(torch.cat(vs).to(DEV), ptr.to(DEV), nf, k1)
    eptr = eptr.cpu().tolist()
    ei = ei.cpu()
    assert eptr[0] == 0 and eptr[-1] == ei.shape[1]
    for g, v in enumerate(vs):
        ref = K.build_edges_stable(v, nf[g], k1[g])
        assert eptr[g + 1] - eptr[g] == ref.shape[1], (g, eptr[g + 1] - eptr[g], ref.shape[1])
        mine = ei[:, eptr[g]:eptr[g + 1]]
        assert torch.equal(mine, ref), (g, int((mine != ref).any(0).sum()))


@pytest.mark.parametrize('kind', KINDS)
def test_kernel_switch_at_1024_nodes(kind):
    """1023 and 1024 nodes: the first launch; 1025: listed for the second one (32 distances per lane)."""
    vs = [_points(kind, n, 2, 10 + i) for i, n in enumerate((1023, 1024, 1025))]
    _check(vs, [500, 1024, 513], [6, 5, 4], kind == 'tied')


@pytest.mark.parametrize('kind', KINDS)
def test_second_launch_with_an_empty_list_and_large_graph_last(kind):
    """More than 1024 nodes in the batch but no graph above 1024: the second kNN launch runs and finds nothing listed.
    Then a batch whose only large graph comes last (its nodes are listed by the last workgroups of the first launch)."""
    _check([_points(kind, 600, 2, 20), _points(kind, 500, 2, 21)], [300, 500], [5, 7], kind == 'tied')
    _check([_points(kind, 300, 2, 22), _points(kind, 40, 2, 23), _points(kind, 1100, 2, 24)], [100, 40, 600], [4, 3, 5],
           kind == 'tied')


@pytest.mark.parametrize('k1', [5, 16, 17])
@pytest.mark.parametrize('kind', KINDS)
def test_register_limit_2048(kind, k1):
    """2047 and 2048 candidates: 32 per lane in registers (2048 fills the last slot of every lane); 2049: streamed top-16 at
    k1 = 5 and 16, recompute per round at k1 = 17.  The free pass of the second graph is at the limit too, the third graph's
    beyond it."""
    C = 3 if k1 == 17 else 2
    vs = [_points(kind, n, C, 30 + i) for i, n in enumerate((2047, 2048, 2049))]
    _check(vs, [1000, 2048, 2049], [k1] * 3, kind == 'tied')


@pytest.mark.parametrize('n_free', [(0, 1, 1000, 1024), (1025, 2048, 2049, 2100)])
@pytest.mark.parametrize('k1', [5, 17])
@pytest.mark.parametrize('kind', KINDS)
def test_pass_split(kind, k1, n_free):
    """2100 nodes: the pass over all nodes streams (k1 = 5) or recomputes (k1 = 17); the pass over the free ones has
    n_free candidates, so up to 2048 the same node runs the register form there, beyond it the first pass's form again.
    Nodes i >= n_free have no free-pass neighbours (n_free = 0: nobody has): the reference's edges hold only what they
    should, and any extra neighbour would add columns."""
    v = _points(kind, 2100, 2, 40)
    _check([v] * len(n_free), list(n_free), [k1] * len(n_free), kind == 'tied')


def _dense_tied(M):
    """A dense lattice input (12 x 12 points, 16 rows per point on average) in which lane 7 of a wave (candidates 7, 71, ...)
    meets 20 copies of one point x in its first 20 trips and lane 9 20 more later; and three copies of a point y, 1/16 beside
    x and nearer to x than to anything else: row 100 and, in lane 7 BEHIND its copies of x, rows 1607 and 1927."""
    v = K.lattice(M, 2, 0.125, 50 + M, 2, side=12)
    x = torch.tensor([0.125, -0.25])
    for j in range(20):
        v[64 * j + 7] = x
        v[64 * (j + 15) + 9] = x
    for i in (100, 64 * 25 + 7, 64 * 30 + 7):
        v[i] = x + torch.tensor([0.0625, 0.0])
    return v


@pytest.mark.parametrize('k1', [16, 17])
@pytest.mark.parametrize('M', [2304, 2305])
def test_streaming_trip(M, k1):
    """2304 = 9 trips of 4 x 64 candidates exactly, 2305 = one candidate in a tenth trip; k1 = 16 is the streamed per-lane
    top-16, k1 = 17 the recompute form.  Host-side conditions on the input: (a) seen from x, one lane holds more than 16
    candidates at the k-th distance (0); (b) seen from y, the k-th distance is that of x, lane 7 holds more than 16
    candidates at it, and two NEARER candidates (y itself) reach lane 7 after them -- a per-lane list is full of entries at
    one distance when a closer one arrives, and must give up its highest index at that distance, not its lowest (the
    streamed form did the latter until its insertion was fixed: rows 7 and 71 were missing from y's neighbours)."""
    v = _dense_tied(M)
    d = K.sqdist64(v[7:8], v)[0]
    at_kth = np.flatnonzero(d == np.sort(d)[k1 - 1])
    assert np.bincount(at_kth % 64, minlength=64).max() > 16 and at_kth.size > k1
    d = K.sqdist64(v[100:101], v)[0]
    kth = np.sort(d)[k1 - 1]
    lane7 = np.arange(7, M, 64)
    assert kth == 0.0625 ** 2 and (d < kth).sum() == 3
    assert (d[lane7] == kth).sum() > 16 and (d[lane7[17:]] < kth).sum() == 2 and (d[lane7[:17]] == kth).all()
    assert {7, 71} <= set(K.knn_stable(v, k1)[100].tolist())
    _check([v], [2250], [k1], True)
    _check([_points('random', M, 2, 60 + M)], [M], [k1])


@pytest.mark.parametrize('kind', KINDS)
def test_lane_edges_and_degenerate_graphs(kind):
    """1, 63, 64 and 65 nodes (one lane short of, exactly, and one past a wave's first slot); k1 = 1 (self loops only);
    k1 >= N (everybody is everybody's neighbour); n_free > N (clamped) and n_free = 0."""
    vs = [_points(kind, n, 2, 70 + i) for i, n in enumerate((1, 63, 64, 65))]
    tied = kind == 'tied'
    _check(vs, [1, 30, 64, 33], [3, 2, 4, 5], tied)
    _check(vs, [1, 30, 0, 65], [1, 1, 1, 1], tied)
    _check(vs, [5, 100, 64, 1000], [1, 63, 70, 65], tied)


@pytest.mark.parametrize('kind', KINDS)
def test_empty_graphs_in_a_batch(kind):
    """gnnmp.h puts no lower bound on a graph's node count: a graph of zero nodes, first, in the middle and last, has no
    edges (edge_ptr repeats) and does not disturb its neighbours in the batch."""
    sizes = (0, 50, 0, 0, 70, 0)
    vs = [_points(kind, n, 2, 80 + i) for i, n in enumerate(sizes)]
    _check(vs, [0, 25, 3, 0, 70, 1], [4, 4, 2, 1, 6, 3], kind == 'tied')


def _star(n, seed):
    """The hub construction: node 5 at the origin, the others on the unit sphere (pairwise ~ sqrt(2), the hub at 1), so at
    k1 = 2 the hub is the second neighbour of every node.  64 dimensions: in 7, a few hundred points on the sphere have
    neighbours closer than the hub and its bucket stays small."""
    x = torch.randn(n, 64, generator=torch.Generator().manual_seed(seed))
    x = x / x.norm(dim=1, keepdim=True)
    x[5] = 0.0
    return x


@pytest.mark.parametrize('k1_max', [2, 33])
def test_unique_stage_at_its_cap(k1_max):
    """gb_unique sorts a bucket of up to cap entries in LDS and a larger one in place: the hub's bucket at cap - 1, cap and
    cap + 1 entries (sizes found and asserted on the host), cap = 256 at k1_max = 2 and 264 at k1_max = 33 (a companion graph
    with k1 = 33 in the batch moves the boundary; the stars keep k1 = 2)."""
    cap = max(256, 8 * k1_max)
    vs, nf = [], []
    for target in (cap - 1, cap, cap + 1):
        found = None
        for n in range(150, 160):
            v = _star(n, 90 + n)
            for f in range(target - n - 6, target - n + 12):                 # hub bucket ~ n + n_free + 4
                if 6 <= f <= n and K.bucket_sizes(v, f, 2)[5] == target:
                    found = (v, f)
                    break
            if found:
                break
        assert found is not None, target
        b = K.bucket_sizes(found[0], found[1], 2)
        assert b[5] == target and np.delete(b, 5).max() < cap - 1            # the hub alone is at the boundary
        vs.append(found[0])
        nf.append(found[1])
    k1 = [2, 2, 2]
    if k1_max > 2:
        vs.append(torch.rand(40, 64, generator=torch.Generator().manual_seed(99)))
        nf.append(20)
        k1.append(k1_max)
    _check(vs, nf, k1)


@pytest.mark.parametrize('kind', KINDS)
def test_large_k1(kind):
    """k1_max >= 257: gb_unique's LDS request (32 bytes x 8 k1_max) passes 64 KB, for which the launch raises the kernel's
    dynamic-LDS limit first, as the other kernels with large LDS do.  300 nodes at k1 = 260."""
    _check([_points(kind, 300, 2, 100)], [150], [260], kind == 'tied')
