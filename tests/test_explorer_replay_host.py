"""The host side of gnnmp.explorer_replay, no GPU: the schedule against a literal restatement of the reference's loop
(train_explorer.py:120-204), the float64 loss against the reference's expression on a dense policy, and the dataset's draws
against the reference's numpy call order (algorithm/dijkstra.py:94, MazeEnv.uniform_sample)."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import explorer_replay as er


def reference_loop(epoch, iters, seed):
    """train_explorer.py:120-204 with everything but the loop order taken out: which samples are backpropagated before which
    ``optimizer.step()``.  No sample is skipped (the `continue` lines do not fire)."""
    np.random.seed(seed)
    T = 0
    steps, pending = [], []
    for iter_i in range(iters):
        indexes = np.random.permutation(epoch)
        for index in indexes:
            pending.append(int(index))               # loss.backward()
            if T % 8 == 0:
                steps.append(pending)                # optimizer.step(); optimizer.zero_grad()
                pending = []
            T += 1
    return steps, pending


@pytest.mark.parametrize('n, iters, sizes, n_dropped', [(11, 3, [1, 8, 8, 8, 8], 0), (5, 2, [1, 8], 1)])
def test_schedule_is_the_reference_loop(n, iters, sizes, n_dropped):
    groups, dropped = er.explorer_schedule(n, iters=iters, group=8, rng=np.random.RandomState(77))
    steps, pending = reference_loop(n, iters, 77)
    assert [len(g) for g in groups] == sizes == [len(s) for s in steps]
    assert len(dropped) == n_dropped == len(pending)
    for g, s in zip(groups, steps):
        assert g.dtype == np.int64 and g.tolist() == s
    assert dropped.tolist() == pending
    # every sample of every permutation is there once, in order
    flat = [i for g in groups for i in g.tolist()] + dropped.tolist()
    rng = np.random.RandomState(77)
    assert flat == [int(i) for _ in range(iters) for i in rng.permutation(n)]


def test_schedule_default_generator_is_1234():
    a, da = er.explorer_schedule(9, iters=2)
    b, db = er.explorer_schedule(9, iters=2, rng=np.random.RandomState(1234))
    assert [g.tolist() for g in a] == [g.tolist() for g in b] and da.tolist() == db.tolist()


def _handmade():
    """Three dense little graphs with hand-made frontiers, as the dict of episodes.policy_frontier on the host."""
    gen = torch.Generator().manual_seed(5)
    sizes = [4, 3, 5, 2, 3, 2]
    eis, eptr = [], [0]
    for N in sizes:                                   # every ordered pair, self loops included: E = N^2
        src, dst = torch.meshgrid(torch.arange(N), torch.arange(N), indexing='ij')
        eis.append(torch.stack([src.reshape(-1), dst.reshape(-1)]))
        eptr.append(eptr[-1] + N * N)
    E, B = eptr[-1], len(sizes)
    scores = (torch.rand(E, generator=gen) * 44 - 32).float()
    lists = [[3, 1, 7, 12, 1],                        # edge 1 twice, the label at position 2
             [4],                                     # one entry: loss 0
             [0, 24, 5, 6, 7, 8, 9],                  # the label at the last position
             [1, 2], [0, 1, 2], [1, 3]]               # status != 0, frontier_len == 0, label == -1
    label = [2, 0, 6, 0, 0, -1]
    status = [0, 0, 0, 2, 0, 0]
    flen = [len(x) for x in lists]
    flen[4] = 0
    frontier = torch.full((2 * E + B,), -7, dtype=torch.int32)
    for b, ids in enumerate(lists):
        off = 2 * eptr[b] + b
        frontier[off:off + len(ids)] = torch.tensor(ids, dtype=torch.int32) + eptr[b]
    fr = {'frontier': frontier, 'frontier_len': torch.tensor(flen, dtype=torch.int32), 'label': torch.tensor(label, dtype=torch.int32),
          'status': torch.tensor(status, dtype=torch.int32), 'edge_ptr': torch.tensor(eptr, dtype=torch.int32), 'total_edges': E}
    return sizes, eis, eptr, scores, lists, label, fr


def test_reference_loss_is_the_reference_expression():
    sizes, eis, eptr, scores, lists, label, fr = _handmade()
    s64 = scores.double().requires_grad_(True)
    loss, terms, counted = er.frontier_loss_reference(s64, fr, divisor=2.0)
    assert counted.tolist() == [True, True, True, False, False, False]
    want = []
    for b in range(3):
        N, ei = sizes[b], eis[b]
        sb = s64[eptr[b]:eptr[b + 1]]
        P = sb.new_zeros(N, N).index_put((ei[1], ei[0]), sb)              # the dense policy: P[target, source]
        ids = torch.tensor(lists[b])
        frontier = (ei[1][ids], ei[0][ids])
        want.append(-P[frontier].log_softmax(dim=0)[label[b]])           # train_explorer.py:172
    want = torch.stack(want)
    assert terms.dtype == torch.float64 and torch.equal(terms[3:], torch.zeros(3, dtype=torch.float64))
    assert float((terms[:3] - want).detach().abs().max()) <= 1e-14 * float(want.detach().abs().max())
    assert float(terms[1].detach()) == 0.0
    assert abs(float(loss.detach()) - float(want.detach().sum()) / 2.0) <= 1e-14 * float(want.detach().sum())
    g, = torch.autograd.grad(loss, s64)
    gw, = torch.autograd.grad(want.sum() / 2.0, s64)
    assert float((g - gw).abs().max()) <= 1e-15
    assert not g[eptr[3]:].any()                                          # the three problems that do not count


def test_dataset_draws_follow_the_reference_call_order():
    LIMITS = np.array([1., 1., 8. * 5e-2])                               # environment/env_config.py:3-5
    for dim in (2, 3):
        got = er.draw_maze_points(7, dim, rng=np.random.RandomState(4321))
        np.random.seed(4321)
        for pts in got:
            n = np.random.randint(100, 400)                               # dijkstra.py:94
            sample = np.random.uniform(-LIMITS[:dim], LIMITS[:dim], (n, dim))       # MazeEnv.uniform_sample(n)
            assert pts.dtype == np.float64 and pts.shape == (n, dim) and np.array_equal(pts, sample)
    a = er.draw_maze_points(3, 2)
    b = er.draw_maze_points(3, 2, rng=np.random.RandomState(1234))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
