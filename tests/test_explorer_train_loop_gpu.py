"""gnnmp.explorer_replay.train_explorer_maze end to end: the reference's loop (train_explorer.py:96-210) over a device dataset.

16 synthetic maze2 problems of 100 to 150 nodes on 15 x 15 maps with 20 % obstacles (a quarter of them the fixtures' real
mazes, as random_maps of tests/test_episodes_gpu.py builds them), iters = 2, from `weights_maze`: the steps taken are
explorer_schedule's groups, every step loss is finite, the trainable parameters move, the parameters behind the reference's
detach() (node_attentions, edge_attentions, obs_node_code, obs_edge_code) do not move bit for bit, and a second run from the
same seeds gives the same losses and the same state dict bit for bit.  The same for maze3 with 4 problems and iters = 1: finite
losses and the counted share.

Condition on the inputs: at least half of all samples are counted.  The seeds are picked so that the host restatement alone
keeps it (`host_counted_share`: the points of draw_maze_points, the host's kNN graph, tests/episodes_host.label_edges and
shortest_paths with a uniformly drawn goal per sample; a sample is skipped when only the goal is reachable).  The points are
plain uniform draws, so a good part of them lies inside obstacles and reaches nothing.  On the CPU it gives: maze2, seed 1234:
21 of 32 samples counted (share 0.66), 1468 of 2050 nodes (0.72) reach another node; maze3, seed 959: 2 of 4 samples counted
(share 0.50), 221 of 505 nodes (0.44) reach another node -- the stick robot is free at few of the uniform points --, and 0.71
of the nodes of the one problem the run steps on (the first of the permutation), the best of the seeds 1 .. 1200."""
import numpy as np
import pytest
import torch

import gnnmp
from gnnmp import explorer_replay as er
from conftest import golden_files, load_weights
import episodes_host as H

DEV = 'cuda:0'
SEEDS = {2: 1234, 3: 959}
FROZEN = ('node_attentions', 'edge_attentions', 'obs_node_code', 'obs_edge_code')


def maps_of(n, seed, w=15):
    rng = np.random.default_rng(seed)
    maps = (rng.random((n, w, w)) < 0.2).astype(np.float64)
    fixture_maps = []
    for f in golden_files('episodes_'):
        with np.load(f) as z:
            if z['map'].shape[0] == w:
                fixture_maps.append(z['map'].astype(np.float64))
    for i in range(0, n, 4):                         # a quarter of them real mazes
        maps[i] = fixture_maps[i % len(fixture_maps)]
    return maps


def host_counted_share(dim, n, iters, seed):
    """(counted samples, samples, nodes with another node in reach, nodes, the share of such nodes in the first problem of the
    first permutation) by the host restatement alone."""
    from gnnmp.graph_build import build_edges
    maps = maps_of(n, seed)
    rng = np.random.RandomState(seed)
    points = er.draw_maze_points(n, dim, 100, 151, rng)
    goals = np.random.RandomState(seed + 1)
    graphs = []
    for pts, m in zip(points, maps):
        ei = build_edges(torch.from_numpy(pts).float(), pts.shape[0], 5).numpy()
        _, cost = H.label_edges(pts, ei, m)
        graphs.append((pts.shape[0], ei, cost))
    counted = samples = 0
    for _ in range(iters):
        for N, ei, cost in graphs:
            samples += 1
            counted += H.shortest_paths(N, ei, cost, int(goals.choice(N)))[2] > 1
    reach = []
    for N, ei, cost in graphs:
        free = np.isfinite(cost) & (ei[0] != ei[1])
        reach.append(len(set(ei[0][free].tolist()) | set(ei[1][free].tolist())))
    first = int(rng.permutation(n)[0])
    return counted, samples, sum(reach), sum(g[0] for g in graphs), reach[first] / graphs[first][0]


def model_of(dim):
    m = gnnmp.EncoderProcessDecoder(2, dim, 32, 2)
    m.load_state_dict(load_weights('weights_maze' if dim == 2 else 'weights_maze_3'))
    return m


def run(dim, n, iters):
    model = model_of(dim)
    before = {k: v.detach().clone().to(DEV) for k, v in model.state_dict().items()}
    hist = er.train_explorer_maze(model, maps_of(n, SEEDS[dim]), dim, DEV, iters=iters, seed=SEEDS[dim], n_lo=100, n_hi=151)
    return before, {k: v.detach().clone() for k, v in model.state_dict().items()}, hist


@pytest.mark.gpu
def test_maze2_loop_follows_the_schedule_moves_the_weights_and_repeats():
    n, iters = 16, 2
    before, after, hist = run(2, n, iters)
    # the steps are explorer_schedule's groups (the generator draws the points first, as train_explorer_maze does)
    rng = np.random.RandomState(SEEDS[2])
    er.draw_maze_points(n, 2, 100, 151, rng)
    groups, dropped = er.explorer_schedule(n, iters=iters, group=8, rng=rng)
    assert [len(g) for g in groups] == [1, 8, 8, 8] and len(dropped) == 7
    assert len(hist) == iters and sum(len(h['losses']) for h in hist) == len(groups)
    assert [len(h['losses']) for h in hist] == [2, 2] and [h['samples'] for h in hist] == [9, 16]
    losses = [x for h in hist for x in h['losses']]
    print('\nlosses %s' % losses)
    assert np.isfinite(losses).all() and all(np.isfinite(h['mean']) and h['steps_per_s'] > 0 for h in hist)
    counted, samples = sum(h['counted'] for h in hist), sum(h['samples'] for h in hist)
    skipped = sum(h['single'] + h['empty'] for h in hist)
    print('counted %d of %d samples (single %s, empty %s)' % (counted, samples, [h['single'] for h in hist], [h['empty'] for h in hist]))
    assert counted + skipped == samples == 25 and 2 * counted >= samples
    moved = []
    for name, b in before.items():
        if name.startswith(FROZEN):
            assert torch.equal(after[name], b), name
        elif not torch.equal(after[name], b):
            moved.append(name)
    print('moved: %s' % moved)
    # the blocks the training forward differentiates through (the rest of the state dict is never read by forward())
    assert all(name in moved for name in before if name.startswith('policy.'))
    for block in ('node_code.', 'edge_code.', 'encoder.', 'process.', 'decoder.'):
        assert any(name.startswith(block) for name in moved), block
    # a second run from the same seeds: the same losses and the same state dict, bit for bit
    _, after2, hist2 = run(2, n, iters)
    assert [h['losses'] for h in hist2] == [h['losses'] for h in hist]
    assert [(h['counted'], h['single'], h['empty']) for h in hist2] == [(h['counted'], h['single'], h['empty']) for h in hist]
    for name in after:
        assert torch.equal(after[name], after2[name]), name
    # the checkpoint goes back into the network under the reference's names
    gnnmp.EncoderProcessDecoder(2, 2, 32, 2).load_state_dict({k: v.cpu() for k, v in after.items()})


@pytest.mark.gpu
def test_maze3_loop_runs():
    _, _, hist = run(3, 4, 1)
    assert len(hist) == 1 and len(hist[0]['losses']) == 1 and hist[0]['samples'] == 1
    assert np.isfinite(hist[0]['losses']).all()
    print('\nmaze3: loss %s, counted %d of %d' % (hist[0]['losses'], hist[0]['counted'], hist[0]['samples']))
    assert 2 * hist[0]['counted'] >= hist[0]['samples']


def test_host_restatement_keeps_the_counted_share():
    """No GPU: the condition on the inputs, by the host restatement alone (the figures of the module docstring)."""
    for dim, n, iters in ((2, 16, 2), (3, 4, 1)):
        counted, samples, reach, nodes, first = host_counted_share(dim, n, iters, SEEDS[dim])
        print('\nmaze%d: %d of %d samples counted, %d of %d nodes reach another node, %.2f of the first problem\'s'
              % (dim, counted, samples, reach, nodes, first))
        assert 2 * counted >= samples and first >= 0.5
