#!/usr/bin/env python
"""Run ON THE GPU BOX: the explorer's training supervision on the device (gnnmp.episodes) for B synthetic maze2 problems of
100-400 nodes -- milliseconds per optimizer step for each stage: edge labels, shortest paths, training forward + backward
(one train_scores per loop value, loop drawn from randint(1, 10) as train_explorer.py:148), the episodes (explore +
replay) and the loss -- next to the plain-Python restatement of the same supervision (tests/episodes_host.py: labels,
dijkstra, explore, policy_data) on the host, with hostenv.limit_host_threads(): timed on the first 8 problems of each batch and
scaled to B (an extrapolation, labelled as such).  The stages are disjoint: fwd+bwd starts its backward from dloss/dscores,
the loss column is the loss's own forward and backward."""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import gnnmp  # noqa: E402
from gnnmp import episodes as ep, hostenv  # noqa: E402
from gnnmp.weights import load_weights  # noqa: E402
import episodes_host as H  # noqa: E402  (timed host baseline only)

DEV = 'cuda:0'
REPS = 10


def problems(B, seed):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(100, 401, B).tolist()
    pts = np.concatenate([rng.uniform(-1, 1, (n, 2)) for n in sizes])
    maps = (rng.random((B, 15, 15)) < 0.2).astype(np.float64)
    return sizes, pts, maps


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    hostenv.limit_host_threads()
    m = gnnmp.EncoderProcessDecoder(2, 2, 32, 2)
    m.load_state_dict(load_weights('weights_maze'))
    m.to(DEV).train()
    print('explorer training supervision on the device, synthetic maze2 problems of 100-400 nodes (15 x 15 maps, 20 %% '
          'obstacles), weights_maze, fp32, one MI355X; host baseline with %d torch threads' % torch.get_num_threads())
    print('%5s %8s | %8s %8s %10s %9s %9s | %9s | %s' % ('B', 'edges', 'labels', 'paths', 'fwd+bwd', 'episodes', 'loss f+b',
                                                        'total ms', 'host restatement ms (8 of the problems timed, x B / 8)'))
    for B in (8, 64, 256):
        sizes, pts, maps = problems(B, 100 + B)
        nptr = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        p64 = torch.from_numpy(pts).to(DEV)
        g = ep.maze_training_graphs(p64, nptr, maps, 2)
        gen = torch.Generator(device=DEV).manual_seed(1)
        cgen = torch.Generator().manual_seed(1)
        goal, loops = ep.draw_device(g, 10, gen, cgen)
        paths = ep.shortest_paths(g, goal)
        start = ep.draw_start(g, paths, gen)

        def fwd():
            return ep.forward_scores(m, g, paths['goal'], loops)
        scores = fwd()
        step, status = ep.explore_steps(g, scores, start, paths['goal'], paths['n_valid'])
        s = ep.draw_step(step, gen)
        fr = ep.policy_frontier(g, scores, paths, start, paths['goal'], s, status)
        sd = scores.detach().requires_grad_(True)
        ep.frontier_loss(sd, fr)[0].sum().backward()
        d_scores = sd.grad.clone()                         # dloss / dscores: the backward below starts from it

        t_lab = timed(lambda: ep.label_maze(g, p64, torch.from_numpy(maps), 2))
        t_path = timed(lambda: ep.shortest_paths(g, goal))

        def fb():                                          # forward + backward, the loss itself timed on its own below
            fwd().backward(d_scores)
        t_fb = timed(fb)

        def episodes():
            st, ss = ep.explore_steps(g, scores, start, paths['goal'], paths['n_valid'])
            ep.policy_frontier(g, scores, paths, start, paths['goal'], s, ss)
        t_ep = timed(episodes)
        def loss_fb():
            x = scores.detach().requires_grad_(True)
            ep.frontier_loss(x, fr)[0].sum().backward()
        t_loss = timed(loss_fb)
        # host restatement of the same problems (labels + dijkstra + explore + policy_data), up to 8 of them, scaled to B
        ei = g.edge_index.cpu().numpy()
        sc = scores.detach().cpu().numpy()
        go, stt, sp = paths['goal'].cpu().numpy(), start.cpu().numpy(), s.cpu().numpy()
        nh = min(B, 8)
        t0 = time.perf_counter()
        for b in range(nh):
            e0, e1 = g.edge_ptr_host[b], g.edge_ptr_host[b + 1]
            n0, n1 = g.node_ptr_host[b], g.node_ptr_host[b + 1]
            eb = ei[:, e0:e1]
            fr_h, c_h = H.label_edges(pts[n0:n1], eb, maps[b])
            H.episode(n1 - n0, eb, fr_h, c_h, sc[e0:e1], int(go[b]), int(stt[b]), lambda st_, b=b: int(sp[b]))
        host = (time.perf_counter() - t0) / nh * B * 1e3
        st_h = np.bincount(status.cpu().numpy(), minlength=4)
        total = t_lab + t_path + t_fb + t_ep + t_loss
        print('%5d %8d | %8.3f %8.3f %10.3f %9.3f %9.3f | %9.3f | %10.0f  (status ok/single/empty: %d/%d/%d, max step %d)'
              % (B, g.total_edges, t_lab, t_path, t_fb, t_ep, t_loss, total, host, st_h[0], st_h[1], st_h[2],
                 int(step.max())))


if __name__ == '__main__':
    main()
