#!/usr/bin/env python
"""Run ON THE GPU BOX: the explorer's training supervision on the device (gnnmp.episodes) for B synthetic maze2 problems of
100-400 nodes -- milliseconds per optimizer step for each stage: edge labels, shortest paths, training forward + backward
(one train_scores per loop value, loop drawn from randint(1, 10) as train_explorer.py:148), the episodes (explore +
replay) and the loss -- next to the plain-Python restatement of the same supervision (tests/episodes_host.py: labels,
dijkstra, explore, policy_data) on the host, with hostenv.limit_host_threads(): timed on the first 8 problems of each batch and
scaled to B (an extrapolation, labelled as such).  The stages are disjoint: fwd+bwd starts its backward from dloss/dscores,
the loss column is the loss's own forward and backward.

Second table: the same forward + backward as ONE train_scores_batch over all problems (episodes.forward_scores_batched) next to
the grouped form, in the same process and on the same draws: three timed repetitions of each leg (each the mean of 10 steps
after a warm-up step that is not timed), the kernel launches of the training path per step and the workspace bytes.
`--write FILE` also writes that table to FILE (profiles/explorer_train_batch.txt)."""
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


def train_launches(loop):
    """Kernel launches of one training forward + backward at `loop` iterations, counted from csrc/api.cpp
    (explorer_train_forward_body / _backward_body, one pair behind both forms): forward 18 + 8 per iteration, backward 35 + 25
    per iteration (a weight gradient is two launches; the decoder gradient waits in a buffer of its own and t_seed_dh fetches
    it).  Not counted: the frozen attention front stage (once per call in both forms), memsets, torch's own kernels."""
    return 18 + 8 * loop + 35 + 25 * loop


def workspace_bytes(m, g, goal, loops, batched):
    """Bytes of training workspace alive during one step: the batched call's one buffer, or the sum over the grouped calls
    (they run one after the other, but autograd keeps every group's buffer until its backward)."""
    import ctypes
    from gnnmp import _lib
    L = _lib.lib()
    need = ctypes.c_size_t()
    if batched:
        b = g.batch(goal)
        _lib.check(L.gnnmp_explorer_train_workspace_bytes(m._native(DEV), ctypes.byref(m._cbatch(b)), max(loops), ctypes.byref(need)), 'ws')
        return need.value
    total = 0
    for lp in sorted(set(loops)):
        b, _ = g.subset([i for i, x in enumerate(loops) if x == lp], goal)
        _lib.check(L.gnnmp_explorer_train_workspace_bytes(m._native(DEV), ctypes.byref(m._cbatch(b)), lp, ctypes.byref(need)), 'ws')
        total += need.value
    return total


def main():
    out_path = sys.argv[sys.argv.index('--write') + 1] if '--write' in sys.argv else None
    legs = []
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

        def fb_batched():
            ep.forward_scores_batched(m, g, paths['goal'], loops).backward(d_scores)
        # the two legs in turn, three repetitions each (timed() runs one untimed warm-up step first)
        reps_g, reps_b = [t_fb], []
        for r in range(3):
            reps_b.append(timed(fb_batched))
            if r < 2:
                reps_g.append(timed(fb))
        legs.append(dict(B=B, edges=g.total_edges, loops=sorted(set(loops)), grouped=reps_g, batched=reps_b,
                         launches_g=sum(train_launches(lp) for lp in set(loops)), launches_b=train_launches(max(loops)),
                         ws_g=workspace_bytes(m, g, paths['goal'], loops, False), ws_b=workspace_bytes(m, g, paths['goal'], loops, True)))

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
    lines = ['explorer training forward + backward per optimizer step, grouped (one train_scores per distinct loop value) vs batched '
             '(one train_scores_batch), same process, same draws (loop = 10, seed 1), synthetic maze2 problems of 100-400 nodes, fp32, one MI355X',
             'ms per step: three repetitions per leg, each the mean of %d steps after an untimed warm-up step' % REPS,
             '%5s %8s %-22s | %-26s | %-26s | %7s | %9s %9s | %12s %12s' % ('B', 'edges', 'loop values', 'grouped ms', 'batched ms', 'ratio',
                                                                          'launch g', 'launch b', 'ws bytes g', 'ws bytes b')]
    for x in legs:
        lines.append('%5d %8d %-22s | %-26s | %-26s | %7.2f | %9d %9d | %12d %12d'
                     % (x['B'], x['edges'], ','.join(map(str, x['loops'])), ' '.join('%8.3f' % t for t in x['grouped']),
                        ' '.join('%8.3f' % t for t in x['batched']), min(x['grouped']) / max(x['batched']), x['launches_g'],
                        x['launches_b'], x['ws_g'], x['ws_b']))
    last = legs[-1]
    lines.append('ratio = fastest grouped / slowest batched repetition.  At %d problems the slowest batched repetition (%.3f ms) is %s the '
                 'fastest grouped one (%.3f ms).' % (last['B'], max(last['batched']), 'below' if max(last['batched']) < min(last['grouped'])
                                                     else 'NOT below', min(last['grouped'])))
    lines.append('launches: kernel launches of the training path per step (train_launches() of tools/train_episodes_bench.py); '
                 'ws bytes g: sum over the groups, all held until their backward')
    print()
    print('\n'.join(lines))
    if out_path:
        with open(out_path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
