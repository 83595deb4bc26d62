#!/usr/bin/env python
"""Record tests/golden/episodes_*.npz: the explorer's training supervision (train_explorer.py:124-176) computed by the
UNMODIFIED reference functions -- construct_graph and dijkstra (algorithm/dijkstra.py), explore and policy_data
(train_explorer.py) -- on real MazeEnv problems (maze_files/mazes_15_{2,3}_3000.npz).

Runs only in the authoring container, like tools/gen_golden.py: the reference's third-party imports resolve to
tools/standins/, tensorboardX (imported by train_explorer.py, never called by the functions used here) to an empty module.
What is written is data: the map, the float64 samples, the coalesced edges with the reference's free flags and costs, the
per-edge scores handed to explore, start / goal, dist / prev, the explore step, the replay step and the resulting frontier
(as edge ids, cell (a, c) = edge (c -> a)) and label.
"""
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
os.environ.setdefault('CUDA_VISIBLE_DEVICES', '')
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, 'tools', 'standins'))
sys.path.insert(0, REPO)
sys.modules.setdefault('tensorboardX', types.SimpleNamespace(SummaryWriter=None))

import numpy as np  # noqa: E402
import torch  # noqa: E402

os.chdir(REF)
from algorithm.dijkstra import construct_graph, dijkstra  # noqa: E402
from environment import MazeEnv  # noqa: E402
import model as ref_model  # noqa: E402
from train_explorer import explore, policy_data  # noqa: E402

import gnnmp  # noqa: E402,F401
from gnnmp.weights import load_weights  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
INF = float('inf')


def reference_graph(env, n):
    points = env.uniform_sample(n=n)
    edge_cost, neighbors, edge_index, edge_free = construct_graph(env, points)
    ei = np.asarray(edge_index).T.astype(np.int64)                  # [2, E] (source, target), coalesced order
    # construct_graph keeps the costs per target in edge order: back to one cost per edge
    cursor = {}
    cost = np.empty(ei.shape[1])
    for e in range(ei.shape[1]):
        t = int(ei[1, e])
        k = cursor.get(t, 0)
        cost[e] = edge_cost[t][k]
        cursor[t] = k + 1
    return points, ei, np.asarray(edge_free, dtype=np.uint8).reshape(-1), cost, neighbors, edge_cost


def model_scores(dim, points, ei, env, loop, seed):
    torch.manual_seed(seed)
    m = ref_model.EncoderProcessDecoder(2, dim, 32, 2)
    m.load_state_dict(load_weights('weights_maze' if dim == 2 else 'weights_maze_3'), strict=True)
    m.train()
    v = torch.FloatTensor(points)
    goal = v[0]
    P = m(goal=goal, loop=loop, v=v, obstacles=torch.FloatTensor(env.obstacles), free=v, collided=v,
          edge_index=torch.LongTensor(ei))
    return P.detach()[torch.from_numpy(ei[1]), torch.from_numpy(ei[0])].numpy().astype(np.float32)


def record(name, env, dim, points, ei, free, cost, neighbors, edge_cost, scores, goal, start, max_steps, replay_rng):
    N = len(points)
    dist, prev = dijkstra(list(range(N)), neighbors, edge_cost, goal)
    prev[goal] = goal
    d = np.array([dist[i] for i in range(N)])
    p = np.array([-1 if prev[i] == INF else int(prev[i]) for i in range(N)], dtype=np.int32)
    n_valid = int((d != INF).sum())
    out = dict(map=env.map.astype(np.float64), points=points.astype(np.float64), edge_index=ei.astype(np.int32),
               edge_free=free, edge_cost=cost, scores=scores, goal=goal, start=start, max_steps=max_steps, dist=d,
               prev=p, n_valid=n_valid, status=0, step=-1, replay_step=-1, frontier=np.zeros(0, np.int32), label=-1)
    if n_valid == 1:
        out['status'] = 1
    else:
        P = torch.zeros(N, N)
        P[torch.from_numpy(ei[1]), torch.from_numpy(ei[0])] = torch.from_numpy(scores)
        cost_arr = np.zeros((N, N))
        for x in neighbors:
            for y, c in zip(neighbors[x], edge_cost[x]):
                cost_arr[x, y] = c
        try:
            step = explore(cost_arr, P.clone(), start, goal, max_steps)
        except Exception:
            out['status'] = 2
            step = None
        if step is not None:
            s = int(replay_rng(step))
            _, idx, frontier = policy_data(cost_arr, dist, prev, P.clone(), start, goal, s)
            eid = {(int(ei[1, e]), int(ei[0, e])): e for e in range(ei.shape[1])}
            rows, cols = np.asarray(frontier[0]), frontier[1].numpy()
            out.update(step=int(step), replay_step=s, label=int(idx),
                       frontier=np.array([eid[(int(a), int(c))] for a, c in zip(rows, cols)], dtype=np.int32))
    path = os.path.join(OUT, 'episodes_%s.npz' % name)
    np.savez_compressed(path, dim=dim, **out)
    print('%-28s N=%4d E=%5d n_valid=%4d status=%d step=%4d replay=%4d |frontier|=%4d label=%d  %6.1f KB'
          % (name, N, ei.shape[1], n_valid, out['status'], out['step'], out['replay_step'], len(out['frontier']),
             out['label'], os.path.getsize(path) / 1024))
    return out


def dup_start(free, ei, N, start, goal, scores, max_steps):
    """Whether the reference's roll-out explores the start twice (via tests/episodes_host, which the fixtures check)."""
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import episodes_host as H
    cl = H._Clone(N, ei, scores, goal)
    try:
        explored, _, _ = H._rollout(cl, free, start, goal, max_steps, True)
    except RuntimeError:
        return False
    return explored.count(start) > 1


def main():
    envs = {2: MazeEnv(dim=2, map_file='maze_files/mazes_15_2_3000.npz'),
            3: MazeEnv(dim=3, map_file='maze_files/mazes_15_3_3000.npz')}

    def problem(dim, index, n, seed):
        env = envs[dim]
        env.init_new_problem(index)
        np.random.seed(seed)
        return env, reference_graph(env, n)

    def rand_scores(E, seed, quant=None, zeros=0.0):
        r = np.random.RandomState(seed)
        s = r.standard_normal(E).astype(np.float32)
        if quant:
            s = (np.round(s * quant) / quant).astype(np.float32)
        if zeros:
            z = r.rand(E) < zeros
            s[z] = np.where(r.rand(int(z.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
        return s

    def pick(dist_ok, r):
        return int(r.choice(np.flatnonzero(dist_ok)))

    def valid_of(ei, cost, N, goal, nb, ec):
        dist, _ = dijkstra(list(range(N)), nb, ec, goal)
        return np.array([dist[i] != INF for i in range(N)])

    def free_goal(r, N, ei, cost, nb, ec):
        while True:                      # a goal in free space, connected to a good part of the graph
            g = int(r.randint(N))
            valid = valid_of(ei, cost, N, g, nb, ec)
            if valid.sum() > 8:
                return g, valid

    def far_start(N, nb, ec, goal):
        dist, _ = dijkstra(list(range(N)), nb, ec, goal)
        d = np.array([dist[i] for i in range(N)])
        return int(np.argmax(np.where(d == INF, -1.0, d)))

    half = lambda step: step // 2          # noqa: E731
    full = lambda step: step               # noqa: E731

    for dim, tag in ((2, 'maze2'), (3, 'maze3')):
        env, (pts, ei, fr, cost, nb, ec) = problem(dim, 11 if dim == 2 else 5, 160 if dim == 2 else 300, 100 + dim)
        N = len(pts)
        r = np.random.RandomState(7 + dim)
        goal, valid = free_goal(r, N, ei, cost, nb, ec)
        start = pick(valid, r)
        sm = model_scores(dim, pts, ei, env, 3, 5)
        record('%s_model' % tag, env, dim, pts, ei, fr, cost, nb, ec, sm, goal, start, 1000, half)
        record('%s_random' % tag, env, dim, pts, ei, fr, cost, nb, ec, rand_scores(ei.shape[1], 3), goal, start, 1000, full)

    # maze2: ties, zeros, start == goal, a hit cap, a single valid node, an emptied frontier, a duplicated start row
    env, (pts, ei, fr, cost, nb, ec) = problem(2, 23, 220, 301)
    N, E = len(pts), ei.shape[1]
    r = np.random.RandomState(31)
    goal, valid = free_goal(r, N, ei, cost, nb, ec)
    start = pick(valid, r)
    record('maze2_ties', env, 2, pts, ei, fr, cost, nb, ec, rand_scores(E, 4, quant=2), goal, start, 1000, half)
    record('maze2_zeros', env, 2, pts, ei, fr, cost, nb, ec, rand_scores(E, 5, zeros=0.3), goal, start, 1000, half)
    record('maze2_startgoal', env, 2, pts, ei, fr, cost, nb, ec, rand_scores(E, 6), goal, goal, 1000, full)
    record('maze2_cap', env, 2, pts, ei, fr, cost, nb, ec, rand_scores(E, 7), goal, far_start(N, nb, ec, goal), 10, full)
    far = far_start(N, nb, ec, goal)
    sz = np.zeros(E, np.float32)
    sz[ei[1] == far] = rand_scores(E, 8)[ei[1] == far]              # only the start's row: the frontier runs dry
    record('maze2_empty', env, 2, pts, ei, fr, cost, nb, ec, sz, goal, far, 1000, full)
    for g in range(N):                                               # a goal whose only finite distance is its own
        if valid_of(ei, cost, N, g, nb, ec).sum() == 1:
            record('maze2_single', env, 2, pts, ei, fr, cost, nb, ec, rand_scores(E, 9), g, g, 1000, full)
            break
    else:
        raise SystemExit('no single-valid-node goal in this problem')
    for seed in range(1000):
        s = rand_scores(E, 1000 + seed)
        if dup_start(fr, ei, N, start, goal, s, 1000):
            record('maze2_dupstart', env, 2, pts, ei, fr, cost, nb, ec, s, goal, start, 1000, full)
            break
    else:
        raise SystemExit('no duplicated start row found')


if __name__ == '__main__':
    main()
