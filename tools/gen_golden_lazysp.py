#!/usr/bin/env python
"""Record tests/golden/lazysp_*.npz: runs of the UNMODIFIED reference LazySP (algorithm/lazy_sp.py:147-196 over
algorithm/dijkstra.py and environment/maze_env.py) on real MazeEnv problems, each as
``np.random.seed(seed); env.init_new_problem(idx); LazySP(env, batch_size=batch, T=t_max, k=k).plan()``.

Runs only in the authoring container, like tools/gen_golden_episodes.py: the reference's third-party imports resolve to
tools/standins/.  What is written is data: the map, init / goal state, seed and settings, the float64 samples, the
collision-check total, the path's node ids, the final T, both edge sets as unordered pairs, the number of Dijkstra runs
(lazy_sp.dijkstra wrapped at run time), the blocked edges in the order they were found (remove_neighbor wrapped) and per
round N, cumulative checks and set sizes (informed_sample wrapped: its call opens a round, so it closes the one before).
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
os.environ.setdefault('CUDA_VISIBLE_DEVICES', '')
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, 'tools', 'standins'))

import numpy as np  # noqa: E402

os.chdir(REF)
import algorithm.lazy_sp as lazy_sp  # noqa: E402
from environment import MazeEnv  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
INF = float('inf')


def run(env, idx, seed, batch, t_max, k):
    np.random.seed(seed)
    env.init_new_problem(idx)
    planner = lazy_sp.LazySP(env, batch_size=batch, T=t_max, k=k)
    c0 = env.collision_check_count
    runs, first_inf, order, rounds = [0], [None], [], []
    real_dijkstra = lazy_sp.dijkstra

    def snapshot():
        rounds.append((len(planner.samples), env.collision_check_count - c0, len(planner.valid_edges) // 2,
                       len(planner.invalid_edges) // 2))

    def counted(nodes, edges, costs, source):
        dist, prev = real_dijkstra(nodes, edges, costs, source)
        if first_inf[0] is None:
            first_inf[0] = dist[1] == INF
        runs[0] += 1
        return dist, prev

    real_sample, real_remove = planner.informed_sample, planner.remove_neighbor

    def sample(n):
        if planner.T > 0:
            snapshot()
        return real_sample(n)

    def remove(edge_cost, neighbors, n1, n2):
        order.append((n1, n2))
        return real_remove(edge_cost, neighbors, n1, n2)

    planner.informed_sample, planner.remove_neighbor = sample, remove
    lazy_sp.dijkstra = counted
    try:
        samples, checks, path, T, _, valid, invalid = planner.plan()
    finally:
        lazy_sp.dijkstra = real_dijkstra
    snapshot()
    pts = np.array(samples, dtype=np.float64)
    ids = {tuple(p): i for i, p in enumerate(samples)}
    un = lambda s: np.array(sorted((a, b) for a, b in s if a < b), dtype=np.int32).reshape(-1, 2)      # noqa: E731
    return dict(map=env.map.astype(np.float64), init_state=np.asarray(env.init_state, dtype=np.float64),
                goal_state=np.asarray(env.goal_state, dtype=np.float64), seed=seed, batch=batch, t_max=t_max, k=k, index=idx,
                samples=pts, checks=int(checks), path_ids=np.array([ids[tuple(p)] for p in path], dtype=np.int32), T=int(T),
                valid_edges=un(valid), invalid_edges=un(invalid), dijkstra_runs=runs[0],
                invalid_order=np.array(order, dtype=np.int32).reshape(-1, 2), rounds=np.array(rounds, dtype=np.int64).reshape(-1, 4),
                first_dist1_inf=bool(first_inf[0]))


def record(name, dim, rec):
    path = os.path.join(OUT, 'lazysp_%s.npz' % name)
    np.savez_compressed(path, dim=dim, **rec)
    print('%-28s N=%4d checks=%6d path=%3d runs=%4d rounds=%2d T=%4d first_inf=%d  %5.1f KB'
          % (name, rec['samples'].shape[0], rec['checks'], len(rec['path_ids']), rec['dijkstra_runs'], len(rec['rounds']),
             rec['T'], rec['first_dist1_inf'], os.path.getsize(path) / 1024))


def main():
    envs = {2: MazeEnv(dim=2, map_file='maze_files/mazes_hard.npz'), 3: MazeEnv(dim=3, map_file='maze_files/mazes_hard_3.npz')}
    for dim, batch, t_max in ((2, 50, 300), (2, 20, 100), (3, 50, 200)):
        for idx in range(4):
            record('maze%d_b%d_t%d_i%d' % (dim, batch, t_max, idx), dim, run(envs[dim], idx, 1000 + idx, batch, t_max, 10))
    # a stick-robot problem solved in round 1
    for idx in range(4, 200):
        rec = run(envs[3], idx, 1000 + idx, 50, 50, 10)
        if len(rec['path_ids']):
            record('maze3_round1_i%d' % idx, 3, rec)
            break
    else:
        raise SystemExit('no stick problem solved in round 1')
    # dist[1] infinite on the very first Dijkstra (k = 2: every node keeps itself and one neighbour)
    for idx in range(200):
        rec = run(envs[2], idx, 1000 + idx, 20, 60, 2)
        if rec['first_dist1_inf']:
            record('maze2_firstinf_i%d' % idx, 2, rec)
            break
    else:
        raise SystemExit('no problem whose first Dijkstra leaves the start unreachable')
    # batch = 1: N = 3 in round 1
    record('maze2_b1_t6_i1', 2, run(envs[2], 1, 1001, 1, 6, 10))
    record('maze3_b1_t4_i0', 3, run(envs[3], 0, 1000, 1, 4, 10))


if __name__ == '__main__':
    main()
