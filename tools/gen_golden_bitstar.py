#!/usr/bin/env python
"""Record tests/golden/bitstar_*.npz: runs of the UNMODIFIED reference BIT* (algorithm/bit_star.py:18-334 over
environment/maze_env.py) on real MazeEnv problems, each as what eval_bit.eval_bit runs for one problem:
``np.random.seed(seed); env.init_new_problem(idx); bit = BITStar(env, batch_size=batch, T=t_max, sampling=None);
bit.plan(INF, time_budget=300, refine_time_budget=0); bit.get_best_path()``.

Runs only in the authoring container, like tools/gen_golden_lazysp.py: the reference's third-party imports resolve to
tools/standins/.  What is written is data: the map, init / goal state, seed and settings, the points (start, goal, the free
draws in order), the vertices in order, parents and g by point id, the remaining samples in order, the check total,
g_scores[goal], T, the ids of get_best_path() and the doubles drawn (np.random.random wrapped at run time); per batch the
radius, the cumulative attempts and the cumulative sampling checks (the planner's ``sampling`` attribute wrapped); and the
counters vertex_expansions, edge_pops, edge_checks, rewired, filtered, max_edge_queue and ties_at_pop (the module's ``heapq``
name and the planner's expand_vertex / is_edge_free wrapped).  The tie case hands BITStar's own ``sampling=`` argument a
crafted mirror-symmetric pool, so the reference itself runs it.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
os.environ.setdefault('CUDA_VISIBLE_DEVICES', '')
os.environ.setdefault('MPLBACKEND', 'Agg')
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, 'tools', 'standins'))

import heapq  # noqa: E402

import numpy as np  # noqa: E402

os.chdir(REF)
import algorithm.bit_star as bit_star  # noqa: E402
from environment import MazeEnv  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
INF = float('inf')


class CountingHeap:
    """Stands in for the name ``heapq`` inside algorithm.bit_star while one plan runs."""

    def __init__(self, planner, count):
        self.planner, self.count = planner, count
        self.after_pop, self.popped_was_vertex = 0, False

    def heappush(self, q, item):
        heapq.heappush(q, item)
        if q is self.planner.edge_queue:
            self.count['max_edge_queue'] = max(self.count['max_edge_queue'], len(q))

    def heappop(self, q):
        if len(q) > 1 and sum(item[0] == q[0][0] for item in q) > 1:
            self.count['ties_at_pop'] += 1
        item = heapq.heappop(q)             # raises on an empty vertex queue, as the planner expects
        if q is self.planner.edge_queue:
            self.count['edge_pops'] += 1
            self.after_pop, self.popped_was_vertex = len(q), item[1][1] in self.planner.vertices
        return item

    def heapify(self, q):
        if q is self.planner.edge_queue:    # the filter after an accepted edge
            self.count['filtered'] += self.after_pop - len(q)
            self.count['rewired'] += bool(self.popped_was_vertex)
        heapq.heapify(q)


def run(env, idx, seed, batch, t_max, pool=None):
    np.random.seed(seed)
    env.init_new_problem(idx)
    dim = env.config_dim
    count = dict(vertex_expansions=0, edge_pops=0, edge_checks=0, rewired=0, filtered=0, max_edge_queue=0, ties_at_pop=0)
    state = dict(attempts=0, sampling_checks=0)
    r_by_batch, used_by_batch, checks_by_batch = [], [], []
    handed = []

    def crafted(c_best, n, vertices):
        assert c_best == INF and n == batch
        handed.append(pool[len(handed)])
        return [tuple(p) for p in handed[-1]]

    planner = bit_star.BITStar(env, batch_size=batch, T=t_max, sampling=crafted if pool is not None else None)
    c0 = env.collision_check_count
    real_random, real_sampling, real_expand, real_edge_free = np.random.random, planner.sampling, planner.expand_vertex, planner.is_edge_free

    def random(*a):
        assert a == (dim,)
        state['attempts'] += 1
        return real_random(*a)

    def sampling(c_best, n, vertices):
        if used_by_batch:
            r_by_batch.append(float(planner.r))
        before = env.collision_check_count
        out = real_sampling(c_best, n, vertices)
        state['sampling_checks'] += env.collision_check_count - before
        used_by_batch.append(state['attempts'])
        checks_by_batch.append(state['sampling_checks'])
        return out

    def expand(point):
        count['vertex_expansions'] += 1
        return real_expand(point)

    def edge_free(edge):
        count['edge_checks'] += 1
        return real_edge_free(edge)

    np.random.random, planner.sampling, planner.expand_vertex, planner.is_edge_free = random, sampling, expand, edge_free
    bit_star.heapq = CountingHeap(planner, count)
    try:
        samples, edges, checks, g_goal, T, _ = planner.plan(INF, time_budget=300, refine_time_budget=0)
        path = planner.get_best_path()
    finally:
        np.random.random, bit_star.heapq = real_random, heapq
    r_by_batch.append(float(planner.r))
    assert checks == env.collision_check_count - c0 and len(r_by_batch) == len(used_by_batch)
    # point ids: start, goal, then the free draws in the order they joined the samples
    order = [tuple(planner.start), tuple(planner.goal)]
    seen = set(order)
    drawn = set(planner.vertices) | set(planner.samples)
    assert len(drawn) == len(planner.vertices) + len(planner.samples) == 2 + len(used_by_batch) * batch
    if pool is not None:
        order += [tuple(p) for b in handed for p in b]
    else:                                    # the draws again, from the same seed: the free ones are the planner's points
        rs = np.random.RandomState(seed)
        low, ranges = planner.bounds[:, 0], planner.ranges
        for _ in range(state['attempts']):
            p = tuple(low + rs.random_sample(dim) * ranges)
            if p in drawn:
                assert p not in seen
                seen.add(p)
                order.append(p)
    assert set(order) == drawn and len(order) == len(drawn)
    ids = {p: i for i, p in enumerate(order)}
    n = len(order)
    parents = np.full(n, -1, dtype=np.int32)
    for child, parent in planner.edges.items():
        parents[ids[child]] = ids[parent]
    g = np.array([planner.get_g_score(p) for p in order], dtype=np.float64)
    rec = dict(map=env.map.astype(np.float64), init_state=np.asarray(env.init_state, dtype=np.float64),
               goal_state=np.asarray(env.goal_state, dtype=np.float64), seed=seed, batch=batch, t_max=t_max, index=idx,
               points=np.array(order, dtype=np.float64).reshape(n, dim), vertices=np.array([ids[p] for p in planner.vertices], dtype=np.int32),
               parents=parents, g=g, samples_left=np.array([ids[p] for p in samples], dtype=np.int32), checks=int(checks),
               g_goal=float(g_goal), T=int(T), path_ids=np.array([ids[p] for p in path], dtype=np.int32),
               draws=state['attempts'] * dim, r_by_batch=np.array(r_by_batch, dtype=np.float64),
               used_by_batch=np.array(used_by_batch, dtype=np.int64), checks_by_batch=np.array(checks_by_batch, dtype=np.int64),
               never_connected=bool(len(planner.vertices) == 1), crafted=pool is not None, **count)
    if pool is not None:
        rec['pool'] = np.array(pool, dtype=np.float64)
    return rec


def record(name, dim, rec):
    path = os.path.join(OUT, 'bitstar_%s.npz' % name)
    np.savez_compressed(path, dim=dim, **rec)
    print('%-24s N=%4d vertices=%3d T=%4d solved=%d checks=%6d path=%2d expansions=%3d pops=%4d rewired=%3d filtered=%4d '
          'max_queue=%3d ties=%d  %5.1f KB' % (name, rec['points'].shape[0], len(rec['vertices']), rec['T'], rec['g_goal'] < INF,
                                              rec['checks'], len(rec['path_ids']), rec['vertex_expansions'], rec['edge_pops'],
                                              rec['rewired'], rec['filtered'], rec['max_edge_queue'], rec['ties_at_pop'],
                                              os.path.getsize(path) / 1024), flush=True)


class CraftedEnv:
    """A one-problem MazeEnv look-alike over the reference's own checker: a crafted map with start and goal."""

    def __new__(cls, grid, start, goal):
        env = MazeEnv(dim=2, map_file='maze_files/mazes_hard.npz')
        env.maps = np.asarray(grid, dtype=env.maps.dtype)[None]
        env.init_states = np.asarray(start, dtype=np.float64)[None]
        env.goal_states = np.asarray(goal, dtype=np.float64)[None]
        env.size, env.order, env.episode_i = 1, [0], 0
        return env


def tie_case():
    """A 15 x 15 map, border wall and a short wall across the middle column; start (0, -0.6), goal (0, 0.6); a pool of
    mirror pairs (a, b), (-a, b), both free: mirror images are at the same distance from start and goal."""
    grid = np.zeros((15, 15))
    grid[0, :] = grid[-1, :] = grid[:, 0] = grid[:, -1] = 1
    grid[5:10, 7] = 1                        # map[x][y]: cells 5..9 in x of the middle row in y
    env = CraftedEnv(grid, (0.0, -0.6), (0.0, 0.6))
    env.init_new_problem(0)
    rs = np.random.RandomState(77)
    pool = []
    for _ in range(6):
        pts = []
        while len(pts) < 10:
            a, b = rs.uniform(0.05, 0.85), rs.uniform(-0.85, 0.85)
            if env._state_fp(np.array((a, b))) and env._state_fp(np.array((-a, b))):
                pts += [(a, b), (-a, b)]
        pool.append(pts)
    env.collision_check_count = 0
    return env, np.array(pool, dtype=np.float64)


def main():
    envs = {2: MazeEnv(dim=2, map_file='maze_files/mazes_hard.npz'), 3: MazeEnv(dim=3, map_file='maze_files/mazes_hard_3.npz')}

    def first(dim, batch, t_max, start, want, what):
        for idx in range(start, 400):
            rec = run(envs[dim], idx, 1000 + idx, batch, t_max)
            if want(rec):
                return idx, rec
        else:
            raise SystemExit('no case: ' + what)

    solved = lambda r: r['g_goal'] < INF      # noqa: E731
    for idx in range(4):
        record('maze2_b50_t1000_i%d' % idx, 2, run(envs[2], idx, 1000 + idx, 50, 1000))
    idx, rec = first(2, 50, 1000, 33, lambda r: solved(r) and r['rewired'] >= 50 and len(r['vertices']) > 128, 'many rewirings')
    record('maze2_b50_t1000_i%d' % idx, 2, rec)
    idx, rec = first(2, 7, 35, 16, lambda r: solved(r) and r['T'] < 35, 'batch 7 solved early')
    record('maze2_b7_t35_i%d' % idx, 2, rec)
    idx, rec = first(2, 7, 35, 19, lambda r: not solved(r) and r['rewired'] > 0 and r['T'] == 35, 'batch 7 unsolved with rewirings')
    record('maze2_b7_t35_i%d' % idx, 2, rec)
    idx, rec = first(2, 7, 35, 18, lambda r: not solved(r) and r['never_connected'], 'batch 7 never connected')
    record('maze2_b7_t35_i%d' % idx, 2, rec)
    idx, rec = first(2, 7, 30, 19, lambda r: not solved(r) and r['T'] == 35, 'batch 7, t_max 30 ends at T = 35')
    record('maze2_b7_t30_i%d' % idx, 2, rec)
    for start, want, what in ((0, lambda r: solved(r) and r['T'] > 100, 'maze3 solved after several batches'),
                              (6, lambda r: solved(r) and r['T'] <= 100, 'maze3 solved early'),
                              (4, lambda r: not solved(r) and r['rewired'] > 50, 'maze3 unsolved with rewirings'),
                              (1, lambda r: not solved(r) and len(r['vertices']) < 64, 'maze3 unsolved, a small tree')):
        idx, rec = first(3, 50, 300, start, want, what)
        record('maze3_b50_t300_i%d' % idx, 3, rec)
    env, pool = tie_case()
    rec = run(env, 0, 1000, 10, 60, pool=pool)
    if rec['ties_at_pop'] == 0:
        raise SystemExit('the mirror pool gave no tied pop')
    record('maze2_ties_b10_t60', 2, rec)
    record('maze2_b1_t4_i1', 2, run(envs[2], 1, 1001, 1, 4))
    record('maze3_b1_t4_i0', 3, run(envs[3], 0, 1000, 1, 4))


if __name__ == '__main__':
    main()
