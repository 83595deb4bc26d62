#!/usr/bin/env python
"""Record tests/golden/lazysp_*.npz: runs of the UNMODIFIED reference LazySP (algorithm/lazy_sp.py:147-196 over
algorithm/dijkstra.py and environment/maze_env.py) on real MazeEnv problems, each as
``np.random.seed(seed); env.init_new_problem(idx); LazySP(env, batch_size=batch, T=t_max, k=k).plan()``.

Runs only in the authoring container, like tools/gen_golden_episodes.py: the reference's third-party imports resolve to
tools/standins/.  What is written is data: the map, init / goal state, seed and settings, the float64 samples, the
collision-check total, the path's node ids, the final T, both edge sets as unordered pairs, the number of Dijkstra runs
(lazy_sp.dijkstra wrapped at run time), the blocked edges in the order they were found (remove_neighbor wrapped) and per
round N, cumulative checks and set sizes (informed_sample wrapped: its call opens a round, so it closes the one before).

lazysp_lattice_*.npz: inputs on a dyadic lattice, where keys and relaxed distances tie exactly.
  * lazysp_lattice_dijkstra.npz: the reference's own dijkstra() called directly on lattice graphs (graph g: ``g_points``,
    ``g_edges`` [E, 2] (source, target) in the order of the neighbour lists, ``g_costs``, and its ``g_dist`` / ``g_prev``, -1
    where the reference leaves infinity) -- its order among equal keys with no kNN involved.
  * lazysp_lattice_<case>.npz: whole LazySP runs whose draws (``attempts``, raw doubles, distinct lattice points) are handed
    to informed_sample's get_random_point.  A lattice ties the kNN too, so these runs set GNNMP_STANDIN_KNN=input (the
    stand-in's float32, lower-index mode) and construct_graph is wrapped to assert that every round's edge set equals
    gnnmp.lazysp.graph_edges; a case where it does not would be written as lazysp_lattice_<case>_hostoracle.npz from
    gnnmp.lazysp.plan_host alone.  The tie counters (extract_ties, relax_ties) are plan_host's on the same attempts, taken
    once its result equals the reference's in every field.
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


def run(env, idx, seed, batch, t_max, k, attempts=None, knn_equal=None):
    np.random.seed(seed)
    env.init_new_problem(idx)
    planner = lazy_sp.LazySP(env, batch_size=batch, T=t_max, k=k)
    if attempts is not None:
        rows = iter(attempts)
        planner.get_random_point = lambda: tuple(planner.bounds[:, 0] + next(rows) * planner.ranges)
        real_construct = planner.construct_graph

        def construct(k1, points, env_):
            out = real_construct(k1, points, env_)
            from gnnmp import lazysp
            knn_equal.append(np.array_equal(out[2], lazysp.graph_edges(np.array(points), k1)))
            return out
        planner.construct_graph = construct
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


class CraftedEnv:
    """A one-problem MazeEnv look-alike over the reference's own checker: a crafted map with start and goal."""

    def __new__(cls, grid, start, goal):
        dim = len(start)
        env = MazeEnv(dim=dim, map_file='maze_files/mazes_hard.npz' if dim == 2 else 'maze_files/mazes_hard_3.npz')
        env.maps = np.asarray(grid, dtype=env.maps.dtype)[None]
        env.init_states = np.asarray(start, dtype=np.float64)[None]
        env.goal_states = np.asarray(goal, dtype=np.float64)[None]
        env.size, env.order, env.episode_i = 1, [0], 0
        return env


def wall_map(gap):
    """15 x 15, free but for a wall of one cell across the middle in both index directions (a cross), with a gap of one cell
    in each arm when ``gap``: start (-0.5, -0.5) and goal (0.5, 0.5) lie in opposite quarters."""
    m = np.zeros((15, 15))
    m[7, :] = m[:, 7] = 1
    if gap:
        m[7, 2] = m[2, 7] = m[7, 12] = m[12, 7] = 0
    return m


START, GOAL = (-0.5, -0.5), (0.5, 0.5)
Z_RAW = (0.25, 0.5, 0.75)                    # the stick's angle -0.4 + 0.8 z: three planes, -0.2, 0 and 0.2; start and goal at 0


def ends(dim):
    return (START, GOAL) if dim == 2 else (START + (0.0,), GOAL + (0.0,))


def lattice_attempts(side, seed, dim=2):
    """Every point of the side x side lattice of raw doubles {j / side} (x = -1 + 2 j / side) -- for the stick robot in each
    of the planes Z_RAW -- but start and goal, shuffled: distinct rows, [n, dim]."""
    j = np.arange(side) / float(side)
    raw = np.stack(np.meshgrid(*((j, j) if dim == 2 else (j, j, np.array(Z_RAW))), indexing='ij'), axis=-1).reshape(-1, dim)
    pts = np.array((-1.0, -1.0, -0.4)[:dim]) + raw * np.array((2.0, 2.0, 0.8)[:dim])
    keep = ~((pts == ends(dim)[0]).all(axis=1) | (pts == ends(dim)[1]).all(axis=1))
    assert keep.sum() == len(raw) - 2
    return raw[keep][np.random.RandomState(seed).permutation(len(raw) - 2)]


# (name, lattice side, batch, t_max, k, gap in the wall): Dijkstra on 63, 64, 65 and 129 nodes and on both sides of the device's
# LDS node count (1024); several rounds where the node count is reached in small batches (a closed wall: never solved)
LATTICE_CASES = (('b61_t61', 16, 61, 61, 10, True), ('b31_t62_closed', 16, 31, 62, 10, False), ('b21_t63', 16, 21, 63, 10, True),
                 ('b9_t63_closed', 16, 9, 63, 10, False), ('b127_t127', 32, 127, 127, 10, True), ('b1022_t1022', 64, 1022, 1022, 10, True),
                 ('b1023_t1023', 64, 1023, 1023, 10, True),
                 # the stick robot: 65 nodes in three rounds, 129 in one
                 ('maze3_b21_t63_closed', 16, 21, 63, 10, False), ('maze3_b127_t127', 16, 127, 127, 10, True))


def highest_id(key):
    return len(key) - 1 - int(np.argmin(np.asarray(key)[::-1]))


# the neighbouring rules (tests/test_lazysp_ties_host.py swaps in the same two): inputs are chosen so that each one matters
MUTATIONS = (('extract_index', highest_id), ('relax_improves', lambda alt, dist: alt <= dist))


def with_rule(attr, rule, call):
    from gnnmp import lazysp
    real = getattr(lazysp, attr)
    setattr(lazysp, attr, rule)
    try:
        return call()
    except (RuntimeError, ValueError):       # a cycle in prev, or the attempts ran out: moved
        return None
    finally:
        setattr(lazysp, attr, real)


def lattice_dijkstra():
    """The reference's dijkstra() on lattice graphs built as construct_graph builds them (neighbour lists by target, in the
    coalesced order), a tenth of the unordered pairs taken out as invalidated edges are."""
    from gnnmp import lazysp
    out, report = {}, []
    def graph(n, side, seed):
        raw = lattice_attempts(side, seed)[:n - 2]
        pts = np.concatenate((np.array([GOAL, START]), -1.0 + raw * 2.0))
        rs = np.random.RandomState(seed + 100)
        edges = lazysp.graph_edges(pts, lazysp.k1_of(10, n))
        dead = {(a, b) for a, b in edges.tolist() if a < b and rs.random_sample() < 0.1}
        edges = np.array([(a, b) for a, b in edges.tolist() if (min(a, b), max(a, b)) not in dead], dtype=np.int32)
        dense = np.full((n, n), INF)
        dense[edges[:, 1], edges[:, 0]] = np.linalg.norm(pts[edges[:, 1]] - pts[edges[:, 0]], axis=1)
        return pts, edges, dense

    for g, (n, side) in enumerate(((63, 16), (64, 16), (65, 16), (129, 16), (129, 32))):
        # the first graph of this size's own sequence on which BOTH neighbouring rules give another prev than the host
        # restatement's: an input that cannot tell the rules apart pins nothing
        for seed in range(500 + g, 500 + g + 2000, 10):
            pts, edges, dense = graph(n, side, seed)
            base = lazysp._dijkstra(dense, False)[1]
            if all(not np.array_equal(with_rule(attr, rule, lambda: lazysp._dijkstra(dense, False)[1]), base) for attr, rule in MUTATIONS):
                break
        else:
            raise SystemExit('no %d-node graph that both mutated rules move' % n)
        cost, neighbors = lazy_sp.defaultdict(list), lazy_sp.defaultdict(list)
        for a, b in edges:
            cost[b].append(np.linalg.norm(pts[b] - pts[a]))
            neighbors[b].append(a)
        dist, prev = lazy_sp.dijkstra(list(range(n)), neighbors, cost, 0)
        costs = np.array([np.linalg.norm(pts[b] - pts[a]) for a, b in edges])
        dense = np.full((n, n), INF)
        dense[edges[:, 1], edges[:, 0]] = costs
        st = dict(extract_ties=0, relax_ties=0)
        lazysp._dijkstra(dense, False, st)
        out.update({'%d_points' % g: pts, '%d_edges' % g: edges, '%d_costs' % g: costs,
                    '%d_dist' % g: np.array([dist[v] for v in range(n)], dtype=np.float64),
                    '%d_prev' % g: np.array([-1 if prev[v] == INF else prev[v] for v in range(n)], dtype=np.int32),
                    '%d_extract_ties' % g: st['extract_ties'], '%d_relax_ties' % g: st['relax_ties']})
        report.append('n=%d side=%d E=%d unreachable=%d extract_ties=%d relax_ties=%d'
                      % (n, side, len(edges), int(np.sum(np.array([dist[v] for v in range(n)]) == INF)), st['extract_ties'], st['relax_ties']))
    path = os.path.join(OUT, 'lazysp_lattice_dijkstra.npz')
    np.savez_compressed(path, graphs=len(report), **out)
    print('lattice_dijkstra: %s  %5.1f KB' % ('; '.join(report), os.path.getsize(path) / 1024), flush=True)


def lattice_main():
    sys.path.insert(0, REPO)
    from gnnmp import lazysp
    EXACT_FIELDS = ('checks', 'path_ids', 'T', 'valid_edges', 'invalid_edges', 'dijkstra_runs', 'invalid_order', 'rounds')
    lattice_dijkstra()
    os.environ['GNNMP_STANDIN_KNN'] = 'input'
    for name, side, batch, t_max, k, gap in LATTICE_CASES:
        dim = 3 if name.startswith('maze3') else 2
        env = CraftedEnv(wall_map(gap), *ends(dim))
        problem = dict(map=wall_map(gap), init_state=np.array(ends(dim)[0]), goal_state=np.array(ends(dim)[1]))
        plan = lambda: lazysp.plan_host(problem, 0, batch=batch, t_max=t_max, k=k, attempts=attempts)      # noqa: E731
        same = lambda a, b: a is not None and all(np.array_equal(np.asarray(a[key]), np.asarray(b[key])) for key in EXACT_FIELDS)      # noqa: E731
        # the first shuffle of this case's own sequence whose run BOTH neighbouring rules change (chosen on the host
        # restatement, before the reference runs)
        for seed in range(700 + side + batch, 700 + side + batch + 3000, 10):
            attempts = lattice_attempts(side, seed, dim)
            host = plan()
            if all(not same(with_rule(attr, rule, plan), host) for attr, rule in MUTATIONS):
                break
        else:
            raise SystemExit('%s: no shuffle that both mutated rules move' % name)
        knn_equal = []
        rec = run(env, 0, 0, batch, t_max, k, attempts=attempts, knn_equal=knn_equal)
        if all(knn_equal):
            assert np.array_equal(host['samples'], rec['samples'])
            for key in EXACT_FIELDS:
                a, b = np.asarray(host[key]), np.asarray(rec[key])
                assert a.shape == b.shape and np.array_equal(a, b), '%s: plan_host differs from the reference in %s' % (name, key)
        else:                                # the stand-in kNN chose other neighbours among equals: plan_host is the oracle
            name += '_hostoracle'
            rec.update({key: host[key] for key in EXACT_FIELDS + ('samples',)})
        rec.pop('first_dist1_inf')
        rec.update(attempts=attempts[:host['draws']], lattice=True, side=side, knn_equal=all(knn_equal), extract_ties=host['extract_ties'],
                   relax_ties=host['relax_ties'], max_walk_edges=int(host['walk_edges'].max()) if len(host['walk_edges']) else 0)
        path = os.path.join(OUT, 'lazysp_lattice_%s.npz' % name)
        np.savez_compressed(path, dim=dim, **rec)
        print('lattice_%-22s N=%4d checks=%6d path=%3d runs=%4d rounds=%2d T=%4d knn_equal=%s carried=%s extract_ties=%d relax_ties=%d  '
              '%5.1f KB' % (name, rec['samples'].shape[0], rec['checks'], len(rec['path_ids']), rec['dijkstra_runs'], len(rec['rounds']),
                            rec['T'], knn_equal, rec['rounds'][:, 2:].tolist(), rec['extract_ties'], rec['relax_ties'],
                            os.path.getsize(path) / 1024), flush=True)


def main():
    if sys.argv[1:] == ['lattice']:          # only the crafted cases
        return lattice_main()
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
    lattice_main()


if __name__ == '__main__':
    main()
