#!/usr/bin/env python
"""Record tests/golden/rrtstar_*.npz: runs of the UNMODIFIED reference RRT* -- ``NEXT_plan(env, model=None, T=t_max,
g_explore_eps=1., stop_when_success=...)`` (algorithm/tsa.py:12-139, 222-281 over algorithm/search_tree.py and
environment/maze_env.py), what eval_rrt.py runs -- on real MazeEnv problems, each as
``np.random.seed(seed); env.init_new_problem(idx); NEXT_plan(...)``.

Runs only in the authoring container, like tools/gen_golden_lazysp.py: the reference's third-party imports resolve to
tools/standins/ (the maze RRT* itself is numpy only).  What is written is data: the map, init / goal state, seed and settings,
every field of the search tree (states, parents, rewired_parents, freesp, in_goal_region, costs, path_lengths,
cumulated_collision_checks), success, the returned i, the node ids of search_tree.path() and the number of doubles drawn
(np.random.rand and env.uniform_sample wrapped at run time).  Printed per case, and stored: iterations that took the
direct-steer branch, second-pass checks on collided neighbours, goal tests inside rewiring that counted a _state_fp, nodes
whose rewired parent differs from the parent they were grown from.
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
import algorithm.tsa as tsa  # noqa: E402
from environment import MazeEnv  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')


def run(env, idx, seed, t_max, stop=True):
    np.random.seed(seed)
    env.init_new_problem(idx)
    dim = env.dim
    count = dict(draws=0, direct=0, collided2=0, goal_rechecks=0, rewired=0)
    state = dict(in_rewire=False, tree=None)
    real_rand, real_uniform, real_steer, real_rewire = np.random.rand, env.uniform_sample, tsa.RRT_steer, tsa.RRTS_rewire_last
    real_step, real_goal, real_rewire_to = env.step, env.in_goal_region, tsa.rewire_to

    def rand(*a):
        count['draws'] += 1
        return real_rand(*a)

    def uniform(*a, **kw):
        count['draws'] += dim
        return real_uniform(*a, **kw)

    def steer(env_, sample_state, nearest, dist):
        count['direct'] += bool(dist < env_.RRT_EPS)
        return real_steer(env_, sample_state, nearest, dist)

    def rewire(env_, search_tree, *a, **kw):
        state['in_rewire'], state['tree'] = True, search_tree
        try:
            return real_rewire(env_, search_tree, *a, **kw)
        finally:
            state['in_rewire'] = False

    def step(*a, **kw):
        if state['in_rewire']:
            tree = state['tree']
            hit = np.flatnonzero((tree.states == kw['state']).all(axis=1))
            count['collided2'] += bool(len(hit) and not tree.freesp[hit[0]])
        return real_step(*a, **kw)

    def goal(s):
        before = env.collision_check_count
        r = real_goal(s)
        count['goal_rechecks'] += bool(state['in_rewire'] and env.collision_check_count > before)
        return r

    def rewire_to(search_tree, child_idx, new_parent_idx):
        count['rewired'] += child_idx != -1
        return real_rewire_to(search_tree, child_idx, new_parent_idx)

    np.random.rand, env.uniform_sample, tsa.RRT_steer, tsa.RRTS_rewire_last = rand, uniform, steer, rewire
    env.step, env.in_goal_region, tsa.rewire_to = step, goal, rewire_to
    try:
        tree, success, i = tsa.NEXT_plan(env=env, model=None, T=t_max, g_explore_eps=1., stop_when_success=stop, UCB_type='kde')
    finally:
        np.random.rand, tsa.RRT_steer, tsa.RRTS_rewire_last, tsa.rewire_to = real_rand, real_steer, real_rewire, real_rewire_to
        del env.uniform_sample, env.step, env.in_goal_region
    states = np.asarray(tree.states, dtype=np.float64)
    ids = tree.path()[0]                     # states; the walk over rewired_parents from the last node is redone for the ids
    walk = []
    if tree.in_goal_region[-1]:
        cur = len(states) - 1
        while True:
            walk.append(cur)
            if cur == 0:
                break
            cur = tree.rewired_parents[cur]
        walk.reverse()
        assert len(walk) == len(ids) and all(np.array_equal(states[w], p) for w, p in zip(walk, ids))
    par = lambda xs: np.array([-1 if x is None else x for x in xs], dtype=np.int32)      # noqa: E731
    return dict(map=env.map.astype(np.float64), init_state=np.asarray(env.init_state, dtype=np.float64),
                goal_state=np.asarray(env.goal_state, dtype=np.float64), seed=seed, t_max=t_max, stop_when_success=bool(stop),
                index=idx, states=states, parents=par(tree.parents), rewired_parents=par(tree.rewired_parents),
                freesp=np.array(tree.freesp, dtype=bool), in_goal_region=np.array(tree.in_goal_region, dtype=bool),
                costs=np.array(tree.costs, dtype=np.float64), path_lengths=np.array(tree.path_lengths, dtype=np.float64),
                cumulated_collision_checks=np.array(tree.cumulated_collision_checks, dtype=np.int64), success=bool(success),
                i=int(i), path_ids=np.array(walk, dtype=np.int32), draws=count['draws'], direct_steer=count['direct'],
                collided_second_pass=count['collided2'], goal_rechecks=count['goal_rechecks'], second_pass_rewires=count['rewired'],
                rewired=int((par(tree.parents) != par(tree.rewired_parents)).sum()),
                first_rand=float(np.random.RandomState(seed).random_sample()))


def record(name, dim, rec):
    path = os.path.join(OUT, 'rrtstar_%s.npz' % name)
    np.savez_compressed(path, dim=dim, **rec)
    print('%-26s n=%4d i=%4d success=%d checks=%6d path=%3d draws=%5d direct_steer=%3d collided_2nd_pass=%4d goal_rechecks=%2d '
          'rewired=%3d (second pass %3d)  %5.1f KB' % (name, rec['states'].shape[0], rec['i'], rec['success'], rec['cumulated_collision_checks'][-1],
                                    len(rec['path_ids']), rec['draws'], rec['direct_steer'], rec['collided_second_pass'],
                                    rec['goal_rechecks'], rec['rewired'], rec['second_pass_rewires'], os.path.getsize(path) / 1024))


def main():
    envs = {2: MazeEnv(dim=2, map_file='maze_files/mazes_hard.npz'), 3: MazeEnv(dim=3, map_file='maze_files/mazes_hard_3.npz')}

    def first(dim, t_max, want, what, start=0, stop=True, seed_of=lambda idx: 1000 + idx, n=1):      # noqa: E731
        out = []
        for idx in range(start, 400):
            rec = run(envs[dim], idx, seed_of(idx), t_max, stop)
            if want(rec):
                out.append((idx, rec))
                if len(out) == n:
                    return out
        raise SystemExit('no case: ' + what)

    # solved maze2 problems: idx 13 (iteration 145), and a later one with more than 100 rewires
    record('maze2_t300_i13', 2, run(envs[2], 13, 1013, 300))
    for idx in (12, 16):
        rec = run(envs[2], idx, 1000 + idx, 300)
        if rec['success'] and rec['rewired'] > 100:
            record('maze2_t300_i%d' % idx, 2, rec)
            break
    else:
        raise SystemExit('neither idx 12 nor idx 16 is solved with more than 100 rewires')
    for idx, rec in first(2, 100, lambda r: not r['success'], 'two unsolved maze2 problems at T = 100', n=2):
        record('maze2_t100_i%d' % idx, 2, rec)
    record('maze3_t300_i8', 3, run(envs[3], 8, 1008, 300))
    for idx, rec in first(3, 100, lambda r: not r['success'], 'two unsolved maze3 problems at T = 100', n=2):
        record('maze3_t100_i%d' % idx, 3, rec)
    for dim in (2, 3):
        for t_max in (1, 2):
            record('maze%d_t%d_i0' % (dim, t_max), dim, run(envs[dim], 0, 1000, t_max))
    # finds the goal and goes on
    idx, rec = first(2, 300, lambda r: r['success'] and 0 < int(np.argmax(r['in_goal_region'])) < 250, 'a maze2 problem that goes on',
                     stop=False)[0]
    record('maze2_t300_goon_i%d' % idx, 2, rec)
    # the very first rand() is below model_eps: the first sample is the goal state
    seed = next(s for s in range(1000, 3000) if np.random.RandomState(s).random_sample() < 0.05)
    record('maze2_t100_firstgoal_s%d' % seed, 2, run(envs[2], 1, seed, 100))


if __name__ == '__main__':
    main()
