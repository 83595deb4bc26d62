#!/usr/bin/env python
"""Record tests/golden/oracle_smooth_*.npz: the smoother's training targets (train_smoother.py:98) computed by the
UNMODIFIED reference functions -- joint_smoother_ratio, joint_smoother, random_path_smoother, prune_path (smoother.py)
over MazeEnv(dim=2) -- on paths of real problems of maze_files/mazes_15_2_3000.npz.

Runs only in the authoring container, like tools/gen_golden_episodes.py: the reference's third-party imports resolve to
tools/standins/.  The reference is not edited: np.random.uniform / np.random.randint are wrapped to record what it drew,
the module-level names random_path_smoother / prune_path that joint_smoother* look up are wrapped to snapshot the path
and env.collision_check_count after every stage, and the name ``Exception`` that prune_path's ``except`` looks up is
shadowed in the module's globals by a class nothing raises, so that an exception the reference would have swallowed
surfaces here (no recorded case has one).

What is written is data: the map, the input path, the draws, the path / float32 flags / check count after every stage and
the result.  Input paths are Dijkstra paths from the problem's start to its goal over construct_graph of uniform samples
(algorithm/dijkstra.py), cast to float32 rows as the planner's paths are.

Every case is also run through tests/oracle_smooth_host.py, which must agree bit for bit and report neither a distance
tie nor identical waypoints (the two places where the reference follows Python's hashing).
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
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.modules.setdefault('tensorboardX', types.SimpleNamespace(SummaryWriter=None))

import numpy as np  # noqa: E402

os.chdir(REF)
from algorithm.dijkstra import construct_graph, dijkstra  # noqa: E402
from environment import MazeEnv  # noqa: E402
import smoother as ref  # noqa: E402

import oracle_smooth_host as H  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
INF = float('inf')
KIND = {'random': 0, 'prune': 1, 'iter': 2}


class _Never(BaseException):
    pass


def graph_path(env, n, seed):
    """Dijkstra path init_state -> goal_state over construct_graph of n uniform samples, or None."""
    np.random.seed(seed)
    points = env.uniform_sample(n=n)
    points[0], points[1] = env.init_state, env.goal_state
    edge_cost, neighbors, _, _ = construct_graph(env, points)
    dist, prev = dijkstra(list(range(n)), neighbors, edge_cost, 1)
    if dist[0] == INF:
        return None
    path, cur = [0], 0
    while cur != 1:
        cur = prev[cur]
        path.append(cur)
    return points[path].astype(np.float32)


def as_arrays(path):
    xy = np.array([[float(p[0]), float(p[1])] for p in path], dtype=np.float64).reshape(-1, 2)
    return xy, np.array([isinstance(p[0], np.float32) for p in path], dtype=bool)


def run_reference(env, path32, in32, ratio, iters, random_iter, prune_iter, seed, swallow=False):
    """The reference on one path.  Returns the recorded draws, stages and result."""
    tuples = [tuple(node) for node in path32] if in32 else [tuple(float(x) for x in node) for node in path32]
    actions, idxs, stages = [], [], []
    uniform, randint = np.random.uniform, np.random.randint
    orig_random, orig_prune = ref.random_path_smoother, ref.prune_path

    def rec_uniform(*a, **k):
        x = uniform(*a, **k)
        actions.append(np.array(x, dtype=np.float64))
        return x

    def rec_randint(*a, **k):
        x = randint(*a, **k)
        idxs.append(int(x))
        return x

    def note(kind, p):
        stages.append((KIND[kind], *as_arrays(p), int(env.collision_check_count)))

    state = {'live': None}

    def rec_random(path, *a, **k):
        if state['live'] is not None:
            note('iter', path)                       # the previous iteration's result is this one's input
        n0 = len(idxs)
        out = orig_random(path, *a, **k)
        if len(idxs) == n0:                          # len(path) <= 2: the reference draws nothing; the slots stay zero
            actions.extend([np.zeros(2)] * random_iter)
            idxs.extend([0] * random_iter)
        note('random', out)
        state['live'] = out
        return out

    def rec_prune(path, *a, **k):
        out = orig_prune(path, *a, **k)
        note('prune', out)
        return out

    env.collision_check_count = 0
    np.random.seed(seed)
    np.random.uniform, np.random.randint = rec_uniform, rec_randint
    ref.random_path_smoother, ref.prune_path = rec_random, rec_prune
    ref.Exception = Exception if swallow else _Never
    try:
        fn = ref.joint_smoother_ratio if ratio else ref.joint_smoother
        result = fn(tuples, env, iters, random_iter, prune_iter)
    finally:
        np.random.uniform, np.random.randint = uniform, randint
        ref.random_path_smoother, ref.prune_path = orig_random, orig_prune
        del ref.Exception
    note('iter', result)
    n_draw = iters * random_iter
    assert len(actions) == len(idxs) == n_draw, (len(actions), len(idxs))
    action = np.array(actions).reshape(iters, random_iter, 2)
    node_idx = np.array(idxs, dtype=np.int32).reshape(iters, random_iter)
    return action, node_idx, stages, as_arrays(result), int(env.collision_check_count)


def record(name, env, path32, in32=True, ratio=True, iters=5, random_iter=100, prune_iter=100, seed=0, want=None,
           aborted=False):
    """``aborted``: the case is recorded as one whose prune_path swallows an exception (status STATUS_UNREACHABLE); any
    other case must run with no exception raised inside prune_path."""
    action, node_idx, stages, (res_xy, res32), checks = run_reference(env, path32, in32, ratio, iters, random_iter, prune_iter,
                                                                     seed, swallow=aborted)
    # the host restatement on the same draws: equal everywhere, no tie, no duplicate
    trace = []
    xy_in = path32.astype(np.float64)
    hx, h32, hc, hs = H.smooth(xy_in, in32, env.map, action, node_idx=node_idx, iters=iters, random_iter=random_iter,
                               prune_iter=prune_iter, ratio=ratio, trace=trace)
    assert hs == (H.STATUS_UNREACHABLE if aborted else 0), (name, hs)
    assert hc == checks and hx.tobytes() == res_xy.tobytes() and (h32 == res32).all(), name
    assert len(trace) == len(stages), (name, len(trace), len(stages))
    for (k, x, f, c), (hk, hxx, hf, hcc) in zip(stages, trace):
        assert k == KIND[hk] and x.tobytes() == hxx.tobytes() and (f == hf).all() and c == hcc, (name, k)
    for _, x, _, _ in stages:
        assert len({(a, b) for a, b in x}) == len(x), name + ': identical waypoints'
    if want is not None and not want(path32, stages, res32):
        return False
    ptr = np.cumsum([0] + [len(x) for _, x, _, _ in stages]).astype(np.int32)
    path = os.path.join(OUT, 'oracle_smooth_%s.npz' % name)
    np.savez_compressed(
        path, map=env.map.astype(np.uint8), path=path32.astype(np.float32), in32=in32, ratio=ratio, iters=iters,
        random_iter=random_iter, prune_iter=prune_iter, action=action, node_idx=node_idx,
        stage_kind=np.array([k for k, _, _, _ in stages], dtype=np.int32), stage_ptr=ptr,
        stage_xy=np.concatenate([x for _, x, _, _ in stages] + [np.zeros((0, 2))]),
        stage_is32=np.concatenate([f for _, _, f, _ in stages] + [np.zeros(0, bool)]),
        stage_checks=np.array([c for _, _, _, c in stages], dtype=np.int64),
        result=res_xy, result_is32=res32, checks=np.int64(checks), status=np.int32(hs))
    lens = [len(x) for k, x, _, _ in stages if k == KIND['prune']]
    print('%-22s P=%3d in32=%d ratio=%d checks=%6d prune lens=%s kept32=%d  %5.1f KB'
          % (name, len(path32), in32, ratio, checks, lens, int(res32.sum()), os.path.getsize(path) / 1024))
    return True


def main():
    env = MazeEnv(dim=2, map_file='maze_files/mazes_15_2_3000.npz')

    def problem_path(index, n, seed, tries=1):
        env.init_new_problem(index)
        for t in range(tries):                       # a k = 5 graph does not always join start and goal: next seed
            p = graph_path(env, n, seed + 1000 * t)
            if p is not None:
                return p
        return None

    # >= 6 ordinary paths of 5-30 waypoints
    # (and the first whose prune_path cannot reach path[next] and gives up in its except, recorded as such)
    kept, have_abort = [], False
    for index, n, seed in [(11 + 29 * i, 150 + 50 * (i % 6), i + 1) for i in range(40)]:
        p = problem_path(index, n, seed, 20)
        if p is None or not 5 <= len(p) <= 30:
            continue
        try:
            if len(kept) < 7:
                record('p%d' % index, env, p, seed=seed)
                kept.append((index, n, seed))
        except KeyError:
            if not have_abort:
                record('abort', env, p, seed=seed, aborted=True)
                have_abort = True
        if len(kept) >= 7 and have_abort:
            break
    assert len(kept) >= 6 and have_abort, (kept, have_abort)
    # the same two paths on the all-float64 route, and joint_smoother (paths shrink) for two
    for index, n, seed in kept[:2]:
        p = problem_path(index, n, seed, 20)
        record('p%d_f64' % index, env, p, in32=False, seed=seed)
        record('p%d_joint' % index, env, p, ratio=False, seed=seed)
    # lengths 1, 2 and 3
    p = problem_path(11, 300, 1, 20)
    record('len1', env, p[:1], seed=11)
    env.init_new_problem(11)
    record('len2', env, np.array([p[0], p[1]], dtype=np.float32), seed=12)
    record('len3', env, np.array([p[0], p[1], p[2]], dtype=np.float32), seed=13)

    prune_lens = lambda stages: [len(x) for k, x, _, _ in stages if k == KIND['prune']]      # noqa: E731

    def search(name, want, start=2000, **kw):
        for index in range(start, start + 400):
            p = problem_path(index, 120, index)
            if p is None or not 4 <= len(p) <= 30:
                continue
            try:
                if record(name, env, p, seed=index, want=want, **kw):
                    print('   (%s: problem %d)' % (name, index))
                    return
            except KeyError:                         # a prune that gives up: the 'abort' case covers that
                continue
        raise SystemExit('no case found for ' + name)

    # a prune that removes nothing
    search('keepall', lambda p, st, r32: any(n == len(p) for n in prune_lens(st)))
    # a prune that removes >= 3 consecutive waypoints: the kept source indices jump by >= 4
    def drops3(p, st, r32):
        for (k0, x0, _, _), (k1, x1, _, _) in zip(st[:-1], st[1:]):
            if k0 == KIND['random'] and k1 == KIND['prune']:
                pos = {(a, b): i for i, (a, b) in enumerate(x0)}
                src = [pos[(a, b)] for a, b in x1]
                if any(y - x >= 4 for x, y in zip(src[:-1], src[1:])):
                    return True
        return False
    search('drop3', drops3)
    # a perturbed (float64) waypoint that is kept by a prune next to dropped ones: a float64 end of a re-spaced segment
    def f64_end(p, st, r32):
        for (k0, x0, f0, _), (k1, x1, f1, _) in zip(st[:-1], st[1:]):
            if k0 == KIND['random'] and k1 == KIND['prune']:
                pos = {(a, b): i for i, (a, b) in enumerate(x0)}
                src = [pos[(a, b)] for a, b in x1]
                for (x, y), fa, fb in zip(zip(src[:-1], src[1:]), f1[:-1], f1[1:]):
                    if y - x >= 2 and not (fa and fb):
                        return True
        return False
    search('f64end', f64_end, start=2200)


if __name__ == '__main__':
    main()
