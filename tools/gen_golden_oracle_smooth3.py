#!/usr/bin/env python
"""Record tests/golden/oracle_smooth3_*.npz: the smoother's training targets for the stick robot, computed by the
UNMODIFIED reference functions -- joint_smoother_ratio, joint_smoother, random_path_smoother, prune_path (smoother.py)
over MazeEnv(dim=3) -- on paths of real problems of maze_files/mazes_15_3_3000.npz.

The dim = 3 companion of tools/gen_golden_oracle_smooth.py, whose recording harness (run_reference: the wrapped
np.random draws, the stage snapshots, the shadowed ``Exception``) it shares in method; see that file's docstring.  Runs
only in the authoring container.  What is written is data: the map, the input path, the draws, the path / float32 flags /
check count after every stage, the result, and two annotations computed here: ``wrap_pairs`` (indices i of consecutive
input waypoints with |z[i + 1] - z[i]| > 0.4, whose edge check interpolates along the wrapped displacement) and
``z_rejected`` ([iteration, trial] of the trials whose perturbed waypoint leaves |z| <= 0.4 inside the map).

Every case is also run through tests/oracle_smooth3_host.py, which must agree bit for bit after every stage and report
neither a distance tie nor identical waypoints (the two places where the reference follows Python's hashing).
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

import oracle_smooth3_host as H3  # noqa: E402
import oracle_smooth_host as H  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
INF = float('inf')
KIND = {'random': 0, 'prune': 1, 'iter': 2}
DIM = 3


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
    xyz = np.array([[float(c) for c in p] for p in path], dtype=np.float64).reshape(-1, DIM)
    return xyz, np.array([isinstance(p[0], np.float32) for p in path], dtype=bool)


def run_reference(env, path32, in32, ratio, iters, random_iter, prune_iter, seed):
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
            actions.extend([np.zeros(DIM)] * random_iter)
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
    ref.Exception = _Never                           # an exception prune_path would swallow surfaces here
    try:
        fn = ref.joint_smoother_ratio if ratio else ref.joint_smoother
        result = fn(tuples, env, iters, random_iter, prune_iter)
    finally:
        np.random.uniform, np.random.randint = uniform, randint
        ref.random_path_smoother, ref.prune_path = orig_random, orig_prune
        del ref.Exception
    note('iter', result)
    assert len(actions) == len(idxs) == iters * random_iter, (len(actions), len(idxs))
    action = np.array(actions).reshape(iters, random_iter, DIM)
    node_idx = np.array(idxs, dtype=np.int32).reshape(iters, random_iter)
    return action, node_idx, stages, as_arrays(result), int(env.collision_check_count)


def record(name, env, path32, in32=True, ratio=True, iters=5, random_iter=100, prune_iter=100, seed=0, want=None):
    action, node_idx, stages, (res_xyz, res32), checks = run_reference(env, path32, in32, ratio, iters, random_iter,
                                                                      prune_iter, seed)
    # the reference run itself: no identical waypoints at any stage
    for _, x, _, _ in stages:
        assert len({tuple(r) for r in x}) == len(x), name + ': identical waypoints'
    # the host restatement on the same draws: equal everywhere, no tie, no duplicate
    trace = []
    xyz_in = path32.astype(np.float64)
    kw = dict(iters=iters, random_iter=random_iter, prune_iter=prune_iter, ratio=ratio)
    hx, h32, hc, hs = H3.smooth(xyz_in, in32, env.map, action, node_idx=node_idx, trace=trace, **kw)
    assert hs == 0, (name, hs)                       # in particular no STATUS_TIE and no STATUS_DUPLICATE
    assert hc == checks and hx.tobytes() == res_xyz.tobytes() and (h32 == res32).all(), name
    assert len(trace) == len(stages), (name, len(trace), len(stages))
    for (k, x, f, c), (hk, hxx, hf, hcc) in zip(stages, trace):
        assert k == KIND[hk] and x.tobytes() == hxx.tobytes() and (f == hf).all() and c == hcc, (name, k)
    zrej = np.array(H3.z_rejected_trials(xyz_in, in32, env.map, action, node_idx, **kw), dtype=np.int32).reshape(-1, 2)
    dz = np.abs(np.diff(path32[:, 2].astype(np.float64)))
    wrap = np.nonzero(dz > 0.4)[0].astype(np.int32)
    info = dict(path=path32, stages=stages, res32=res32, zrej=zrej, wrap=wrap)
    if want is not None and not want(info):
        return False
    ptr = np.cumsum([0] + [len(x) for _, x, _, _ in stages]).astype(np.int32)
    path = os.path.join(OUT, 'oracle_smooth3_%s.npz' % name)
    np.savez_compressed(
        path, map=env.map.astype(np.uint8), path=path32.astype(np.float32), in32=in32, ratio=ratio, iters=iters,
        random_iter=random_iter, prune_iter=prune_iter, action=action, node_idx=node_idx,
        stage_kind=np.array([k for k, _, _, _ in stages], dtype=np.int32), stage_ptr=ptr,
        stage_xy=np.concatenate([x for _, x, _, _ in stages] + [np.zeros((0, DIM))]),
        stage_is32=np.concatenate([f for _, _, f, _ in stages] + [np.zeros(0, bool)]),
        stage_checks=np.array([c for _, _, _, c in stages], dtype=np.int64),
        result=res_xyz, result_is32=res32, checks=np.int64(checks), status=np.int32(hs), wrap_pairs=wrap, z_rejected=zrej)
    lens = [len(x) for k, x, _, _ in stages if k == KIND['prune']]
    print('%-12s P=%3d in32=%d ratio=%d checks=%7d prune lens=%s kept32=%d wrap=%s zrej=%s  %5.1f KB'
          % (name, len(path32), in32, ratio, checks, lens, int(res32.sum()), wrap.tolist(), zrej[:3].tolist(),
             os.path.getsize(path) / 1024), flush=True)
    return True


def prune_lens(stages):
    return [len(x) for k, x, _, _ in stages if k == KIND['prune']]


def kept_sources(stages):
    """For every (random, prune) stage pair: the indices the pruned waypoints had in the random stage's path."""
    out = []
    for (k0, x0, _, _), (k1, x1, f1, _) in zip(stages[:-1], stages[1:]):
        if k0 == KIND['random'] and k1 == KIND['prune']:
            pos = {tuple(r): i for i, r in enumerate(x0)}
            out.append(([pos[tuple(r)] for r in x1], f1))
    return out


def mixed_edge(info):
    """A float32-input run in which some waypoint is float64 after a random stage while a neighbour is still float32: the
    next stage's edge checks between them take the float64 flow on an upcast float32 end."""
    for k, _, f, _ in info['stages']:
        if k == KIND['random'] and any(a != b for a, b in zip(f[:-1], f[1:])):
            return True
    return False


def main():
    env = MazeEnv(dim=3, map_file='maze_files/mazes_15_3_3000.npz')

    def problem_path(index, n, seed, tries=1):
        env.init_new_problem(index)
        for t in range(tries):                       # a k = 5 graph does not always join start and goal: next seed
            p = graph_path(env, n, seed + 1000 * t)
            if p is not None:
                return p
        return None

    def search(name, want, start, n=100, lo=4, hi=24, span=300, pre=None, **kw):
        """The first problem from ``start`` whose recorded run satisfies ``want``; ``pre`` filters the input paths first."""
        for index in range(start, start + span):
            p = problem_path(index, n, index)
            if p is None or not lo <= len(p) <= hi or (pre is not None and not pre(p)):
                continue
            try:
                if record(name, env, p, seed=index, want=want, **kw):
                    print('   (%s: problem %d)' % (name, index), flush=True)
                    return index, p
            except KeyError:                         # a prune that gives up (the 2-D 'abort' fixture covers that route)
                continue
        raise SystemExit('no case found for ' + name)

    # ordinary float32 paths (each must contain a mixed float32 / float64 edge check), one of them again on the all-float64
    # route and through joint_smoother
    kept = []
    start = 11
    for i in range(3):
        index, p = search('p%d' % i, mixed_edge, start, n=120 + 40 * i, lo=5, hi=20)
        kept.append((index, p))
        start = index + 29
    index, p = kept[0]
    env.init_new_problem(index)
    record('p0_f64', env, p, in32=False, seed=index)
    record('p0_joint', env, p, ratio=False, seed=index)
    # lengths 1, 2 and 3
    record('len1', env, p[:1], seed=11)
    record('len2', env, p[:2], seed=12)
    record('len3', env, p[:3], seed=13)
    # a short run
    record('short', env, p, iters=2, random_iter=20, seed=14)
    # a prune that removes nothing / one that removes >= 3 consecutive waypoints
    search('keepall', lambda c: any(n == len(c['path']) for n in prune_lens(c['stages'])), 400)
    search('drop3', lambda c: any(y - x >= 4 for src, _ in kept_sources(c['stages']) for x, y in zip(src[:-1], src[1:])), 500,
           n=160, lo=6)
    # a consecutive pair whose |dz| > 0.4: the edge check interpolates along the wrapped displacement
    search('wrap', lambda c: len(c['wrap']) > 0, 700, n=60, lo=3, span=1000,
           pre=lambda p: (np.abs(np.diff(p[:, 2].astype(np.float64))) > 0.4).any())
    # a trial rejected because z left +-0.4 (z_rejected says which)
    search('zreject', lambda c: len(c['zrej']) > 0, 900, n=100, span=1000, pre=lambda p: (np.abs(p[1:-1, 2]) > 0.36).any())


if __name__ == '__main__':
    main()
