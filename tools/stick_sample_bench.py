#!/usr/bin/env python
"""Rejection sampling of the stick robot (maze3): the device sampler (gnnmp_stick_sample) against the host's one-by-one
loop (Maze3D.sample_n_points, the route of eval_gnn_device_rounds) and the host's vectorised look-ahead sampler
(Maze3D.sample_n_points_stream), and the planner built on each.  Run on an MI355X; not part of bench.py.

  python tools/stick_sample_bench.py                 -> profiles/stick_sample_bench.txt

Problems: the 40 of tests/golden/evalset_maze3_first40_b200_k12_s9.npz, repeated to 256, at batch = 200 and batch = 500.
  device kernel    one gnnmp_stick_sample launch between two events, the draws already in device memory: median of 7 after 2
                   warm-up launches
  device sampler   planner.sample_maze_problems_device, wall clock: the host's draws, their copy, the launch, the wait and
                   the generator's re-advance; median of 5
  host, vectorised planner.sample_maze_problems, wall clock, median of 3
  host, one by one Maze3D.sample_n_points on the first 8 problems, scaled to 256
Planner: problems/s of eval_gnn_device (device sampling, then host sampling) and of eval_gnn_device_rounds(t_max = batch) on
the 40 fixture problems at the fixture's batch and k, best of 3 after one warm-up run each.  Nothing is asserted but that the
three samplers agree."""
import argparse
import ctypes
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--problems', type=int, default=256)
    a = ap.parse_args()
    import numpy as np
    import torch
    import gnnmp
    from gnnmp import _lib, planner
    from gnnmp.maze2d import LIMITS3, Maze3D
    from gnnmp.weights import load_weights
    dev = 'cuda:0'
    with np.load(os.path.join(REPO, 'tests', 'golden', 'evalset_maze3_first40_b200_k12_s9.npz')) as f:
        maps, init, goal = f['maps'], f['init_states'], f['goal_states']
        seed, fx_batch, k = int(f['seed']), int(f['batch']), int(f['k'])
    n_fx = maps.shape[0]
    B = a.problems
    problems = [dict(map=maps[i % n_fx], init_state=init[i % n_fx], goal_state=goal[i % n_fx]) for i in range(B)]
    lines = ['stick-robot sampling (gnnmp_stick_sample) on %s, %d problems' % (torch.cuda.get_device_name(0), B),
             '%6s %14s %14s %14s %14s %12s %12s' % ('batch', 'kernel ms/pr', 'device ms/pr', 'host vec ms/pr', 'host 1x1 ms/pr',
                                                  'draws/pr', 'checks/pr')]
    for batch in (200, 500):
        # host, one by one (8 problems) and vectorised (all)
        np.random.seed(seed)
        t0 = time.perf_counter()
        for pr in problems[:8]:
            e = Maze3D(np.asarray(pr['map'])[None], np.asarray(pr['init_state'])[None], np.asarray(pr['goal_state'])[None])
            e.init_new_problem(0)
            e.sample_n_points(batch, need_negative=True)
        one_ms = (time.perf_counter() - t0) * 1e3 / 8
        vec = []
        for rep in range(3):
            np.random.seed(seed)
            t0 = time.perf_counter()
            envs, vs, _, _ = planner.sample_maze_problems(problems, batch, k)
            vec.append((time.perf_counter() - t0) * 1e3 / B)
        st_host = np.random.get_state()
        # device sampler, wall clock
        wall = []
        for rep in range(6):
            np.random.seed(seed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d = planner.sample_maze_problems_device(problems, batch, k, dev)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3 / B)
        st_dev = np.random.get_state()
        assert st_host[0] == st_dev[0] and np.array_equal(st_host[1], st_dev[1]) and st_host[2:] == st_dev[2:]
        assert torch.equal(d['v'].cpu(), torch.cat(vs))
        checks = [e.collision_check_count for e in d['envs']]
        assert checks == [e.collision_check_count for e in envs]
        # the launch alone
        np.random.seed(seed)
        draws = int(B * batch * 12) + 4096
        att = torch.from_numpy(np.random.uniform(-LIMITS3, LIMITS3, (draws, 3))).to(dev)
        v = torch.empty(B * (2 + 2 * batch), 3, dtype=torch.float32, device=dev)
        nptr = torch.empty(B + 1, dtype=torch.int32, device=dev)
        used = torch.empty(B, dtype=torch.int32, device=dev)
        chk = torch.empty(B, dtype=torch.int64, device=dev)
        state = torch.zeros(2, dtype=torch.int64, device=dev)
        init64 = torch.from_numpy(np.ascontiguousarray(np.asarray([pr['init_state'] for pr in problems], dtype=np.float64))).to(dev)
        sb = _lib.MazeSampleBatch(B, int(maps.shape[1]), batch, draws, att.data_ptr(), d['maps'].data_ptr(), init64.data_ptr(),
                                  d['goal64'].data_ptr())
        L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
        ts = []
        for rep in range(9):
            state.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(L.gnnmp_stick_sample(ctypes.byref(sb), state.data_ptr(), v.data_ptr(), nptr.data_ptr(), used.data_ptr(),
                                            chk.data_ptr(), state.data_ptr() + 8, st), 'gnnmp_stick_sample')
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        cursor, ok = state.cpu().tolist()
        assert ok & 0xffffffff and chk.cpu().tolist() == checks and torch.equal(v[:int(nptr[-1])], d['v'])
        lines.append('%6d %14.4f %14.4f %14.3f %14.1f %12.0f %12.0f' % (batch, float(np.median(ts[2:])) / B, float(np.median(wall[1:])),
                                                                       float(np.median(vec)), one_ms, cursor / B, np.mean(checks)))
    # the planner on the fixture
    env = Maze3D(maps, init, goal)
    m = gnnmp.EncoderProcessDecoder(2, 3, 32, 2).eval()
    m.load_state_dict(load_weights('weights_maze_3'))
    runs = [('eval_gnn_device, device sampling', lambda: planner.eval_gnn_device(env, range(n_fx), m, None, seed=seed, batch=fx_batch,
                                                                                 k=k, device=dev)),
            ('eval_gnn_device, host sampling (vectorised)', lambda: planner.eval_gnn_device(env, range(n_fx), m, None, seed=seed,
                                                                                            batch=fx_batch, k=k, device=dev,
                                                                                            device_sampling=False)),
            ('eval_gnn_device_rounds (host, one by one)', lambda: planner.eval_gnn_device_rounds(env, range(n_fx), m, None, seed=seed,
                                                                                                 batch=fx_batch, t_max=fx_batch, k=k,
                                                                                                 device=dev))]
    lines.append('planner on the %d fixture problems, batch = t_max = %d, k = %d, no smoother: problems/s, best of 3' % (n_fx, fx_batch, k))
    for name, fn in runs:
        fn()
        best = 1e30
        for rep in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        lines.append('%-48s %10.1f' % (name, n_fx / best))
    text = '\n'.join(lines) + '\n'
    print(text)
    out = a.out or os.path.join(REPO, 'profiles', 'stick_sample_bench.txt')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
