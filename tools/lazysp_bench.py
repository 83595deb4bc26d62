#!/usr/bin/env python
"""The LazySP baseline on the device next to the device GNN planner, on the same problems.  Run on an MI355X; not part of
bench.py.

  python tools/lazysp_bench.py                 -> profiles/lazysp_bench.txt

Sets: the first 1000 problems of tests/golden/evalset_mazehard_first1000.npz (point robot) and the 40 of
evalset_maze3_first40_b200_k12_s9.npz (stick robot).  LazySP runs at the reference's setting (batch = 50, t_max = 1000, k = 10,
eval_bit.py:118) through lazysp.eval_lazysp_device; the GNN planner at its own (batch = 500, t_max = 500, k = 30) through
planner.eval_gnn_device_streams, without a smoother.  Both use one sample stream per problem with planner.stream_seeds(1234).
Legs alternate (lazysp, gnn per set); every leg is a child process under its own ``timeout``; wall clock of one run after one
warm-up run.  The LazySP leg adds the per-stage split (``timings``: device waits after every stage, so from a run of its own).
The CPU yardstick is lazysp.plan_host on a sample of the set's problems on one core, scaled to problems/s.  No rate is asserted
anywhere.  After a leg that fails, whatever the exit status, nothing more is started on the GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
LAZY = dict(batch=50, t_max=1000, k=10)
GNN = dict(batch=500, t_max=500, k=30)


def _load(name):
    import numpy as np
    import gnnmp
    from gnnmp.maze2d import Maze2D, Maze3D
    from gnnmp.weights import load_weights
    if name == 'maze2':
        with np.load(os.path.join(REPO, 'tests', 'golden', 'evalset_mazehard_first1000.npz')) as f:
            env = Maze2D(f['maps'], f['init_states'], f['goal_states'])
        m = gnnmp.EncoderProcessDecoder(2, 2, 32, 2).eval()
        m.load_state_dict(load_weights('weights_maze'))
    else:
        with np.load(os.path.join(REPO, 'tests', 'golden', 'evalset_maze3_first40_b200_k12_s9.npz')) as f:
            env = Maze3D(f['maps'], f['init_states'], f['goal_states'])
        m = gnnmp.EncoderProcessDecoder(2, 3, 32, 2).eval()
        m.load_state_dict(load_weights('weights_maze_3'))
    return env, m


def child(name, which, cpu_sample):
    import numpy as np
    import torch
    from gnnmp import lazysp, planner
    env, m = _load(name)
    dev = 'cuda:0'
    res = {'set': name, 'planner': which, 'problems': env.size}
    if which == 'lazysp':
        run = lambda **kw: lazysp.eval_lazysp_device(env, range(env.size), seed=1234, device=dev, **LAZY, **kw)      # noqa: E731
    else:
        run = lambda **kw: planner.eval_gnn_device_streams(env, range(env.size), m, None, seed=1234, device=dev, **GNN, **kw)      # noqa: E731
    for rep in range(2):                                           # the first run warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    checks = out['collision'] if which == 'lazysp' else out['collision_explore']
    res.update(seconds=dt, rate=env.size / dt, solved=int(out['n_success']), checks=float(checks))
    if which == 'lazysp':
        tm = {}
        run(timings=tm)
        res['timings_ms'] = {k: 1e3 * v for k, v in tm.items()}
        seeds = planner.stream_seeds(1234, range(env.size))
        t0 = time.perf_counter()
        for i in range(cpu_sample):
            lazysp.plan_host(dict(map=env.maps[i], init_state=env.init_states[i], goal_state=env.goal_states[i]), seeds[i], **LAZY)
        res['cpu_rate'] = cpu_sample / (time.perf_counter() - t0)
        res['cpu_sample'] = cpu_sample
    print('RESULT ' + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--limit', type=int, default=420, help='seconds per leg')
    ap.add_argument('--cpu-sample', type=int, default=4, help='problems of each set plan_host runs for the CPU yardstick')
    ap.add_argument('--child', nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.cpu_sample)
    lines = ['LazySP baseline (lazysp.eval_lazysp_device, batch = %(batch)d, t_max = %(t_max)d, k = %(k)d)' % LAZY
             + ' next to the device GNN planner (planner.eval_gnn_device_streams, batch = %(batch)d, t_max = %(t_max)d, k = %(k)d, no '
               'smoother)' % GNN, 'one sample stream per problem, seeds = planner.stream_seeds(1234); wall clock of one warm run',
             '%-6s %-8s %9s %12s %8s %14s' % ('set', 'planner', 'problems', 'problems/s', 'solved', 'mean checks')]
    extra, got_all = [], {}
    stop = False
    for name in ('maze2', 'maze3'):
        for which in ('lazysp', 'gnn'):
            cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--cpu-sample', str(a.cpu_sample),
                   '--child', name, which]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            got = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
            if p.returncode != 0 or not got:
                lines.append('%-6s %-8s did not finish (exit %d)' % (name, which, p.returncode))
                print(p.stdout[-2000:])
                lines.append('stopped: nothing more is started on the GPU after a leg that failed')
                stop = True
                break
            r = json.loads(got[-1][7:])
            got_all[(name, which)] = r
            lines.append('%-6s %-8s %9d %12.1f %8d %14.2f' % (name, which, r['problems'], r['rate'], r['solved'], r['checks']))
            if which == 'lazysp':
                extra.append('%s lazysp, stage wall clock with a device wait after each stage (ms): %s'
                             % (name, ', '.join('%s %.1f' % kv for kv in r['timings_ms'].items())))
                extra.append('%s lazysp, CPU yardstick: plan_host on the first %d problems, one core: %.3f problems/s -> device / CPU = %.0fx'
                             % (name, r['cpu_sample'], r['cpu_rate'], r['rate'] / r['cpu_rate']))
        if stop:
            break
    for name in ('maze2', 'maze3'):
        if (name, 'lazysp') in got_all and (name, 'gnn') in got_all:
            lz, gn = got_all[(name, 'lazysp')], got_all[(name, 'gnn')]
            lines.append('%s: mean checks LazySP %.2f against GNN explorer %.2f (%.1f%% saved); solved %d against %d of %d'
                         % (name, lz['checks'], gn['checks'], 100.0 * (1.0 - gn['checks'] / lz['checks']), lz['solved'], gn['solved'],
                            lz['problems']))
    text = '\n'.join(lines + extra) + '\n'
    print(text)
    with open(a.out or os.path.join(REPO, 'profiles', 'lazysp_bench.txt'), 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
