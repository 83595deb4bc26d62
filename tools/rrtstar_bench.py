#!/usr/bin/env python
"""The RRT* baseline on the device next to LazySP and the device GNN planner, on the same problems and seeds.  Run on an MI355X;
not part of bench.py.

  python tools/rrtstar_bench.py                 -> profiles/rrtstar_bench.txt

Sets: the first 1000 problems of tests/golden/evalset_mazehard_first1000.npz (point robot) and the 40 of
evalset_maze3_first40_b200_k12_s9.npz (stick robot).  RRT* runs at eval_rrt.py's setting (t_max = 1000, stop_when_success) through
rrtstar.eval_rrt_device on the whole set, once per way of drawing; its rate is set against rrtstar.plan_host on a sample of the
same problems on one core.  The comparison table -- success, mean collision checks, mean path cost -- covers the first
``--compare`` problems of each set for RRT*, LazySP (lazysp.eval_lazysp_device, batch = 50, t_max = 1000, k = 10) and the GNN
explorer (planner.eval_gnn_device_streams, batch = 500, t_max = 500, k = 30, no smoother), all with one sample stream per problem
and planner.stream_seeds(1234).  Every leg is a child process under its own ``timeout``; wall clock of one run after one warm-up
run.  No rate is asserted anywhere.  After a leg that fails, whatever the exit status, nothing more is started on the GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
RRT = dict(t_max=1000)
LAZY = dict(batch=50, t_max=1000, k=10)
GNN = dict(batch=500, t_max=500, k=30)
# the unmodified reference (eval_rrt.py's NEXT_plan, T = 1000) on one CPU core of the authoring machine, for scale
REFERENCE_CPU = 'about 0.2 s per maze2 problem and 0.4 - 0.8 s per maze3 problem'


def _load(name, need_model):
    import numpy as np
    import gnnmp
    from gnnmp.maze2d import Maze2D, Maze3D
    from gnnmp.weights import load_weights
    if name == 'maze2':
        with np.load(os.path.join(REPO, 'tests', 'golden', 'evalset_mazehard_first1000.npz')) as f:
            env = Maze2D(f['maps'], f['init_states'], f['goal_states'])
    else:
        with np.load(os.path.join(REPO, 'tests', 'golden', 'evalset_maze3_first40_b200_k12_s9.npz')) as f:
            env = Maze3D(f['maps'], f['init_states'], f['goal_states'])
    m = None
    if need_model:
        m = gnnmp.EncoderProcessDecoder(2, env.dim, 32, 2).eval()
        m.load_state_dict(load_weights('weights_maze' if name == 'maze2' else 'weights_maze_3'))
    return env, m


def child(name, which, compare, cpu_sample):
    import numpy as np
    import torch
    from gnnmp import lazysp, planner, rrtstar
    env, m = _load(name, which == 'gnn')
    dev = 'cuda:0'
    n_cmp = min(compare, env.size)
    res = {'set': name, 'planner': which}

    def timed(run):
        for rep in range(2):                                       # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        return out, dt
    if which == 'rrtstar':
        rows = []

        def run(draws):
            del rows[:]
            return rrtstar.eval_rrt_device(env, range(env.size), seed=1234, device=dev, draws=draws, rows_out=rows, **RRT)
        for draws in ('host', 'device'):
            _, dt = timed(lambda: run(draws))
            res['rate_' + draws] = env.size / dt
        tm = {}
        rrtstar.eval_rrt_device(env, range(env.size), seed=1234, device=dev, timings=tm, **RRT)
        res['timings_ms'] = {k: 1e3 * v for k, v in tm.items()}
        res['problems'] = env.size
        res['all'] = dict(solved=int(sum(r[0] for r in rows)), checks=float(np.mean([r[1] for r in rows])),
                          cost=float(np.mean([r[2] for r in rows if r[0]] or [float('nan')])), nodes=float(np.mean([r[3] for r in rows])))
        part = rows[:n_cmp]
        res.update(compared=n_cmp, solved=int(sum(r[0] for r in part)), checks=float(np.mean([r[1] for r in part])),
                   cost=float(np.mean([r[2] for r in part if r[0]] or [float('nan')])))
        seeds = planner.stream_seeds(1234, range(env.size))
        t0 = time.perf_counter()
        same = True
        for i in range(cpu_sample):
            h = rrtstar.plan_host(dict(map=env.maps[i], init_state=env.init_states[i], goal_state=env.goal_states[i]), seeds[i], **RRT)
            same = same and (int(h['success']), int(h['cumulated_collision_checks'][-1]) - int(h['cumulated_collision_checks'][1]),
                             float(h['path_lengths'][-1]), h['states'].shape[0], h['i']) == tuple(rows[i])
        res['cpu_rate'] = cpu_sample / (time.perf_counter() - t0)
        res['cpu_sample'], res['cpu_same'] = cpu_sample, bool(same)
    elif which == 'lazysp':
        out, dt = timed(lambda: lazysp.eval_lazysp_device(env, range(n_cmp), seed=1234, device=dev, **LAZY))
        res.update(compared=n_cmp, rate=n_cmp / dt, solved=int(out['n_success']), checks=float(out['collision']),
                   cost=float(out['solution_cost']))
    else:
        out, dt = timed(lambda: planner.eval_gnn_device_streams(env, range(n_cmp), m, None, seed=1234, device=dev, **GNN))
        res.update(compared=n_cmp, rate=n_cmp / dt, solved=int(out['n_success']), checks=float(out['collision_explore']),
                   cost=float(out['solution_cost']))
    print('RESULT ' + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--limit', type=int, default=170, help='seconds per leg')
    ap.add_argument('--compare', type=int, default=250, help='problems of each set in the comparison table')
    ap.add_argument('--cpu-sample', type=int, default=8, help='problems of each set plan_host runs for the CPU yardstick')
    ap.add_argument('--child', nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.compare, a.cpu_sample)
    lines = ['RRT* baseline on the device (rrtstar.eval_rrt_device, t_max = %(t_max)d, stop_when_success; tools/rrtstar_bench.py)' % RRT,
             'one sample stream per problem, seeds = planner.stream_seeds(1234); wall clock of one warm run; nothing here is a promise',
             '%-6s %9s %18s %20s %16s %8s %12s %10s %10s' % ('set', 'problems', 'problems/s (host', 'problems/s (device', 'plan_host 1 core',
                                                           'solved', 'mean checks', 'mean cost', 'mean nodes'),
             '%-6s %9s %18s %20s %16s' % ('', '', 'draws)', 'draws)', 'problems/s')]
    table = ['', 'comparison on the same problems and seeds (LazySP: batch = %d, t_max = %d, k = %d; ' % (LAZY['batch'], LAZY['t_max'], LAZY['k'])
             + 'GNN explorer: batch = %d, t_max = %d, k = %d, no smoother)' % (GNN['batch'], GNN['t_max'], GNN['k']),
             "RRT* checks are eval_rrt's: cumulated_collision_checks[-1] - cumulated_collision_checks[1], the first iteration's checks "
             'subtracted; RRT* cost is path_lengths[-1]',
             '%-6s %-8s %9s %12s %8s %14s %12s' % ('set', 'planner', 'problems', 'problems/s', 'solved', 'mean checks', 'mean cost')]
    extra = []
    stop = False
    for name in ('maze2', 'maze3'):
        for which in ('rrtstar', 'lazysp', 'gnn'):
            cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--cpu-sample', str(a.cpu_sample),
                   '--compare', str(a.compare), '--child', name, which]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            got = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
            if p.returncode != 0 or not got:
                table.append('%-6s %-8s did not finish (exit %d)' % (name, which, p.returncode))
                print(p.stdout[-3000:])
                table.append('stopped: nothing more is started on the GPU after a leg that failed')
                stop = True
                break
            r = json.loads(got[-1][7:])
            if which == 'rrtstar':
                lines.append('%-6s %9d %18.1f %20.1f %16.2f %8d %12.2f %10.4f %10.1f'
                             % (name, r['problems'], r['rate_host'], r['rate_device'], r['cpu_rate'], r['all']['solved'], r['all']['checks'],
                                r['all']['cost'], r['all']['nodes']))
                extra.append('%s rrtstar, stage wall clock with a device wait after each stage (ms, host draws): %s'
                             % (name, ', '.join('%s %.1f' % kv for kv in r['timings_ms'].items())))
                extra.append('%s rrtstar, CPU yardstick: plan_host on the first %d problems, one core: %.2f problems/s -> device / CPU = %.0fx '
                             '(host draws); its rows equal the device rows: %s'
                             % (name, r['cpu_sample'], r['cpu_rate'], r['rate_host'] / r['cpu_rate'], r['cpu_same']))
                table.append('%-6s %-8s %9d %12s %8d %14.2f %12.4f' % (name, which, r['compared'], '(above)', r['solved'], r['checks'], r['cost']))
            else:
                table.append('%-6s %-8s %9d %12.1f %8d %14.2f %12.4f' % (name, which, r['compared'], r['rate'], r['solved'], r['checks'], r['cost']))
        if stop:
            break
    extra.append('for scale, the unmodified reference on one CPU core (eval_rrt.py, T = 1000): ' + REFERENCE_CPU)
    text = '\n'.join(lines + table + [''] + extra) + '\n'
    print(text)
    with open(a.out or os.path.join(REPO, 'profiles', 'rrtstar_bench.txt'), 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
