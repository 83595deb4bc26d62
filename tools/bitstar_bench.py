#!/usr/bin/env python
"""The BIT* baseline on the device next to LazySP, RRT* and the device GNN planner, on the same problems and seeds.  Run on an
MI355X; not part of bench.py.

  python tools/bitstar_bench.py                 -> profiles/bitstar_bench.txt

Sets: the first 1000 problems of tests/golden/evalset_mazehard_first1000.npz (point robot) and the 40 of
evalset_maze3_first40_b200_k12_s9.npz (stick robot).  BIT* runs at eval_bit's setting (batch = 50, t_max = 1000, the search for
the first solution) through bitstar.eval_bit_device on the whole set; the two ways of drawing alternate, ``--reps`` runs each
after one warm-up run each, and the median is reported.  The stages (sampling, radius table, search launch, results) are timed
in a run of their own with a device wait after each.  Its rate is set against bitstar.plan_host on a sample of the same problems
on one core.  The comparison table -- solved, mean collision checks, mean path cost -- covers the first ``--compare`` problems
of each set for BIT*, LazySP (lazysp.eval_lazysp_device, batch = 50, t_max = 1000, k = 10), RRT* (rrtstar.eval_rrt_device,
t_max = 1000) and the GNN explorer (planner.eval_gnn_device_streams, batch = 500, t_max = 500, k = 30, no smoother), all with one
sample stream per problem and planner.stream_seeds(1234).  Every leg is a child process under its own ``timeout``.  No rate is
asserted anywhere.  After a leg that fails, whatever the exit status, nothing more is started on the GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
BIT = dict(batch=50, t_max=1000)
LAZY = dict(batch=50, t_max=1000, k=10)
RRT = dict(t_max=1000)
GNN = dict(batch=500, t_max=500, k=30)
# the unmodified reference (eval_bit's BITStar.plan, batch 50, T = 1000) on one CPU core of the authoring machine, for scale
REFERENCE_CPU = 'about 0.01 - 1 s per maze2 problem'


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


def child(name, which, compare, cpu_sample, reps):
    import numpy as np
    import torch
    from gnnmp import bitstar, lazysp, planner, rrtstar
    env, m = _load(name, which == 'gnn')
    dev = 'cuda:0'
    n_cmp = min(compare, env.size)
    res = {'set': name, 'planner': which}

    def clock(run):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    def timed(run):
        clock(run)                                                 # the first run warms up
        return clock(run)
    if which == 'bitstar':
        rows = []

        def run(draws):
            del rows[:]
            return bitstar.eval_bit_device(env, range(env.size), seed=1234, device=dev, draws=draws, rows_out=rows, **BIT)
        times = {'host': [], 'device': []}
        for draws in ('host', 'device'):
            clock(lambda: run(draws))
        for _ in range(reps):
            for draws in ('host', 'device'):                       # the legs alternate
                times[draws].append(clock(lambda: run(draws))[1])
        for draws in times:
            res['rate_' + draws] = env.size / float(np.median(times[draws]))
        tm = {}
        bitstar.eval_bit_device(env, range(env.size), seed=1234, device=dev, timings=tm, **BIT)
        res['timings_ms'] = {k: 1e3 * v for k, v in tm.items()}
        res['problems'] = env.size
        res['all'] = dict(solved=int(sum(r[0] for r in rows)), checks=float(np.mean([r[1] for r in rows])),
                          cost=float(np.mean([r[2] for r in rows if r[0]] or [float('nan')])), vertices=float(np.mean([r[3] for r in rows])),
                          nodes=float(np.mean([r[4] for r in rows])))
        part = rows[:n_cmp]
        res.update(compared=n_cmp, solved=int(sum(r[0] for r in part)), checks=float(np.mean([r[1] for r in part])),
                   cost=float(np.mean([r[2] for r in part if r[0]] or [float('nan')])))
        seeds = planner.stream_seeds(1234, range(env.size))
        t0 = time.perf_counter()
        same = True
        for i in range(cpu_sample):
            h = bitstar.plan_host(dict(map=env.maps[i], init_state=env.init_states[i], goal_state=env.goal_states[i]), seeds[i], **BIT)
            same = same and (int(h['g_goal'] < float('inf')), h['checks'], h['g_goal'], len(h['vertices']), h['points'].shape[0],
                             h['T']) == tuple(rows[i])
        res['cpu_rate'] = cpu_sample / (time.perf_counter() - t0)
        res['cpu_sample'], res['cpu_same'] = cpu_sample, bool(same)
    elif which == 'lazysp':
        out, dt = timed(lambda: lazysp.eval_lazysp_device(env, range(n_cmp), seed=1234, device=dev, **LAZY))
        res.update(compared=n_cmp, rate=n_cmp / dt, solved=int(out['n_success']), checks=float(out['collision']),
                   cost=float(out['solution_cost']))
    elif which == 'rrtstar':
        out, dt = timed(lambda: rrtstar.eval_rrt_device(env, range(n_cmp), seed=1234, device=dev, **RRT))
        res.update(compared=n_cmp, rate=n_cmp / dt, solved=int(out[0]), checks=float(out[1]), cost=float(out[2]))
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
    ap.add_argument('--reps', type=int, default=3, help='timed runs per way of drawing')
    ap.add_argument('--sets', default='maze2,maze3')
    ap.add_argument('--child', nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.compare, a.cpu_sample, a.reps)
    lines = ['BIT* baseline on the device (bitstar.eval_bit_device, batch = %(batch)d, t_max = %(t_max)d, first solution; '
             'tools/bitstar_bench.py)' % BIT,
             'one sample stream per problem, seeds = planner.stream_seeds(1234); median wall clock of %d warm runs per way of drawing, '
             'alternating; nothing here is a promise' % a.reps,
             '%-6s %9s %18s %20s %16s %8s %12s %10s %10s %10s' % ('set', 'problems', 'problems/s (host', 'problems/s (device', 'plan_host 1 core',
                                                                'solved', 'mean checks', 'mean cost', 'vertices', 'mean N'),
             '%-6s %9s %18s %20s %16s' % ('', '', 'draws)', 'draws)', 'problems/s')]
    table = ['', 'comparison on the same problems and seeds (LazySP: batch = %d, t_max = %d, k = %d; RRT*: t_max = %d; '
             % (LAZY['batch'], LAZY['t_max'], LAZY['k'], RRT['t_max'])
             + 'GNN explorer: batch = %d, t_max = %d, k = %d, no smoother)' % (GNN['batch'], GNN['t_max'], GNN['k']),
             "BIT* cost is g_scores[goal]; RRT* checks are eval_rrt's (the first iteration's checks subtracted), its cost is path_lengths[-1]",
             '%-6s %-8s %9s %12s %8s %14s %12s' % ('set', 'planner', 'problems', 'problems/s', 'solved', 'mean checks', 'mean cost')]
    extra = []
    stop = False
    for name in a.sets.split(','):
        for which in ('bitstar', 'lazysp', 'rrtstar', 'gnn'):
            cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--cpu-sample', str(a.cpu_sample),
                   '--compare', str(a.compare), '--reps', str(a.reps), '--child', name, which]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            got = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
            if p.returncode != 0 or not got:
                table.append('%-6s %-8s did not finish (exit %d)' % (name, which, p.returncode))
                print(p.stdout[-3000:])
                table.append('stopped: nothing more is started on the GPU after a leg that failed')
                stop = True
                break
            r = json.loads(got[-1][7:])
            if which == 'bitstar':
                lines.append('%-6s %9d %18.1f %20.1f %16.2f %8d %12.2f %10.4f %10.1f %10.1f'
                             % (name, r['problems'], r['rate_host'], r['rate_device'], r['cpu_rate'], r['all']['solved'], r['all']['checks'],
                                r['all']['cost'], r['all']['vertices'], r['all']['nodes']))
                extra.append('%s bitstar, stage wall clock with a device wait after each stage (ms, host draws; sampling = attempt blocks + '
                             'gnnmp_bitstar_sample + its readback, plan = the gnnmp_bitstar_plan launch alone): %s'
                             % (name, ', '.join('%s %.1f' % kv for kv in r['timings_ms'].items())))
                extra.append('%s bitstar, CPU yardstick: plan_host on the first %d problems, one core: %.2f problems/s -> device / CPU = %.0fx '
                             '(host draws); its rows equal the device rows: %s'
                             % (name, r['cpu_sample'], r['cpu_rate'], r['rate_host'] / r['cpu_rate'], r['cpu_same']))
                table.append('%-6s %-8s %9d %12s %8d %14.2f %12.4f' % (name, which, r['compared'], '(above)', r['solved'], r['checks'], r['cost']))
            else:
                table.append('%-6s %-8s %9d %12.1f %8d %14.2f %12.4f' % (name, which, r['compared'], r['rate'], r['solved'], r['checks'], r['cost']))
        if stop:
            break
    extra.append('for scale, the unmodified reference on one CPU core (eval_bit, batch 50, T = 1000): ' + REFERENCE_CPU)
    text = '\n'.join(lines + table + [''] + extra) + '\n'
    print(text)
    with open(a.out or os.path.join(REPO, 'profiles', 'bitstar_bench.txt'), 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
