#!/usr/bin/env python
"""NEXT's guided planner on the device next to LazySP, RRT*, BIT* and the device GNN planner, on the same problems and seeds.
Run on an MI355X; not part of bench.py.

  python tools/next_plan_bench.py               -> profiles/next_plan_bench.txt

Sets: the first 1000 problems of tests/golden/evalset_mazehard_first1000.npz (point robot, next_2) and the 40 of
evalset_maze3_first40_b200_k12_s9.npz (stick robot, next_3); the checkpoints are tests/golden/next_{2,3}_weights.npz.  NEXT runs at
eval_next's setting (t_max = 1000, g_explore_eps = 0.1, k = 10, stop at the first success) through next_plan.eval_next_device on
the whole set, ``--reps`` runs after one warm-up run, the median is reported; the stages (pb_forward, draws, the launch alone,
results) are timed in a run of their own with a device wait after each.  Its rate is set against next_plan.plan_host on the
device model (three network calls and three host round trips an iteration) on a sample of the same problems.  The NEXT row of
the comparison table -- solved, mean collision checks with eval_next's first-iteration quirk, mean path cost -- covers the first
``--compare`` problems of each set; the rows of the other planners are read from profiles/bitstar_bench.txt, which
tools/bitstar_bench.py measures on the same problems with planner.stream_seeds(1234).  Every leg is a child process under its
own ``timeout``.  No rate is asserted anywhere.  After a leg that fails, whatever the exit status, nothing more is started on
the GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
NEXT = dict(t_max=1000)


def _load(name):
    import numpy as np
    from gnnmp.maze2d import Maze2D, Maze3D
    from gnnmp.next_model import Model2D
    if name == 'maze2':
        with np.load(os.path.join(REPO, 'tests', 'golden', 'evalset_mazehard_first1000.npz')) as f:
            env = Maze2D(f['maps'], f['init_states'], f['goal_states'])
    else:
        with np.load(os.path.join(REPO, 'tests', 'golden', 'evalset_maze3_first40_b200_k12_s9.npz')) as f:
            env = Maze3D(f['maps'], f['init_states'], f['goal_states'])
    with np.load(os.path.join(REPO, 'tests', 'golden', 'next_%d_weights.npz' % env.dim)) as f:
        model = Model2D(None, dim=env.dim, device='cuda:0').load_state_dict({k: f[k] for k in f.files})
    return env, model


def child(name, compare, cpu_sample, reps):
    import numpy as np
    import torch
    from gnnmp import next_plan, planner
    env, model = _load(name)
    dev = 'cuda:0'
    n_cmp = min(compare, env.size)
    res = {'set': name, 'problems': env.size}
    rows = []

    def run():
        del rows[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        next_plan.eval_next_device(env, range(env.size), model.net, seed=1234, device=dev, rows_out=rows, **NEXT)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    run()
    res['rate'] = env.size / float(np.median([run() for _ in range(reps)]))
    tm = {}
    next_plan.eval_next_device(env, range(env.size), model.net, seed=1234, device=dev, timings=tm, **NEXT)
    res['timings_ms'] = {k: 1e3 * v for k, v in tm.items()}
    res['all'] = dict(solved=int(sum(r[0] for r in rows)), checks=float(np.mean([r[1] for r in rows])),
                      cost=float(np.mean([r[2] for r in rows if r[0]] or [float('nan')])), nodes=float(np.mean([r[3] for r in rows])),
                      guided=float(np.mean([r[5] for r in rows])))
    part = rows[:n_cmp]
    res.update(compared=n_cmp, solved=int(sum(r[0] for r in part)), checks=float(np.mean([r[1] for r in part])),
               cost=float(np.mean([r[2] for r in part if r[0]] or [float('nan')])))
    seeds = planner.stream_seeds(1234, range(env.size))
    t0 = time.perf_counter()
    same = True
    for i in range(cpu_sample):
        pr = dict(map=env.maps[i], init_state=env.init_states[i], goal_state=env.goal_states[i])
        model.set_problem(pr)
        eps = next_plan.default_eps([seeds[i]], NEXT['t_max'], 10, env.dim)[0]
        h = next_plan.plan_host(pr, seeds[i], next_plan.NoiseModel(model, eps), **NEXT)
        same = same and (int(h['success']), h['states'].shape[0], h['i'], h['stats']['guided']) == (rows[i][0], rows[i][3], rows[i][4], rows[i][5])
    model.check_status()
    res['host_rate'] = cpu_sample / (time.perf_counter() - t0)
    res['cpu_sample'], res['cpu_same'] = cpu_sample, bool(same)
    print('RESULT ' + json.dumps(res), flush=True)


def _other_rows(compare):
    """The comparison rows of the other planners as tools/bitstar_bench.py wrote them (same problems, same seeds)."""
    path = os.path.join(REPO, 'profiles', 'bitstar_bench.txt')
    rows = []
    if os.path.exists(path):
        for ln in open(path).read().splitlines():
            parts = ln.split()
            if len(parts) >= 7 and parts[0] in ('maze2', 'maze3') and parts[1] in ('bitstar', 'lazysp', 'rrtstar', 'gnn') \
                    and parts[2] == str(compare if parts[0] == 'maze2' else min(compare, 40)):
                rows.append(ln)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--limit', type=int, default=400, help='seconds per leg')
    ap.add_argument('--compare', type=int, default=250, help='problems of each set in the comparison table')
    ap.add_argument('--cpu-sample', type=int, default=2, help='problems of each set plan_host runs on the device model')
    ap.add_argument('--reps', type=int, default=3, help='timed runs')
    ap.add_argument('--sets', default='maze2,maze3')
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.compare, a.cpu_sample, a.reps)
    lines = ['NEXT guided planner on the device (next_plan.eval_next_device, t_max = %(t_max)d, g_explore_eps = 0.1, k = 10, c = 1, stop at '
             'the first success; tools/next_plan_bench.py)' % NEXT,
             'one numpy stream and one noise block per problem, seeds = planner.stream_seeds(1234); median wall clock of %d warm runs; '
             'nothing here is a promise' % a.reps,
             '%-6s %9s %12s %22s %8s %12s %10s %10s %12s' % ('set', 'problems', 'problems/s', 'plan_host problems/s', 'solved', 'mean checks',
                                                          'mean cost', 'mean nodes', 'mean guided')]
    table = ['', "comparison on the same problems and seeds; NEXT and RRT* checks are eval_next's / eval_rrt's (the first iteration's checks "
             'subtracted), their cost is path_lengths[-1]; the other rows are those of profiles/bitstar_bench.txt',
             '%-6s %-8s %9s %12s %8s %14s %12s' % ('set', 'planner', 'problems', 'problems/s', 'solved', 'mean checks', 'mean cost')]
    extra = []
    for name in a.sets.split(','):
        cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--cpu-sample', str(a.cpu_sample),
               '--compare', str(a.compare), '--reps', str(a.reps), '--child', name]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
        if p.returncode != 0 or not got:
            table.append('%-6s %-8s did not finish (exit %d)' % (name, 'next', p.returncode))
            print(p.stdout[-3000:])
            table.append('stopped: nothing more is started on the GPU after a leg that failed')
            break
        r = json.loads(got[-1][7:])
        lines.append('%-6s %9d %12.1f %22.3f %8d %12.2f %10.4f %10.1f %12.1f'
                     % (name, r['problems'], r['rate'], r['host_rate'], r['all']['solved'], r['all']['checks'], r['all']['cost'],
                        r['all']['nodes'], r['all']['guided']))
        extra.append('%s, stage wall clock with a device wait after each stage (ms; plan = the gnnmp_next_plan launch alone): %s'
                     % (name, ', '.join('%s %.1f' % kv for kv in r['timings_ms'].items())))
        extra.append('%s, plan_host on the device model (per problem: one stream, three network calls and host round trips an iteration) on '
                     'the first %d problems: %.3f problems/s -> device loop / plan_host = %.0fx; its (success, nodes, i, guided) equal the '
                     'device rows: %s' % (name, r['cpu_sample'], r['host_rate'], r['rate'] / r['host_rate'], r['cpu_same']))
        table.append('%-6s %-8s %9d %12.1f %8d %14.2f %12.4f' % (name, 'next', r['compared'], r['rate'], r['solved'], r['checks'], r['cost']))
    table.extend(_other_rows(a.compare))
    text = '\n'.join(lines + table + [''] + extra) + '\n'
    print(text)
    with open(a.out or os.path.join(REPO, 'profiles', 'next_plan_bench.txt'), 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
