#!/usr/bin/env python
"""The streams planner with its draws on the host against the same planner with its draws on the device, from the same build:
planner.eval_gnn_device_streams(draws='host') -- B numpy RandomState objects drawn in a Python loop per round, the path of
the commit before, so it is the yardstick -- against draws='device' (gnnmp.rng.MTStreams: numpy's MT19937 per problem in
one launch).  Run on an MI355X; not part of bench.py.

  python tools/mt_streams_bench.py                     -> profiles/mt_streams_bench.txt

Sets: the first 150 problems of tests/golden/evalset_mazehard_first1000.npz and the 40 of evalset_maze3_first40_b200_k12_s9.npz,
both at batch = 100, t_max = 300, k = 12, without a smoother (tools/rounds_streams_bench.py's).  One process, one GPU; every
run is a child process under its own ``timeout``; host and device legs alternate (--reps pairs per set, after one warm-up run
inside each child), the best wall clock of a leg is kept and every one is listed.  The 'sampling' share comes from a run of
its own with ``timings`` (they add a device wait per stage).  Both legs solve the same instances: the rows are compared and a
difference is reported.  No threshold is asserted.  After a run that fails, whatever the exit status, nothing more is started
on the GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
BATCH, T_MAX, K = 100, 300, 12


def _load(name):
    import numpy as np
    import gnnmp
    from gnnmp.maze2d import Maze2D, Maze3D
    from gnnmp.weights import load_weights
    if name == 'maze2':
        with np.load(os.path.join(REPO, 'tests', 'golden', 'evalset_mazehard_first1000.npz')) as f:
            env = Maze2D(f['maps'][:150], f['init_states'][:150], f['goal_states'][:150])
        m = gnnmp.EncoderProcessDecoder(2, 2, 32, 2).eval()
        m.load_state_dict(load_weights('weights_maze'))
    else:
        with np.load(os.path.join(REPO, 'tests', 'golden', 'evalset_maze3_first40_b200_k12_s9.npz')) as f:
            env = Maze3D(f['maps'], f['init_states'], f['goal_states'])
        m = gnnmp.EncoderProcessDecoder(2, 3, 32, 2).eval()
        m.load_state_dict(load_weights('weights_maze_3'))
    return env, m


def child(name, draws):
    import hashlib
    import torch
    from gnnmp import planner
    env, m = _load(name)
    kw = dict(seed=5, batch=BATCH, t_max=T_MAX, k=K, device='cuda:0', draws=draws)
    planner.eval_gnn_device_streams(env, range(env.size), m, None, **kw)          # warm-up
    torch.cuda.synchronize()
    rows = []
    t0 = time.perf_counter()
    out = planner.eval_gnn_device_streams(env, range(env.size), m, None, rows_out=rows, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tm = {}
    planner.eval_gnn_device_streams(env, range(env.size), m, None, timings=tm, **kw)
    res = {'set': name, 'draws': draws, 'problems': env.size, 'seconds': dt, 'rate': env.size / dt, 'solved': int(out['n_success']),
           'rows': hashlib.sha256(repr(rows).encode()).hexdigest()[:16], 'timings_ms': {k: 1e3 * v for k, v in tm.items()}}
    print('RESULT ' + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=2, help='host / device pairs per set')
    ap.add_argument('--limit', type=int, default=240, help='seconds per run')
    ap.add_argument('--child', nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1])
    lines = ["streams planner (eval_gnn_device_streams), draws='host' (numpy RandomState per problem in a Python loop: the commit "
             "before) against draws='device' (gnnmp_mt19937_uniform)",
             'batch = %d, t_max = %d, k = %d, no smoother; one warm run per child, legs alternating' % (BATCH, T_MAX, K),
             '%-6s %-7s %9s %12s %8s %14s %12s' % ('set', 'draws', 'problems', 'problems/s', 'solved', 'sampling ms', 'of all stages')]
    runs, failed = {}, False
    for name in ('maze2', 'maze3'):
        for rep in range(a.reps):
            for draws in ('host', 'device'):
                cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', name, draws]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                got = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
                if p.returncode != 0 or not got:
                    lines.append('%-6s %-7s did not finish (exit %d)' % (name, draws, p.returncode))
                    print(p.stdout[-2000:])
                    lines.append('stopped: nothing more is started on the GPU after a run that failed')
                    failed = True
                    break
                r = json.loads(got[-1][7:])
                runs.setdefault((name, draws), []).append(r)
                samp, total = r['timings_ms'].get('sampling', 0.), sum(r['timings_ms'].values())
                lines.append('%-6s %-7s %9d %12.1f %8d %14.1f %11.1f%%' % (name, draws, r['problems'], r['rate'], r['solved'], samp,
                                                                          100. * samp / max(total, 1e-9)))
            if failed:
                break
        if failed:
            break
    for name in ('maze2', 'maze3'):
        h, d = runs.get((name, 'host')), runs.get((name, 'device'))
        if h and d:
            bh, bd = max(r['rate'] for r in h), max(r['rate'] for r in d)
            sh, sd = min(r['timings_ms']['sampling'] for r in h), min(r['timings_ms']['sampling'] for r in d)
            same = len({r['rows'] for r in h + d}) == 1
            lines.append('%s: best of %d, device / host = %.2fx problems/s (%.1f / %.1f); sampling stage %.1f ms -> %.1f ms; rows %s'
                         % (name, len(h), bd / bh, bd, bh, sh, sd, 'identical' if same else 'DIFFER'))
    text = '\n'.join(lines) + '\n'
    print(text)
    out = a.out or os.path.join(REPO, 'profiles', 'mt_streams_bench.txt')
    with open(out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
