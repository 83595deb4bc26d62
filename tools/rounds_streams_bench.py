#!/usr/bin/env python
"""Resample rounds on the device, two ways, from the same build: planner.eval_gnn_device_rounds (one global sample stream,
speculation over chunks; unchanged, so it stands in for the commit before) against planner.eval_gnn_device_streams (one
stream per problem, round r of all unfinished problems as one batch).  Run on an MI355X; not part of bench.py.

  python tools/rounds_streams_bench.py                 -> profiles/rounds_streams_bench.txt

Sets: the first 150 problems of tests/golden/evalset_mazehard_first1000.npz and the 40 of evalset_maze3_first40_b200_k12_s9.npz,
both at batch = 100, t_max = 300, k = 12, without a smoother.  One process, one GPU; every run is a child process under its own
``timeout``.  Wall clock of one run after one warm-up run each (--reps for more, the best is kept).  The streams differ, so
the two planners solve slightly different instances: the success counts are printed beside the rates.  ``timings`` of the new
path (they add device waits, so they come from a run of their own; 'sampling' holds the per-round read of the sampler's status /
used / collided counts) and the device time of the three new launches and of gnnmp_maze_explore_ex between them (events
around each launch in a replay of round 0 of the set, median of 5) follow.  After a run that fails, whatever the exit
status, nothing more is started on the GPU."""
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


def _launch_times(env, model, dev):
    """Device time (ms) of the sampler, gather, explore and carry launches in round 0 of the whole set."""
    import numpy as np
    import torch
    from gnnmp import planner
    from gnnmp.graph_build import build_edges_gpu, k1_of
    B, dim = env.size, env.config_dim
    lim = np.asarray(env.SAMPLE_LIMITS)
    as64 = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(dev)      # noqa: E731
    maps, init64, goal64 = as64(env.maps), as64(env.init_states.reshape(B, dim)), as64(env.goal_states.reshape(B, dim))
    blocks = [np.random.RandomState(i).uniform(-lim, lim, (BATCH * 16, dim)) for i in range(B)]
    ptr = np.concatenate(([0], np.cumsum([b.shape[0] for b in blocks])))
    att = torch.from_numpy(np.concatenate(blocks)).to(dev)
    out = {'sample': [], 'gather': [], 'output fills + explore_ex': [], 'carry': []}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return r, a.elapsed_time(b)
    for rep in range(7):
        store = planner.MazeRoundsStore(B, T_MAX, planner.rounds_pair_cap(BATCH, T_MAX, K), dim, dev)
        torch.cuda.synchronize()
        (_, _, status), t_s = timed(lambda: planner.maze_sample_streams(store, att, ptr, maps, init64, goal64, BATCH))
        assert not status.any().item()
        rows = B * (BATCH + 2) + int(store.n_coll.sum().item())
        g, t_g = timed(lambda: planner.maze_rounds_gather(store, B, rows))
        ei, edge_ptr = build_edges_gpu(g['v'], g['node_ptr'], g['n_free'], [k1_of(K, BATCH + 2)] * B)
        scores = torch.rand(ei.shape[1], generator=torch.Generator().manual_seed(rep)).to(dev)
        torch.cuda.synchronize()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        cstat = planner.maze_rounds_explore(store, g, ei, edge_ptr, scores, maps, goal64, between=e1.record)
        e2.record()
        e2.synchronize()
        assert not cstat.any().item()
        if rep >= 2:
            out['sample'].append(t_s); out['gather'].append(t_g)
            out['output fills + explore_ex'].append(e0.elapsed_time(e1)); out['carry'].append(e1.elapsed_time(e2))
    return {k: float(np.median(v)) for k, v in out.items()}


def child(name, which, reps):
    import numpy as np
    import torch
    from gnnmp import planner
    env, m = _load(name)
    dev = 'cuda:0'
    fn = planner.eval_gnn_device_rounds if which == 'rounds' else planner.eval_gnn_device_streams
    kw = dict(seed=5, batch=BATCH, t_max=T_MAX, k=K, device=dev)
    res = {'set': name, 'planner': which, 'problems': env.size}
    best = None
    for rep in range(reps + 1):                                   # the first run warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(env, range(env.size), m, None, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rep:
            best = dt if best is None else min(best, dt)
    res.update(seconds=best, rate=env.size / best, solved=int(out['n_success']), multi=int((np.array(out['rounds']) > 1).sum()),
               max_rounds=int(max(out['rounds'])))
    if which == 'streams':
        tm = {}
        planner.eval_gnn_device_streams(env, range(env.size), m, None, timings=tm, **kw)
        res['timings_ms'] = {k: 1e3 * v for k, v in tm.items()}
        res['launch_ms'] = _launch_times(env, m, dev)
    print('RESULT ' + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=1)
    ap.add_argument('--limit', type=int, default=240, help='seconds per run')
    ap.add_argument('--child', nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.reps)
    lines = ['resample rounds on the device: global stream (eval_gnn_device_rounds) against one stream per problem '
             '(eval_gnn_device_streams)', 'batch = %d, t_max = %d, k = %d, no smoother; wall clock of one warm run' % (BATCH, T_MAX, K),
             '%-6s %-8s %9s %12s %8s %12s %11s' % ('set', 'planner', 'problems', 'problems/s', 'solved', 'multi-round', 'max rounds')]
    rates, extra = {}, []
    for name in ('maze2', 'maze3'):
        for which in ('rounds', 'streams'):
            cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), '--child',
                   name, which]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            got = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
            if p.returncode != 0 or not got:
                lines.append('%-6s %-8s did not finish (exit %d)' % (name, which, p.returncode))
                print(p.stdout[-2000:])
                lines.append('stopped: nothing more is started on the GPU after a run that failed')
                break
            r = json.loads(got[-1][7:])
            rates[(name, which)] = r['rate']
            lines.append('%-6s %-8s %9d %12.1f %8d %12d %11d' % (name, which, r['problems'], r['rate'], r['solved'], r['multi'],
                                                                r['max_rounds']))
            if which == 'streams':
                extra.append('%s streams, stage wall clock with a device wait after each stage (ms): %s'
                             % (name, ', '.join('%s %.1f' % kv for kv in r['timings_ms'].items())))
                extra.append('%s streams, device time of one launch over all %d problems, round 0 (ms): %s'
                             % (name, r['problems'], ', '.join('%s %.3f' % kv for kv in r['launch_ms'].items())))
        else:
            continue
        break
    for name in ('maze2', 'maze3'):
        if (name, 'rounds') in rates and (name, 'streams') in rates:
            lines.append('%s: streams / rounds = %.1fx' % (name, rates[(name, 'streams')] / rates[(name, 'rounds')]))
    lines += extra
    text = '\n'.join(lines) + '\n'
    print(text)
    out = a.out or os.path.join(REPO, 'profiles', 'rounds_streams_bench.txt')
    with open(out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
