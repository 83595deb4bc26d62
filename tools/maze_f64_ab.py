#!/usr/bin/env python
"""The kernels that check float64 maze states, timed with two builds of libgnnmp.so in alternation: a comparison build
(--other, e.g. the parent commit's csrc/ compiled with build()'s flags) against the in-tree one.  Run on an MI355X; not part
of bench.py.

  python tools/maze_f64_ab.py --other /path/to/other/libgnnmp.so [--reps 5]      -> profiles/maze_f64_ab.txt

Every repeat is a child process of its own (GNNMP_LIB names the comparison build, or is unset), one at a time, the order
reversed every other repeat; after a child that fails nothing more is started.  Legs, in ms:
  label            gnnmp_episode_label_maze on the problems of tools/train_episodes_bench.py (256 synthetic problems of 100-400
                   nodes, kNN edges; maze3 = the same points with a drawn orientation), its timed(): mean of 20 calls after one
                   warm-up call; and on 64 problems of 200 nodes with random pairs of the whole square as edges on 64 x 64 maps
                   (0.2 % obstacles): the bisection at its full depth
  stick steer      planner.steer_maze_batch, the steer3 fixtures repeated to 1024 paths: median of 7 launches after 2
  stick sample     gnnmp_stick_sample as tools/stick_sample_bench.py times the launch alone, 256 problems, batch 200: same
  streams          tools/rounds_streams_bench.py _launch_times(): round 0 of the per-problem sample streams, maze3 and maze2
The margin is the spread (max - min) of the comparison build's own repeats."""
import argparse
import ctypes
import glob
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, os.path.join(REPO, 'tools'))
DEV = 'cuda:0'


def child():
    import torch
    import gnnmp  # noqa: F401
    from gnnmp import _lib, episodes as ep, planner
    from gnnmp.maze2d import LIMITS3
    import train_episodes_bench as TEB
    import rounds_streams_bench as RSB
    res = {}

    def median_launch(fn, reps=9, warm=2):
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts[warm:]))

    # ---- label stage (tools/train_episodes_bench.py: problems(), timed()), maze2 and maze3, B = 256
    for dim in (2, 3):
        sizes, pts2, maps = TEB.problems(256, 100 + 256)
        rng = np.random.default_rng(7)
        pts = pts2 if dim == 2 else np.concatenate([pts2, rng.uniform(-0.4, 0.4, (pts2.shape[0], 1))], axis=1)
        nptr = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        p64 = torch.from_numpy(np.ascontiguousarray(pts)).to(DEV)
        g = ep.maze_training_graphs(p64, nptr, maps, dim)
        maps_d = torch.from_numpy(maps).to(DEV)
        res['label maze%d B=256 (E=%d)' % (dim, g.total_edges)] = TEB.timed(lambda: ep.label_maze(g, p64, maps_d, dim), reps=20)
        res['_free%d' % dim] = int(g.edge_free.sum())

    # ---- label stage on long edges: 64 x 64 maps, 0.2 % obstacles, random pairs of the whole square (bisection depth up to 7)
    rng = np.random.default_rng(9)
    B, n = 64, 200
    pts = rng.uniform(-1, 1, (B * n, 2))
    maps = (rng.random((B, 64, 64)) < 0.002).astype(np.float64)
    ei = []
    for b in range(B):
        s = rng.integers(0, n, 2000)
        t = rng.integers(0, n, 2000)
        pairs = sorted({(int(x), int(y)) for x, y in zip(s, t) if x != y} | {(int(y), int(x)) for x, y in zip(s, t) if x != y})
        ei.append(np.array(pairs, dtype=np.int64).T)
    nptr = (np.arange(B + 1) * n).tolist()
    eptr = np.concatenate([[0], np.cumsum([e.shape[1] for e in ei])]).tolist()
    E = eptr[-1]
    p64 = torch.from_numpy(pts).to(DEV)
    g = ep.TrainingGraphs(p64.float(), torch.from_numpy(np.concatenate(ei, axis=1)).to(DEV), nptr, eptr,
                          torch.empty(E, dtype=torch.uint8, device=DEV), torch.empty(E, dtype=torch.float64, device=DEV),
                          torch.zeros(B, 2, device=DEV), list(range(B + 1)))
    maps_d = torch.from_numpy(maps).to(DEV)
    res['label maze2 long edges w=64 (E=%d)' % E] = TEB.timed(lambda: ep.label_maze(g, p64, maps_d, 2), reps=20)
    res['_free_long'] = int(g.edge_free.sum())

    # ---- stick steering: the steer3 fixtures repeated to 1024 paths, one launch (planner.steer_maze_batch)
    cases = []
    for f in sorted(glob.glob(os.path.join(REPO, 'tests', 'golden', 'steer3_*.npz'))):
        with np.load(f) as z:
            if not bool(z['raised']):
                cases.append({k: z[k] for k in ('old_path', 'new_path', 'map')})
    idx = [i % len(cases) for i in range(1024)]
    lens = [len(cases[i]['old_path']) for i in idx]
    ptr = torch.tensor(np.concatenate(([0], np.cumsum(lens))), dtype=torch.int32, device=DEV)
    old = torch.from_numpy(np.concatenate([cases[i]['old_path'] for i in idx])).to(DEV)
    new = torch.from_numpy(np.concatenate([cases[i]['new_path'] for i in idx])).to(DEV)
    mp = torch.from_numpy(np.stack([cases[i]['map'].astype(np.float64) for i in idx])).to(DEV)
    chk = torch.zeros(1024, dtype=torch.int64, device=DEV)
    st = torch.zeros(1024, dtype=torch.int32, device=DEV)
    tmp = torch.empty_like(old)
    res['stick steer 1024 paths'] = median_launch(lambda: planner.steer_maze_batch(old, new, ptr, mp, checks=chk, status=st, tmp=tmp))
    res['_steer_checks'] = int(chk.sum())

    # ---- stick sampling: the launch alone as tools/stick_sample_bench.py times it, 256 problems, batch 200
    with np.load(os.path.join(REPO, 'tests', 'golden', 'evalset_maze3_first40_b200_k12_s9.npz')) as f:
        maps, init, goal = f['maps'], f['init_states'], f['goal_states']
    B, batch = 256, 200
    sel = [i % maps.shape[0] for i in range(B)]
    as64 = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(DEV)      # noqa: E731
    maps_d, init64, goal64 = as64(maps[sel]), as64(init[sel].reshape(B, 3)), as64(goal[sel].reshape(B, 3))
    np.random.seed(9)
    draws = int(B * batch * 12) + 4096
    att = torch.from_numpy(np.random.uniform(-LIMITS3, LIMITS3, (draws, 3))).to(DEV)
    v = torch.empty(B * (2 + 2 * batch), 3, dtype=torch.float32, device=DEV)
    nptr_d = torch.empty(B + 1, dtype=torch.int32, device=DEV)
    used = torch.empty(B, dtype=torch.int32, device=DEV)
    chk = torch.empty(B, dtype=torch.int64, device=DEV)
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    sb = _lib.MazeSampleBatch(B, int(maps.shape[1]), batch, draws, att.data_ptr(), maps_d.data_ptr(), init64.data_ptr(), goal64.data_ptr())
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream


    def sample():
        state.zero_()
        _lib.check(L.gnnmp_stick_sample(ctypes.byref(sb), state.data_ptr(), v.data_ptr(), nptr_d.data_ptr(), used.data_ptr(),
                                        chk.data_ptr(), state.data_ptr() + 8, stream), 'gnnmp_stick_sample')


    res['stick sample 256 problems batch 200'] = median_launch(sample)
    assert state.cpu().tolist()[1] & 0xffffffff
    res['_sample_checks'] = int(chk.sum())

    # ---- round 0 of the per-problem sample streams (tools/rounds_streams_bench.py: _launch_times), maze3 and maze2
    for name in ('maze3', 'maze2'):
        env, m = RSB._load(name)
        for k, t in RSB._launch_times(env, m, DEV).items():
            res['streams %s: %s' % (name, k)] = t

    print('RESULT ' + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--other', default=None, help='the comparison build of libgnnmp.so')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'maze_f64_ab.txt'))
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child()
    if not a.other:
        ap.error('--other is required')
    runs = {'other': [], 'this': []}
    for rep in range(a.reps):
        for which in (('other', 'this') if rep % 2 == 0 else ('this', 'other')):
            env = dict(os.environ)
            env.pop('GNNMP_LIB', None)
            if which == 'other':
                env['GNNMP_LIB'] = os.path.abspath(a.other)
            p = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), '--child'], env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
            if p.returncode != 0 or not line:
                print('child %s rep %d failed rc %d\n%s\n%s' % (which, rep, p.returncode, p.stdout[-3000:], p.stderr[-3000:]), flush=True)
                sys.exit(1)
            runs[which].append(json.loads(line[0][7:]))
            print(which, rep, 'ok', flush=True)
    legs = [k for k in runs['this'][0] if not k.startswith('_')]
    lines = ['python tools/maze_f64_ab.py --other <comparison build> --reps %d: the comparison build ("other") against the in-tree one '
             '("this"), alternating child processes in one session on one MI355X' % a.reps,
             'ms per leg (see the tool for what each leg times); median and spread (max - min) over the %d processes of each build; '
             'margin = the spread of "other"' % a.reps,
             '%-46s | %10s %10s | %10s %10s | %10s  %s' % ('leg', 'other med', 'spread', 'this med', 'spread', 'this/other', 'verdict')]
    for k in legs:
        x = np.array([r[k] for r in runs['other']])
        y = np.array([r[k] for r in runs['this']])
        mx, my = float(np.median(x)), float(np.median(y))
        sx, sy = float(x.max() - x.min()), float(y.max() - y.min())
        verdict = 'slower beyond the spread' if my > mx + sx else ('faster beyond the spread' if my < mx - sx else 'within the spread')
        lines.append('%-46s | %10.4f %10.4f | %10.4f %10.4f | %10.3f  %s' % (k, mx, sx, my, sy, my / mx, verdict))
        lines.append('%-46s   other %s' % ('', ' '.join('%.4f' % t for t in x)))
        lines.append('%-46s   this  %s' % ('', ' '.join('%.4f' % t for t in y)))
    same = all(runs['this'][0][k] == r[k] for rr in runs.values() for r in rr for k in r if k.startswith('_'))
    lines.append('work done (free edges, check counts) identical in every process: %s  %s'
                 % (same, {k: v for k, v in runs['this'][0].items() if k.startswith('_')}))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
