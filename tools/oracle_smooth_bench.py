#!/usr/bin/env python
"""Throughput of gnnmp.oracle_smooth (joint_smoother_ratio, iters = 5, device-form draws) for 2048 and 6000 maze2 paths
under HIP events after a warm-up, against tests/oracle_smooth_host.py on a sample of the same paths on 16 CPU processes
(scaled to the batch), plus collision checks per second and the split trials / prune (a run with prune_iter = 0 does the
perturbation trials only).  The paths are the recorded fixtures' input paths (tests/golden/oracle_smooth_*.npz) repeated
with their own maps; every repeat gets its own draws.  ``--dim 3`` does the same for the stick robot: [sumP, 3] paths from
tests/golden/oracle_smooth3_*.npz against tests/oracle_smooth3_host.py (seconds per path there: keep --host-sample small).

    python tools/oracle_smooth_bench.py [--dim 2] [--paths 2048 6000] [--host-sample 32] [--reps 5]
"""
import argparse
import multiprocessing as mp
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import oracle_smooth3_host as H3  # noqa: E402
import oracle_smooth_host as H  # noqa: E402


def _host_one(args):
    path, maze, action, u = args
    t0 = time.perf_counter()
    r = (H3 if path.shape[1] == 3 else H).smooth(path, True, maze, action, u=u)
    return time.perf_counter() - t0, r[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--paths', type=int, nargs='+', default=[2048, 6000])
    ap.add_argument('--host-sample', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--dim', type=int, default=2, choices=(2, 3), help='2: point robot (default), 3: stick robot')
    a = ap.parse_args()
    import torch
    import gnnmp  # noqa: F401
    from gnnmp import oracle_smooth as OS
    dev = torch.device('cuda:0')
    fix = {n: f for n, f in (H3 if a.dim == 3 else H).fixtures().items() if bool(f['ratio']) and bool(f['in32']) and len(f['path']) >= 5}
    names = sorted(fix)
    print('paths: the %d recorded input paths of >= 5 waypoints (%s), repeated' % (len(names), ', '.join(
        '%s:%d' % (n, len(fix[n]['path'])) for n in names)))
    for B in a.paths:
        pick = [names[i % len(names)] for i in range(B)]
        paths = np.concatenate([fix[n]['path'] for n in pick]).astype(np.float32)
        ptr = np.cumsum([0] + [len(fix[n]['path']) for n in pick])
        maps = np.stack([fix[n]['map'] for n in pick])
        pt, mt = torch.from_numpy(paths).to(dev), torch.from_numpy(maps).to(dev)
        ptr_t = torch.from_numpy(ptr.astype(np.int32)).to(dev)
        draws = OS.draw_device(B, generator=torch.Generator(device=dev).manual_seed(B), dim=a.dim)
        res = {}
        for label, prune_iter in (('full', 100), ('trials only (prune_iter = 0)', 0)):
            r = OS.smooth(pt, ptr_t, mt, draws, prune_iter=prune_iter)            # warm-up
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = OS.smooth(pt, ptr_t, mt, draws, prune_iter=prune_iter)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            res[label] = (float(np.median(ms)), int(r['checks'].sum()), r)
            print('B = %5d  %-30s median of %d: %9.3f ms  (min %.3f, max %.3f; includes the wrapper\'s input copies)  '
                  '%.0f paths/s  %d checks  %.3e checks/s'
                  % (B, label, a.reps, res[label][0], min(ms), max(ms), B / res[label][0] * 1e3, res[label][1],
                     res[label][1] / res[label][0] * 1e3))
        full, trials = res['full'][0], res['trials only (prune_iter = 0)'][0]
        print('B = %5d  split: trials %.1f %%, prune + re-spacing %.1f %% of the full run (difference of the two runs; the '
              'trials of a run without prune see longer paths later on, so this is an estimate)'
              % (B, 100 * trials / full, 100 * (1 - trials / full)))
        status = res['full'][2]['status'].cpu().numpy()
        print('B = %5d  status bits seen: %s' % (B, sorted(set(int(s) for s in status))))
        # the host restatement on a sample of the same paths with the same draws, 16 processes
        k = min(a.host_sample, B)
        sel = np.linspace(0, B - 1, k).astype(int)
        act, u = draws['action'].cpu().numpy(), draws['u'].cpu().numpy()
        jobs = [(paths[ptr[b]:ptr[b + 1]].astype(np.float64), maps[b], act[b], u[b]) for b in sel]
        t0 = time.perf_counter()
        with mp.get_context('fork').Pool(16) as pool:
            out = pool.map(_host_one, jobs)
        wall = time.perf_counter() - t0
        dev_checks = res['full'][2]['checks'].cpu().numpy()[sel]
        same = all(int(c) == int(o[1]) for c, o in zip(dev_checks, out))
        per = float(np.mean([o[0] for o in out]))
        print('B = %5d  host restatement: %d sampled paths on 16 processes: %.2f s wall, %.3f s per path in one process; '
              'scaled to the batch on 16 processes: %.1f s  -> device speed-up %.0fx (scaled, not measured on the whole batch); '
              'sampled check counts equal the device\'s: %s'
              % (B, k, wall, per, per * B / 16, per * B / 16 / (full * 1e-3), same))


if __name__ == '__main__':
    main()
