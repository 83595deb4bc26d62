#!/usr/bin/env python
"""Device steering of the smoothing stage for the stick robot (gnnmp_stick_steer) against the host's
planner.smooth_step, on maze3 paths.  Run on an MI355X; not part of bench.py.

  python tools/stick_steer_bench.py                 -> profiles/stick_steer_bench.txt
  python tools/stick_steer_bench.py --resources     -> profiles/stick_steer_resources.txt (no GPU: compiles
                                                       csrc/maze_kernels.hip with the compiler's resource report)

Paths: the rounds planner's solutions of the first problems of tests/golden/evalset_maze3_first40_b200_k12_s9.npz,
repeated to 64 / 256 / 1024 paths.  Proposals: a seeded, untrained ModelSmoother(3, 3, 6, 128) whose last layer is scaled
by 0.05 (maze3 has no trained checkpoint).  Device time: one gnnmp_stick_steer launch between two events, median of 7
after 2 warm-up launches.  Host time: smooth_step over Maze3D once per distinct path on one core, summed with the
repetition counts."""
import argparse
import os
import re
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def resources(out):
    src = os.path.join(REPO, 'gnn-motion-planning_amd', 'csrc', 'maze_kernels.hip')
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fno-honor-nans', '-fPIC', '-c',
           '-Rpass-analysis=kernel-resource-usage', src, '-o', os.devnull]
    text = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.PIPE, universal_newlines=True, check=True).stderr
    lines, keep = [], False
    for ln in text.splitlines():
        m = re.search(r'remark:\s+(.*?)\s*\[-Rpass-analysis', ln)
        if not m:
            continue
        if m.group(1).startswith('Function Name'):
            keep = 'maze_steer_kernel' in m.group(1)
        if keep:
            lines.append(m.group(1))
    with open(out, 'w') as f:
        f.write('hipcc --offload-arch=gfx950 -O3 -fno-honor-nans -Rpass-analysis=kernel-resource-usage, maze_kernels.hip\n'
                '(ILi3E = stick robot, ILi2E = point robot)\n' + '\n'.join(lines) + '\n')
    print(open(out).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--problems', type=int, default=12)
    a = ap.parse_args()
    if a.resources:
        return resources(a.out or os.path.join(REPO, 'profiles', 'stick_steer_resources.txt'))
    import numpy as np
    import torch
    import gnnmp
    from gnnmp import _lib, planner
    from gnnmp.maze2d import Maze3D
    from gnnmp.weights import load_weights
    dev = 'cuda:0'
    with np.load(os.path.join(REPO, 'tests', 'golden', 'evalset_maze3_first40_b200_k12_s9.npz')) as f:
        env = Maze3D(f['maps'], f['init_states'], f['goal_states'])
        seed, batch, k = int(f['seed']), int(f['batch']), int(f['k'])
    m = gnnmp.EncoderProcessDecoder(2, 3, 32, 2).eval()
    m.load_state_dict(load_weights('weights_maze_3'))
    torch.manual_seed(0)
    ms = gnnmp.ModelSmoother(3, 3, 6, 128)
    sd = {key: t.clone() for key, t in ms.state_dict().items()}
    sd['smooth_node.weight'] *= 0.05
    sd['smooth_node.bias'] *= 0.05
    ms.load_state_dict(sd)
    ms.eval()
    det = []
    planner.eval_gnn_device_rounds(env, range(a.problems), m, None, seed=seed, batch=batch, t_max=batch, k=k, device=dev,
                                   details_out=det)
    det = [d for d in det if d['success'] and len(d['path']) >= 3]
    olds, news, maps, host_ms, host_checks = [], [], [], [], []
    with torch.no_grad():
        for d in det:
            v, nf = d['v'], d['n_free']
            data = planner.obs_data(d['env'], [x for x in v[:nf]], [x for x in v[nf:]], dev, for_smoother=True)
            path_t = torch.from_numpy(np.ascontiguousarray(d['path'], dtype=np.float32)).to(dev)
            new = ms(path=path_t, edge_index=planner.chain_edge_index(len(d['path'])).to(dev), loop=1, **data).cpu().numpy()
            olds.append(np.ascontiguousarray(d['path'], dtype=np.float32)); news.append(new)
            maps.append(np.asarray(d['env'].map, dtype=np.float64))
            e = d['env']
            c0, t0 = e.collision_check_count, time.perf_counter()
            planner.smooth_step([r.copy() for r in olds[-1]], new, e)
            host_ms.append((time.perf_counter() - t0) * 1e3)
            host_checks.append(e.collision_check_count - c0)
    lines = ['stick steering (gnnmp_stick_steer) on %s' % torch.cuda.get_device_name(0),
             '%d distinct paths (P = %s), host checks per path %s' % (len(olds), [len(o) for o in olds], host_checks),
             '%8s %12s %14s %10s %14s' % ('paths', 'device ms', 'host ms (1 core)', 'speed-up', 'checks')]
    for n in (64, 256, 1024):
        idx = [i % len(olds) for i in range(n)]
        lens = [len(olds[i]) for i in idx]
        ptr = torch.tensor(np.concatenate(([0], np.cumsum(lens))), dtype=torch.int32, device=dev)
        old_d = torch.from_numpy(np.concatenate([olds[i] for i in idx])).to(dev)
        new_d = torch.from_numpy(np.concatenate([news[i] for i in idx])).to(dev)
        maps_d = torch.from_numpy(np.stack([maps[i] for i in idx])).to(dev)
        # the ABI call alone between the events: every buffer exists beforehand (checks only accumulates while timing)
        out_d, tmp_d = torch.empty_like(old_d), torch.empty_like(old_d)
        acc = torch.zeros(n, dtype=torch.int64, device=dev)
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
        ts = []
        for rep in range(9):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(L.gnnmp_stick_steer(n, int(old_d.shape[0]), int(maps_d.shape[1]), maps_d.data_ptr(), ptr.data_ptr(),
                                           old_d.data_ptr(), new_d.data_ptr(), out_d.data_ptr(), tmp_d.data_ptr(),
                                           acc.data_ptr(), status.data_ptr(), st), 'gnnmp_stick_steer')
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        out, checks, status = planner.steer_maze_batch(old_d, new_d, ptr, maps_d)
        assert int(status.sum()) == 0 and torch.equal(out, out_d)
        assert checks.cpu().tolist() == [host_checks[i] for i in idx]
        assert acc.cpu().tolist() == [9 * host_checks[i] for i in idx]
        dev_ms = float(np.median(ts[2:]))
        h = sum(host_ms[i] for i in idx)
        lines.append('%8d %12.3f %14.1f %9.0fx %14d' % (n, dev_ms, h, h / dev_ms, int(checks.sum())))
    text = '\n'.join(lines) + '\n'
    print(text)
    out = a.out or os.path.join(REPO, 'profiles', 'stick_steer_bench.txt')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
