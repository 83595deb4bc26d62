#!/usr/bin/env python
"""The 3-D NEXT network kernels (the arm families) on an MI355X; not part of bench.py.

  python tools/next3d_bench.py                        -> profiles/next3d_bench.txt      (needs the GPU)
  python tools/next3d_bench.py --resources            -> profiles/next3d_resources.txt  (compiles only; no GPU needed)
  python tools/next3d_bench.py --cpu-reference DIR    appends the unmodified reference's CPU times (next_model/model3D.py under
                                                      DIR, which is not part of this repository) to the bench file

Timed with torch.cuda.Event around ``--reps`` back-to-back calls after ``--warmup`` calls of the same shape, the legs taken in
turn over ``--rounds`` rounds (so drift of a shared host hits every leg alike); per leg the median over rounds and the spread
(min .. max).  Legs: pb_forward at B = 1, 16, 64 (20 rounds, the recorded kuka7 maps repeated) and state_forward at S = 1, 12 and
1024 (problem_of_state shuffled over 16 problems).  For pb_forward the share of the fp32 MFMA peak counts the work the algorithm
needs -- per problem 2 x 3375 x (243 x 64 for hidden, 2 x 1728 x 64 for h0 and c0, and per round 1728 x 64 for conv plus
128 x 256 for the LSTM product) = 20.95 GFLOP at 20 rounds, 0.135 ms at 155 TFLOP/s -- over the measured time; the padding (27
tiles of 128 voxels, hidden's 9 channels to 16), the attention and the transcendentals are not counted, and the stages that run
on the double-precision MFMA are counted at the fp32 figure all the same.  No rate is asserted anywhere."""
import argparse
import os
import re
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PEAK_FP32_MFMA = 155e12
VOXELS = 3375
GOLD = os.path.join(REPO, 'tests', 'golden')


def flops_per_problem(iters=20):
    conv = VOXELS * 1728 * 64
    return 2 * (VOXELS * 243 * 64 + 2 * conv + iters * (conv + VOXELS * 128 * 256))


def resources(out):
    src = os.path.join(REPO, 'gnn-motion-planning_amd', 'csrc', 'next3d_kernels.hip')
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fno-honor-nans', '-fPIC', '-c', '-Rpass-analysis=kernel-resource-usage',
           src, '-o', os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True).stdout
    lines = ['# hipcc -Rpass-analysis=kernel-resource-usage over csrc/next3d_kernels.hip (gfx950, the build\'s flags)',
             '# LDS is static in every kernel; next3d_round_kernel<double x 4> serves the first round, <float x 4> the others']
    for ln in text.splitlines():
        m = re.search(r'remark: (?:\S+: )?\s*(Function Name: \S+|\s+(?:TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|'
                      r'LDS Size \[bytes/block\]): \d+)', ln)
        if m:
            lines.append(m.group(1).rstrip())
    open(out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def _fixture():
    import numpy as np
    from gnnmp import next_model3d
    w = next_model3d.load_npz_weights(os.path.join(GOLD, 'next_7_weights.npz'), os.path.join(GOLD, 'next_7_weights_b.npz'))
    with np.load(os.path.join(GOLD, 'next3d_kuka7_net.npz')) as f:
        return w, f['maps'].astype(np.float32), f['goals'], f['states']


def bench(args):
    import numpy as np
    import torch
    import gnnmp  # noqa: F401
    from gnnmp import next_model3d
    if not torch.cuda.is_available():
        raise SystemExit('next3d_bench: needs the GPU (nothing is measured on a CPU)')
    dev = torch.device('cuda:0')
    w, maps3, goals3, states24 = _fixture()
    net = next_model3d.NextNet3D(7, 3).load_state_dict(w)
    rng = np.random.RandomState(3)
    pick = np.arange(64) % 3
    maps = torch.from_numpy(maps3[pick]).to(dev)
    goals = torch.from_numpy(goals3[pick] + rng.uniform(-0.05, 0.05, (64, 10)).astype(np.float32)).to(dev)
    pb_all = net.pb_forward(maps[:16], goals[:16])
    legs = []
    for B in (1, 16, 64):
        legs.append(('pb_forward B=%d' % B, B, (lambda B=B: net.pb_forward(maps[:B], goals[:B]))))
    for S in (1, 12, 1024):
        st = torch.from_numpy(states24[rng.randint(0, 24, S)] + rng.uniform(-0.05, 0.05, (S, 10)).astype(np.float32)).to(dev)
        of = torch.from_numpy(rng.randint(0, 16, S).astype(np.int32)).to(dev)
        legs.append(('state_forward S=%d over 16 problems' % S, S, (lambda st=st, of=of: net.state_forward(st, of, pb_all))))
    for _, _, fn in legs:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    net.check_status()
    times = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, _, fn in legs:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.reps):
                fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / args.reps)
        net.check_status()
    lines = ['# tools/next3d_bench.py on %s: ms a call, median over %d rounds of %d calls (min .. max), %d warm-up calls a leg'
             % (torch.cuda.get_device_name(0), args.rounds, args.reps, args.warmup),
             '# includes the %d launches of a pb_forward and, per call, the allocation of the output tensor (state_forward: and its '
             'two status words)' % (4 + 20)]
    per_problem_64 = None
    for name, n, _ in legs:
        t = np.array(times[name])
        line = '%-40s %9.4f ms  (%.4f .. %.4f)  %10.1f per second' % (name, np.median(t), t.min(), t.max(), n / np.median(t) * 1e3)
        if name.startswith('pb_forward'):
            rate = n * flops_per_problem() / (np.median(t) * 1e-3)
            line += '  %6.2f TFLOP/s useful = %4.1f %% of the fp32 MFMA peak' % (rate / 1e12, 100 * rate / PEAK_FP32_MFMA)
            per_problem_64 = np.median(t) / n
        lines.append(line)
    floor = flops_per_problem() / PEAK_FP32_MFMA * 1e3
    lines += ['# %.2f GFLOP a problem at 20 rounds (counted from the shapes, padding excluded) = %.3f ms at %.0f TFLOP/s.'
              % (flops_per_problem() / 1e9, floor, PEAK_FP32_MFMA / 1e12),
              '# B = 64: %.3f ms a problem, %.1f x that floor.' % (per_problem_64, per_problem_64 / floor)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def cpu_reference(args):
    """Times of the unmodified reference module on this machine's CPUs, appended to the bench file."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.abspath(args.cpu_reference))
    sys.path.insert(0, os.path.join(REPO, 'tools', 'standins'))
    os.environ.setdefault('CUDA_VISIBLE_DEVICES', '')
    from next_model.model3D import PPN
    import gnnmp  # noqa: F401
    torch.set_num_threads(args.threads)
    w, maps3, goals3, states24 = _fixture()
    net = PPN(False, env_width=15, cap=8, dim=7, point_dim=3)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in w.items()})
    net.eval()
    lines = []
    with torch.no_grad():
        m, g = torch.from_numpy(maps3[:1]), torch.from_numpy(goals3[:1])
        pb = net.pb_forward(g, m)
        t = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            net.pb_forward(g, m)
            t.append((time.perf_counter() - t0) * 1e3)
        lines.append('# CPU yardstick: the unmodified reference (next_model/model3D.py:PPN, fp32, %d torch threads of %d CPUs, on a host '
                     'without a GPU -- the reference is timed where a copy of it exists): pb_forward of one problem %.0f ms '
                     '(median of %d, %.0f .. %.0f)' % (args.threads, os.cpu_count(), np.median(t), len(t), min(t), max(t)))
        for S in (1, 12, 1024):
            st = torch.from_numpy(states24[np.arange(S) % 24])
            net.state_forward(st, pb)
            t = []
            for _ in range(3 if S > 100 else args.rounds):
                t0 = time.perf_counter()
                net.state_forward(st, pb)
                t.append((time.perf_counter() - t0) * 1e3)
            lines.append('#   state_forward S=%d (one call, one problem): %.1f ms (%.1f .. %.1f)' % (S, np.median(t), min(t), max(t)))
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--cpu-reference', default=None, metavar='DIR')
    ap.add_argument('--threads', type=int, default=8)
    ap.add_argument('--out', default=None)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    if args.resources:
        resources(args.out or os.path.join(REPO, 'profiles', 'next3d_resources.txt'))
        return
    args.out = args.out or os.path.join(REPO, 'profiles', 'next3d_bench.txt')
    if args.cpu_reference:
        cpu_reference(args)
    else:
        bench(args)


if __name__ == '__main__':
    main()
