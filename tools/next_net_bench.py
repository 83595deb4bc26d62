#!/usr/bin/env python
"""The NEXT network kernels on an MI355X; not part of bench.py.

  python tools/next_net_bench.py                  -> profiles/next_net_bench.txt      (needs the GPU)
  python tools/next_net_bench.py --resources      -> profiles/next_net_resources.txt  (compiles only; no GPU needed)

Timed with torch.cuda.Event around ``--reps`` back-to-back calls after ``--warmup`` calls of the same shape, the legs taken in
turn over ``--rounds`` rounds (so drift of the shared host hits every leg alike); per leg the median over rounds and the spread
(min .. max).  Legs: pb_forward at B = 1, 64, 1000 (20 rounds, real maze2 maps of the evaluation set) and state_forward at
S = 12 and 12 x 1000 (12 states a problem, problem_of_state shuffled).  For pb_forward the share of the fp32 MFMA peak counts
the work the algorithm needs -- per problem 2 x (225 x 81 x 64 for hidden, 2 x 225 x 576 x 64 for h0 and c0, and per round
225 x 576 x 64 for conv plus 225 x 128 x 256 for the LSTM product) = 0.66 GFLOP at 20 rounds -- over the measured time against
157.3 TFLOP/s; the padding (16 row tiles, hidden's 9 channels to 16), the attention and the transcendentals are not counted.
No rate is asserted anywhere.  The CPU yardstick (unmodified reference, 4 torch threads, authoring machine): pb_forward 30-90 ms
a problem, state_forward of 64 states 26-70 ms."""
import argparse
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PEAK_FP32_MFMA = 157.3e12
CELLS = 225


def flops_per_problem(iters=20):
    conv = CELLS * 576 * 64
    return 2 * (CELLS * 81 * 64 + 2 * conv + iters * (conv + CELLS * 128 * 256))


def resources(out):
    src = os.path.join(REPO, 'gnn-motion-planning_amd', 'csrc', 'next_kernels.hip')
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fno-honor-nans', '-fPIC', '-c', '-Rpass-analysis=kernel-resource-usage',
           src, '-o', os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True).stdout
    lines = ['# hipcc -Rpass-analysis=kernel-resource-usage over csrc/next_kernels.hip (gfx950, the build\'s flags)',
             '# next_pb_kernel also uses %d bytes of dynamic LDS a workgroup (h, the conv output, the zero rows, the attention scratch)'
             % (2 * 257 * 68 * 4 + 96 * 8)]
    for ln in text.splitlines():
        m = re.search(r'remark: (?:\S+: )?\s*(Function Name: \S+|\s+(?:TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|'
                      r'LDS Size \[bytes/block\]): \d+)', ln)
        if m:
            lines.append(m.group(1).rstrip())
    open(out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def bench(args):
    import numpy as np
    import torch
    import gnnmp  # noqa: F401
    from gnnmp import next_model
    if not torch.cuda.is_available():
        raise SystemExit('next_net_bench: needs the GPU (nothing is measured on a CPU)')
    dev = torch.device('cuda:0')
    gold = os.path.join(REPO, 'tests', 'golden')
    with np.load(os.path.join(gold, 'next_2_weights.npz')) as f:
        net = next_model.NextNet(2).load_state_dict({k: f[k] for k in f.files})
    with np.load(os.path.join(gold, 'evalset_mazehard_first1000.npz')) as f:
        maps = torch.from_numpy(f['maps'][:1000].astype(np.float32)).to(dev)
        goals = torch.from_numpy(f['goal_states'][:1000].astype(np.float32)).to(dev)
    rng = np.random.RandomState(3)
    pb_all = net.pb_forward(maps, goals)
    legs = []
    for B in (1, 64, 1000):
        legs.append(('pb_forward B=%d' % B, B, (lambda B=B: net.pb_forward(maps[:B], goals[:B]))))
    for nb in (1, 1000):
        S = 12 * nb
        st = torch.from_numpy(rng.uniform(-1, 1, (S, 2)).astype(np.float32)).to(dev)
        of = torch.from_numpy(rng.permutation(np.repeat(np.arange(nb), 12)).astype(np.int32)).to(dev)
        legs.append(('state_forward S=%d over %d problems' % (S, nb), S, (lambda st=st, of=of, nb=nb: net.state_forward(st, of, pb_all[:nb]))))
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
    lines = ['# tools/next_net_bench.py on %s: ms a call, median over %d rounds of %d calls (min .. max), %d warm-up calls a leg'
             % (torch.cuda.get_device_name(0), args.rounds, args.reps, args.warmup),
             '# includes the launch and, per call, the allocation of the output tensor (state_forward: and its two status words)']
    for name, n, _ in legs:
        t = np.array(times[name])
        line = '%-44s %9.4f ms  (%.4f .. %.4f)  %10.1f per second' % (name, np.median(t), t.min(), t.max(), n / np.median(t) * 1e3)
        if name.startswith('pb_forward'):
            rate = n * flops_per_problem() / (np.median(t) * 1e-3)
            line += '  %6.2f TFLOP/s useful = %4.1f %% of the fp32 MFMA peak' % (rate / 1e12, 100 * rate / PEAK_FP32_MFMA)
        lines.append(line)
    lines += ['# %.3f GFLOP a problem at 20 rounds (counted from the shapes, padding excluded).' % (flops_per_problem() / 1e9),
              '# Which limit: one workgroup a problem, one workgroup a CU (140 KB of LDS), so a call takes ceil(B / CUs) times the',
              '# latency of one problem on one CU: B = 1 and B = 64 measure that latency with most of the chip idle, B = 1000 is 4',
              '# such passes on 256 CUs.  Inside the CU, counted from the code: 2176 MFMAs a wave a round (1152 convolution + 1024',
              '# LSTM) x 2 waves a SIMD x 32 cycles = 139 k cycles a round, 2.96 M cycles a problem with the three opening',
              '# convolutions = 1.23 ms at a nominal 2.4 GHz; the rest of the measured latency is not MFMA issue.  Not measured (no',
              '# counter run was taken): how that rest splits between the weight stream from L2 (every wave loads all 278 KB a',
              '# round), the LDS operand reads, the accurate expf / tanhf of the LSTM and the two barriers a round, and the clock.',
              '# CPU yardstick (unmodified reference, 4 torch threads, authoring machine): pb_forward 30-90 ms a problem,',
              '# state_forward of 64 states 26-70 ms.']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    if args.resources:
        resources(args.out or os.path.join(REPO, 'profiles', 'next_net_resources.txt'))
    else:
        args.out = args.out or os.path.join(REPO, 'profiles', 'next_net_bench.txt')
        bench(args)


if __name__ == '__main__':
    main()
