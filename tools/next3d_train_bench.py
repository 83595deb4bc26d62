#!/usr/bin/env python
"""3-D NEXT training on the device (gnnmp.next_train3d.NextNet3DTrain, the arm families) on an MI355X; not part of bench.py.

  python tools/next3d_train_bench.py                  -> profiles/next3d_train_bench.txt      (needs the GPU)
  python tools/next3d_train_bench.py --resources      -> profiles/next3d_train_resources.txt  (compiles only; no GPU needed)

Legs, for kuka7 (next_7, point_dim 3) at 20 rounds and 8 states a path: one ``train_step`` (labels on the host, forward, loss,
backward, Adam) at 8 problems -- the reference's step -- and at 64; and the three library calls of a step on their own
(``gnnmp_next3d_train_forward``, ``gnnmp_next3d_state_backward``, ``gnnmp_next3d_pb_backward``).  Timed with torch.cuda.Event
around ``--reps`` back-to-back calls after ``--warmup`` calls, the legs taken in turn over ``--rounds`` rounds; per leg the median
over rounds and the spread.  The yardstick is the float32 torch restatement of tests/next3d_train_host.py (forward, loss,
backward, Adam) on this machine's CPU threads (at most 16), wall clock, median of ``--cpu-reps`` steps after one warm-up step.
No rate is asserted anywhere."""
import argparse
import ctypes
import os
import re
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
KINDS = r'TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]'
FLAGS = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fno-honor-nans', '-fPIC', '-c', '-Rpass-analysis=kernel-resource-usage']
DIM, PD, ITERS, PER_PATH = 7, 3, 20, 8


def _usage(name):
    src = os.path.join(REPO, 'gnn-motion-planning_amd', 'csrc', name)
    text = subprocess.run(FLAGS + [src, '-o', os.devnull], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                          check=True).stdout
    out = []
    for ln in text.splitlines():
        m = re.search(r'remark: (?:\S+: )?\s*(Function Name: \S+|\s+(?:%s): \d+)' % KINDS, ln)
        if m:
            out.append(m.group(1).rstrip())
    return out


def resources(out):
    """The training kernels' figures, and the inference kernels' figures again next to the recorded ones: the bodies moved into
    next3d_pb.hpp, the figures of profiles/next3d_resources.txt must not have moved."""
    lines = ['# hipcc -Rpass-analysis=kernel-resource-usage over csrc/next3d_train_kernels.hip (gfx950, the build\'s flags)',
             '# dynamic LDS a workgroup, beside the static figure below: next3d_attn_bwd_kernel %d bytes (2 x 3376 + 24 doubles,'
             % ((2 * 3376 + 24) * 8 + 128 * (97 + 65) * 4),
             '# 128 x (97 + 65) floats) of the 163840 a workgroup can have; nothing grows with the number of rounds.']
    train = _usage('next3d_train_kernels.hip')
    lines += train
    scratch = [int(ln.split(':')[1]) for ln in train if 'ScratchSize' in ln]
    lines.append('# scratch: %s' % ('none in any kernel' if not any(scratch) else 'PRESENT -- a finding to remove'))
    recorded = [ln.rstrip() for ln in open(os.path.join(REPO, 'profiles', 'next3d_resources.txt')) if not ln.startswith('#')]
    now = _usage('next3d_kernels.hip')
    same = [ln.strip() for ln in recorded] == [ln.strip() for ln in now]
    lines.append('# csrc/next3d_kernels.hip compiled again over next3d_pb.hpp: %s profiles/next3d_resources.txt (%d lines compared)'
                 % ('every figure equals' if same else 'DIFFERS FROM', len(now)))
    if not same:
        lines += ['# now: ' + ln for ln in now]
    open(out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    if not same or any(scratch):
        raise SystemExit(1)


def _batch(np, B):
    gold = os.path.join(REPO, 'tests', 'golden')
    with np.load(os.path.join(gold, 'next3d_kuka7_net.npz')) as f:
        base = f['maps'].astype(np.float32)
    rng = np.random.RandomState(11)
    maps = np.stack([np.roll(base[b % base.shape[0]], b // base.shape[0], axis=b % 3) for b in range(B)])
    goals = np.concatenate([rng.uniform(-1, 1, (B, PD)), rng.uniform(-2, 2, (B, DIM))], axis=1).astype(np.float32)
    paths = rng.uniform(-2, 2, (B * PER_PATH, DIM))
    points = rng.uniform(-1, 1, (B * PER_PATH, PD))
    ptr = np.arange(B + 1, dtype=np.int64) * PER_PATH
    return maps, goals, points, paths, ptr


def bench(args):
    import numpy as np
    import torch
    import gnnmp  # noqa: F401
    from gnnmp import _lib, next_train, next_train3d
    import next3d_train_host as host
    if not torch.cuda.is_available():
        raise SystemExit('next3d_train_bench: needs the GPU (nothing is measured on a CPU alone)')
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = torch.device('cuda:0')
    w = host.load_weights(DIM)
    legs, cpu = [], {}
    for B in (8, 64):
        maps, goals, points, paths, ptr = _batch(np, B)
        net = next_train3d.NextNet3DTrain(DIM, PD, device=dev).load_state_dict(w)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        dmaps, dgoals = torch.from_numpy(maps).to(dev), torch.from_numpy(goals).to(dev)
        rows_np = np.concatenate([points, paths], axis=1).astype(np.float32)
        rows = torch.from_numpy(rows_np).to(dev)
        of = torch.from_numpy(np.repeat(np.arange(B, dtype=np.int32), np.diff(ptr))).to(dev)
        tag = 'kuka7 B=%-2d ' % B
        legs.append((tag + 'train_step', lambda net=net, opt=opt, a=dmaps, g=dgoals, x=points, p=paths, q=ptr:
                     net.train_step(opt, a, g, x, p, q, 0.5, None, None, ITERS)))

        def fwd(net=net, a=dmaps, g=dgoals, s=rows, o=of):
            return net.forward(a, g, s, o, ITERS)
        legs.append((tag + 'gnnmp_next3d_train_forward (with the two packings)', fwd))
        y = fwd()
        ctx = y.grad_fn
        g_, s_, o_, packed, packed_t, pb_rep, ws = ctx.held
        dy = torch.randn_like(y)
        dpb, dw = torch.empty_like(pb_rep), torch.empty_like(packed)
        d = _lib.Next3dTrainBwd(B, int(s_.shape[0]), DIM, PD, 15, ITERS, g_.data_ptr(), s_.data_ptr(), o_.data_ptr(), packed.data_ptr(),
                                packed_t.data_ptr(), pb_rep.data_ptr(), dy.data_ptr(), dpb.data_ptr(), dw.data_ptr(), ws.data_ptr(),
                                ws.numel())
        keep = (ctx, dy, dpb, dw, d)

        def call(name, d=d, keep=keep):
            _lib.check(getattr(_lib.lib(), name)(ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream), name)
        legs.append((tag + 'gnnmp_next3d_state_backward', lambda call=call: call('gnnmp_next3d_state_backward')))
        legs.append((tag + 'gnnmp_next3d_pb_backward', lambda call=call: call('gnnmp_next3d_pb_backward')))
        # the yardstick: the float32 restatement on the CPU
        leaves = host.leaves(w, torch.float32)
        copt = torch.optim.Adam(list(leaves.values()), lr=1e-3)
        actions, values = next_train3d.path_labels(paths, ptr, 0.5)
        actions, values = torch.from_numpy(actions), torch.from_numpy(values)
        ts = []
        for _ in range(args.cpu_reps + 1):
            t0 = time.perf_counter()
            loss = next_train.loss_from_outputs(host.forward(leaves, maps, goals, rows_np, of.cpu().numpy(), ITERS), actions, values, ptr)
            copt.zero_grad()
            loss.backward()
            copt.step()
            ts.append((time.perf_counter() - t0) * 1e3)
            print('# CPU float32 restatement, B=%d: %.0f ms' % (B, ts[-1]), flush=True)
        cpu[tag] = float(np.median(ts[1:]))
    # a net's backward legs run on the workspace of that net's latest forward (the same shapes every time)
    order = legs
    for _, fn in order:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in order}
    for _ in range(args.rounds):
        for name, fn in order:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.reps):
                fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / args.reps)
    lines = ['# tools/next3d_train_bench.py on %s: ms a call, median over %d rounds of %d calls (min .. max), %d warm-up calls a leg'
             % (torch.cuda.get_device_name(0), args.rounds, args.reps, args.warmup),
             '# kuka7 (dim 7, point_dim 3), %d rounds, %d states a path; train_step = labels on the host + forward + loss + backward + Adam'
             % (ITERS, PER_PATH),
             '# CPU yardstick: the float32 torch restatement (tests/next3d_train_host.py), one step, %d torch threads, median of %d'
             % (torch.get_num_threads(), args.cpu_reps)]
    for name, _ in order:
        t = np.array(times[name])
        line = '%-66s %9.3f ms  (%.3f .. %.3f)' % (name, np.median(t), t.min(), t.max())
        if name.endswith('train_step'):
            tag = name[:-len('train_step')]
            line += '   CPU float32 restatement %9.1f ms = %.1f x' % (cpu[tag], cpu[tag] / np.median(t))
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--cpu-reps', type=int, default=1)
    args = ap.parse_args()
    if args.resources:
        resources(args.out or os.path.join(REPO, 'profiles', 'next3d_train_resources.txt'))
    else:
        args.out = args.out or os.path.join(REPO, 'profiles', 'next3d_train_bench.txt')
        bench(args)


if __name__ == '__main__':
    main()
