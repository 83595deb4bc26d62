#!/usr/bin/env python
"""NEXT training on the device (gnnmp.next_train.NextNetTrain) on an MI355X; not part of bench.py.

  python tools/next_train_bench.py                  -> profiles/next_train_bench.txt      (needs the GPU)
  python tools/next_train_bench.py --resources      -> profiles/next_train_resources.txt  (compiles only; no GPU needed)

Legs: one ``train_step`` (labels on the host, forward, loss, backward, Adam) at 8 problems -- the reference's step -- and at 64,
for both robots, at 20 rounds, 10 states a path; and the three library calls of a step on their own (``gnnmp_next_train_forward``,
``gnnmp_next_state_backward``, ``gnnmp_next_pb_backward``).  Timed with torch.cuda.Event around ``--reps`` back-to-back calls
after ``--warmup`` calls, the legs taken in turn over ``--rounds`` rounds; per leg the median over rounds and the spread.  The
yardstick is the float32 torch restatement of tests/next_train_host.py (forward, loss, backward, Adam) on this machine's CPU
threads, wall clock, median of ``--cpu-reps`` steps.  No rate is asserted anywhere."""
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


def resources(out):
    src = os.path.join(REPO, 'gnn-motion-planning_amd', 'csrc', 'next_train_kernels.hip')
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fno-honor-nans', '-fPIC', '-c', '-Rpass-analysis=kernel-resource-usage',
           src, '-o', os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True).stdout
    buf = 2 * 257 * 68 * 4
    lines = ['# hipcc -Rpass-analysis=kernel-resource-usage over csrc/next_train_kernels.hip (gfx950, the build\'s flags)',
             '# dynamic LDS a workgroup, beside the static figure below: next_pb_train_kernel %d bytes (as next_pb_kernel),' % (buf + 96 * 8),
             '# next_pb_bwd_kernel %d (dh and dx rows, a zero row each), next_attn_bwd_kernel %d (628 doubles, 225 x (97 + 65) floats)'
             % (buf, 628 * 8 + 225 * (97 + 65) * 4),
             '# of the 163840 a workgroup can have; none grows with the number of rounds.']
    scratch = []
    for ln in text.splitlines():
        m = re.search(r'remark: (?:\S+: )?\s*(Function Name: \S+|\s+(?:%s): \d+)' % KINDS, ln)
        if m:
            lines.append(m.group(1).rstrip())
            if 'ScratchSize' in m.group(1):
                scratch.append(int(m.group(1).split(':')[1]))
    lines.append('# scratch: %s' % ('none in any kernel' if not any(scratch) else 'PRESENT -- a finding to remove'))
    open(out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def _batch(np, dim, B, per_path=10):
    gold = os.path.join(REPO, 'tests', 'golden')
    with np.load(os.path.join(gold, 'evalset_mazehard_first1000.npz')) as f:
        maps = f['maps'][:B].astype(np.float32)
    rng = np.random.RandomState(5 + dim)
    goals = rng.uniform(-1, 1, (B, dim)).astype(np.float32)
    paths = rng.uniform(-1, 1, (B * per_path, dim))
    ptr = np.arange(B + 1, dtype=np.int64) * per_path
    return maps, goals, paths, ptr


def bench(args):
    import numpy as np
    import torch
    import gnnmp  # noqa: F401
    from gnnmp import _lib, next_train
    import next_train_host as host
    if not torch.cuda.is_available():
        raise SystemExit('next_train_bench: needs the GPU (nothing is measured on a CPU alone)')
    dev = torch.device('cuda:0')
    gold = os.path.join(REPO, 'tests', 'golden')
    legs, cpu = [], {}
    for dim in (2, 3):
        with np.load(os.path.join(gold, 'next_%d_weights.npz' % dim)) as f:
            w = {k: f[k] for k in f.files}
        for B in (8, 64):
            maps, goals, paths, ptr = _batch(np, dim, B)
            net = next_train.NextNetTrain(dim, device=dev).load_state_dict(w)
            opt = torch.optim.Adam(net.parameters(), lr=1e-3)
            dmaps, dgoals = torch.from_numpy(maps).to(dev), torch.from_numpy(goals).to(dev)
            states = torch.from_numpy(paths.astype(np.float32)).to(dev)
            of = torch.from_numpy(np.repeat(np.arange(B, dtype=np.int32), np.diff(ptr))).to(dev)
            tag = 'dim %d B=%-2d ' % (dim, B)
            legs.append((tag + 'train_step', lambda net=net, opt=opt, a=dmaps, g=dgoals, p=paths, q=ptr: net.train_step(opt, a, g, p, q, 20)))

            def fwd(net=net, a=dmaps, g=dgoals, s=states, o=of):
                return net.forward(a, g, s, o, 20)
            legs.append((tag + 'gnnmp_next_train_forward (with the two packings)', fwd))
            y = fwd()
            ctx = y.grad_fn
            g_, s_, o_, packed, packed_t, pb_rep, ws = ctx.held
            dy = torch.randn_like(y)
            dpb, dw = torch.empty_like(pb_rep), torch.empty_like(packed)
            d = _lib.NextTrainBwd(B, int(s_.shape[0]), dim, 15, 20, g_.data_ptr(), s_.data_ptr(), o_.data_ptr(), packed.data_ptr(),
                                  packed_t.data_ptr(), pb_rep.data_ptr(), dy.data_ptr(), dpb.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel())
            keep = (ctx, dy, dpb, dw, d)

            def call(name, d=d, keep=keep):
                _lib.check(getattr(_lib.lib(), name)(ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream), name)
            legs.append((tag + 'gnnmp_next_state_backward', lambda call=call: call('gnnmp_next_state_backward')))
            legs.append((tag + 'gnnmp_next_pb_backward', lambda call=call: call('gnnmp_next_pb_backward')))
            # the yardstick: the float32 restatement on the CPU
            leaves = host.leaves(w, torch.float32)
            copt = torch.optim.Adam(list(leaves.values()), lr=1e-3)
            actions, values = next_train.path_labels(paths, ptr, dim)
            actions, values = torch.from_numpy(actions), torch.from_numpy(values)
            ts = []
            for _ in range(args.cpu_reps + 1):
                t0 = time.perf_counter()
                loss = next_train.loss_from_outputs(host.forward(leaves, maps, goals, paths.astype(np.float32), of.cpu().numpy(), 20), actions, values, ptr)
                copt.zero_grad()
                loss.backward()
                copt.step()
                ts.append((time.perf_counter() - t0) * 1e3)
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
    lines = ['# tools/next_train_bench.py on %s: ms a call, median over %d rounds of %d calls (min .. max), %d warm-up calls a leg'
             % (torch.cuda.get_device_name(0), args.rounds, args.reps, args.warmup),
             '# 20 rounds, 10 states a path; train_step = labels on the host + forward + loss + backward + Adam',
             '# CPU yardstick: the float32 torch restatement (tests/next_train_host.py), one step, %d torch threads, median of %d'
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
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cpu-reps', type=int, default=3)
    args = ap.parse_args()
    if args.resources:
        resources(args.out or os.path.join(REPO, 'profiles', 'next_train_resources.txt'))
    else:
        args.out = args.out or os.path.join(REPO, 'profiles', 'next_train_bench.txt')
        bench(args)


if __name__ == '__main__':
    main()
