#!/usr/bin/env python
"""The smoother's training loop with the replay on the device (gnnmp.smoother_replay) on an MI355X; not part of bench.py.

  python tools/smoother_train_env_bench.py                  -> profiles/smoother_train_env_bench.txt     (needs the GPU)
  python tools/smoother_train_env_bench.py --resources      -> profiles/smoother_replay_resources.txt    (compiles only; no GPU needed)

Measured: (a) the stage times of ``collect_replay`` (plan, targets, append; wall clock after a synchronise of the stream) for
the first ``--collect`` maze2 and maze3 problems at ``batch = 500``, the second call of each; (b) ms per optimizer step through
``store.batch`` -> ``forward_train_batch`` -> ``path_loss`` -> backward -> SGD against the same 8 samples through a ``SmoothBatch``
built from host lists and ``ModelSmoother.training_loss``, in one process with the legs alternating, three legs each of
``--reps`` steps after ``--warmup`` steps, and the step's two new launches on their own (``store.batch``, ``path_loss_device``; device
events around 200 calls); (c) the wall time of ``train_smoother_maze`` over ``--problems`` maze2 problems.  No
target is set.  One condition is stated with the figures: the replay step is no slower than the ``training_loss`` step by more
than the spread between that step's own three legs; when it does not hold the file says so."""
import argparse
import os
import re
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
KINDS = r'TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]'
sys.path.insert(0, os.path.join(REPO, 'tools'))
from train_smoother_maze import fresh_smoother, load_explorer, load_problems  # noqa: E402  (the sets, explorers and smoother of the training tool)


def _figures(source):
    src = os.path.join(REPO, 'gnn-motion-planning_amd', 'csrc', source)
    from __graft_entry__ import HIPCC_FLAGS                     # the build's own flags
    cmd = ['hipcc'] + HIPCC_FLAGS + ['-c', '-Rpass-analysis=kernel-resource-usage', src, '-o', os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True).stdout
    out = []
    for ln in text.splitlines():
        m = re.search(r'remark: (?:\S+: )?\s*(Function Name: \S+|\s+(?:%s): \d+)' % KINDS, ln)
        if m:
            out.append(m.group(1).rstrip())
    return out


def resources(out):
    figures = _figures('smoother_replay_kernels.hip')
    scratch = [int(ln.split(':')[1]) for ln in figures if 'ScratchSize' in ln]
    lines = ['# hipcc -Rpass-analysis=kernel-resource-usage over csrc/smoother_replay_kernels.hip (gfx950, the build\'s flags)',
             '# append and gather: 256 threads a workgroup, a few words of static LDS (the scan\'s result); path loss: one workgroup of '
             '8 waves; no dynamic LDS'] + figures
    lines.append('# scratch: %s' % ('none in any kernel' if not any(scratch) else 'PRESENT -- a finding to remove'))
    open(out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    return 1 if any(scratch) else 0


def bench(args):
    import numpy as np
    import torch
    import gnnmp  # noqa: F401
    from gnnmp import planner
    from gnnmp import smoother_replay as sr
    from gnnmp.smoother import SmoothBatch
    if not torch.cuda.is_available():
        raise SystemExit('smoother_train_env_bench: needs the GPU (nothing is measured on a CPU alone)')
    dev = torch.device('cuda:0')
    lines = ['# tools/smoother_train_env_bench.py on %s' % torch.cuda.get_device_name(0)]

    explorer = load_explorer

    # (a) collect_replay
    lines.append('# (a) collect_replay: the first problems of the sets under tests/golden, batch 500, k 30, loop 5, seeds '
                 'pass_seeds(1234, i, 0); wall clock a stage, second call')
    stores = {}
    for dim in (2, 3):
        problems = load_problems(dim, args.collect)
        n = len(problems)
        ids = list(range(n))
        model = explorer(dim)
        for rep in range(2):
            store = sr.SmoothReplayStore(dim, n, n * 502, n * 500, n * 500, dev)
            gen = torch.Generator(device=dev)
            gen.manual_seed(1234)
            timings = {}
            t0 = time.perf_counter()
            got = sr.collect_replay(model, problems, ids, sr.pass_seeds(1234, ids, 0), store, dev, generator=gen, timings=timings)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        stores[dim] = store
        lines.append('maze%d, %d problems: %s  total %.1f ms   %s; replay %d samples, %d path / %d free / %d collided rows'
                     % ((dim, n, '  '.join('%s %.1f ms' % (k, 1e3 * timings.get(k, 0.)) for k in ('plan', 'targets', 'append')), 1e3 * wall,
                         got) + store.rows_in_use()))

    # (b) one optimizer step on the same 8 samples
    store = stores[2]
    if len(store) < 8:
        raise SystemExit('smoother_train_env_bench: fewer than 8 samples collected; raise --collect')
    idx = list(range(8))
    loops = [int(x) for x in np.random.RandomState(1234).randint(1, 10, 8)]
    order = sorted(range(8), key=lambda b: -loops[b])
    pp, fp, cp = store.host_path_ptr, store.host_free_ptr, store.host_coll_ptr
    rows = {name: getattr(store, name).cpu() for name in ('path', 'target', 'free', 'collided')}
    host = [dict(path=rows['path'][pp[i]:pp[i + 1]], target=rows['target'][pp[i]:pp[i + 1]], free=rows['free'][fp[i]:fp[i + 1]],
                 collided=rows['collided'][cp[i]:cp[i + 1]]) for i in idx]

    def smoother():
        m = fresh_smoother(2, dev, 0)
        m.train()
        return m, torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    (m_host, o_host), (m_rep, o_rep) = smoother(), smoother()

    def step_host():
        pick = [host[b] for b in order]
        lengths = [q['path'].shape[0] for q in pick]
        edges = torch.from_numpy(planner._chain_edge_indices(lengths))
        off = np.concatenate([[0], np.cumsum([3 * p - 2 for p in lengths])])
        sb = SmoothBatch([q['path'] for q in pick], [q['free'] for q in pick], [q['collided'] for q in pick],
                         [edges[:, a:b] for a, b in zip(off[:-1], off[1:])], dev)
        loss = m_host.training_loss(sb, torch.cat([q['target'] for q in pick]).to(dev), [loops[b] for b in order])
        o_host.zero_grad()
        loss.backward()
        o_host.step()

    def step_replay():
        sb, targets, od = store.batch(idx, loops)
        pred = m_rep.forward_train_batch(sb, [loops[b] for b in od])
        loss = sr.path_loss(pred, targets, sb.path_ptr, 8)
        o_rep.zero_grad()
        loss.backward()
        o_rep.step()
    legs = [('SmoothBatch from lists + training_loss', step_host), ('store.batch + path_loss', step_replay)]
    for _, fn in legs:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in legs}
    for _ in range(3):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / args.reps)
    lines.append('# (b) ms an optimizer step on the same 8 maze2 samples (%d path rows, loops %s), SGD; wall clock around %d steps a leg, '
                 '%d warm-up steps, the legs alternating, three each' % (int(pp[8]), loops, args.reps, args.warmup))
    for name, _ in legs:
        lines.append('%-40s %s ms' % (name, '  '.join('%8.3f' % t for t in times[name])))
    h, r = times[legs[0][0]], times[legs[1][0]]
    spread = max(h) - min(h)
    holds = float(np.median(r)) <= float(np.median(h)) + spread
    lines.append('condition "the replay step is no slower than the training_loss step by more than the spread between that step\'s own '
                 'legs (%.3f ms)": %s (median replay step - median training_loss step = %+.3f ms)'
                 % (spread, 'HOLDS' if holds else 'DOES NOT HOLD', float(np.median(r)) - float(np.median(h))))

    # the two new launches of the replay step on their own: device events around 200 calls each
    sb, targets, od = store.batch(idx, loops)
    pred = torch.rand_like(sb.path)

    def per_call(fn, n=200):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    lines.append('on their own (device events around 200 calls, host-side allocation and launch included): store.batch (upload + gather '
                 'launch) %.4f ms, path_loss_device (three output allocations + the loss launch, %d interior elements in the longest '
                 'path) %.4f ms' % (per_call(lambda: store.batch(idx, loops)), (sb.max_path - 2) * 2,
                                    per_call(lambda: sr.path_loss_device(pred, targets, sb.path_ptr, 8))))

    # (c) train_smoother_maze
    problems = load_problems(2, args.problems)
    ms = fresh_smoother(2, dev, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hist, _ = sr.train_smoother_maze(ms, explorer(2), problems, dev, data_iter=args.data_iter, passes=args.passes)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    lines.append('# (c) train_smoother_maze over %d maze2 problems (data_iter %d, passes %d, batch 500, chunk 256), a fresh network'
                 % (len(problems), args.data_iter, args.passes))
    lines.append('wall %.1f s; collected %s; replay %d samples; pass means %s; lr %s'
                 % (wall, hist['collect'], hist['replay'], ' '.join('%.5f' % e['mean'] for e in hist['train']),
                    ' '.join('%g' % e['lr'] for e in hist['train'])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--collect', type=int, default=200, help='problems of the collect_replay timing (a set may hold fewer)')
    ap.add_argument('--problems', type=int, default=300, help='problems of the train_smoother_maze run')
    ap.add_argument('--data-iter', type=int, default=3)
    ap.add_argument('--passes', type=int, default=20)
    args = ap.parse_args()
    if args.resources:
        sys.exit(resources(args.out or os.path.join(REPO, 'profiles', 'smoother_replay_resources.txt')))
    args.out = args.out or os.path.join(REPO, 'profiles', 'smoother_train_env_bench.txt')
    bench(args)


if __name__ == '__main__':
    main()
