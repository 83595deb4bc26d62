#!/usr/bin/env python
"""NEXT's training loop with the replay on the device (gnnmp.next_replay) on an MI355X; not part of bench.py.

  python tools/next_train_env_bench.py                  -> profiles/next_train_env_bench.txt    (needs the GPU)
  python tools/next_train_env_bench.py --resources      -> profiles/next_replay_resources.txt   (compiles only; no GPU needed)

Measured: (a) the stage times of ``collect_replay`` (pb_forward, plan, append, fallback; wall clock after a synchronise of the
stream) for the first 200 maze2 problems at ``t_max = 1000``, at explore rate 1.0 and 0.1, the second call of each; (b) ms per
optimizer step of ``train_replay``'s step (``store.batch`` -> forward -> ``path_loss`` -> backward -> Adam) against the existing
``NextNetTrain.train_step`` on the same 8 paths, in one process with the legs taken in turn, the ``train_step`` leg twice, medians
over ``--rounds`` rounds of ``--reps`` steps after ``--warmup`` steps; (c) the wall time of ``train_env_maze`` over 400 problems
(two chunks of 200, L = 10).  No target is set.  One condition is stated with the figures: the replay step is no slower than
``train_step`` by more than the spread between the two ``train_step`` legs; when it does not hold the file says so."""
import argparse
import os
import re
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
KINDS = r'TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]'
PINNED = (('next_kernels.hip', 'next_net_resources.txt'), ('next_train_kernels.hip', 'next_train_resources.txt'),
          ('next_plan_kernels.hip', 'next_plan_resources.txt'))


def _figures(source):
    src = os.path.join(REPO, 'gnn-motion-planning_amd', 'csrc', source)
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fno-honor-nans', '-fPIC', '-c', '-Rpass-analysis=kernel-resource-usage',
           src, '-o', os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True).stdout
    out = []
    for ln in text.splitlines():
        m = re.search(r'remark: (?:\S+: )?\s*(Function Name: \S+|\s+(?:%s): \d+)' % KINDS, ln)
        if m:
            out.append(m.group(1).rstrip())
    return out


def resources(out):
    figures = _figures('next_replay_kernels.hip')
    scratch = [int(ln.split(':')[1]) for ln in figures if 'ScratchSize' in ln]
    lds = [int(ln.split(':')[1]) for ln in figures if 'LDS Size' in ln]
    lines = ['# hipcc -Rpass-analysis=kernel-resource-usage over csrc/next_replay_kernels.hip (gfx950, the build\'s flags)',
             '# one wave a workgroup in every kernel; no dynamic LDS'] + figures
    lines.append('# scratch: %s; LDS: %s' % ('none in any kernel' if not any(scratch) else 'PRESENT -- a finding to remove',
                                              'none in any kernel' if not any(lds) else 'see above'))
    for source, recorded in PINNED:
        path = os.path.join(REPO, 'profiles', recorded)
        want = [ln.rstrip() for ln in open(path).read().splitlines() if ln.strip() and not ln.startswith('#')]
        got = [ln for ln in _figures(source)]
        name, moved = '', []
        for w, g in zip(want, got):
            if w.startswith('Function Name'):
                name = w.split()[-1]
            if w.strip() != g.strip():
                moved.append('%s %s -> %s' % (name, w.strip(), g.strip().split(': ')[-1]))
        if len(want) != len(got):
            moved.append('%d lines recorded, %d now' % (len(want), len(got)))
        lines.append('# csrc/%s against profiles/%s: %s' % (source, recorded, 'all %d lines reproduced' % len(want) if not moved else
                                                           'DIFFERS from the recorded file: ' + '; '.join(moved)))
    open(out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def _problems(np, n):
    with np.load(os.path.join(REPO, 'tests', 'golden', 'evalset_mazehard_first1000.npz')) as f:
        return [dict(map=f['maps'][i], init_state=f['init_states'][i], goal_state=f['goal_states'][i]) for i in range(n)]


def bench(args):
    import numpy as np
    import torch
    import gnnmp  # noqa: F401
    from gnnmp import next_model, next_replay, next_train
    if not torch.cuda.is_available():
        raise SystemExit('next_train_env_bench: needs the GPU (nothing is measured on a CPU alone)')
    dev = torch.device('cuda:0')
    with np.load(os.path.join(REPO, 'tests', 'golden', 'next_2_weights.npz')) as f:
        w = {k: f[k] for k in f.files}
    lines = ['# tools/next_train_env_bench.py on %s' % torch.cuda.get_device_name(0)]

    # (a) collect_replay, 200 maze2 problems
    problems = _problems(np, 400)
    net = next_model.NextNet(2).load_state_dict(w)
    ids = list(range(200))
    lines.append('# (a) collect_replay: 200 maze2 problems (evalset_mazehard_first1000, seeds i), t_max 1000, fallback 50 / 1000, the '
                 'shipped checkpoint; wall clock a stage, second call')
    store = None
    for rate in (1.0, 0.1):
        for rep in range(2):
            store = next_replay.ReplayStore(2, 200, 200 * 1002, dev)
            timings = {}
            t0 = time.perf_counter()
            got = next_replay.collect_replay(net, problems[:200], ids, ids, store, dev, rate, t_max=1000, timings=timings)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        lines.append('explore rate %.1f: %s  total %.1f ms   solved by NEXT %d, by the fallback %d, unsolved %d; replay %d paths, %d states'
                     % (rate, '  '.join('%s %.1f ms' % (k, 1e3 * timings[k]) for k in ('pb_forward', 'plan', 'append', 'fallback')),
                        1e3 * wall, got['next'], got['fallback'], got['unsolved'], len(store), store.n_states))

    # (b) one optimizer step on the same 8 paths: NextNetTrain.train_step against train_replay's step
    idx = list(range(8))
    maps_all = torch.from_numpy(np.ascontiguousarray([np.asarray(p['map'], dtype=np.float32) for p in problems[:200]])).to(dev)
    goals_all = torch.from_numpy(np.ascontiguousarray([np.asarray(p['goal_state'], dtype=np.float32) for p in problems[:200]])).to(dev)
    pid = torch.from_numpy(store.host_problem[idx]).to(dev)
    ptr = store.host_ptr[:9]
    paths = store.states64[:int(ptr[-1])].cpu().numpy()
    gmaps, ggoals = maps_all[pid].contiguous(), goals_all[pid].contiguous()
    nets = [next_train.NextNetTrain(2, device=dev).load_state_dict(w) for _ in range(3)]
    opts = [torch.optim.Adam(n.parameters(), lr=1e-3) for n in nets]

    def step_host(k):
        nets[k].train_step(opts[k], gmaps, ggoals, paths, ptr, 20)

    def step_replay(k):
        b = store.batch(idx)
        p = torch.from_numpy(np.asarray(b['problems'], dtype=np.int64)).to(dev)
        y = nets[k].forward(maps_all.index_select(0, p), goals_all.index_select(0, p), b['states32'], b['problem_of_state'], 20)
        loss = next_replay.path_loss(y, b['actions'], b['values'], b['ptr'], 8)
        opts[k].zero_grad()
        loss.backward()
        opts[k].step()
    legs = [('NextNetTrain.train_step (first leg)', lambda: step_host(0)), ("train_replay's step", lambda: step_replay(1)),
            ('NextNetTrain.train_step (second leg)', lambda: step_host(2))]
    for _, fn in legs:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / args.reps)
    lines.append('# (b) ms an optimizer step on the same 8 paths (%d states), 20 rounds, Adam; wall clock around %d steps, median over %d '
                 'rounds (min .. max), %d warm-up steps a leg, the legs taken in turn' % (int(ptr[-1]), args.reps, args.rounds, args.warmup))
    med = {}
    for name, _ in legs:
        t = np.array(times[name])
        med[name] = float(np.median(t))
        lines.append('%-40s %9.3f ms  (%.3f .. %.3f)' % (name, med[name], t.min(), t.max()))
    a, r, a2 = (med[name] for name, _ in legs)
    spread = abs(a - a2)
    holds = r <= min(a, a2) + spread
    lines.append('condition "the replay step is no slower than train_step by more than the spread between the two train_step legs '
                 '(%.3f ms)": %s (replay step - faster train_step leg = %+.3f ms)' % (spread, 'HOLDS' if holds else 'DOES NOT HOLD', r - min(a, a2)))

    # (c) train_env_maze over 400 problems
    tn = next_train.NextNetTrain(2, device=dev).load_state_dict(w)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hist = next_replay.train_env_maze(tn, problems, dev, chunk=200, L=10, t_max=1000)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    lines.append('# (c) train_env_maze over 400 maze2 problems (2 chunks of 200, L 10, t_max 1000, fallback 50 / 1000)')
    lines.append('wall %.1f s; %s' % (wall, '; '.join('chunk %d: rate %.2f, NEXT %d / fallback %d / unsolved %d, replay %d, %d steps, loss %.4f -> %.4f'
                                                      % (i, h['explore_eps'], h['next'], h['fallback'], h['unsolved'], h['replay'], len(h['losses']),
                                                         h['losses'][0] if h['losses'] else float('nan'),
                                                         h['losses'][-1] if h['losses'] else float('nan')) for i, h in enumerate(hist))))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    if args.resources:
        resources(args.out or os.path.join(REPO, 'profiles', 'next_replay_resources.txt'))
    else:
        args.out = args.out or os.path.join(REPO, 'profiles', 'next_train_env_bench.txt')
        bench(args)


if __name__ == '__main__':
    main()
