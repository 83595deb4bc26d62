#!/usr/bin/env python
"""The explorer's training loop with the dataset on the device (gnnmp.explorer_replay) on an MI355X; not part of bench.py.

  python tools/explorer_train_env_bench.py                  -> profiles/explorer_train_env_bench.txt      (needs the GPU)
  python tools/explorer_train_env_bench.py --resources      -> profiles/explorer_replay_resources.txt     (compiles only; no GPU needed)

Measured, with device events around ``--reps`` calls after ``--warmup`` calls, the two legs of every comparison alternating in one
process, three legs each: (a) the loss of train_explorer.py:172 forward and backward, ``explorer_replay.frontier_loss`` against
``episodes.frontier_loss``, on the frontiers of a real roll-out (random scores) of 8, 64 and 256 maze2 problems; (b)
``ExplorerDataset.batch`` against ``TrainingGraphs.subset`` at the same sizes; (c) one whole optimizer step on the same 8 problems
and the same draws, ``training_step`` (``subset`` inside the forward, the torch loss) on a resident ``TrainingGraphs`` against
``dataset.batch`` + the same pipeline + the kernel loss; (d) the wall time of ``train_explorer_maze`` over ``--problems`` maze2
problems with ``--iters`` iterations.  No target is set for the loss kernel's gain.  One condition is stated with the figures:
the new step is no slower than the old one by more than the spread between the old step's own three legs; when it does not hold
the file says so."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
from smoother_train_env_bench import _figures  # noqa: E402  (hipcc's resource remarks of one source file, the build's flags)
from train_explorer_maze import fresh_explorer, load_maps  # noqa: E402  (the maps and the network of the training tool)


def resources(out):
    figures = _figures('explorer_replay_kernels.hip')
    scratch = [int(ln.split(':')[1]) for ln in figures if 'ScratchSize' in ln]
    lines = ['# hipcc -Rpass-analysis=kernel-resource-usage over csrc/explorer_replay_kernels.hip (gfx950, the build\'s flags)',
             '# gather: 256 threads a workgroup, 40 bytes of static LDS (the scan\'s result); frontier loss: one wave a workgroup, 64 KB of '
             'static LDS (the per-edge counts of one problem, 16384 edges); no dynamic LDS'] + figures
    lines.append('# scratch: %s' % ('none in any kernel' if not any(scratch) else 'PRESENT -- a finding to remove'))
    open(out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    return 1 if any(scratch) else 0


def bench(args):
    import numpy as np
    import torch
    import gnnmp  # noqa: F401
    from gnnmp import episodes as ep
    from gnnmp import explorer_replay as er
    if not torch.cuda.is_available():
        raise SystemExit('explorer_train_env_bench: needs the GPU (nothing is measured on a CPU alone)')
    dev = torch.device('cuda:0')
    lines = ['# tools/explorer_train_env_bench.py on %s; ms a call, device events around %d calls after %d, legs alternating, three each'
             % (torch.cuda.get_device_name(0), args.reps, args.warmup)]

    def legs(pairs, reps=args.reps, warmup=args.warmup):
        """[(name, fn)] -> {name: [ms a call] x 3}."""
        for _, fn in pairs:
            for _ in range(warmup):
                fn()
        times = {name: [] for name, _ in pairs}
        for _ in range(3):
            for name, fn in pairs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / reps)
        return times
    fmt = lambda ts: '  '.join('%8.4f' % t for t in ts)      # noqa: E731

    maps = load_maps(2, 256)
    t0 = time.perf_counter()
    dataset = er.build_maze_dataset(maps, 2, dev)
    torch.cuda.synchronize()
    lines.append('# dataset: %d maze2 problems, %d nodes, %d edges, built in %.2f s (second build: see (d))'
                 % (len(dataset), int(dataset.host_node_ptr[-1]), int(dataset.host_edge_ptr[-1]), time.perf_counter() - t0))
    full = ep.TrainingGraphs(dataset.v, dataset.edge_index, dataset.host_node_ptr.tolist(), dataset.host_edge_ptr.tolist(),
                             dataset.edge_free, dataset.edge_cost, dataset.obstacles, dataset.host_obs_ptr.tolist(),
                             points64=dataset.points64)

    # (a) the loss, (b) the batch assembly
    gen = torch.Generator(device=dev)
    for B in (8, 64, 256):
        idx = list(range(min(B, len(dataset))))
        g = dataset.batch(idx)
        gen.manual_seed(1234)
        goal, _ = ep.draw_device(g, 10, gen, torch.Generator().manual_seed(1234))
        paths = ep.shortest_paths(g, goal)
        start = ep.draw_start(g, paths, gen)
        scores = torch.randn(g.total_edges, device=dev, generator=gen)
        step, status = ep.explore_steps(g, scores, start, paths['goal'], paths['n_valid'])
        fr = ep.policy_frontier(g, scores, paths, start, paths['goal'], ep.draw_step(step, gen), status)
        s_old, s_new = scores.clone().requires_grad_(True), scores.clone().requires_grad_(True)

        def old_loss():
            s_old.grad = None
            ep.frontier_loss(s_old, fr)[0].sum().backward()

        def new_loss():
            s_new.grad = None
            er.frontier_loss(s_new, fr).backward()
        old_loss(), new_loss()
        t_old, ok = ep.frontier_loss(s_old, fr)
        _, t_new, counted = er.frontier_loss(s_new, fr, return_terms=True)
        diff = float((t_old.detach() - t_new).abs().max())
        gdiff = float((s_old.grad - s_new.grad).abs().max())
        t = legs([('episodes.frontier_loss', old_loss), ('explorer_replay.frontier_loss', new_loss)])
        lines.append('# (a) loss forward + backward, %d problems (%d edges, %d counted, longest frontier %d); the two agree to %.1e (terms) '
                     'and %.1e (gradient)' % (len(idx), g.total_edges, int(counted.sum()), int(fr['frontier_len'].max()), diff, gdiff))
        for name in t:
            lines.append('%-34s %s ms' % (name, fmt(t[name])))
        zero = torch.zeros(len(dataset), dtype=torch.int32, device=dev)
        t = legs([('TrainingGraphs.subset', lambda: full.subset(idx, zero)), ('ExplorerDataset.batch', lambda: dataset.batch(idx))])
        lines.append('# (b) batch assembly, %d problems (%d nodes)' % (len(idx), g.total_nodes))
        for name in t:
            lines.append('%-34s %s ms' % (name, fmt(t[name])))

    # (c) one optimizer step on the same 8 problems and the same draws
    idx = list(range(8))
    resident = dataset.batch(idx)
    cpu_gen = torch.Generator()

    def explorer():
        m = fresh_explorer(2, 0, 'weights_maze').to(dev).train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        opt.zero_grad()
        return m, opt
    (m_old, o_old), (m_new, o_new) = explorer(), explorer()

    def step_old():
        gen.manual_seed(7)
        cpu_gen.manual_seed(7)
        loss, _ = ep.training_step(m_old, resident, loop=10, generator=gen, cpu_generator=cpu_gen)
        loss.backward()
        o_old.step()
        o_old.zero_grad()

    def step_new():
        gen.manual_seed(7)
        cpu_gen.manual_seed(7)
        g = dataset.batch(idx)
        goal, loops = ep.draw_device(g, 10, gen, cpu_gen)
        paths = ep.shortest_paths(g, goal)
        start = ep.draw_start(g, paths, gen)
        scores = ep.forward_scores(m_new, g, paths['goal'], loops)
        step, status = ep.explore_steps(g, scores, start, paths['goal'], paths['n_valid'])
        fr = ep.policy_frontier(g, scores, paths, start, paths['goal'], ep.draw_step(step, gen), status)
        er.frontier_loss(scores, fr).backward()
        o_new.step()
        o_new.zero_grad()
    t = legs([('training_step (subset, torch loss)', step_old), ('dataset.batch + kernel loss', step_new)], reps=args.step_reps,
             warmup=args.warmup)
    cpu_gen.manual_seed(7)
    lines.append('# (c) one optimizer step (Adam) on the same 8 maze2 problems (%d nodes) and the same draws (loops %s), %d steps a leg'
                 % (resident.total_nodes, torch.randint(1, 10, (8,), generator=cpu_gen).tolist(), args.step_reps))
    for name in t:
        lines.append('%-36s %s ms' % (name, fmt(t[name])))
    old, new = list(t.values())
    spread = max(old) - min(old)
    holds = float(np.median(new)) <= float(np.median(old)) + spread
    lines.append('condition "the new step is no slower than the old one by more than the spread between the old step\'s own legs '
                 '(%.3f ms)": %s (median new step - median old step = %+.3f ms)'
                 % (spread, 'HOLDS' if holds else 'DOES NOT HOLD', float(np.median(new)) - float(np.median(old))))

    # (d) train_explorer_maze
    maps = load_maps(2, args.problems)
    model = fresh_explorer(2, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hist = er.train_explorer_maze(model, maps, 2, dev, iters=args.iters)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    steps = sum(len(h['losses']) for h in hist)
    lines.append('# (d) train_explorer_maze over %d maze2 problems, iters %d, a fresh network, dataset build included' % (len(maps), args.iters))
    lines.append('wall %.2f s; %d optimizer steps; steps/s inside the iterations %s; mean loss an iteration %s; counted %s of %s samples '
                 '(single %s, empty %s)'
                 % (wall, steps, ' '.join('%.1f' % h['steps_per_s'] for h in hist), ' '.join('%.4f' % h['mean'] for h in hist),
                    [h['counted'] for h in hist], [h['samples'] for h in hist], [h['single'] for h in hist], [h['empty'] for h in hist]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50, help='calls a leg of (a) and (b)')
    ap.add_argument('--step-reps', type=int, default=20, help='optimizer steps a leg of (c)')
    ap.add_argument('--problems', type=int, default=256, help='problems of the train_explorer_maze run')
    ap.add_argument('--iters', type=int, default=2)
    args = ap.parse_args()
    if args.resources:
        sys.exit(resources(args.out or os.path.join(REPO, 'profiles', 'explorer_replay_resources.txt')))
    args.out = args.out or os.path.join(REPO, 'profiles', 'explorer_train_env_bench.txt')
    bench(args)


if __name__ == '__main__':
    main()
