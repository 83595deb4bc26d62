#!/usr/bin/env python
"""Train the explorer for maze problems on the device (gnnmp.explorer_replay.train_explorer_maze: the reference's
train_explorer.py over the labelled graphs of algorithm/dijkstra.py) and save the checkpoint;
``gnnmp.EncoderProcessDecoder.load_state_dict`` and the reference's ``EncoderProcessDecoder`` take it.  Needs the GPU.

  python tools/train_explorer_maze.py --dim 2 --problems 2000 --iters 20 --out explorer_maze.pt
  python tools/train_explorer_maze.py --dim 3 --problems 40 --set my_mazes.npz --out explorer_maze3.pt

``--set``: an .npz with ``maps`` [n, w, w] (default: the evaluation set under tests/golden, which holds 1000 maze2 and 40 maze3
problems).  ``--init``: a shipped checkpoint to start from (``weights_maze`` / ``weights_maze_3``); default: a fresh network, its
initial weights drawn under ``torch.manual_seed(seed)``, as the reference trains it."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SETS = {2: 'evalset_mazehard_first1000.npz', 3: 'evalset_maze3_first40_b200_k12_s9.npz'}


def load_maps(dim, n, path=None):
    """The maps of the first ``n`` problems of ``path`` (default: the dimension's set under tests/golden)."""
    import numpy as np
    with np.load(path or os.path.join(REPO, 'tests', 'golden', SETS[dim])) as f:
        return np.asarray(f['maps'][:min(int(n), f['maps'].shape[0])])


def fresh_explorer(dim, seed, init=None):
    """An ``EncoderProcessDecoder`` for the dimension: untrained (drawn under ``torch.manual_seed(seed)``) or a shipped one."""
    import gnnmp
    import torch
    torch.manual_seed(int(seed))
    m = gnnmp.EncoderProcessDecoder(2, dim, 32, 2)
    if init:
        from gnnmp.weights import load_weights
        m.load_state_dict(load_weights(init))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dim', type=int, choices=(2, 3), required=True)
    ap.add_argument('--problems', type=int, required=True)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', required=True)
    ap.add_argument('--set', default=None)
    ap.add_argument('--init', default=None)
    ap.add_argument('--loop', type=int, default=10)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--batched', action='store_true', help='one train_scores_batch per step instead of one pass per loop value')
    ap.add_argument('--device', default='cuda:0')
    args = ap.parse_args()
    import torch
    import gnnmp  # noqa: F401
    from gnnmp import explorer_replay
    if not torch.cuda.is_available():
        raise SystemExit('train_explorer_maze: needs the GPU (the kernels are the only implementation)')
    maps = load_maps(args.dim, args.problems, args.set)
    if len(maps) < args.problems:
        print('the set holds %d problems; training on those' % len(maps))
    model = fresh_explorer(args.dim, args.seed, args.init)
    t0 = time.perf_counter()
    explorer_replay.train_explorer_maze(
        model, maps, args.dim, args.device, iters=args.iters, loop=args.loop, lr=args.lr, seed=args.seed, batched=args.batched,
        log=lambda it, e: print('iteration %d: %d steps, mean loss %.6f, %d of %d samples counted (single %d, empty %d), %.1f steps/s'
                                % (it, len(e['losses']), e['mean'], e['counted'], e['samples'], e['single'], e['empty'],
                                   e['steps_per_s']), flush=True))
    print('%d problems; %.1f s' % (len(maps), time.perf_counter() - t0))
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, args.out)
    print('saved the checkpoint to %s' % args.out)


if __name__ == '__main__':
    main()
