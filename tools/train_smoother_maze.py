#!/usr/bin/env python
"""Train a path smoother for maze problems on the device (gnnmp.smoother_replay.train_smoother_maze: train_smoother.py's
train_env) and save the checkpoint of the best pass; ``gnnmp.ModelSmoother.load_state_dict`` and the reference's
``ModelSmoother`` take it.  Needs the GPU.

  python tools/train_smoother_maze.py --dim 3 --problems 2000 --out smooth_maze3.pt
  python tools/train_smoother_maze.py --dim 2 --problems 500 --set my_mazes.npz --out smooth_maze2.pt

``--set``: an .npz with ``maps`` [n, w, w], ``init_states`` and ``goal_states`` [n, dim] (default: the evaluation set under
tests/golden, which holds 1000 maze2 and 40 maze3 problems).  The explorer is the shipped checkpoint of the dimension."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SETS = {2: ('evalset_mazehard_first1000.npz', 'weights_maze'), 3: ('evalset_maze3_first40_b200_k12_s9.npz', 'weights_maze_3')}


def load_problems(dim, n, path=None):
    """The first ``n`` problems of ``path`` (default: the dimension's set under tests/golden) as problem dicts."""
    import numpy as np
    with np.load(path or os.path.join(REPO, 'tests', 'golden', SETS[dim][0])) as f:
        n = min(int(n), f['maps'].shape[0])
        return [dict(map=f['maps'][i], init_state=f['init_states'][i], goal_state=f['goal_states'][i]) for i in range(n)]


def load_explorer(dim):
    """The shipped explorer checkpoint of the dimension."""
    import gnnmp
    from gnnmp.weights import load_weights
    m = gnnmp.EncoderProcessDecoder(2, dim, 32, 2).eval()
    m.load_state_dict(load_weights(SETS[dim][1]))
    return m


def fresh_smoother(dim, device, seed):
    """An untrained ``ModelSmoother`` for the dimension, its initial weights drawn under ``torch.manual_seed(seed)``."""
    import gnnmp
    import torch
    torch.manual_seed(int(seed))
    return gnnmp.ModelSmoother(workspace_size=2, config_size=dim, embed_size=128, obs_size=6).to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dim', type=int, choices=(2, 3), required=True)
    ap.add_argument('--problems', type=int, required=True)
    ap.add_argument('--out', required=True)
    ap.add_argument('--set', default=None)
    ap.add_argument('--data-iter', type=int, default=3)
    ap.add_argument('--passes', type=int, default=20)
    ap.add_argument('--batch', type=int, default=500)
    ap.add_argument('--chunk', type=int, default=256)
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--device', default='cuda:0')
    args = ap.parse_args()
    import torch
    import gnnmp  # noqa: F401
    from gnnmp import smoother_replay
    if not torch.cuda.is_available():
        raise SystemExit('train_smoother_maze: needs the GPU (the kernels are the only implementation)')
    problems = load_problems(args.dim, args.problems, args.set)
    if len(problems) < args.problems:
        print('the set holds %d problems; training on those' % len(problems))
    explorer = load_explorer(args.dim)
    model_s = fresh_smoother(args.dim, args.device, args.seed)
    t0 = time.perf_counter()
    history, best = smoother_replay.train_smoother_maze(
        model_s, explorer, problems, args.device, data_iter=args.data_iter, passes=args.passes, chunk=args.chunk, batch=args.batch,
        seed=args.seed, log=lambda p, e: print('pass %d: mean loss %.6f over %d steps, lr %g' % (p, e['mean'], len(e['losses']), e['lr']), flush=True))
    for it, c in enumerate(history['collect']):
        print('collection pass %d: %s' % (it, c))
    print('replay %d samples; %.1f s' % (history['replay'], time.perf_counter() - t0))
    torch.save({k: v.cpu() for k, v in best.items()}, args.out)
    print('saved the best pass to %s' % args.out)


if __name__ == '__main__':
    main()
