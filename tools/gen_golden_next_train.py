#!/usr/bin/env python
"""Record the NEXT training fixtures under tests/golden/ from the UNMODIFIED reference (train_next.py's get_label and loss,
next_model/model2D.py), on the CPU.  For next_2 and next_3:

  next_train_maze{2,3}.npz             problems 3 and 11 (maps, goals, inits), a path of 7 and one of 10 states (a seeded polyline
                                       from the init state to the goal with steps both longer and shorter than RRT_EPS and, for
                                       the stick robot, across the orientation's period), get_label's outputs (float64), and the
                                       loss of every case in fp32 and from the same module in .double()
  next_train_maze{2,3}_i20_g32.npz     the per-parameter gradients of train()'s loss over both problems, fp32 module
  next_train_maze{2,3}_i20_d64.npz     the .double() module's gradients minus the fp32 ones, stored in float32: g64 = g32 + d64
                                       to 1e-7 of the DIFFERENCE, which keeps each file under 1 MiB
  next_train_maze{2,3}_i{0,1,2}_*.npz  the same on problem 3 alone at iters 0, 1, 2

The loss is train()'s: per (problem, path) sample set_problem, net_forward(path, use_np=False), MSELoss on the value column
plus MSELoss on the action columns, summed and divided by the number of problems.

Runs only in the authoring container, like tools/gen_golden_next.py: the reference's third-party imports resolve to
tools/standins/.  What is written is data only.
"""
import copy
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
os.environ.setdefault('CUDA_VISIBLE_DEVICES', '')
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, 'tools', 'standins'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

os.chdir(REF)
from environment import MazeEnv  # noqa: E402
from next_model.model2D import Model2D  # noqa: E402
from train_next import get_label  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
FILES = {2: 'maze_files/mazes_hard.npz', 3: 'maze_files/mazes_15_3_3000.npz'}


def make_path(rng, init, goal, n, dim):
    """init -> goal through n - 2 seeded waypoints; one step shorter than RRT_EPS, and for dim 3 one across the period."""
    lim = np.array([1., 1., 0.4])[:dim]
    pts = [np.array(init, dtype=np.float64)]
    for k in range(n - 2):
        t = (k + 1.) / (n - 1)
        pts.append(np.clip((1 - t) * pts[0] + t * np.array(goal, dtype=np.float64) + rng.uniform(-0.15, 0.15, dim) * lim, -lim, lim))
    pts.append(np.array(goal, dtype=np.float64))
    pts[2] = pts[1] + rng.uniform(-0.02, 0.02, dim) * lim / lim.max()          # a short step
    pts[2] = np.clip(pts[2], -lim, lim)
    if dim == 3:
        pts[3][2], pts[4][2] = 0.37, -0.36                                       # the short way round crosses +-0.4
    return np.array(pts)


def loss_fp32(model, env, probs, paths):
    total = 0.
    for pb, path in zip(probs, paths):
        model.set_problem(pb)
        action, value = get_label(path, env)
        action_pred, value_pred = model.net_forward(np.array(path), use_np=False)
        total = total + torch.nn.MSELoss()(torch.FloatTensor(value), value_pred) + torch.nn.MSELoss()(torch.FloatTensor(action), action_pred)
    return total / len(probs)


def loss_fp64(net64, env, probs, paths, dim):
    total = 0.
    for pb, path in zip(probs, paths):
        maze = torch.FloatTensor(pb['map'].reshape(1, 15, 15)).double()
        goal = torch.FloatTensor(pb['goal_state'].reshape(1, dim)).double()
        pb_rep = net64.pb_forward(goal, maze)
        action, value = get_label(path, env)
        y = net64.state_forward(torch.FloatTensor(np.array(path)).double(), pb_rep)
        total = total + torch.nn.MSELoss()(torch.FloatTensor(value).double(), y[:, -1]) \
            + torch.nn.MSELoss()(torch.FloatTensor(action).double(), y[:, :dim])
    return total / len(probs)


def grads(net, loss):
    names = [k for k, _ in net.named_parameters()]
    gs = torch.autograd.grad(loss, [p for _, p in net.named_parameters()], allow_unused=True)
    return {k: (np.zeros(tuple(p.shape)) if g is None else g.detach().numpy()) for k, g, (_, p) in zip(names, gs, net.named_parameters())}


def main():
    torch.set_num_threads(4)
    for dim in (2, 3):
        env = MazeEnv(dim=dim, map_file=FILES[dim])
        model = Model2D(env=env, cuda=False, dim=dim)
        model.net.load_state_dict(torch.load('data/weights/next_%d.pt' % dim, map_location='cpu'))
        net64 = copy.deepcopy(model.net).double()
        net64.attention_g.coords = net64.attention_g.coords.double()
        rng = np.random.RandomState(300 + dim)
        probs = [copy.deepcopy(env.init_new_problem(i)) for i in (3, 11)]
        paths = [make_path(rng, p['init_state'], p['goal_state'], n, dim) for p, n in zip(probs, (7, 10))]
        labels = [get_label(p, env) for p in paths]
        rec = dict(dim=dim, maps=np.stack([p['map'] for p in probs]).astype(np.float32),
                   goals=np.stack([p['goal_state'] for p in probs]).astype(np.float32),
                   inits=np.stack([p['init_state'] for p in probs]).astype(np.float32),
                   paths=np.concatenate(paths), path_ptr=np.array([0, 7, 17], dtype=np.int64),
                   actions=np.concatenate([np.array(a) for a, _ in labels]), values=np.concatenate([np.array(v) for _, v in labels]))
        for iters, npb in ((20, 2), (0, 1), (1, 1), (2, 1)):
            model.net.iters = net64.iters = iters
            l32 = loss_fp32(model, env, probs[:npb], paths[:npb])
            l64 = loss_fp64(net64, env, probs[:npb], paths[:npb], dim)
            g32, g64 = grads(model.net, l32), grads(net64, l64)
            rec['loss32_i%d' % iters], rec['loss64_i%d' % iters] = float(l32.detach()), float(l64.detach())
            np.savez_compressed(os.path.join(OUT, 'next_train_maze%d_i%d_g32.npz' % (dim, iters)),
                                **{k: v.astype(np.float32) for k, v in g32.items()})
            np.savez_compressed(os.path.join(OUT, 'next_train_maze%d_i%d_d64.npz' % (dim, iters)),
                                **{k: (g64[k] - g32[k].astype(np.float64)).astype(np.float32) for k in g64})
            print('next_train_maze%d iters %2d: loss %.9g / %.15g' % (dim, iters, rec['loss32_i%d' % iters], rec['loss64_i%d' % iters]))
            for k in g64:
                m = np.abs(g64[k]).max()
                print('    %-34s max|g64| %.3e  own %.3e  own / max %.2e' % (k, m, np.abs(g32[k] - g64[k]).max(),
                                                                          np.abs(g32[k] - g64[k]).max() / max(m, 1e-300)))
        model.net.iters = 20
        np.savez_compressed(os.path.join(OUT, 'next_train_maze%d.npz' % dim), **rec)


if __name__ == '__main__':
    main()
