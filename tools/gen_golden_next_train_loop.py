#!/usr/bin/env python
"""Record the fixtures of NEXT's training LOOP under tests/golden/ from the UNMODIFIED reference: train_next.py's train() itself
(permutations, groups of 8, the carry-over of the trailing samples into the next pass, Adam), on the CPU.  For next_2 and next_3:

  next_train_loop_maze{2,3}.npz   a replay of 11 made-up paths over 11 maze problems (seeded polylines as in
                                  tools/gen_golden_next_train.py), train(L=3) at 20 rounds from the shipped checkpoint with
                                  Adam(lr=1e-3) and np.random.seed(1234): 3 optimizer steps with 8, 11 and 11 terms.  Recorded:
                                  the problems, the paths, the permutations train() drew, the index groups of the steps, the
                                  per-step losses (loss / 8) of the float32 module and of the same module in .double(), and
                                  the .double() run's final parameters as a float32 difference from the start.

train() runs unmodified; what it is handed are stand-ins: a stub pbar and writer (the writer receives the summed loss of every
step, which is how it is recorded), np.random.permutation wrapped to log what it returns, and for the .double() run a model
object that does Model2D.set_problem / net_forward with its float32 inputs cast to double, and a torch namespace inside
train_next whose FloatTensor casts to double (train() builds its targets with torch.FloatTensor).

Runs only in the authoring container, like tools/gen_golden_next_train.py: the reference's third-party imports resolve to
tools/standins/.  What is written is data only.
"""
import copy
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_next_train import FILES, OUT, make_path  # noqa: E402  (sets up the reference's import path and cwd)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import train_next  # noqa: E402
from environment import MazeEnv  # noqa: E402
from next_model.model2D import Model2D  # noqa: E402

PROBLEMS = (3, 11, 0, 1, 2, 4, 5, 6, 7, 8, 9)
LENGTHS = (7, 10, 5, 12, 8, 6, 9, 11, 7, 10, 13)
L, SEED, LR, ITERS = 3, 1234, 1e-3, 20


class Pbar:
    def set_description(self, text):
        pass


class Writer:
    def __init__(self):
        self.action_step, self.total_step, self.totals = 0, 0, []

    def add_scalar(self, tag, value, step):
        if tag == 'train/total':
            self.totals.append(float(value.detach()))


class Model64:
    """Model2D.set_problem / net_forward(use_np=False) over a .double() net."""

    def __init__(self, net, dim):
        self.net, self.dim = net, dim

    def set_problem(self, problem):
        maze = torch.FloatTensor(problem['map'].reshape(1, 15, 15)).double()
        goal = torch.FloatTensor(problem['goal_state'].reshape(1, self.dim)).double()
        self.pb_rep = self.net.pb_forward(goal, maze)

    def net_forward(self, states, use_np=True):
        assert not use_np
        y = self.net.state_forward(torch.FloatTensor(states).double(), self.pb_rep)
        return y[:, :self.dim], y[:, -1]


def run_train(model, net, replay, env, double):
    perms = []
    real_perm, real_torch = np.random.permutation, train_next.torch

    def permutation(n):
        perms.append(real_perm(n))
        return perms[-1]
    writer = Writer()
    np.random.permutation = permutation
    if double:
        shim = types.SimpleNamespace(nn=torch.nn, FloatTensor=lambda x: torch.FloatTensor(x).double())
        train_next.torch = shim
    try:
        np.random.seed(SEED)
        train_next.train(model, torch.optim.Adam(net.parameters(), lr=LR), replay, env, pbar=Pbar(), writer=writer, L=L)
    finally:
        np.random.permutation, train_next.torch = real_perm, real_torch
    return np.array(perms), np.array(writer.totals) / 8.


def main():
    torch.set_num_threads(4)
    for dim in (2, 3):
        env = MazeEnv(dim=dim, map_file=FILES[dim])
        model = Model2D(env=env, cuda=False, dim=dim)
        model.net.load_state_dict(torch.load('data/weights/next_%d.pt' % dim, map_location='cpu'))
        model.net.iters = ITERS
        net64 = copy.deepcopy(model.net).double()
        net64.attention_g.coords = net64.attention_g.coords.double()
        start = {k: v.detach().clone() for k, v in net64.named_parameters()}
        rng = np.random.RandomState(500 + dim)
        probs = [copy.deepcopy(env.init_new_problem(i)) for i in PROBLEMS]
        paths = [make_path(rng, p['init_state'], p['goal_state'], n, dim) for p, n in zip(probs, LENGTHS)]
        replay = [(i, path) for i, path in zip(PROBLEMS, paths)]
        perms32, loss32 = run_train(model, model.net, replay, env, False)
        perms64, loss64 = run_train(Model64(net64, dim), net64, replay, env, True)
        assert np.array_equal(perms32, perms64) and len(loss32) == len(loss64) == 3
        groups, running = [], []
        for perm in perms64:
            for batch_i, index in enumerate(perm):
                running.append(int(index))
                if batch_i % 8 == 7:
                    groups.append(running)
                    running = []
        rec = dict(dim=dim, L=L, lr=LR, iters=ITERS, seed=SEED, problem_index=np.array(PROBLEMS, dtype=np.int64),
                   maps=np.stack([p['map'] for p in probs]).astype(np.float32),
                   goals=np.stack([p['goal_state'] for p in probs]).astype(np.float32),
                   inits=np.stack([p['init_state'] for p in probs]).astype(np.float32),
                   paths=np.concatenate(paths), path_ptr=np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64),
                   problem=np.arange(len(PROBLEMS), dtype=np.int64), perms=perms64.astype(np.int64),
                   groups=np.concatenate(groups).astype(np.int64),
                   group_ptr=np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64),
                   loss32=loss32.astype(np.float64), loss64=loss64.astype(np.float64))
        for k, v in net64.named_parameters():
            rec['d64.' + k] = (v.detach() - start[k]).numpy().astype(np.float32)
        out = os.path.join(OUT, 'next_train_loop_maze%d.npz' % dim)
        np.savez_compressed(out, **rec)
        print('next_train_loop_maze%d: groups %s  loss32 %s  loss64 %s  %d bytes'
              % (dim, [len(g) for g in groups], loss32.tolist(), loss64.tolist(), os.path.getsize(out)))


if __name__ == '__main__':
    main()
