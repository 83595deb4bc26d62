"""NextNetTrain.train_step: 10 Adam steps (lr 1e-3) on the two recorded problems of each robot at 20 rounds, next to the same
10 steps of the float64 and of the float32 torch restatement (tests/next_train_host.py) on the CPU.

The loss falls; at every step |loss - loss64| <= max(1e-4 |loss64|, 4 own) + 1e-6 with own = |loss32 - loss64| of the
restatement at that step (the project's bar, applied to the trajectory); the exported state_dict, loaded into the inference
network NextNet, reproduces the trained module's y bit for bit.  Run with -s for the three trajectories."""
import os

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_model, next_train
import next_train_host as host

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda:0'
STEPS, LR, ITERS = 10, 1e-3, 20


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}


def _host_trajectory(w, fx, dtype):
    ptr = fx['path_ptr'][:3]
    n = int(ptr[-1])
    actions, values = next_train.path_labels(fx['paths'][:n], ptr, int(fx['dim']))
    actions, values = torch.from_numpy(actions).to(dtype), torch.from_numpy(values).to(dtype)
    states = fx['paths'][:n].astype(np.float32)
    of = np.repeat(np.arange(2), np.diff(ptr))
    leaves = host.leaves(w, dtype)
    opt = torch.optim.Adam(list(leaves.values()), lr=LR)
    losses = []
    for _ in range(STEPS):
        loss = next_train.loss_from_outputs(host.forward(leaves, fx['maps'][:2], fx['goals'][:2], states, of, ITERS), actions, values, ptr)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


@pytest.mark.parametrize('dim', [2, 3])
def test_ten_adam_steps_follow_the_float64_restatement(dim):
    w = _load('next_%d_weights.npz' % dim)
    fx = _load('next_train_maze%d.npz' % dim)
    l64 = _host_trajectory(w, fx, torch.float64)
    l32 = _host_trajectory(w, fx, torch.float32)
    net = next_train.NextNetTrain(dim, device=DEV).load_state_dict(w)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    ptr = fx['path_ptr'][:3]
    n = int(ptr[-1])
    maps = torch.from_numpy(fx['maps'][:2]).to(DEV)
    goals = torch.from_numpy(fx['goals'][:2]).to(DEV)
    losses = [net.train_step(opt, maps, goals, fx['paths'][:n], ptr, ITERS) for _ in range(STEPS)]
    losses = [float(v) for v in losses]
    net.check_status()
    for i in range(STEPS):
        own = abs(l32[i] - l64[i])
        bar = max(1e-4 * abs(l64[i]), 4 * own) + 1e-6
        print('dim %d step %d: device %.9g  float64 %.9g  float32 %.9g  |device - float64| %.2e  bar %.2e'
              % (dim, i, losses[i], l64[i], l32[i], abs(losses[i] - l64[i]), bar))
    assert losses[-1] < losses[0]
    for i in range(STEPS):
        assert abs(losses[i] - l64[i]) <= max(1e-4 * abs(l64[i]), 4 * abs(l32[i] - l64[i])) + 1e-6, i

    # the trained parameters, exported and loaded into the inference network
    states = torch.from_numpy(fx['paths'][:n].astype(np.float32)).to(DEV)
    of = torch.from_numpy(np.repeat(np.arange(2, dtype=np.int32), np.diff(ptr))).to(DEV)
    with torch.no_grad():
        y = net.forward(maps, goals, states, of, ITERS)
    sd = net.state_dict()
    assert any(not np.array_equal(sd[k].cpu().numpy(), w[k]) for k in w)                 # it did train
    plain = next_model.NextNet(dim).load_state_dict(sd)
    assert torch.equal(y, plain.state_forward(states, of, plain.pb_forward(maps, goals, ITERS)))
    plain.check_status()
