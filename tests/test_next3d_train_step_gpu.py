"""NextNet3DTrain.train_step: 4 Adam steps (lr 1e-3) on the recorded kuka7 problem 0 at 2 rounds, next to the same steps of the
float64 and of the float32 torch restatement (tests/next3d_train_host.py) on the CPU.

At every step |loss - loss64| <= max(1e-4 |loss64|, 4 own) + 1e-6 with own = |loss32 - loss64| of the restatement at that step
(the margin of tests/test_next_train_step_gpu.py); the loss falls; the exported state_dict, loaded into the inference network
NextNet3D, reproduces the trained module's y bit for bit.  Run with -s for the three trajectories."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_model3d, next_train, next_train3d
import next3d_train_host as host

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STEPS, LR, ITERS, DIM = 4, 1e-3, 2, 7


def _host_trajectory(w, rec, dtype):
    maps, goals, rows, of, ptr, _, _ = host.case_inputs(rec, ITERS)
    n = int(ptr[-1])
    actions, values = next_train3d.path_labels(rec['paths'][:n], ptr, float(rec['rrt_eps']), rec['lo'], rec['hi'])
    actions, values = torch.from_numpy(actions).to(dtype), torch.from_numpy(values).to(dtype)
    leaves = host.leaves(w, dtype)
    opt = torch.optim.Adam(list(leaves.values()), lr=LR)
    losses = []
    for _ in range(STEPS):
        loss = next_train.loss_from_outputs(host.forward(leaves, maps, goals, rows, of, ITERS), actions, values, ptr)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def test_adam_steps_follow_the_float64_restatement():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    w = host.load_weights(DIM)
    rec = host.load_case(DIM)
    pd = int(rec['point_dim'])
    l64 = _host_trajectory(w, rec, torch.float64)
    l32 = _host_trajectory(w, rec, torch.float32)
    net = next_train3d.NextNet3DTrain(DIM, pd, device=DEV).load_state_dict(w)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    maps, goals, rows, of, ptr, _, _ = host.case_inputs(rec, ITERS)
    n = int(ptr[-1])
    maps_d, goals_d = torch.from_numpy(maps).to(DEV), torch.from_numpy(goals).to(DEV)
    losses = [float(net.train_step(opt, maps_d, goals_d, rec['points'][:n], rec['paths'][:n], ptr, float(rec['rrt_eps']), rec['lo'],
                                   rec['hi'], ITERS)) for _ in range(STEPS)]
    net.check_status()
    for i in range(STEPS):
        own = abs(l32[i] - l64[i])
        bar = max(1e-4 * abs(l64[i]), 4 * own) + 1e-6
        print('step %d: device %.9g  float64 %.9g  float32 %.9g  |device - float64| %.2e  bar %.2e'
              % (i, losses[i], l64[i], l32[i], abs(losses[i] - l64[i]), bar))
    assert losses[-1] < losses[0]
    for i in range(STEPS):
        assert abs(losses[i] - l64[i]) <= max(1e-4 * abs(l64[i]), 4 * abs(l32[i] - l64[i])) + 1e-6, i

    # the trained parameters, exported and loaded into the inference network
    rows_d = torch.from_numpy(rows).to(DEV)
    of_d = torch.from_numpy(of).to(DEV)
    with torch.no_grad():
        y = net.forward(maps_d, goals_d, rows_d, of_d, ITERS)
    sd = net.state_dict()
    assert any(not np.array_equal(sd[k].cpu().numpy(), w[k]) for k in w)                 # it did train
    assert all(torch.equal(sd['attention_s.' + k[12:]], sd[k]) for k in sd if k.startswith('attention_g.'))
    plain = next_model3d.NextNet3D(DIM, pd).load_state_dict(sd)
    assert torch.equal(y, plain.state_forward(rows_d, of_d, plain.pb_forward(maps_d, goals_d, ITERS)))
    plain.check_status()
