"""NEXT's training loop on the host, no GPU: gnnmp.next_replay.train_replay_host over the float64 torch restatement
(tests/next_train_host.py) against train() of the UNMODIFIED reference, recorded by tools/gen_golden_next_train_loop.py on a
replay of 11 paths with L = 3 (tests/golden/next_train_loop_maze{2,3}.npz).

  * the schedule: the permutations of RandomState(1234) are the recorded ones, the index groups equal the recording exactly
    (8 / 11 / 11 terms: the trailing 3 samples of a pass join the first step of the next) and every step divides by 8;
  * every step loss: |loss - l64| <= max(1e-4 |l64|, 4 |l32 - l64|) + 1e-6 with l64 / l32 the reference's recorded .double()
    and float32 losses (the project's bar, the reference as the yardstick);
  * the host restatement of gnnmp_next_path_loss and its dy against torch autograd of next_train.loss_from_outputs in float64,
    scaled to the divisor, for divisor 8 with 8 and with 11 paths.
Run with -s for the figures."""
import os

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_replay, next_train
import next_train_host as host

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}


def _groups(fx):
    return [fx['groups'][a:b].tolist() for a, b in zip(fx['group_ptr'][:-1], fx['group_ptr'][1:])]


@pytest.mark.parametrize('dim', [2, 3])
def test_schedule_is_the_recorded_one(dim):
    fx = _load('next_train_loop_maze%d.npz' % dim)
    groups, perms = next_replay.replay_schedule(len(fx['problem']), int(fx['L']), 8, np.random.RandomState(int(fx['seed'])))
    assert np.array_equal(np.array(perms), fx['perms'])
    assert groups == _groups(fx)
    assert [len(g) for g in groups] == [8, 11, 11]
    # the carry-over: step 2 is the 3 trailing samples of pass 0, then the first 8 of pass 1; the tail of the last pass is dropped
    assert groups[1] == fx['perms'][0][8:].tolist() + fx['perms'][1][:8].tolist()
    assert groups[2] == fx['perms'][1][8:].tolist() + fx['perms'][2][:8].tolist()
    default, _ = next_replay.replay_schedule(11, 3)
    assert default == groups                                     # the default stream is RandomState(1234)
    assert next_replay.replay_schedule(7, 5)[0] == []            # fewer samples than a group: train() never steps
    assert [len(g) for g in next_replay.replay_schedule(16, 2)[0]] == [8, 8, 8, 8]


@pytest.mark.parametrize('dim', [2, 3])
def test_float64_loop_follows_the_reference(dim):
    fx = _load('next_train_loop_maze%d.npz' % dim)
    w = _load('next_%d_weights.npz' % dim)
    leaves = host.leaves(w, torch.float64)
    opt = torch.optim.Adam(list(leaves.values()), lr=float(fx['lr']))
    fwd = lambda maps, goals, states, of, iters: host.forward(leaves, maps, goals, states, of, iters)      # noqa: E731
    losses, groups = next_replay.train_replay_host(fwd, opt, fx['paths'], fx['path_ptr'], fx['problem'], fx['maps'], fx['goals'], dim,
                                                   L=int(fx['L']), group=8, rng=np.random.RandomState(int(fx['seed'])),
                                                   iters=int(fx['iters']))
    assert groups == _groups(fx)
    assert len(losses) == 3
    for i, (l, l64, l32) in enumerate(zip(losses, fx['loss64'], fx['loss32'])):
        bar = max(1e-4 * abs(l64), 4 * abs(l32 - l64)) + 1e-6
        print('dim %d step %d (%d terms): host %.12g  reference .double() %.12g  float32 %.9g  |host - l64| %.2e  bar %.2e'
              % (dim, i, len(groups[i]), l, l64, l32, abs(l - l64), bar))
        assert abs(l - l64) <= bar, i
    # the parameters after the three steps, against the .double() run's (start + recorded difference): printed, not asserted --
    # Adam moves a parameter by about lr a step whatever the size of its gradient, so a gradient at rounding level may differ
    worst = 0.
    for k, v in leaves.items():
        ref = w[k].astype(np.float64) + fx['d64.' + k].astype(np.float64)
        worst = max(worst, float(np.abs(v.detach().numpy() - ref).max()))
    print('dim %d: max |parameter - reference .double() parameter| after 3 steps %.3e (Adam, lr 1e-3)' % (dim, worst))


@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('G', [8, 11])
def test_path_loss_restatement_against_autograd(dim, G):
    rng = np.random.RandomState(40 + dim + G)
    lens = rng.randint(1, 14, G)
    lens[0], lens[-1] = 1, 13
    ptr = np.concatenate([[0], np.cumsum(lens)])
    S = int(ptr[-1])
    y, actions, values = rng.randn(S, dim + 1), 0.05 * rng.randn(S, dim), -rng.rand(S)
    terms, loss, dy = next_replay.path_loss_reference(y, actions, values, ptr, 8)
    yt = torch.from_numpy(y).requires_grad_(True)
    ref = next_train.loss_from_outputs(yt, torch.from_numpy(actions), torch.from_numpy(values), ptr) * (G / 8.)
    ref.backward()
    assert abs(loss - float(ref.detach())) <= 1e-13 * abs(float(ref.detach()))
    assert np.abs(dy - yt.grad.numpy()).max() <= 1e-13 * np.abs(yt.grad.numpy()).max()
    for g in range(G):
        a, b = ptr[g], ptr[g + 1]
        assert abs(terms[g, 0] - ((values[a:b] - y[a:b, dim]) ** 2).mean()) <= 1e-14
        assert abs(terms[g, 1] - ((actions[a:b] - y[a:b, :dim]) ** 2).mean()) <= 1e-14
