"""gnnmp.next_replay.train_replay on the device against train() of the UNMODIFIED reference, recorded by
tools/gen_golden_next_train_loop.py (tests/golden/next_train_loop_maze{2,3}.npz): a replay of 11 paths, L = 3, 20 rounds, Adam
(lr 1e-3) from the shipped checkpoint, the permutations of np.random.seed(1234).

  * the index groups are the recorded ones (8 / 11 / 11 terms, every step divided by 8);
  * every step loss: |loss - l64| <= max(1e-4 |l64|, 4 |l32 - l64|) + 1e-6 with l64 / l32 the reference's recorded .double() and
    float32 losses;
  * the loss of step 3 is below step 1's exactly when the recording's is;
  * the exported state_dict, loaded into the inference network NextNet, reproduces the trained module's y bit for bit;
  * a second run gives bit-equal parameters and losses.
Run with -s for the figures."""
import os

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_model, next_replay, next_train

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda:0'


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}


def _run(dim, fx, w):
    net = next_train.NextNetTrain(dim, device=DEV).load_state_dict(w)
    opt = torch.optim.Adam(net.parameters(), lr=float(fx['lr']))
    store = next_replay.ReplayStore(dim, len(fx['problem']), len(fx['paths']), DEV)
    store.append_paths(fx['paths'], fx['path_ptr'], fx['problem'])
    maps, goals = torch.from_numpy(fx['maps']).to(DEV), torch.from_numpy(fx['goals']).to(DEV)
    seen = []
    losses, groups = next_replay.train_replay(net, opt, store, maps, goals, L=int(fx['L']), group=8,
                                              rng=np.random.RandomState(int(fx['seed'])), iters=int(fx['iters']),
                                              log=lambda step, loss: seen.append(step))
    net.check_status()
    assert seen == list(range(len(groups)))
    assert all(l.device.type == 'cuda' and l.dim() == 0 for l in losses)
    return net, store, maps, goals, [float(l) for l in losses], groups


@pytest.mark.parametrize('dim', [2, 3])
def test_three_steps_follow_the_recorded_train(dim):
    fx = _load('next_train_loop_maze%d.npz' % dim)
    w = _load('next_%d_weights.npz' % dim)
    net, store, maps, goals, losses, groups = _run(dim, fx, w)
    want = [fx['groups'][a:b].tolist() for a, b in zip(fx['group_ptr'][:-1], fx['group_ptr'][1:])]
    assert groups == want and [len(g) for g in groups] == [8, 11, 11]
    l64, l32 = fx['loss64'], fx['loss32']
    for i in range(3):
        bar = max(1e-4 * abs(l64[i]), 4 * abs(l32[i] - l64[i])) + 1e-6
        print('dim %d step %d (%d terms): device %.9g  reference .double() %.9g  float32 %.9g  |device - l64| %.2e  bar %.2e'
              % (dim, i, len(groups[i]), losses[i], l64[i], l32[i], abs(losses[i] - l64[i]), bar))
    for i in range(3):
        assert abs(losses[i] - l64[i]) <= max(1e-4 * abs(l64[i]), 4 * abs(l32[i] - l64[i])) + 1e-6, i
    assert (losses[2] < losses[0]) == bool(l64[2] < l64[0])

    # the trained parameters, exported and loaded into the inference network
    sd = net.state_dict()
    assert any(not np.array_equal(sd[k].cpu().numpy(), w[k]) for k in w)                 # it did train
    b = store.batch(groups[1])
    pid = torch.from_numpy(np.asarray(b['problems'], dtype=np.int64)).to(DEV)
    with torch.no_grad():
        y = net.forward(maps[pid], goals[pid], b['states32'], b['problem_of_state'], int(fx['iters']))
    plain = next_model.NextNet(dim).load_state_dict(sd)
    assert torch.equal(y, plain.state_forward(b['states32'], b['problem_of_state'], plain.pb_forward(maps[pid], goals[pid], int(fx['iters']))))
    plain.check_status()
    worst = max(float(np.abs(sd[k].cpu().numpy().astype(np.float64) - (w[k].astype(np.float64) + fx['d64.' + k])).max())
                for k in w if not k.startswith('attention_s.'))
    print('dim %d: max |parameter - reference .double() parameter| after 3 steps %.3e (printed, not asserted: Adam moves a '
          'parameter by about lr = 1e-3 a step whatever the size of its gradient)' % (dim, worst))

    # a second run: the same bits
    net2, _, _, _, losses2, groups2 = _run(dim, fx, w)
    assert groups2 == groups and losses2 == losses
    sd2 = net2.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
