"""The smoother's training passes over the device replay (gnnmp.smoother_replay.train_replay: store.batch ->
ModelSmoother.forward_train_batch -> path_loss -> SGD) against the fp64 oracle (oracle.ref_cpu in training mode) with torch's
own float64 SGD on the same schedule.  The oracle is pinned to the reference by the goldens of tests/test_smoother_parity.py
and tests/test_smoother_autograd_gpu.py; the arithmetic around it here is torch's.

    (a) one step through store + path_loss next to ModelSmoother.training_loss on a host-built batch, twin modules with the
        same weights: pred has the same bits, and both sets of gradients satisfy the project's gradient bar
        |g - g64| <= max(1e-4 max|g64|, 4 own) + 1e-6 per tensor (tests/test_smoother_train_batch_gpu.py's reference()).
    (b) train_replay over 11 samples, 2 passes = four steps with 8, 3, 8 and 3 terms: every step's loss satisfies
        |loss - l64| <= max(1e-4 |l64|, 4 |l32 - l64|) + 1e-6 with l64 / l32 the float64 / float32 oracle trajectories.
    (c) the history's lr follows ReduceLROnPlateau(patience=0) applied to its means, and the best state is the pass with the
        lowest mean.

Every sample keeps test_smoother_autograd_scale_gpu's kNN margin at every step's weights (asserted on the host in fp64; the
seeds were picked on the CPU so that it holds)."""
import numpy as np
import pytest
import torch

from conftest import load_weights
from gnnmp import planner
from gnnmp import smoother_replay as sr
from gnnmp.smoother import SMOOTHER_TRAINABLE, SmoothBatch
from oracle import ref_cpu
from test_smoother_autograd_scale_gpu import KNN_MARGIN, _knn_margin, _mse_inner, _problem
from test_smoother_parity import CONF, make
from test_smoother_train_batch_gpu import grads, reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAME = 'smooth_2d_attv3'
STEP_SEED = 4102            # (a): eight samples with a loop count each
REPLAY_SEED = 4209          # (b), (c): eleven samples
SCHEDULE_SEED = 77
LR, MOMENTUM, WEIGHT_DECAY = 1e-3, 0.9, 1e-4
_CACHE = {}


def _samples(seed, n):
    C, scale = CONF[NAME]
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        P, F, Co, loop = (int(torch.randint(lo, hi, (1,), generator=gen)) for lo, hi in ((4, 30), (20, 120), (1, 60), (1, 10)))
        out.append(_problem(gen, C, P, F, Co, scale, loop))
    return out


def _store_of(samples):
    C = CONF[NAME][0]
    store = sr.SmoothReplayStore(C, len(samples), sum(q['path'].shape[0] for q in samples), sum(q['free'].shape[0] for q in samples),
                                 sum(q['collided'].shape[0] for q in samples), DEV)
    ptr = lambda counts: torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=DEV)      # noqa: E731
    n = store.append(torch.cat([q['path'] for q in samples]).to(DEV), torch.cat([q['target'] for q in samples]).to(DEV),
                     ptr([q['path'].shape[0] for q in samples]),
                     torch.cat([torch.cat((q['free'], q['collided'])) for q in samples]).to(DEV),
                     ptr([q['free'].shape[0] + q['collided'].shape[0] for q in samples]),
                     torch.tensor([q['free'].shape[0] for q in samples], dtype=torch.int32, device=DEV),
                     torch.ones(len(samples), dtype=torch.int32, device=DEV), torch.arange(len(samples), dtype=torch.int32, device=DEV))
    assert n == len(samples)
    return store


def _sgd(params):
    return torch.optim.SGD(params, lr=LR, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY)


def test_one_step_through_the_store_next_to_training_loss():
    """(a)"""
    samples = _samples(STEP_SEED, 8)
    loops = [q['loop'] for q in samples]
    assert len(set(loops)) > 2 and loops != sorted(loops, reverse=True)      # the longest-first order is not the stored one
    ref = reference('replay_step', NAME, samples, _mse_inner)                 # asserts the kNN margin of every sample
    store = _store_of(samples)
    # through the store
    m1 = make(NAME).to(DEV)
    m1.train()
    sb, targets, order = store.batch(list(range(8)), loops)
    pred1 = m1.forward_train_batch(sb, [loops[b] for b in order])
    loss1 = sr.path_loss(pred1, targets, sb.path_ptr, 8)
    loss1.backward()
    # the same eight samples, in the same order, as a host-built batch through training_loss
    pick = [samples[b] for b in order]
    edges = torch.from_numpy(planner._chain_edge_indices([q['path'].shape[0] for q in pick]))
    off = np.concatenate([[0], np.cumsum([3 * q['path'].shape[0] - 2 for q in pick])])
    host = SmoothBatch([q['path'] for q in pick], [q['free'] for q in pick], [q['collided'] for q in pick],
                       [edges[:, a:b] for a, b in zip(off[:-1], off[1:])], DEV)
    m2 = make(NAME).to(DEV)
    m2.train()
    loss2 = m2.training_loss(host, torch.cat([q['target'] for q in pick]).to(DEV), [q['loop'] for q in pick])
    loss2.backward()
    m3 = make(NAME).to(DEV)
    m3.train()
    pred3 = m3.forward_train_batch(host, [q['loop'] for q in pick])
    assert torch.equal(pred1.detach(), pred3.detach())                        # the same bits
    l64 = float(_mse_inner(ref['o64'], samples))
    l32 = float(_mse_inner(ref['o32'], samples))
    bar = max(1e-4 * abs(l64), 4 * abs(l32 - l64)) + 1e-6
    print('\nloss through the store %.9e, training_loss %.9e, oracle64 %.9e, oracle32 %.9e, bar %.2e'
          % (float(loss1.detach()), float(loss2.detach()), l64, l32, bar))
    assert abs(float(loss1.detach()) - l64) <= bar and abs(float(loss2.detach()) - l64) <= bar
    for what, m in (('store + path_loss', m1), ('training_loss', m2)):
        g = grads(m)
        for k in SMOOTHER_TRAINABLE:
            err = (g[k] - ref['g64'][k]).abs().max().item()
            print('%s %s gradient err %.3e bar %.3e' % (what, k, err, ref['bars'][k]))
            assert err <= ref['bars'][k], (what, k, err, ref['bars'][k])


def _oracle_trajectory(samples, schedule, dtype, check_margin):
    """The schedule through the oracle with torch's SGD in ``dtype``: the loss of every step."""
    C, scale = CONF[NAME]
    w = load_weights(NAME)
    wd = {k: (t.to(dtype).clone().requires_grad_(True) if t.is_floating_point() and 'running' not in k else t) for k, t in w.items()}
    opt = _sgd([wd[k] for k in SMOOTHER_TRAINABLE])
    losses = []
    for steps in schedule:
        for idx, loops in steps:
            probs = [dict(samples[int(i)], loop=int(l)) for i, l in zip(idx, loops)]
            if check_margin:
                now = {k: (t.detach() if torch.is_tensor(t) else t) for k, t in wd.items()}
                for i, q in zip(idx, probs):
                    assert _knn_margin(now, scale, q) > KNN_MARGIN, ('step', len(losses), 'sample', int(i))
            outs = [ref_cpu.smoother_forward(wd, q['path'].to(dtype), q['free'].to(dtype), q['collided'].to(dtype), q['edge_index'],
                                             q['loop'], scale, training=True) for q in probs]
            loss = _mse_inner(outs, probs)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    return losses


def _replay_case():
    if 'replay' not in _CACHE:
        samples = _samples(REPLAY_SEED, 11)
        schedule = sr.replay_schedule(11, passes=2, group=8, rng=np.random.RandomState(SCHEDULE_SEED))
        assert [len(idx) for steps in schedule for idx, _ in steps] == [8, 3, 8, 3]
        _CACHE['replay'] = dict(samples=samples, schedule=schedule, l64=_oracle_trajectory(samples, schedule, torch.float64, True),
                                l32=_oracle_trajectory(samples, schedule, torch.float32, False))
    return _CACHE['replay']


def test_train_replay_follows_the_oracle_with_float64_sgd():
    """(b)"""
    c = _replay_case()
    m = make(NAME).to(DEV)
    history, best = sr.train_replay(m, _sgd(m.parameters()), _store_of(c['samples']), passes=2, group=8,
                                    rng=np.random.RandomState(SCHEDULE_SEED))
    got = [x for entry in history for x in entry['losses']]
    assert len(got) == 4 and [len(entry['losses']) for entry in history] == [2, 2]
    for step, (loss, l64, l32) in enumerate(zip(got, c['l64'], c['l32'])):
        bar = max(1e-4 * abs(l64), 4 * abs(l32 - l64)) + 1e-6
        print('\nstep %d: loss %.9e, oracle64 %.9e, oracle32 %.9e, err %.2e, bar %.2e' % (step, loss, l64, l32, abs(loss - l64), bar))
        assert np.isfinite(loss) and abs(loss - l64) <= bar, step
    for entry in history:                                         # what train() returns is the undivided sum
        assert np.allclose(entry['sums'], np.array(entry['losses']) * np.array([8, 3]), rtol=0, atol=0)
        assert entry['mean'] == float(np.mean(entry['sums'])) and entry['lr'] == LR
    assert best is not None


def test_history_lr_and_best_state():
    """(c)"""
    c = _replay_case()
    m = make(NAME).to(DEV)
    opt = _sgd(m.parameters())
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, 'min', patience=0)
    states = []
    history, best = sr.train_replay(m, opt, _store_of(c['samples']), passes=4, group=8, rng=np.random.RandomState(SCHEDULE_SEED),
                                    scheduler=scheduler,
                                    log=lambda p, entry: states.append({k: v.detach().clone() for k, v in m.state_dict().items()}))
    assert len(history) == len(states) == 4
    means = [entry['mean'] for entry in history]
    print('\nmeans %s\nlr %s' % (means, [entry['lr'] for entry in history]))
    probe = torch.nn.Parameter(torch.zeros(1))
    twin_opt = _sgd([probe])
    twin = torch.optim.lr_scheduler.ReduceLROnPlateau(twin_opt, 'min', patience=0)
    for entry in history:
        assert entry['lr'] == twin_opt.param_groups[0]['lr']
        twin.step(entry['mean'])
    assert opt.param_groups[0]['lr'] == twin_opt.param_groups[0]['lr']
    low = int(np.argmin(means))                                   # the first pass with the lowest mean
    assert set(best) == set(states[low])
    assert all(torch.equal(best[k], states[low][k]) for k in best)
    fresh = make(NAME)
    fresh.load_state_dict(best)
