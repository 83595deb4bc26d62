"""The device forward / backward of NEXT training (gnnmp.next_train.NextNetTrain over csrc/next_train_kernels.hip) on the
recorded shapes: 2 problems with paths of 7 and 10 states at 20 rounds, 1 problem with 7 states at 0, 1 and 2 rounds.

  * the forward's y and pb_rep are the inference kernels' bits;
  * train()'s loss against the reference's recorded losses (the bound of tests/test_next_train_gpu.py);
  * the gradients against the unmodified reference's recorded fp32 / .double() gradients through the project's gradient bar,
    next_train_host.check_bar: per tensor |g - g64| <= max(1e-4 max|g64|, 4 own) + 1e-6, own = max|g32 - g64|;
  * indexing (problem_of_state in any order, a problem without states), run-to-run bits, the status words, the empty call, a backward
    after a later forward.
Run with -s for error / bar per tensor."""
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
CASES = ((20, 2), (0, 1), (1, 1), (2, 1))
_CACHE = {}


def _load(name):
    if name not in _CACHE:
        with np.load(os.path.join(GOLDEN, name)) as f:
            _CACHE[name] = {k: f[k] for k in f.files}
    return _CACHE[name]


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _net(dim):
    return next_train.NextNetTrain(dim, device=DEV).load_state_dict(_load('next_%d_weights.npz' % dim))


def _recorded(dim, iters):
    g32 = {k: v.astype(np.float64) for k, v in _load('next_train_maze%d_i%d_g32.npz' % (dim, iters)).items()}
    d64 = _load('next_train_maze%d_i%d_d64.npz' % (dim, iters))
    return g32, {k: g32[k] + d64[k].astype(np.float64) for k in g32}


def _case(dim, iters, npb):
    fx = _load('next_train_maze%d.npz' % dim)
    ptr = fx['path_ptr'][:npb + 1]
    n = int(ptr[-1])
    of = np.repeat(np.arange(npb, dtype=np.int32), np.diff(ptr))
    return dict(fx=fx, ptr=ptr, maps=_t(fx['maps'][:npb]), goals=_t(fx['goals'][:npb]), states=_t(fx['paths'][:n].astype(np.float32)),
                of=_t(of, torch.int32), actions=_t(fx['actions'][:n].astype(np.float32)), values=_t(fx['values'][:n].astype(np.float32)))


def _grads(net, loss):
    for p in net.parameters():
        p.grad = None
    loss.backward()
    return {k: p.grad.detach().clone() for k, p in net.named_parameters()}


def _train_loss_and_grads(net, c, iters):
    y = net.forward(c['maps'], c['goals'], c['states'], c['of'], iters)
    loss = next_train.loss_from_outputs(y, c['actions'], c['values'], c['ptr'])
    return y, loss, _grads(net, loss)


@pytest.mark.parametrize('dim', [2, 3])
def test_forward_has_the_bits_of_the_inference_kernels(dim):
    net = _net(dim)
    plain = next_model.NextNet(dim).load_state_dict(_load('next_%d_weights.npz' % dim))
    for iters, npb in CASES:
        c = _case(dim, iters, npb)
        with torch.no_grad():
            y = net.forward(c['maps'], c['goals'], c['states'], c['of'], iters)
        pb = plain.pb_forward(c['maps'], c['goals'], iters)
        assert torch.equal(net.pb_rep, pb), iters
        assert torch.equal(y, plain.state_forward(c['states'], c['of'], pb)), iters
    net.check_status()
    plain.check_status()


@pytest.mark.parametrize('dim', [2, 3])
def test_loss_value_against_the_recorded_reference(dim):
    net = _net(dim)
    for iters, npb in CASES:
        c = _case(dim, iters, npb)
        with torch.no_grad():
            y = net.forward(c['maps'], c['goals'], c['states'], c['of'], iters)
        loss = float(next_train.loss_from_outputs(y, c['actions'], c['values'], c['ptr']))
        l64 = float(c['fx']['loss64_i%d' % iters])
        own = abs(float(c['fx']['loss32_i%d' % iters]) - l64)
        print('dim %d iters %2d: loss %.9g  reference fp64 %.9g  (reference fp32 off by %.2e)' % (dim, iters, loss, l64, own))
        assert abs(loss - l64) <= max(1e-4 * abs(l64), 4 * own) + 1e-6
    net.check_status()


@pytest.mark.parametrize('iters,npb', CASES)
@pytest.mark.parametrize('dim', [2, 3])
def test_gradients_against_the_recorded_reference(dim, iters, npb):
    net = _net(dim)
    g32, g64 = _recorded(dim, iters)
    _, _, got = _train_loss_and_grads(net, _case(dim, iters, npb), iters)
    net.check_status()
    assert set(got) == set(next_train.param_shapes(dim)) == set(g64)
    for k, shape in next_train.param_shapes(dim).items():
        assert tuple(got[k].shape) == tuple(shape) and bool(torch.isfinite(got[k]).all()), k
    assert torch.equal(got['lstm.bias_ih'], got['lstm.bias_hh'])
    bad = host.check_bar(got, g32, g64, 'dim %d iters %2d' % (dim, iters))
    assert not bad, bad


def _index_case(dim, n_problems):
    fx = _load('next_train_maze%d.npz' % dim)
    pick = [0, 1, 0, 1][:n_problems]
    maps = fx['maps'][pick].copy()
    goals = fx['goals'][[1, 0, 1, 0][:n_problems]].copy()          # problems 2 and 3: a map with the other problem's goal
    states = fx['paths'][[0, 8, 3, 12, 5]].astype(np.float32)
    of = np.array([2, 0, 2, 0, 2], dtype=np.int32)
    dy = np.random.default_rng(11 + dim).standard_normal((5, dim + 1)).astype(np.float32)
    return maps, goals, states, of, dy


@pytest.mark.parametrize('dim', [2, 3])
def test_indexing_any_order_and_a_problem_without_states(dim):
    """3 problems, 5 states, problem_of_state = [2, 0, 2, 0, 2]: problem 1 has no state.  A random dy, 2 rounds, held to the
    float32 / float64 restatement through the gradient bar; a fourth problem with no states changes no bit."""
    iters = 2
    got = {}
    for n_problems in (3, 4):
        maps, goals, states, of, dy = _index_case(dim, n_problems)
        net = _net(dim)
        y = net.forward(_t(maps), _t(goals), _t(states), _t(of, torch.int32), iters)
        got[n_problems] = (y.detach().clone(), _grads(net, (y * _t(dy)).sum()))
        net.check_status()
    maps, goals, states, of, dy = _index_case(dim, 3)
    _, g32, _, g64 = host.oracle_pair(_load('next_%d_weights.npz' % dim), maps, goals, states, of, iters,
                                      lambda y: (y * torch.from_numpy(dy).to(y.dtype)).sum())
    bad = host.check_bar(got[3][1], g32, g64, 'dim %d indexing' % dim)
    assert not bad, bad
    assert torch.equal(got[3][0], got[4][0])
    for k in got[3][1]:
        assert torch.equal(got[3][1][k], got[4][1][k]), k


@pytest.mark.parametrize('dim', [2, 3])
def test_two_runs_give_the_same_bits(dim):
    net = _net(dim)
    c = _case(dim, 20, 2)
    y1, _, g1 = _train_loss_and_grads(net, c, 20)
    y2, _, g2 = _train_loss_and_grads(net, c, 20)
    assert torch.equal(y1, y2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize('dim', [2, 3])
def test_a_problem_index_outside_the_batch_is_reported_and_takes_no_part(dim):
    iters = 2
    maps, goals, states, of, dy = _index_case(dim, 3)
    bad_row = 1
    of_bad = of.copy()
    of_bad[bad_row] = 3                                             # == B
    keep = np.array([i for i in range(5) if i != bad_row])
    net = _net(dim)
    y = net.forward(_t(maps), _t(goals), _t(states), _t(of_bad, torch.int32), iters)
    g_bad = _grads(net, (y[_t(keep, torch.int64)] * _t(dy[keep])).sum())
    with pytest.raises(RuntimeError, match='outside'):
        net.check_status()
    assert bool(torch.isnan(y[bad_row]).all())
    ref = _net(dim)
    y_ref = ref.forward(_t(maps), _t(goals), _t(states[keep]), _t(of[keep], torch.int32), iters)
    g_ref = _grads(ref, (y_ref * _t(dy[keep])).sum())
    ref.check_status()
    assert torch.equal(y[_t(keep, torch.int64)].detach(), y_ref.detach())
    for k in g_ref:
        assert torch.equal(g_bad[k], g_ref[k]), k


@pytest.mark.parametrize('dim', [2, 3])
def test_empty_call_gives_an_empty_y_and_zero_gradients_without_the_library(dim):
    net = _net(dim)
    c = _case(dim, 2, 1)
    y = net.forward(c['maps'], c['goals'], c['states'][:0], c['of'][:0], 2)
    assert tuple(y.shape) == (0, dim + 1) and y.requires_grad
    g = _grads(net, y.sum())
    assert all(not bool(v.any()) for v in g.values()) and set(g) == set(next_train.param_shapes(dim))
    assert net._generation == 0 and not net._pending and net._ws is None        # the library was never reached
    y = net.forward(c['maps'][:0], c['goals'][:0], c['states'][:0], c['of'][:0], 2)
    assert tuple(y.shape) == (0, dim + 1)
    with pytest.raises(ValueError):
        net.forward(c['maps'][:0], c['goals'][:0], c['states'], c['of'], 2)
    # backward after a later forward (1 problem, 2 states, 1 round): the workspace holds the later one, whose backward still runs
    one = (c['maps'], c['goals'], c['states'][:2], c['of'][:2], 1)
    y_old = net.forward(*one)
    y_new = net.forward(*one)
    with pytest.raises(RuntimeError, match='later forward'):
        y_old.sum().backward()
    g = _grads(net, y_new.sum())
    assert set(g) == set(next_train.param_shapes(dim)) and all(bool(torch.isfinite(v).all()) for v in g.values())
    assert bool(g['policy.4.bias'].any()) and torch.equal(g['lstm.bias_ih'], g['lstm.bias_hh'])
    net.check_status()
