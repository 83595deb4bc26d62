"""gnnmp_next_path_loss (gnnmp.next_replay.path_loss): loss, terms and dy against float64 torch autograd of
next_train.loss_from_outputs scaled to the divisor, for G = 1, 8 and 11 paths with divisor 8, path lengths that include 1 and 65
(one wave walks a path in chunks of 64 rows), both robots.

Bars: |g - g64| <= max(1e-4 max|g64|, 4 own) + 1e-6 with own the float32 torch result's error (the project's gradient bar), the
same form for the loss and the terms.  Two runs are bit-equal, and the backward of path_loss hands back exactly dy.  Run with
-s for the figures."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_replay, next_train

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENS = {1: [65], 8: [1, 65, 7, 64, 2, 63, 10, 3], 11: [9, 1, 65, 4, 12, 1, 66, 5, 8, 130, 2]}


def _case(dim, G):
    rng = np.random.RandomState(50 + 10 * dim + G)
    ptr = np.concatenate([[0], np.cumsum(LENS[G])]).astype(np.int64)
    S = int(ptr[-1])
    y = rng.randn(S, dim + 1).astype(np.float32)
    actions = (0.05 * rng.randn(S, dim)).astype(np.float32)
    values = (-rng.rand(S)).astype(np.float32)
    return ptr, y, actions, values


def _torch_ref(ptr, y, actions, values, G, dtype):
    yt = torch.from_numpy(y).to(dtype).requires_grad_(True)
    loss = next_train.loss_from_outputs(yt, torch.from_numpy(actions).to(dtype), torch.from_numpy(values).to(dtype), ptr) * (G / 8.)
    loss.backward()
    return float(loss.detach()), yt.grad.numpy().astype(np.float64)


def _bar(ref64, ref32):
    return max(1e-4 * np.abs(ref64).max(), 4 * np.abs(np.asarray(ref32, dtype=np.float64) - ref64).max()) + 1e-6


@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('G', [1, 8, 11])
def test_loss_terms_and_dy_against_float64_autograd(dim, G):
    ptr, y, actions, values = _case(dim, G)
    l64, g64 = _torch_ref(ptr, y, actions, values, G, torch.float64)
    l32, g32 = _torch_ref(ptr, y, actions, values, G, torch.float32)
    dev = lambda a, dt: torch.from_numpy(a).to(device=DEV, dtype=dt)      # noqa: E731
    args = (dev(y, torch.float32), dev(actions, torch.float32), dev(values, torch.float32), dev(ptr, torch.int32), 8)
    terms, loss, dy = next_replay.path_loss_device(*args)
    terms2, loss2, dy2 = next_replay.path_loss_device(*args)
    assert torch.equal(terms, terms2) and torch.equal(loss, loss2) and torch.equal(dy, dy2)        # two runs, the same bits
    terms, loss, dy = terms.cpu().numpy(), float(loss.cpu()), dy.cpu().numpy().astype(np.float64)
    t64, _, _ = next_replay.path_loss_reference(y, actions, values, ptr, 8)
    t32 = np.array([[float(((torch.from_numpy(values[a:b]) - torch.from_numpy(y[a:b, -1])) ** 2).mean()),
                     float(((torch.from_numpy(actions[a:b]) - torch.from_numpy(y[a:b, :-1])) ** 2).mean())]
                    for a, b in zip(ptr[:-1], ptr[1:])])
    print('dim %d G %d: loss %.12g  float64 %.12g  float32 %.9g  err %.2e  bar %.2e' % (dim, G, loss, l64, l32, abs(loss - l64), _bar(l64, l32)))
    print('           terms err %.2e  bar %.2e   dy err %.2e  bar %.2e  (own %.2e)'
          % (np.abs(terms - t64).max(), _bar(t64, t32), np.abs(dy - g64).max(), _bar(g64, g32), np.abs(g32 - g64).max()))
    assert abs(loss - l64) <= _bar(np.array(l64), l32)
    assert np.abs(terms - t64).max() <= _bar(t64, t32)
    assert np.abs(dy - g64).max() <= _bar(g64, g32)
    # the sums are double chains: far inside the bars
    assert abs(loss - l64) <= 1e-12 * abs(l64) and np.abs(terms - t64).max() <= 1e-12 * np.abs(t64).max()
    assert np.abs(dy - g64).max() <= 2.0 ** -23 * np.abs(g64).max()      # one float32 rounding of the float64 gradient


@pytest.mark.parametrize('dim', [2, 3])
def test_backward_of_path_loss_is_dy(dim):
    ptr, y, actions, values = _case(dim, 11)
    dev = lambda a, dt: torch.from_numpy(a).to(device=DEV, dtype=dt)      # noqa: E731
    yd = dev(y, torch.float32).requires_grad_(True)
    a, v, p = dev(actions, torch.float32), dev(values, torch.float32), dev(ptr, torch.int32)
    loss, terms = next_replay.path_loss(yd, a, v, p, 8, return_terms=True)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and not terms.requires_grad
    loss.backward()
    t2, l2, dy = next_replay.path_loss_device(yd.detach(), a, v, p, 8)
    assert torch.equal(yd.grad, dy) and torch.equal(loss.detach().reshape(1), l2) and torch.equal(terms, t2)
    # through a scale, as an optimizer step with a weighted loss would see it
    yd.grad = None
    (next_replay.path_loss(yd, a, v, p, 8) * 0.5).backward()
    assert torch.equal(yd.grad, dy * 0.5)
