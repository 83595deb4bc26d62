"""gnnmp_smooth_path_loss (gnnmp.smoother_replay.path_loss): train_smoother.py:55-58 on the device.

    terms   against path_loss_reference (float64 numpy, the same order of sums): 1e-12 relative
    loss    |loss - l64| <= max(1e-4 |l64|, 4 |l32 - l64|) + 1e-6, l32 the float32 torch expression
    d_pred  within 2 float32 ulps of the float64 value; end rows (and every row of a path without interior) exactly zero
    two runs give the same bits; the backward scales d_pred by a non-unit upstream gradient

Shapes: G = 1, 8, 3 (a short group with divisor 3) and 11 (more paths than the launch has waves); P in {2, 3, 4, 65, 130}
(65 interior elements at C = 2 .. beyond one 64-element chunk); C in {2, 3, 14}."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import smoother_replay as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GROUPS = {'G1': ((130,), 1), 'G8': ((2, 3, 4, 65, 130, 3, 4, 65), 8), 'G3': ((4, 2, 65), 3),
          'G11': ((3, 4, 2, 65, 3, 130, 4, 3, 2, 4, 65), 11)}
_CASES = {}


def _case(C, group):
    """Inputs and the float64 / float32 host values, computed once and left unchanged."""
    key = (C, group)
    if key not in _CASES:
        lengths, divisor = GROUPS[group]
        gen = torch.Generator().manual_seed(1000 * C + len(lengths))
        ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        pred = torch.rand(int(ptr[-1]), C, generator=gen) * 2 - 1
        target = pred + 0.1 * (torch.rand(int(ptr[-1]), C, generator=gen) * 2 - 1)
        terms, l64, d64 = sr.path_loss_reference(pred.numpy(), target.numpy(), ptr, divisor)
        l32 = sum((torch.nn.functional.mse_loss(target[a:b][1:-1], pred[a:b][1:-1]) for a, b in zip(ptr[:-1], ptr[1:]) if b - a > 2),
                  torch.zeros((), dtype=torch.float32)) / divisor
        _CASES[key] = dict(ptr=ptr, divisor=divisor, pred=pred, target=target, terms=terms, l64=float(l64), d64=d64, l32=float(l32))
    return _CASES[key]


@pytest.mark.parametrize('group', list(GROUPS))
@pytest.mark.parametrize('C', [2, 3, 14])
def test_terms_loss_and_gradient(C, group):
    c = _case(C, group)
    ptr = torch.tensor(c['ptr'], dtype=torch.int32, device=DEV)
    pred = c['pred'].to(DEV).requires_grad_(True)
    loss, terms = sr.path_loss(pred, c['target'].to(DEV), ptr, c['divisor'], return_terms=True)
    assert loss.dtype == torch.float32 and loss.shape == () and terms.dtype == torch.float64 and not terms.requires_grad
    got_terms = terms.cpu().numpy()
    assert np.all(np.abs(got_terms - c['terms']) <= 1e-12 * np.abs(c['terms'])), (got_terms, c['terms'])
    err, bar = abs(float(loss.detach()) - c["l64"]), max(1e-4 * abs(c['l64']), 4 * abs(c['l32'] - c['l64'])) + 1e-6
    print('\nC %d %s: loss %.9e, float64 %.9e, float32 torch %.9e, err %.2e, bar %.2e' % (C, group, float(loss.detach()), c['l64'], c['l32'], err, bar))
    assert err <= bar
    (loss * 2.5).backward()                                        # a non-unit upstream gradient
    _, _, d_pred = sr.path_loss_device(pred.detach(), c['target'].to(DEV), ptr, c['divisor'])
    assert torch.equal(pred.grad, d_pred * torch.tensor(2.5, device=DEV))
    d = d_pred.cpu().numpy()
    ulp = np.spacing(np.abs(c['d64']).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(d.astype(np.float64) - c['d64']) <= 2 * ulp)
    for a, b in zip(c['ptr'][:-1], c['ptr'][1:]):
        assert not d[a].any() and not d[b - 1].any()
        if b - a <= 2:
            assert not d[a:b].any()
    # two runs, the same bits
    terms2, loss2, d2 = sr.path_loss_device(pred.detach(), c['target'].to(DEV), ptr, c['divisor'])
    assert torch.equal(terms2, terms) and torch.equal(loss2.reshape(()), loss.detach()) and torch.equal(d2, d_pred)
