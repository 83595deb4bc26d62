"""train()'s loss evaluated on the device (gnnmp.next_train.training_loss over the inference kernels of NextNet) against the
unmodified reference's recorded losses, tests/golden/next_train_maze*.npz.

Bound: |loss - loss64| <= max(1e-4 |loss64|, 4 own) + 1e-6 with own = |loss32 - loss64| of the reference itself, the form of
the project's gradient bar (tests/test_explorer_autograd_gpu.py).  Run with -s for the figures."""
import os

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_model, next_train

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda:0'


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=torch.float32)


@pytest.mark.parametrize('dim', [2, 3])
def test_training_loss_value_against_the_recorded_reference(dim):
    fx = _load('next_train_maze%d.npz' % dim)
    net = next_model.NextNet(dim).load_state_dict(_load('next_%d_weights.npz' % dim))
    for iters, npb in ((20, 2), (0, 1), (1, 1), (2, 1)):
        ptr = fx['path_ptr'][:npb + 1]
        loss = float(next_train.training_loss(net, _t(fx['maps'][:npb]), _t(fx['goals'][:npb]), fx['paths'][:int(ptr[-1])], ptr, iters))
        l64 = float(fx['loss64_i%d' % iters])
        own = abs(float(fx['loss32_i%d' % iters]) - l64)
        print('dim %d iters %2d: loss %.9g  reference fp64 %.9g  (reference fp32 off by %.2e)' % (dim, iters, loss, l64, own))
        assert abs(loss - l64) <= max(1e-4 * abs(l64), 4 * own) + 1e-6
    net.check_status()
