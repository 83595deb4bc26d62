"""The host side of NEXT training, no GPU: the torch restatement the GPU tests use as their oracle
(tests/next_train_host.py) against the float64 host oracle and the reference's recorded gradients; path_labels against the
recorded get_label outputs; unpack_weight_grads as the adjoint of pack_weights."""
import os

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_model, next_train
import next_train_host as host

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}


def recorded_grads(dim, iters):
    """(g32, g64) of the reference: the fp32 module's gradients, and the .double() module's as g32 + the stored difference."""
    g32 = {k: v.astype(np.float64) for k, v in _load('next_train_maze%d_i%d_g32.npz' % (dim, iters)).items()}
    d64 = _load('next_train_maze%d_i%d_d64.npz' % (dim, iters))
    return g32, {k: g32[k] + d64[k].astype(np.float64) for k in g32}


@pytest.mark.parametrize('dim', [2, 3])
def test_restatement_matches_the_float64_host_oracle(dim):
    """Measured: at most 8e-15 on pb_rep and 5e-14 on y (iters 0, 1, 20; values up to about 20); the bound is 2e-13,
    the figure of the 3-D restatement."""
    w = _load('next_%d_weights.npz' % dim)
    fx = _load('next_net_maze%d.npz' % dim)
    with torch.no_grad():
        leaves = host.leaves(w, torch.float64)
        for iters in (0, 1, 20):
            pb = host.pb_forward(leaves, fx['maps'], fx['goals'], iters)
            ref = next_model.pb_forward_host(w, fx['maps'], fx['goals'], iters=iters)
            err_pb = np.abs(pb.numpy() - ref).max()
            y = host.state_forward(leaves, fx['states'], fx['problem_of_state'], pb)
            err_y = np.abs(y.numpy() - next_model.state_forward_host(w, fx['states'], fx['problem_of_state'], ref)).max()
            print('dim %d iters %d: pb_rep %.3e  y %.3e' % (dim, iters, err_pb, err_y))
            assert err_pb <= 2e-13 and err_y <= 2e-13


@pytest.mark.parametrize('iters', [0, 1, 2, 20])
@pytest.mark.parametrize('dim', [2, 3])
def test_restatement_matches_the_recorded_gradients(dim, iters):
    """The restatement in float64 against the reference's .double() gradients of train()'s loss: they differ by float64
    rounding only (the stored g64 carries 1e-7 of own = |g32 - g64|, about 1e-12 of the gradient)."""
    w = _load('next_%d_weights.npz' % dim)
    fx = _load('next_train_maze%d.npz' % dim)
    npb = 2 if iters == 20 else 1
    ptr = fx['path_ptr'][:npb + 1]
    n = int(ptr[-1])
    g32, g64 = recorded_grads(dim, iters)
    leaves = host.leaves(w, torch.float64)
    of = np.repeat(np.arange(npb), np.diff(ptr))
    states = fx['paths'][:n].astype(np.float32)
    y = host.forward(leaves, fx['maps'][:npb], fx['goals'][:npb], states, of, iters)
    actions = torch.from_numpy(fx['actions'][:n].astype(np.float32)).double()
    values = torch.from_numpy(fx['values'][:n].astype(np.float32)).double()
    loss = next_train.loss_from_outputs(y, actions, values, ptr)
    assert abs(float(loss.detach()) - float(fx['loss64_i%d' % iters])) <= 1e-11 * max(1., abs(float(loss.detach())))
    got = host.grads_of(loss, leaves)
    for k in g64:
        err, scale = np.abs(got[k] - g64[k]).max(), np.abs(g64[k]).max()
        own = np.abs(g32[k] - g64[k]).max()
        assert err <= 1e-9 * scale + 1e-6 * own + 1e-13, (k, err, scale, own)


@pytest.mark.parametrize('dim', [2, 3])
def test_path_labels_equal_get_label(dim):
    fx = _load('next_train_maze%d.npz' % dim)
    actions, values = next_train.path_labels(fx['paths'], fx['path_ptr'], dim)
    assert actions.dtype == np.float32 and values.dtype == np.float32
    assert np.array_equal(actions, fx['actions'].astype(np.float32))
    assert np.array_equal(values, fx['values'].astype(np.float32))
    assert not actions[fx['path_ptr'][1:] - 1].any() and not values[fx['path_ptr'][1:] - 1].any()
    steps = np.linalg.norm(actions, axis=1)
    assert (steps <= 0.05 * (1 + 1e-6)).all() and (steps[:-1] > 0.049).sum() >= 8 and ((steps > 0) & (steps < 0.04)).any()
    one = next_train.path_labels(fx['paths'][:7], [0, 7], dim)
    assert np.array_equal(one[0], actions[:7]) and np.array_equal(one[1], values[:7])
    with pytest.raises(ValueError):
        next_train.path_labels(fx['paths'], [0, 7], dim)


@pytest.mark.parametrize('dim', [2, 3])
def test_unpack_is_the_adjoint_of_pack(dim):
    rng = np.random.RandomState(dim)
    shapes = next_train.param_shapes(dim)
    w = {k: rng.standard_normal(s).astype(np.float32) for k, s in shapes.items()}
    packed = next_model.pack_weights(w, dim)
    assert packed.shape[0] == next_model.weights_floats(dim)
    g = rng.standard_normal(packed.shape[0])
    u = next_train.unpack_weight_grads(g, dim)
    assert sorted(u) == sorted(shapes) and all(u[k].shape == shapes[k] for k in shapes)
    lhs = float(packed.astype(np.float64) @ g)
    rhs = sum(float((w[k].astype(np.float64) * u[k]).sum()) for k in w)
    assert abs(lhs - rhs) <= 1e-9 * np.abs(packed.astype(np.float64) * g).sum()
    assert np.array_equal(u['lstm.bias_ih'], u['lstm.bias_hh'])
    # padding lanes get nothing: a gradient that lives only on them unpacks to zeros
    used = np.zeros(packed.shape[0], dtype=bool)
    for k, v in next_train._pack_index(dim).items():
        used[v.reshape(-1)] = True
    assert (~used).sum() > 0
    pad_only = np.where(used, 0., 1.)
    assert all(not v.any() for v in next_train.unpack_weight_grads(pad_only, dim).values())
    ut = next_train.unpack_weight_grads(torch.from_numpy(g), dim)
    assert all(np.array_equal(ut[k].numpy(), u[k]) for k in u)
