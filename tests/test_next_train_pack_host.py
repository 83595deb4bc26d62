"""The packing side of NEXT training, no GPU: device_pack / device_pack_t on CPU tensors against the host packers bit for bit
(random parameters, both dims, the summed LSTM bias included), unpack_weight_grads on the packed position index (the identity,
padding dropped) and on a tensor, and NextNetTrain's state_dict through NextNet.load_state_dict."""
import os

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_model, next_train

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _random_params(dim, seed):
    rng = np.random.default_rng(seed)
    return {k: rng.standard_normal(s).astype(np.float32) * np.float32(rng.uniform(0.01, 3.0)) for k, s in next_train.param_shapes(dim).items()}


@pytest.mark.parametrize('dim', [2, 3])
def test_device_pack_is_bit_equal_to_pack_weights(dim):
    for seed in (0, 1, 2):
        w = _random_params(dim, 100 * dim + seed)
        t = {k: torch.from_numpy(v) for k, v in w.items()}
        host = next_model.pack_weights(w, dim)
        got = next_train.device_pack(t, dim)
        assert got.dtype == torch.float32 and got.shape == (next_model.weights_floats(dim),)
        assert np.array_equal(got.numpy().view(np.uint32), host.view(np.uint32))
        # the one packed LSTM bias is bias_ih + bias_hh, rounded once, and not simply one of the two
        idx = next_train._pack_index(dim)['lstm.bias_ih']
        assert np.array_equal(idx, next_train._pack_index(dim)['lstm.bias_hh'])
        assert np.array_equal(got.numpy()[idx], w['lstm.bias_ih'] + w['lstm.bias_hh'])
        assert not np.array_equal(got.numpy()[idx], w['lstm.bias_ih'])


@pytest.mark.parametrize('dim', [2, 3])
def test_device_pack_t_is_bit_equal_to_pack_weights_t_and_holds_the_transposes(dim):
    w = _random_params(dim, 7 + dim)
    t = {k: torch.from_numpy(v) for k, v in w.items()}
    host = next_train.pack_weights_t(w, dim)
    assert np.array_equal(next_train.device_pack_t(t, dim).numpy().view(np.uint32), host.view(np.uint32))
    assert host.shape == (3 * 36 * 1024 + 128 * 256 + 64,) and not host[-64:].any()
    # conv^T: the packing of the convolution whose weight is the tap-flipped, channel-transposed one
    flipped = dict(w)
    flipped['conv.weight'] = np.ascontiguousarray(np.flip(w['conv.weight'].transpose(1, 0, 2, 3), (2, 3)))
    ref = next_model.pack_weights(flipped, dim)
    lo = next_train._pack_index(dim)['conv.weight'].min()
    assert np.array_equal(host[:36 * 1024], ref[lo:lo + 36 * 1024])
    # the transposed convolution IS the gradient of the convolution with respect to its input
    x = torch.randn(1, 64, 15, 15, dtype=torch.float64, requires_grad=True)
    wc = torch.from_numpy(w['conv.weight']).double()
    d = torch.randn(1, 64, 15, 15, dtype=torch.float64)
    torch.nn.functional.conv2d(x, wc, padding=1).backward(d)
    dx = torch.nn.functional.conv2d(d, torch.from_numpy(flipped['conv.weight']).double(), padding=1)
    assert torch.allclose(x.grad, dx, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('dim', [2, 3])
def test_unpack_of_the_packed_index_is_the_identity_and_padding_is_dropped(dim):
    index = next_train._pack_index(dim)
    n = next_model.weights_floats(dim)
    pos = np.arange(n, dtype=np.float64)
    un = next_train.unpack_weight_grads(pos, dim)
    assert set(un) == set(index) == set(next_train.param_shapes(dim))
    for k, idx in index.items():
        assert np.array_equal(un[k], idx.astype(np.float64)), k
    used = np.zeros(n, dtype=np.int64)
    for k, idx in index.items():
        used[idx.reshape(-1)] += 1
    # every position is hit once, the LSTM bias twice, the padding lanes never: the last attention bias's 3 zeros, columns
    # dim .. 2 of the a3 MLP's first layer, rows dim + 1 .. 3 of the policy's last layer with their biases, and channels
    # 9 .. 15 of the hidden convolution's 9 taps
    assert set(np.unique(used)) <= {0, 1, 2} and int((used == 2).sum()) == 256
    assert int((used == 0).sum()) == 3 + 64 * (3 - dim) + (3 - dim) * 65 + 9 * 7 * 64
    # a gradient that lives only on padding lanes unpacks to zeros
    g = (used == 0).astype(np.float64)
    assert all(not v.any() for v in next_train.unpack_weight_grads(g, dim).values())
    with pytest.raises(ValueError):
        next_train.unpack_weight_grads(pos[:-1], dim)


@pytest.mark.parametrize('dim', [2, 3])
def test_unpack_of_a_tensor_gives_tensors_equal_to_the_numpy_path(dim):
    g = np.random.default_rng(40 + dim).standard_normal(next_model.weights_floats(dim))
    un = next_train.unpack_weight_grads(g, dim)
    tu = next_train.unpack_weight_grads(torch.from_numpy(g), dim)
    assert set(tu) == set(un) and all(isinstance(v, torch.Tensor) and v.dtype == torch.float64 for v in tu.values())
    for k, shape in next_train.param_shapes(dim).items():
        assert tuple(tu[k].shape) == tuple(shape) == un[k].shape and np.array_equal(tu[k].numpy(), un[k]), k
    assert torch.equal(tu['lstm.bias_ih'], tu['lstm.bias_hh'])


@pytest.mark.parametrize('dim', [2, 3])
def test_state_dict_round_trips_through_nextnet(dim):
    with np.load(os.path.join(GOLDEN, 'next_%d_weights.npz' % dim)) as f:
        w = {k: f[k] for k in f.files}
    net = next_train.NextNetTrain(dim, device='cpu').load_state_dict(w)
    names = [k for k, _ in net.named_parameters()]
    assert names == list(next_train.param_shapes(dim)) and all(isinstance(p, torch.nn.Parameter) for p in net.parameters())
    sd = net.state_dict()
    assert set(sd) == set(w)                    # attention_s.* written out as copies of attention_g.*
    for k in sd:
        if k.startswith('attention_s.'):
            assert torch.equal(sd[k], sd['attention_g.' + k[len('attention_s.'):]])
    plain = next_model.NextNet(dim).load_state_dict(sd)
    assert np.array_equal(plain._packed, next_model.pack_weights(w, dim))
    assert np.array_equal(next_train.device_pack(dict(net.named_parameters()), dim).numpy(), plain._packed)
    with pytest.raises(RuntimeError):           # the kernels are the only implementation
        net.forward(torch.zeros(1, 15, 15), torch.zeros(1, dim), torch.zeros(1, dim), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        net.train_step(None, torch.zeros(0, 15, 15), torch.zeros(0, dim), np.zeros((0, dim)), np.zeros(1, dtype=np.int64))
