"""The packing side of 3-D NEXT training, no GPU: gnnmp.next_train3d.unpack_weight_grads is the exact adjoint of
gnnmp.next_model3d.pack_weights, device_pack (run on CPU tensors) is bit-equal to it, and the transposed packing makes the
forward's convolution routine compute the transposed convolution."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gnnmp  # noqa: F401
from gnnmp import next_model3d, next_train3d
import next3d_train_host as host

FAMS = [(7, 3), (14, 6)]


def _random_weights(dim, pd, seed):
    rng = np.random.RandomState(seed)
    return {k: rng.standard_normal(s).astype(np.float32) for k, s in next_train3d.param_shapes(dim, pd).items()}


@pytest.mark.parametrize('dim,pd', FAMS + [(1, 3), (15, 6)])
def test_unpack_is_the_adjoint_of_pack(dim, pd):
    w = _random_weights(dim, pd, 1)
    packed = next_model3d.pack_weights(w, dim, pd).astype(np.float64)
    g = np.random.RandomState(2).standard_normal(packed.shape[0])
    ug = next_train3d.unpack_weight_grads(g, dim, pd)
    lhs = sum(float((ug[k] * w[k].astype(np.float64)).sum()) for k in w)
    rhs = float((g * packed).sum())
    assert abs(lhs - rhs) <= 1e-9 * abs(rhs) + 1e-9, (lhs, rhs)
    assert set(ug) == set(next_train3d.param_shapes(dim, pd)) and all(ug[k].shape == w[k].shape for k in w)
    # the one packed LSTM bias feeds both
    assert np.array_equal(ug['lstm.bias_ih'], ug['lstm.bias_hh'])


@pytest.mark.parametrize('dim,pd', FAMS)
def test_unpack_of_the_packed_index_is_the_identity_and_padding_is_dropped(dim, pd):
    index = next_train3d._pack_index(dim, pd)
    n = next_model3d.pack_weights({k: np.zeros(s, np.float32) for k, s in next_train3d.param_shapes(dim, pd).items()}, dim, pd).shape[0]
    pos = np.arange(n, dtype=np.float64)
    un = next_train3d.unpack_weight_grads(pos, dim, pd)
    for k, idx in index.items():
        assert np.array_equal(un[k], idx.astype(np.float64)), k
    used = np.zeros(n, dtype=np.int64)
    for k, idx in index.items():
        used[idx.reshape(-1)] += 1
    # every position is hit once, the LSTM bias twice, the padding lanes never
    assert set(np.unique(used)) <= {0, 1, 2} and int((used == 2).sum()) == 256
    padding = 16 * (12 - (pd + 3)) + 3 + 64 * (16 - dim) + (16 - (dim + 1)) * 65 + 27 * 7 * 64
    assert int((used == 0).sum()) == padding
    # a gradient that lives only on padding lanes unpacks to zeros
    g = (used == 0).astype(np.float64)
    assert all(not v.any() for v in next_train3d.unpack_weight_grads(g, dim, pd).values())
    # torch in, torch out, same numbers
    tu = next_train3d.unpack_weight_grads(torch.from_numpy(pos), dim, pd)
    assert all(np.array_equal(tu[k].numpy(), un[k]) for k in un)


@pytest.mark.parametrize('dim,pd', FAMS)
def test_device_pack_on_cpu_tensors_is_bit_equal_to_pack_weights(dim, pd):
    w = {k: v for k, v in host.load_weights(dim).items() if not k.startswith('attention_s.')}
    params = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()}
    assert np.array_equal(next_train3d.device_pack(params, dim, pd).numpy(), next_model3d.pack_weights(w, dim, pd))
    assert np.array_equal(next_train3d.device_pack_t(params, dim, pd).numpy(), next_train3d.pack_weights_t(w))
    r = _random_weights(dim, pd, 5)
    params = {k: torch.from_numpy(v) for k, v in r.items()}
    assert np.array_equal(next_train3d.device_pack(params, dim, pd).numpy(), next_model3d.pack_weights(r, dim, pd))
    assert np.array_equal(next_train3d.device_pack_t(params, dim, pd).numpy(), next_train3d.pack_weights_t(r))


def _unpack_conv(packed):
    """The [27 * 64, 64] matrix of a packed 64 -> 64 convolution back as a conv3d weight [cout, cin, 3, 3, 3]."""
    K, N = 27 * 64, 64
    m = packed.reshape(K // 16, N // 16, 4, 16, 4).transpose(0, 2, 4, 1, 3).reshape(K, N)
    return np.ascontiguousarray(m.reshape(27, 64, 64).transpose(2, 1, 0).reshape(64, 64, 3, 3, 3))


def test_the_forward_convolution_over_the_transposed_packing_is_the_input_gradient():
    """_conv27_host (the forward's 27 shifted matmuls) with the weights read back out of pack_weights_t equals torch's gradient
    of conv3d with respect to its input, on data with no axis symmetry (a missed flip on any axis shows)."""
    rng = np.random.RandomState(7)
    w = _random_weights(7, 3, 9)
    packed_t = next_train3d.pack_weights_t(w)
    amap = np.zeros((15, 15, 15))
    amap[1:4, 2:9, 5:7] = 1
    amap[10:14, 0:2, 3:12] = 1
    amap[6, 11, 13] = 1
    for slot, name in enumerate(('conv', 'h0', 'c0')):
        wt = _unpack_conv(packed_t[slot * 108 * 1024:(slot + 1) * 108 * 1024]).astype(np.float64)
        x = torch.from_numpy(rng.standard_normal((1, 64, 15, 15, 15))).requires_grad_(True)
        dout = rng.standard_normal((1, 64, 15, 15, 15)) * (0.25 + amap)[None, None]
        out = F.conv3d(x, torch.from_numpy(w[name + '.weight'].astype(np.float64)), None, padding=1)
        want = torch.autograd.grad(out, x, torch.from_numpy(dout))[0].numpy()
        got = next_model3d._conv27_host(np.ascontiguousarray(dout.transpose(0, 2, 3, 4, 1)), wt, np.zeros(64))
        assert np.abs(got.transpose(0, 4, 1, 2, 3) - want).max() <= 1e-10 * np.abs(want).max(), name
    lstm = packed_t[3 * 108 * 1024:3 * 108 * 1024 + 128 * 256].reshape(16, 8, 4, 16, 4).transpose(0, 2, 4, 1, 3).reshape(256, 128)
    assert np.array_equal(lstm, np.concatenate([w['lstm.weight_ih'], w['lstm.weight_hh']], axis=1))
    assert not packed_t[-64:].any()
