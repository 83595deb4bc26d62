"""The float64 host restatement of the 3-D NEXT network (gnnmp.next_model3d.pb_forward_host / state_forward_host) against the
recorded float64 runs of the unmodified reference module (tools/gen_golden_next3d.py), and the weight packer's shape checks.

Tolerances: float64 against float64, the same mathematics in another summation order (27 shifted matmuls, the reference sums
inside its convolution).  Measured when the fixtures were recorded: pb_rep 2.0e-13 (iters 0), 1.4e-13 (1), 1.1e-13 (2), 8.5e-14
(20) at most over both families (|h0| reaches 258, which is where the first figure comes from); y 4.7e-14 through the restated
pb_rep and through the recorded fp32 one.  The bars are 100 x those, far below the 1e-9 ceiling."""
import os

import numpy as np
import pytest

import gnnmp  # noqa: F401
from gnnmp import next_model3d as nm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FAMILIES = {7: ('next_7', 3), 14: ('next_14', 6)}
PB_TOL, Y_TOL = 2e-11, 5e-12
assert PB_TOL <= 1e-9 and Y_TOL <= 1e-9


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}


def _weights(dim):
    stem = FAMILIES[dim][0]
    return nm.load_npz_weights(*[os.path.join(GOLDEN, stem + s) for s in ('_weights.npz', '_weights_b.npz')])


@pytest.mark.parametrize('dim,iters', [(7, 0), (7, 1), (7, 2), (7, 20), (14, 0), (14, 1), (14, 2)])
def test_pb_forward_host_against_the_recorded_fp64_runs(dim, iters):
    fx = _load('next3d_kuka%d_net.npz' % dim)
    want = _load('next3d_kuka%d_pb0_i%d_f64.npz' % (dim, iters))['pb_rep']
    pb = nm.pb_forward_host(_weights(dim), fx['maps'][:1], fx['goals'][:1], iters=iters)
    assert pb.shape == (1, 64, 15, 15, 15) and pb.dtype == np.float64
    err = float(np.abs(pb[0] - want).max())
    print('kuka%d pb_rep iters %d: max|host - recorded fp64| %.3e (bar %.1e)' % (dim, iters, err, PB_TOL))
    assert err <= PB_TOL


@pytest.mark.parametrize('dim', [7, 14])
def test_state_forward_host_against_the_recorded_fp64_read_out(dim):
    """Through the recorded fp32 pb_rep of both problems: isolates the read-out from pb_forward_host."""
    fx = _load('next3d_kuka%d_net.npz' % dim)
    pb32 = np.stack([_load('next3d_kuka%d_pb%d_i20_f32.npz' % (dim, b))['pb_rep'] for b in (0, 1)])
    y = nm.state_forward_host(_weights(dim), fx['states'], fx['problem_of_state'], pb32)
    assert y.shape == (24, dim + 1)
    err = float(np.abs(y - fx['y64_of32']).max())
    print('kuka%d y: max|host - recorded fp64 read-out| %.3e (bar %.1e)' % (dim, err, Y_TOL))
    assert err <= Y_TOL
    with pytest.raises(ValueError):
        nm.state_forward_host(_weights(dim), fx['states'], fx['problem_of_state'] + 1, pb32)


def test_the_map_axes_are_not_interchangeable():
    """The fixture's third map differs under every permutation of its axes, and so does the restated pb_rep: an index mix-up in
    the voxel order or in the coords channels cannot pass the recorded runs by symmetry."""
    fx = _load('next3d_kuka7_net.npz')
    m = fx['maps'][2]
    for perm in ((0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        assert not np.array_equal(m, m.transpose(perm))
    w = _weights(7)
    a = nm.pb_forward_host(w, m[None], fx['goals'][2:3], iters=0)
    b = nm.pb_forward_host(w, m.transpose(1, 0, 2)[None], fx['goals'][2:3], iters=0)
    assert np.abs(a - b.transpose(0, 1, 3, 2, 4)).max() > 1e-3


@pytest.mark.parametrize('dim', [7, 14])
def test_pack_weights_shapes_and_weights_floats(dim):
    pd = FAMILIES[dim][1]
    w = _weights(dim)
    assert w['attention_g.mlp_share.0.weight'].shape == (16, pd + 3, 1, 1, 1)
    assert w['attention_g.mlp.0.weight'].shape == (64, dim) and w['policy.4.weight'].shape == (dim + 1, 64)
    packed = nm.pack_weights(w, dim, pd)
    assert packed.dtype == np.float32 and packed.shape == (nm.weights_floats(dim, pd),)
    assert nm.weights_floats(6, 3) == nm.weights_floats(14, 6)          # one layout for every checkpoint shape
    for bad_dim, bad_pd in ((dim + 1, pd), (dim, 9 - pd), (0, pd), (16, pd), (dim, 2)):
        with pytest.raises(ValueError):
            nm.pack_weights(w, bad_dim, bad_pd)
    twisted = dict(w)
    twisted['attention_s.mlp.2.bias'] = w['attention_s.mlp.2.bias'] + 1
    with pytest.raises(ValueError, match='attention_s'):
        nm.pack_weights(twisted, dim, pd)


def test_pack_weights_refuses_a_2d_checkpoint():
    w2 = _load('next_3_weights.npz')
    with pytest.raises(ValueError, match='2-D'):
        nm.pack_weights(w2, 3, 3)
    with pytest.raises(ValueError):
        nm.NextNet3D(3, 2)
    with pytest.raises(ValueError):
        nm.NextNet3D(16, 3)


def test_the_packed_convolution_follows_the_tap_order():
    """Element (tap, channel, out) of the packed K x 64 matrix is weight[out, channel, di, dj, dk] with tap = (di 3 + dj) 3 + dk, in
    the B-operand order of next_model._mfma_pack."""
    rng = np.random.RandomState(3)
    weight = rng.standard_normal((64, 9, 3, 3, 3)).astype(np.float32)
    packed = nm._conv_pack(weight).reshape(27, 4, 4, 16, 4)           # [k group = tap][column tile][k quarter][column][step]
    for tap, ch, out in ((0, 0, 0), (5, 8, 17), (26, 3, 63), (13, 4, 32)):
        di, dj, dk = tap // 9, (tap // 3) % 3, tap % 3
        assert packed[tap, out // 16, ch // 4, out % 16, ch % 4] == weight[out, ch, di, dj, dk]
    assert not packed[:, :, 3:, :, :].any() and not packed[:, :, 2, :, 1:].any()      # channels 9 .. 15 are padding
