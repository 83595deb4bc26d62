"""The float64 numpy restatement of the NEXT network (gnnmp.next_model.pb_forward_host / state_forward_host) against recorded
float64 runs of the unmodified reference module (tools/gen_golden_next.py).  Float64 on both sides in another summation order:
values are O(1), K <= 576, 20 rounds, so rounding is about 1e-12; the bar is 1e-9 absolute, at every ``iters``."""
import os

import numpy as np
import pytest

import gnnmp  # noqa: F401
from gnnmp import next_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BAR = 1e-9


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope='module', params=[2, 3])
def family(request):
    dim = request.param
    return dim, _load('next_%d_weights.npz' % dim), _load('next_net_maze%d.npz' % dim), _load('next_net_maze%d_iters.npz' % dim)


def test_pb_forward_host_at_20_rounds(family):
    dim, w, net, _ = family
    pb = next_model.pb_forward_host(w, net['maps'], net['goals'], iters=int(net['iters']))
    assert pb.shape == (2, 64, 15, 15) and pb.dtype == np.float64
    err = np.abs(pb - net['pb_rep64']).max()
    print('maze%d pb_rep host-vs-recorded fp64: %.3e' % (dim, err))
    assert err <= BAR


@pytest.mark.parametrize('iters', [0, 1, 2])
def test_pb_forward_host_at_few_rounds(family, iters):
    dim, w, _, it = family
    pb = next_model.pb_forward_host(w, it['maps'], it['goals'], iters=iters)
    err = np.abs(pb - it['pb_rep64_i%d' % iters]).max()
    print('maze%d iters %d: %.3e' % (dim, iters, err))
    assert err <= BAR


def test_state_forward_host(family):
    dim, w, net, _ = family
    y = next_model.state_forward_host(w, net['states'], net['problem_of_state'], net['pb_rep64'])
    assert y.shape == (net['states'].shape[0], dim + 1)
    assert np.abs(y - net['y64']).max() <= BAR
    y = next_model.state_forward_host(w, net['states'], net['problem_of_state'], net['pb_rep32'])
    assert np.abs(y - net['y64_of32']).max() <= BAR


def test_fixture_states_cover_the_named_cases(family):
    dim, _, net, _ = family
    s, of = net['states'].astype(np.float64), net['problem_of_state']
    assert len(s) >= 40 and set(of.tolist()) == {0, 1}
    assert (np.diff(of) != 0).sum() >= 10                                  # interleaved, not two sorted runs
    for sx in (-1, 1):
        for sy in (-1, 1):
            assert ((s[:, 0] == sx) & (s[:, 1] == sy)).any()
    if dim == 3:
        assert (s[:, 2] == np.float32(0.4)).any() and (s[:, 2] == np.float32(-0.4)).any()
    for b in range(2):
        assert ((s == net['goals'][b]).all(axis=1) & (of == b)).any() and ((s == net['inits'][b]).all(axis=1) & (of == b)).any()


def test_state_forward_host_rejects_a_problem_index_out_of_range(family):
    dim, w, net, _ = family
    with pytest.raises(ValueError):
        next_model.state_forward_host(w, net['states'][:2], [0, 2], net['pb_rep64'])


def test_pack_weights_checks_family_and_shared_attention(family):
    dim, w, _, _ = family
    packed = next_model.pack_weights(w, dim)
    assert packed.dtype == np.float32 and packed.ndim == 1
    with pytest.raises(ValueError):
        next_model.pack_weights(w, 5 - dim)
    bad = dict(w)
    bad['attention_s.mlp.2.bias'] = w['attention_s.mlp.2.bias'] + 1
    with pytest.raises(ValueError):
        next_model.pack_weights(bad, dim)
