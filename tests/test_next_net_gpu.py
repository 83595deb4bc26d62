"""The NEXT network kernels (csrc/next_kernels.hip through gnnmp.next_model.NextNet / Model2D) on the device against recorded
runs of the unmodified reference module and, for shapes the fixtures lack, against the float64 host restatement.

The bar is the project's own, tests/parity_bar.py: |gpu - ref64| <= max(1e-5, 1.25 x the reference's own fp32-vs-fp64 error),
with the own error taken from the fixture itself; against the host restatement the family's recorded own error (pb_rep at 20
rounds, y of the recorded states) stands in, since no fp32 run of the reference exists for those shapes."""
import os

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_model
from parity_bar import assert_fp32_parity, atol_for

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda:0'


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


class Family:
    def __init__(self, dim):
        self.dim = dim
        self.w = _load('next_%d_weights.npz' % dim)
        self.net_fx = _load('next_net_maze%d.npz' % dim)
        self.it_fx = _load('next_net_maze%d_iters.npz' % dim)
        self.net = next_model.NextNet(dim).load_state_dict(self.w)
        self.own_pb = float(np.abs(self.net_fx['pb_rep32'].astype(np.float64) - self.net_fx['pb_rep64']).max())
        self.own_y = float(np.abs(self.net_fx['y32'].astype(np.float64) - self.net_fx['y64']).max())
        # five problems no fixture holds as a batch: the two recorded maps, an all-free and an all-blocked map, a transposed one
        rng = np.random.RandomState(40 + dim)
        m = self.net_fx['maps']
        self.maps5 = np.stack([m[0], np.zeros_like(m[0]), m[1], np.ones_like(m[0]), m[0].T]).astype(np.float32)
        lim = np.array([1., 1., 0.4])[:dim]
        self.goals5 = rng.uniform(-lim, lim, (5, dim)).astype(np.float32)
        self.pb5_64 = next_model.pb_forward_host(self.w, self.maps5, self.goals5, iters=20)
        self.states37 = rng.uniform(-lim, lim, (37, dim)).astype(np.float32)
        self.of37 = rng.randint(0, 5, 37).astype(np.int32)          # unsorted, repeats
        self.y37_64 = next_model.state_forward_host(self.w, self.states37, self.of37, self.pb5_64)
        self._pb5_dev = None

    def pb5_dev(self):
        if self._pb5_dev is None:
            self._pb5_dev = self.net.pb_forward(_t(self.maps5), _t(self.goals5))
        return self._pb5_dev


_FAMILIES = {}


@pytest.fixture(params=[2, 3])
def fam(request):
    if request.param not in _FAMILIES:
        _FAMILIES[request.param] = Family(request.param)
    return _FAMILIES[request.param]


def _within(gpu, ref64, own, what):
    err = float(np.abs(gpu.detach().cpu().numpy().astype(np.float64) - ref64).max()) if ref64.size else 0.0
    print('%s: max|gpu - host64| %.3e (bar %.3e, family own %.3e)' % (what, err, atol_for(own), own))
    assert err <= atol_for(own), '%s: %.3e over the bar %.3e' % (what, err, atol_for(own))


@pytest.mark.parametrize('iters', [0, 1, 2, 20])
def test_pb_rep_against_the_recorded_runs(fam, iters):
    if iters == 20:
        fx, r32, r64 = fam.net_fx, fam.net_fx['pb_rep32'], fam.net_fx['pb_rep64']
    else:
        fx, r32, r64 = fam.it_fx, fam.it_fx['pb_rep32_i%d' % iters], fam.it_fx['pb_rep64_i%d' % iters]
    pb = fam.net.pb_forward(_t(fx['maps']), _t(fx['goals']), iters=iters)
    assert pb.shape == (len(fx['maps']), 64, 15, 15) and pb.dtype == torch.float32
    c = assert_fp32_parity(pb.cpu(), torch.from_numpy(r32), torch.from_numpy(r64), 'maze%d pb_rep iters %d' % (fam.dim, iters))
    print('maze%d pb_rep iters %d: err64 %.3e err32 %.3e own %.3e bar %.3e' % (fam.dim, iters, c['err64'], c['err32'], c['own'], c['atol']))


@pytest.mark.parametrize('through', ['recorded', 'device'])
def test_y_against_the_recorded_runs(fam, through):
    fx = fam.net_fx
    pb = _t(fx['pb_rep32']) if through == 'recorded' else fam.net.pb_forward(_t(fx['maps']), _t(fx['goals']))
    y = fam.net.state_forward(_t(fx['states']), _t(fx['problem_of_state'], torch.int32), pb)
    fam.net.check_status()
    assert y.shape == (len(fx['states']), fam.dim + 1)
    c = assert_fp32_parity(y.cpu(), torch.from_numpy(fx['y32']), torch.from_numpy(fx['y64']), 'maze%d y through %s pb_rep' % (fam.dim, through))
    print('maze%d y through the %s pb_rep: err64 %.3e err32 %.3e own %.3e bar %.3e' % (fam.dim, through, c['err64'], c['err32'], c['own'], c['atol']))
    if through == 'recorded':                                       # against the double read-out of the SAME fp32 pb_rep
        print('maze%d y vs fp64 read-out of the recorded fp32 pb_rep: %.3e' % (fam.dim, np.abs(y.cpu().numpy() - fx['y64_of32']).max()))


@pytest.mark.parametrize('B', [1, 5])
def test_pb_rep_of_other_batches_against_the_host_restatement(fam, B):
    pb = fam.pb5_dev() if B == 5 else fam.net.pb_forward(_t(fam.maps5[:1]), _t(fam.goals5[:1]))
    assert pb.shape == (B, 64, 15, 15)
    _within(pb, fam.pb5_64[:B], fam.own_pb, 'maze%d pb_rep B=%d' % (fam.dim, B))
    if B == 1:                                                      # a problem's result does not depend on its batch
        assert torch.equal(pb[0], fam.pb5_dev()[0])


@pytest.mark.parametrize('S', [1, 11, 17, 37])
def test_y_of_other_state_counts_against_the_host_restatement(fam, S):
    y = fam.net.state_forward(_t(fam.states37[:S]), _t(fam.of37[:S], torch.int32), _t(fam.pb5_64))
    fam.net.check_status()
    assert y.shape == (S, fam.dim + 1)
    _within(y, fam.y37_64[:S], fam.own_y, 'maze%d y S=%d' % (fam.dim, S))


def test_empty_batches(fam):
    pb = fam.net.pb_forward(torch.empty(0, 15, 15, device=DEV), torch.empty(0, fam.dim, device=DEV))
    assert pb.shape == (0, 64, 15, 15)
    y = fam.net.state_forward(torch.empty(0, fam.dim, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV), fam.pb5_dev())
    assert y.shape == (0, fam.dim + 1)
    fam.net.check_status()


def test_problem_index_out_of_range_is_reported_and_leaves_the_other_rows(fam):
    of = fam.of37[:11].copy()
    good = fam.net.state_forward(_t(fam.states37[:11]), _t(of, torch.int32), fam.pb5_dev())
    fam.net.check_status()
    of[3], of[8] = 5, -1
    y = fam.net.state_forward(_t(fam.states37[:11]), _t(of, torch.int32), fam.pb5_dev())
    with pytest.raises(RuntimeError, match='outside'):
        fam.net.check_status()
    fam.net.check_status()                                          # reported once
    keep = np.array([i for i in range(11) if i not in (3, 8)])
    assert torch.equal(y[keep], good[keep])
    assert torch.isnan(y[[3, 8]]).all()


def test_two_runs_are_bit_identical(fam):
    fx = fam.net_fx
    a = fam.net.pb_forward(_t(fx['maps']), _t(fx['goals']))
    b = fam.net.pb_forward(_t(fx['maps']), _t(fx['goals']))
    assert torch.equal(a, b)
    ya = fam.net.state_forward(_t(fx['states']), _t(fx['problem_of_state'], torch.int32), a)
    yb = fam.net.state_forward(_t(fx['states']), _t(fx['problem_of_state'], torch.int32), b)
    assert torch.equal(ya, yb)
    fam.net.check_status()


def test_model2d_agrees_with_nextnet_and_draws_as_torch_does(fam):
    from torch.distributions.multivariate_normal import MultivariateNormal
    fx, dim = fam.net_fx, fam.dim
    problem = dict(map=fx['maps'][0].astype(np.float64), goal_state=fx['goals'][0].astype(np.float64),
                   init_state=fx['inits'][0].astype(np.float64))
    model = next_model.Model2D(None, dim=dim, device=DEV).load_state_dict(fam.w)
    model.set_problem(problem)
    pb = fam.net.pb_forward(_t(fx['maps'][:1]), _t(fx['goals'][:1]))
    assert torch.equal(model.pb_rep, pb)
    states = fx['states'][:10].astype(np.float64)
    y = fam.net.state_forward(_t(states), torch.zeros(10, dtype=torch.int32, device=DEV), pb).cpu().numpy()
    v10 = model.pred_value(states)
    assert v10.shape == (10,) and np.array_equal(v10, y[:, -1])
    v1 = model.pred_value(states[4])
    assert np.ndim(v1) == 0 and v1 == y[4, -1]
    mean, value = model.net_forward(states[4])
    assert mean.shape == (dim,) and np.array_equal(mean, y[4, :dim])
    torch.manual_seed(7)
    actions, priors = model.policy(states[4], 10)
    torch.manual_seed(7)
    m = MultivariateNormal(torch.FloatTensor(y[4, :dim]), torch.eye(dim) * (0.05 * 0.3) ** 2)
    assert len(actions) == len(priors) == 10
    for a, pr in zip(actions, priors):
        want = m.sample()
        assert a.shape == (dim,) and np.array_equal(a, want.numpy())
        assert pr == torch.exp(m.log_prob(want)).item()
    model.check_status()
