"""The 3-D NEXT network kernels (csrc/next3d_kernels.hip through gnnmp.next_model3d.NextNet3D / Model3D) on the device against
recorded runs of the unmodified reference module (next_model/model3D.py, tools/gen_golden_next3d.py) and, for shapes the fixtures
lack, against the float64 host restatement.

The bar is the project's own, tests/parity_bar.py: |gpu - ref64| <= max(1e-5, 1.25 x the reference's own fp32-vs-fp64 error), the
own error taken from the fixture itself.  Against the host restatement the family's recorded own error stands in -- pb_rep at the
SAME number of rounds (the batches no fixture holds run at iters = 2 to keep the CPU side short; after two rounds h is far from
saturated and the reference's own fp32 run is further from its fp64 run than after twenty), y of the recorded states.  The two
shapes without a recorded checkpoint, (dim, point_dim) = (6, 3) and (13, 3), run on seeded random weights; their own error is the
host restatement's, float32 against float64."""
import os

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_model3d as nm
from parity_bar import assert_fp32_parity, atol_for

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda:0'
FAMILIES = {7: ('next_7', 3), 14: ('next_14', 6)}


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _pb(dim, b, iters, prec):
    return _load('next3d_kuka%d_pb%d_i%d_f%d.npz' % (dim, b, iters, prec))['pb_rep']


class Family:
    def __init__(self, dim):
        stem, self.pd = FAMILIES[dim]
        self.dim = dim
        self.w = nm.load_npz_weights(*[os.path.join(GOLDEN, stem + s) for s in ('_weights.npz', '_weights_b.npz')])
        self.fx = _load('next3d_kuka%d_net.npz' % dim)
        self.maps = self.fx['maps'].astype(np.float32)               # two recorded problems, the axis-asymmetric map
        self.goals = self.fx['goals']
        self.net = nm.NextNet3D(dim, self.pd).load_state_dict(self.w)
        self.own_pb2 = float(np.abs(_pb(dim, 0, 2, 32).astype(np.float64) - _pb(dim, 0, 2, 64)).max())
        self.own_y = float(np.abs(self.fx['y32'].astype(np.float64) - self.fx['y64']).max())
        # four problems no fixture holds as a batch: a recorded map, all free, all blocked, the axis-asymmetric map (whose goal
        # point sits on a cube corner), at iters = 2
        free = np.zeros_like(self.maps[0])
        self.maps4 = np.stack([self.maps[0], free, free + 1, self.maps[2]])
        self.goals4 = self.goals[[0, 1, 1, 2]]
        assert np.all(np.abs(self.goals4[3, :self.pd]) == 1)
        self.pb4_64 = nm.pb_forward_host(self.w, self.maps4, self.goals4, iters=2)
        rng = np.random.RandomState(70 + dim)
        self.states17 = self.fx['states'][rng.randint(0, 24, 17)] + rng.uniform(-0.05, 0.05, (17, self.pd + dim)).astype(np.float32)
        self.of17 = rng.randint(0, 4, 17).astype(np.int32)          # unsorted, repeats
        self.y17_64 = nm.state_forward_host(self.w, self.states17, self.of17, self.pb4_64)
        self._pb20 = None

    def pb20_dev(self):
        """pb_rep of the two recorded problems at iters = 20 on the device, computed once."""
        if self._pb20 is None:
            self._pb20 = self.net.pb_forward(_t(self.maps[:2]), _t(self.goals[:2]))
        return self._pb20


_FAMILIES = {}


@pytest.fixture(params=[7, 14])
def fam(request):
    if request.param not in _FAMILIES:
        _FAMILIES[request.param] = Family(request.param)
    return _FAMILIES[request.param]


def _within(gpu, ref64, own, what):
    err = float(np.abs(gpu.detach().cpu().numpy().astype(np.float64) - ref64).max()) if ref64.size else 0.0
    print('%s: max|gpu - host64| %.3e (bar %.3e, own %.3e)' % (what, err, atol_for(own), own))
    assert err <= atol_for(own), '%s: %.3e over the bar %.3e' % (what, err, atol_for(own))


@pytest.mark.parametrize('iters', [0, 1, 2, 20])
def test_pb_rep_against_the_recorded_runs(fam, iters):
    r32, r64 = _pb(fam.dim, 0, iters, 32), _pb(fam.dim, 0, iters, 64)
    pb = fam.net.pb_forward(_t(fam.maps[:1]), _t(fam.goals[:1]), iters=iters)
    assert pb.shape == (1, 64, 15, 15, 15) and pb.dtype == torch.float32
    c = assert_fp32_parity(pb[0].cpu(), torch.from_numpy(r32), torch.from_numpy(r64), 'kuka%d pb_rep iters %d' % (fam.dim, iters))
    print('kuka%d pb_rep iters %d: err64 %.3e err32 %.3e own %.3e bar %.3e' % (fam.dim, iters, c['err64'], c['err32'], c['own'], c['atol']))


@pytest.mark.parametrize('through', ['recorded', 'device'])
def test_y_against_the_recorded_runs(fam, through):
    fx = fam.fx
    pb = _t(np.stack([_pb(fam.dim, b, 20, 32) for b in (0, 1)])) if through == 'recorded' else fam.pb20_dev()
    y = fam.net.state_forward(_t(fx['states']), _t(fx['problem_of_state'], torch.int32), pb)
    fam.net.check_status()
    assert y.shape == (len(fx['states']), fam.dim + 1)
    c = assert_fp32_parity(y.cpu(), torch.from_numpy(fx['y32']), torch.from_numpy(fx['y64']), 'kuka%d y through %s pb_rep' % (fam.dim, through))
    print('kuka%d y through the %s pb_rep: err64 %.3e err32 %.3e own %.3e bar %.3e' % (fam.dim, through, c['err64'], c['err32'], c['own'], c['atol']))
    if through == 'recorded':                                       # against the double read-out of the SAME fp32 pb_rep
        print('kuka%d y vs fp64 read-out of the recorded fp32 pb_rep: %.3e' % (fam.dim, np.abs(y.cpu().numpy() - fx['y64_of32']).max()))


@pytest.mark.parametrize('pick', [(0,), (0, 1, 2), (3, 2, 1)])
def test_pb_rep_of_other_batches_against_the_host_restatement(fam, pick):
    idx = list(pick)
    pb = fam.net.pb_forward(_t(fam.maps4[idx]), _t(fam.goals4[idx]), iters=2)
    assert pb.shape == (len(idx), 64, 15, 15, 15)
    _within(pb, fam.pb4_64[idx], fam.own_pb2, 'kuka%d pb_rep iters 2, problems %s' % (fam.dim, idx))
    if len(idx) == 3:                                               # a problem's result does not depend on its batch
        for slot, problem in enumerate(idx):
            alone = fam.net.pb_forward(_t(fam.maps4[problem:problem + 1]), _t(fam.goals4[problem:problem + 1]), iters=2)
            assert torch.equal(alone[0], pb[slot]), 'problem %d alone and in slot %d' % (problem, slot)


@pytest.mark.parametrize('dim,pd', [(6, 3), (13, 3)])
def test_the_ur5_and_kuka13_shapes_on_random_weights(dim, pd):
    gen = torch.Generator().manual_seed(1000 + dim)
    shapes = {'attention_g.mlp_share.0': (16, pd + 3, 1, 1, 1), 'attention_g.mlp_share.2': (16, 16, 1, 1, 1),
              'attention_g.mlp_share.4': (32, 16, 1, 1, 1), 'attention_g.mlp_share.6': (32, 32, 1, 1, 1),
              'attention_g.mlp_share.8': (64, 32, 1, 1, 1), 'attention_g.mlp_share.10': (1, 64, 1, 1, 1),
              'attention_g.mlp.0': (64, dim), 'attention_g.mlp.2': (8, 64), 'policy.0': (128, 8), 'policy.2': (64, 128),
              'policy.4': (dim + 1, 64), 'hidden': (64, 9, 3, 3, 3), 'h0': (64, 64, 3, 3, 3), 'c0': (64, 64, 3, 3, 3),
              'conv': (64, 64, 3, 3, 3)}
    w = {}
    for name, shape in shapes.items():                              # torch's default initialisation: uniform in +- 1 / sqrt(fan in)
        bound = 1.0 / np.sqrt(np.prod(shape[1:]))
        w[name + '.weight'] = ((torch.rand(shape, generator=gen) * 2 - 1) * bound).numpy()
        w[name + '.bias'] = ((torch.rand(shape[0], generator=gen) * 2 - 1) * bound).numpy()
    for name, shape in (('weight_ih', (256, 64)), ('weight_hh', (256, 64)), ('bias_ih', (256,)), ('bias_hh', (256,))):
        w['lstm.' + name] = ((torch.rand(shape, generator=gen) * 2 - 1) / 8).numpy()
    for k in [k for k in w if k.startswith('attention_g.')]:
        w['attention_s.' + k[len('attention_g.'):]] = w[k]
    rng = np.random.RandomState(dim)
    maps = (rng.uniform(size=(2, 15, 15, 15)) < 0.15).astype(np.float32)
    goals = rng.uniform(-1, 1, (2, pd + dim)).astype(np.float32)
    states = rng.uniform(-1, 1, (5, pd + dim)).astype(np.float32)
    of = np.array([1, 0, 0, 1, 1], dtype=np.int32)
    pb64 = nm.pb_forward_host(w, maps, goals, iters=2)
    pb32 = nm.pb_forward_host(w, maps, goals, iters=2, dtype=np.float32)
    y64 = nm.state_forward_host(w, states, of, pb64)
    y32 = nm.state_forward_host(w, states, of, pb32, dtype=np.float32)
    net = nm.NextNet3D(dim, pd).load_state_dict(w)
    pb = net.pb_forward(_t(maps), _t(goals), iters=2)
    y = net.state_forward(_t(states), _t(of, torch.int32), pb)
    net.check_status()
    assert y.shape == (5, dim + 1)
    _within(pb, pb64, float(np.abs(pb32 - pb64).max()), 'random (%d, %d) pb_rep iters 2' % (dim, pd))
    _within(y, y64, float(np.abs(y32 - y64).max()), 'random (%d, %d) y' % (dim, pd))


@pytest.mark.parametrize('S', [1, 5, 17])
def test_y_of_other_state_counts_against_the_host_restatement(fam, S):
    y = fam.net.state_forward(_t(fam.states17[:S]), _t(fam.of17[:S], torch.int32), _t(fam.pb4_64))
    fam.net.check_status()
    assert y.shape == (S, fam.dim + 1)
    _within(y, fam.y17_64[:S], fam.own_y, 'kuka%d y S=%d' % (fam.dim, S))


def test_empty_batches(fam):
    row = fam.pd + fam.dim
    pb = fam.net.pb_forward(torch.empty(0, 15, 15, 15, device=DEV), torch.empty(0, row, device=DEV))
    assert pb.shape == (0, 64, 15, 15, 15)
    y = fam.net.state_forward(torch.empty(0, row, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV), fam.pb20_dev())
    assert y.shape == (0, fam.dim + 1)
    fam.net.check_status()


def test_problem_index_out_of_range_is_reported_and_leaves_the_other_rows(fam):
    of = fam.of17[:11].copy() % 2
    good = fam.net.state_forward(_t(fam.states17[:11]), _t(of, torch.int32), fam.pb20_dev())
    fam.net.check_status()
    of[3], of[8] = 2, -1
    y = fam.net.state_forward(_t(fam.states17[:11]), _t(of, torch.int32), fam.pb20_dev())
    with pytest.raises(RuntimeError, match='outside'):
        fam.net.check_status()
    fam.net.check_status()                                          # reported once
    keep = np.array([i for i in range(11) if i not in (3, 8)])
    assert torch.equal(y[keep], good[keep])
    assert torch.isnan(y[[3, 8]]).all()


def test_two_runs_are_bit_identical(fam):
    a = fam.net.pb_forward(_t(fam.maps[:2]), _t(fam.goals[:2]))
    assert torch.equal(a, fam.pb20_dev())
    fx = fam.fx
    ya = fam.net.state_forward(_t(fx['states']), _t(fx['problem_of_state'], torch.int32), a)
    yb = fam.net.state_forward(_t(fx['states']), _t(fx['problem_of_state'], torch.int32), a)
    assert torch.equal(ya, yb)
    fam.net.check_status()


def test_the_cached_pb_forward_workspace_carries_nothing_over(fam):
    """The workspace (h, c and the hidden layer) grows for B = 3 and is then reused by smaller calls with other round counts."""
    net = nm.NextNet3D(fam.dim, fam.pd).load_state_dict(fam.w)
    net.pb_forward(_t(fam.maps4[[3, 2, 1]]), _t(fam.goals4[[3, 2, 1]]), iters=2)
    ws = net._ws[str(torch.device(DEV))]
    net.pb_forward(_t(fam.maps4[:1]), _t(fam.goals4[:1]), iters=1)
    used = net.pb_forward(_t(fam.maps4[:1]), _t(fam.goals4[:1]), iters=2)
    assert net._ws[str(torch.device(DEV))] is ws and ws.numel() >= nm.workspace_bytes(3) > nm.workspace_bytes(1)      # the same buffer
    fresh = nm.NextNet3D(fam.dim, fam.pd).load_state_dict(fam.w).pb_forward(_t(fam.maps4[:1]), _t(fam.goals4[:1]), iters=2)
    assert torch.equal(used, fresh)
    _within(used, fam.pb4_64[:1], fam.own_pb2, 'kuka%d pb_rep iters 2 through a used workspace' % fam.dim)


class StubEnv:
    """get_robot_points as a fixed numpy function of the state (the real one is PyBullet's forward kinematics)."""
    RRT_EPS = 0.5

    def __init__(self, pd):
        self.pd = pd

    def get_robot_points(self, state):
        s = np.asarray(state, dtype=np.float64)
        return np.array([np.sin(s[q % s.shape[0]] + 0.3 * q) * 0.9 for q in range(self.pd)])


def test_model3d_agrees_with_nextnet3d_and_draws_as_torch_does(fam):
    from torch.distributions.multivariate_normal import MultivariateNormal
    dim, pd = fam.dim, fam.pd
    env = StubEnv(pd)
    goal = fam.goals[0, pd:].astype(np.float64)
    problem = dict(map=fam.maps[0].astype(np.float64), goal_state=goal, init_state=fam.fx['states'][0, pd:].astype(np.float64))
    model = nm.Model3D(env, dim, point_dim=pd, device=DEV).load_state_dict(fam.w)
    assert model.std == 0.5 * 0.3 and torch.equal(model.var, torch.eye(dim) * (0.5 * 0.3) ** 2)      # the reference's default
    model.iters = 2
    model.set_problem(problem)
    goal_row = np.concatenate([env.get_robot_points(goal), goal]).astype(np.float32)
    pb = fam.net.pb_forward(_t(fam.maps[:1]), _t(goal_row[None]), iters=2)
    assert torch.equal(model.pb_rep, pb)
    states = fam.fx['states'][:10, pd:].astype(np.float64)
    rows = np.array([np.concatenate((env.get_robot_points(s), s)) for s in states])
    y_dev = fam.net.state_forward(torch.FloatTensor(rows).to(DEV), torch.zeros(10, dtype=torch.int32, device=DEV), pb)
    y = y_dev.cpu().numpy()
    v10 = model.pred_value(states)
    assert v10.shape == (10,) and np.array_equal(v10, y[:, -1])
    v1 = model.pred_value(states[4])
    assert np.ndim(v1) == 0 and v1 == y[4, -1]
    mean, value = model.net_forward(states[4])
    assert mean.shape == (dim,) and np.array_equal(mean, y[4, :dim]) and np.ndim(value) == 0
    mean10, value10 = model.net_forward(states)
    assert mean10.shape == (10, dim) and value10.shape == (10,)
    a_t, v_t = model.net_forward(states, use_np=False)              # tensors, never squeezed
    assert torch.equal(a_t, y_dev[:, :dim]) and torch.equal(v_t, y_dev[:, -1])
    a_1, v_1 = model.net_forward(states[4], use_np=False)
    assert a_1.shape == (1, dim) and v_1.shape == (1,)
    torch.manual_seed(7)
    actions, priors = model.policy(states[4], 10)
    torch.manual_seed(7)
    m = MultivariateNormal(torch.FloatTensor(y[4, :dim]), torch.eye(dim) * (0.5 * 0.3) ** 2)
    assert len(actions) == len(priors) == 10
    for a, pr in zip(actions, priors):
        want = m.sample()
        assert a.shape == (dim,) and np.array_equal(a, want.numpy())
        assert pr == torch.exp(m.log_prob(want)).item()
    assert nm.Model3D(env, dim, point_dim=pd, std=0.2, device=DEV).std == 0.2
    model.check_status()
