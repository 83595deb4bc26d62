"""The host side of NEXT's device tree loop (gnnmp_next_plan): the exported symbols and struct mirrors, every argument check
-- they come before any device work, so no GPU is needed and nothing is launched (the pointers handed over are not device
memory) -- ``NoiseModel``'s actions against ``MultivariateNormal.sample()`` bit for bit, and ``plan_host``'s ``min_margin`` on
the recorded reference runs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import _lib, next_plan
from test_next_plan_host import CASES, EXACT, load, replay

ERR_NULL, ERR_DIMS, ERR_ARG = -1, -2, -6
FAKE = 4096
BATCH_PTRS = ('maps', 'init_states', 'goal_states', 'draws', 'pb_rep', 'weights', 'eps')
TREE_PTRS = [f[0] for f in _lib.NextPlanTree._fields_]


def _batch(n_problems=2, dim=2, width=15, t_max=60, stop=1, draws_per_problem=None, g_explore_eps=0.1, c=1.0, k=10, eps_rows=60,
           scale=0.015, **null):
    ptr = {name: None if null.get(name) else FAKE for name in BATCH_PTRS}
    return _lib.NextPlanBatch(n_problems, dim, width, t_max, stop, t_max * (2 + dim) if draws_per_problem is None else draws_per_problem,
                              ptr['maps'], ptr['init_states'], ptr['goal_states'], ptr['draws'], g_explore_eps, c, k, eps_rows, scale,
                              ptr['pb_rep'], ptr['weights'], ptr['eps'])


def _tree(**null):
    return _lib.NextPlanTree(*[None if null.get(name) else FAKE for name in TREE_PTRS])


def _call(b, t):
    return _lib.lib().gnnmp_next_plan(ctypes.byref(b) if b is not None else None, ctypes.byref(t) if t is not None else None, None)


def _struct_fields(text, name):
    body = re.search(r'typedef struct\s*\{([^}]*)\}\s*%s;' % name, text).group(1)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            fields.extend(x.split()[-1].lstrip('*') for x in decl.split(','))
    return fields


def test_symbols_abi_version_and_structs_mirror_the_header():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gnnmp_next_plan', 'gnnmp_next_plan_max_nodes'):
        assert hasattr(L, name), name
    assert _lib.lib().gnnmp_abi_version() == _lib.ABI_VERSION == 9
    assert next_plan.max_nodes() == 1024
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gnnmp.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert [f[0] for f in _lib.NextPlanBatch._fields_] == _struct_fields(text, 'gnnmp_next_plan_batch')
    assert [f[0] for f in _lib.NextPlanTree._fields_] == _struct_fields(text, 'gnnmp_next_plan_tree')
    # the RRT* fields lead both structs, in RRT*'s order
    n_b, n_t = len(_lib.RRTStarBatch._fields_), len(_lib.RRTStarTree._fields_)
    assert _lib.NextPlanBatch._fields_[:n_b] == _lib.RRTStarBatch._fields_
    assert _lib.NextPlanTree._fields_[:n_t] == _lib.RRTStarTree._fields_
    assert _struct_fields(text, 'gnnmp_next_plan_tree')[:n_t] == _struct_fields(text, 'gnnmp_rrtstar_tree')


def test_argument_checks_come_before_any_launch():
    assert _call(None, _tree()) == ERR_NULL and _call(_batch(), None) == ERR_NULL
    for dim in (2, 3):
        for name in BATCH_PTRS:
            assert _call(_batch(dim=dim, **{name: True}), _tree()) == ERR_NULL, name
        for name in TREE_PTRS:
            assert _call(_batch(dim=dim), _tree(**{name: True})) == ERR_NULL, name
    for dim in (0, 1, 4, -2):
        assert _call(_batch(dim=dim), _tree()) == ERR_DIMS, dim
    for width in (0, 14, 16, -15):
        assert _call(_batch(width=width), _tree()) == ERR_DIMS, width
    cap = next_plan.max_nodes()
    for t_max in (0, -1, cap, cap + 1, 2 ** 31 - 1):                 # t_max + 1 above the node cap
        assert _call(_batch(t_max=t_max, draws_per_problem=100), _tree()) == ERR_ARG, t_max
    assert _call(_batch(n_problems=0), _tree()) == ERR_ARG
    for k in (0, -1, 17, 1000):
        assert _call(_batch(k=k), _tree()) == ERR_ARG, k
    for rows in (0, -3):
        assert _call(_batch(eps_rows=rows), _tree()) == ERR_ARG, rows
    for dim in (2, 3):
        for n in (0, 1 + dim, -1, 2 ** 31):
            assert _call(_batch(dim=dim, draws_per_problem=n), _tree()) == ERR_ARG, (dim, n)


def test_python_wrapper_refuses_what_the_loop_cannot_take():
    pr = dict(map=np.zeros((15, 15)), init_state=np.zeros(2), goal_state=np.ones(2) * 0.5)
    with pytest.raises(ValueError):
        next_plan.plan_maze_batch([pr], 'cpu', [1, 2], None)
    with pytest.raises(ValueError):
        next_plan.plan_maze_batch([pr], 'cpu', [1], None, t_max=next_plan.max_nodes())
    with pytest.raises(TypeError):
        next_plan.plan_maze_batch([pr], 'cpu', [1], object(), t_max=10)
    assert next_plan.plan_maze_batch([], 'cpu', [], None) == []


class _StubModel:
    """A model whose network returns a fixed action mean."""

    def __init__(self, mean, std):
        self.mean = np.asarray(mean, dtype=np.float32)
        self.std = std
        self.var = torch.eye(len(self.mean)) * std ** 2

    def net_forward(self, states):
        return self.mean, np.float32(0.25)

    def pred_value(self, states):
        return np.float32(0.25)


@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('std', [0.05 * 0.3, 0.1])
def test_noise_model_actions_equal_multivariate_normal_samples(dim, std):
    from torch.distributions.multivariate_normal import MultivariateNormal
    rows, k = 7, 10
    means = np.random.RandomState(5).uniform(-1, 1, (rows, dim)).astype(np.float32)
    torch.manual_seed(1234)
    eps = torch.stack([torch.stack([torch.randn(dim) for _ in range(k)]) for _ in range(rows)])
    torch.manual_seed(1234)
    var = torch.eye(dim) * std ** 2
    want = [[MultivariateNormal(torch.FloatTensor(means[g]), var).sample().numpy() for _ in range(k)] for g in range(rows)]
    stub = _StubModel(means[0], std)
    model = next_plan.NoiseModel(stub, eps)
    assert model.scale == next_plan.policy_scale(std, dim) and model.scale.dtype == np.float32
    if std == 0.05 * 0.3:
        assert model.scale == np.float32(0.015) == next_plan.policy_scale(None, dim)
    for g in range(rows):
        stub.mean = means[g]
        actions, priors = model.policy(state=np.zeros(dim), k=k)
        assert len(actions) == len(priors) == k
        for j in range(k):
            assert actions[j].dtype == np.float32 and actions[j].shape == (dim,)
            assert np.array_equal(actions[j].view(np.uint32), want[g][j].view(np.uint32)), (g, j)
    assert model.pred_value(np.zeros(dim)) == np.float32(0.25)
    with pytest.raises(IndexError):
        model.policy(state=np.zeros(dim), k=k)                       # the block is used up: nothing is invented


@pytest.mark.parametrize('name', CASES)
def test_plan_host_still_reproduces_the_recorded_run_and_reports_its_margin(name):
    rec = load(name)
    out, model = replay(rec)
    assert model.exhausted()
    for key in EXACT:
        got, want = np.asarray(out[key]), rec[key]
        assert got.shape == want.shape and np.array_equal(got, want.astype(got.dtype)), key
    assert out['w_sum'] == float(rec['w_sum'])
    margin = out['stats']['min_margin']
    assert isinstance(margin, float) and np.isfinite(margin) and margin >= 0.0
    print('%s: min_margin %.3e over %d guided iterations' % (name, margin, out['stats']['guided']))


def test_argmax_margin():
    assert next_plan.argmax_margin([1.0]) == float('inf') and next_plan.argmax_margin([]) == float('inf')
    assert next_plan.argmax_margin([1.0, 3.0, 2.5]) == 0.5
    assert next_plan.argmax_margin([2.0, 2.0, 1.0]) == 0.0
