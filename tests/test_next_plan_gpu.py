"""The device ``Model2D`` behind NEXT's planner.

Teacher-forced: every state the recorded reference runs queried (tools/gen_golden_next.py) goes through the device model, which
must return the recorded answer within the project's fp32 bar, tests/parity_bar.py: the fixtures hold the reference's network
output for every queried state as the run saw it (fp32) and from the same module in .double(), so the bar is
|gpu - ref64| <= max(1e-5, 1.25 x own) with the own error of exactly these states.  Then ``plan_host`` runs on the device model
to the end and must yield a self-consistent tree.  No claim that its decisions equal the recorded ones: the network agrees to
1e-5, not bit for bit."""
import glob
import os

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_model, next_plan, rrtstar
from parity_bar import assert_fp32_parity

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'next_plan_maze*.npz')))
DEV = 'cuda:0'
_MODELS = {}


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}


def _model(dim):
    if dim not in _MODELS:
        _MODELS[dim] = next_model.Model2D(None, dim=dim, device=DEV).load_state_dict(_load('next_%d_weights.npz' % dim))
    return _MODELS[dim]


@pytest.mark.parametrize('name', CASES)
def test_recorded_queries_teacher_forced(name):
    rec = _load(name + '.npz')
    dim = int(rec['dim'])
    model = _model(dim)
    model.set_problem(dict(map=rec['map'], goal_state=rec['goal_state'], init_state=rec['init_state']))
    rows = np.concatenate([[0], np.cumsum(rec['q_n'])])
    # through the interface itself, query by query in the recorded order and shapes
    got = np.full(rec['y32'].shape, np.nan, dtype=np.float32)
    for q in range(len(rec['q_kind'])):
        st = rec['q_states'][rows[q]:rows[q + 1]]
        if rec['q_kind'][q] == 0:
            v = model.pred_value(st[0] if len(st) == 1 else st)
            assert np.shape(v) == (() if len(st) == 1 else (len(st),))
            got[rows[q]:rows[q + 1], -1] = v
        else:
            mean, value = model.net_forward(st[0])                  # what policy() samples around
            assert mean.shape == (dim,)
            got[rows[q], :dim], got[rows[q], -1] = mean, value
    model.check_status()
    is_value = np.repeat(rec['q_kind'] == 0, rec['q_n'])
    assert np.array_equal(rec['y32'][is_value, -1], rec['v_out'])   # the recorded answers ARE the recorded network output
    pick = lambda y, rows_, cols: torch.from_numpy(np.ascontiguousarray(y[rows_][:, cols]))      # noqa: E731
    c = assert_fp32_parity(pick(got, is_value, [-1]), pick(rec['y32'], is_value, [-1]), pick(rec['y64'], is_value, [-1]),
                           name + ' values')
    print('%s: %d values err64 %.3e err32 %.3e own %.3e bar %.3e' % (name, int(is_value.sum()), c['err64'], c['err32'], c['own'], c['atol']))
    if (~is_value).any():
        cols = list(range(dim))
        c = assert_fp32_parity(pick(got, ~is_value, cols), pick(rec['y32'], ~is_value, cols), pick(rec['y64'], ~is_value, cols),
                               name + ' action means')
        print('%s: %d action means err64 %.3e err32 %.3e own %.3e bar %.3e' % (name, int((~is_value).sum()), c['err64'], c['err32'],
                                                                           c['own'], c['atol']))
    # the same states as one batch give the same bits
    y = model.net.state_forward(torch.from_numpy(rec['q_states'].astype(np.float32)).to(DEV),
                                torch.zeros(len(rec['q_states']), dtype=torch.int32, device=DEV), model.pb_rep).cpu().numpy()
    assert np.array_equal(y[is_value, -1], got[is_value, -1]) and np.array_equal(y[~is_value], got[~is_value])


@pytest.mark.parametrize('dim', [2, 3])
def test_plan_host_on_the_device_model_yields_a_consistent_tree(dim):
    rec = _load([c for c in CASES if c.startswith('next_plan_maze%d' % dim)][0] + '.npz')
    model = _model(dim)
    problem = dict(map=rec['map'], goal_state=rec['goal_state'], init_state=rec['init_state'])
    model.set_problem(problem)
    torch.manual_seed(int(rec['seed']))
    out = next_plan.plan_host(problem, int(rec['seed']), model, t_max=60)
    model.check_status()
    n = out['states'].shape[0]
    assert n == out['i'] + 2 and (out['success'] or n == 61)
    assert out['parents'][0] == -1 and (out['parents'][1:] < np.arange(1, n)).all() and (out['parents'][1:] >= 0).all()
    assert out['stats']['guided'] > 0 and len(out['state_values']) == len(out['w']) == len(out['visits']) == n
    assert out['visits'].sum() == n and np.isclose(out['w'].sum(), out['w_sum'], rtol=1e-12)
    # a free node's cost is its rewired parent's cost AT THE TIME of the rewiring plus the edge length; later rewiring of the
    # parent lowers the parent only (descendants keep their costs), so: cost >= parent's final cost + edge, with equality for
    # the nodes whose ancestors were never rewired afterwards.  Collided nodes start at the obstacle cost and the second
    # rewiring pass may lower them.
    rp = out['rewired_parents']
    assert rp[0] == -1 and (rp[1:] >= 0).all() and (rp[1:] < n).all()
    assert (out['costs'][~out['freesp']] <= rrtstar.OBS_COST).all() and (out['costs'] >= 0).all()
    for j in range(1, n):
        if not out['freesp'][j]:
            continue
        assert out['freesp'][rp[j]]
        edge = rrtstar.distances(out['states'][rp[j]], out['states'][j], dim)[0]
        assert out['costs'][j] >= out['costs'][rp[j]] + edge - 1e-12
        # the newest node: its parent's cost cannot have changed since (the second pass lowers a neighbour only below
        # min_cost + dist, and the parent's cost is min_cost - dist), so the sum the rewiring formed is still there, bit for bit
        if j == n - 1:
            assert out['costs'][j] == edge + out['costs'][rp[j]]
    if out['success']:
        ids = out['path_ids']
        assert ids[0] == 0 and ids[-1] == n - 1 and out['in_goal_region'][-1] and (rp[ids[1:]] == ids[:-1]).all()
