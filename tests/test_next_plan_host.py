"""gnnmp.next_plan.plan_host against recorded runs of the unmodified reference ``NEXT_plan`` with its ``Model2D``
(tools/gen_golden_next.py): driven by a replay model that returns the recorded answers -- and asserts that every queried state
equals the recorded one bit for bit -- the restatement must reproduce every tree field exactly.  Float64 numpy on both sides; a
one-ulp exp / log difference between machines could flip only an exact near-tie of an arg-max."""
import glob
import os

import numpy as np
import pytest

import gnnmp  # noqa: F401
from gnnmp import next_plan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'next_plan_maze*.npz')))
EXACT = ('states', 'parents', 'rewired_parents', 'expanded_by_rrt', 'freesp', 'in_goal_region', 'costs', 'path_lengths',
         'cumulated_collision_checks', 'visits', 'state_values', 'w', 'path_ids')


def load(name):
    with np.load(os.path.join(GOLDEN, name + '.npz')) as f:
        return {k: f[k] for k in f.files}


class ReplayModel:
    """Answers ``pred_value`` / ``policy`` from a recorded run, in call order."""

    def __init__(self, rec):
        self.rec, self.dim = rec, int(rec['dim'])
        self.q = self.row = self.v = self.p = 0

    def _next(self, kind, states):
        rec = self.rec
        assert self.q < len(rec['q_kind']), 'more queries than the recorded run made'
        assert rec['q_kind'][self.q] == kind, 'query %d: pred_value / policy out of the recorded order' % self.q
        a = np.asarray(states, dtype=np.float64).reshape(-1, self.dim)
        n = int(rec['q_n'][self.q])
        want = rec['q_states'][self.row:self.row + n]
        assert a.shape == want.shape and (a.view(np.uint64) == want.view(np.uint64)).all(), 'query %d: another state' % self.q
        self.q, self.row = self.q + 1, self.row + n
        return n

    def pred_value(self, states):
        n = self._next(0, states)
        out = self.rec['v_out'][self.v:self.v + n]
        self.v += n
        return out[0] if np.asarray(states).ndim == 1 else out

    def policy(self, state, k=1):
        self._next(1, state)
        actions, priors = self.rec['p_actions'][self.p], self.rec['p_priors'][self.p]
        self.p += 1
        assert k == len(actions)
        return [a for a in actions], list(priors)

    def exhausted(self):
        return self.q == len(self.rec['q_kind'])


def replay(rec):
    model = ReplayModel(rec)
    problem = dict(map=rec['map'], init_state=rec['init_state'], goal_state=rec['goal_state'])
    out = next_plan.plan_host(problem, int(rec['seed']), model, t_max=int(rec['t_max']), g_explore_eps=0.1, stop_when_success=True)
    return out, model


def test_fixture_set_contains_the_named_situations():
    recs = [load(n) for n in CASES]
    assert {int(r['dim']) for r in recs} == {2, 3}
    for dim in (2, 3):
        fam = [r for r in recs if int(r['dim']) == dim]
        assert any(bool(r['success']) and int(r['guided_success']) > 0 for r in fam), 'a success through the guided branch'
        assert any(not bool(r['success']) and int(r['i']) == int(r['t_max']) - 1 for r in fam), 'a run that exhausts t_max'
        assert any(int(r['guided_collided']) > 0 for r in fam), 'guided expansions that collide'
    assert any(int(r['wraps']) > 0 for r in recs if int(r['dim']) == 3), 'a wrap of the angle'


@pytest.mark.parametrize('name', CASES)
def test_plan_host_reproduces_the_recorded_run(name):
    rec = load(name)
    out, model = replay(rec)
    assert model.exhausted(), 'fewer queries than the recorded run made'
    for key in EXACT:
        got, want = np.asarray(out[key]), rec[key]
        assert got.shape == want.shape, key
        assert np.array_equal(got, want.astype(got.dtype)), key
    assert out['w_sum'] == float(rec['w_sum'])
    assert out['success'] == bool(rec['success']) and out['i'] == int(rec['i'])
    st = out['stats']
    assert (st['guided'], st['guided_collided'], st['guided_success']) == (int(rec['guided']), int(rec['guided_collided']),
                                                                          int(rec['guided_success']))
    assert (out['expanded_by_rrt'][1:] == 0).sum() == st['guided']
    if int(rec['wraps']):
        assert st['wraps'] > 0
