"""gnnmp.rrtstar.plan_host against the recorded runs of the reference's RRT* (tests/golden/rrtstar_*.npz, written by
tools/gen_golden_rrtstar.py): every field of the search tree exactly.  No GPU."""
import glob
import os

import numpy as np
import pytest

import gnnmp
from gnnmp import rrtstar
from gnnmp.maze2d import Maze2D, Maze3D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# (the rrtstar_lattice_* fixtures hold crafted draw blocks, no seed: tests/test_rrtstar_ties_host.py)
CASES = sorted(os.path.basename(p)[len('rrtstar_'):-len('.npz')] for p in glob.glob(os.path.join(GOLDEN, 'rrtstar_*.npz'))
               if not os.path.basename(p).startswith('rrtstar_lattice_'))
_HOST = {}


def load_case(name):
    with np.load(os.path.join(GOLDEN, 'rrtstar_%s.npz' % name)) as f:
        return {k: f[k] for k in f.files}


def problem_of(rec):
    return dict(map=rec['map'], init_state=rec['init_state'], goal_state=rec['goal_state'])


def host_plan(problem, seed, t_max, stop=True):
    """plan_host once per (problem, settings): the oracle is shared among the tests (the GPU ones too) and left unchanged."""
    key = (problem['map'].tobytes(), np.asarray(problem['init_state']).tobytes(), np.asarray(problem['goal_state']).tobytes(),
           int(seed), int(t_max), bool(stop))
    if key not in _HOST:
        _HOST[key] = rrtstar.plan_host(problem, seed, t_max=t_max, stop_when_success=stop)
    return _HOST[key]


def assert_same_tree(got, want, what):
    """Field by field: states and costs bit for bit, everything else exactly; shapes and float / bool kinds included."""
    for key in rrtstar.TREE_FIELDS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape, '%s: %s has shape %s, expected %s' % (what, key, g.shape, w.shape)
        assert g.dtype.kind == w.dtype.kind or (g.dtype.kind in 'iu' and w.dtype.kind in 'iu'), '%s: %s dtype' % (what, key)
        if g.dtype.kind == 'f':
            g, w = g.astype(np.float64).view(np.uint64), w.astype(np.float64).view(np.uint64)
        assert np.array_equal(g, w), '%s: %s differs at %s' % (what, key, np.flatnonzero((g != w).reshape(-1))[:8].tolist())
    ids = np.asarray(want['path_ids'], dtype=np.int64)
    assert np.array_equal(got['path'], np.asarray(want['states'])[ids]), '%s: path states' % what


def test_fixture_list():
    """The cases the fixtures must cover between them."""
    recs = {c: load_case(c) for c in CASES}
    r13 = recs['maze2_t300_i13']
    assert bool(r13['success']) and int(r13['i']) == 144 and int(r13['rewired']) == 54
    assert any(int(r['dim']) == 2 and bool(r['success']) and int(r['i']) > 144 and int(r['rewired']) > 100 and bool(r['stop_when_success'])
               for r in recs.values())
    r8 = recs['maze3_t300_i8']
    assert bool(r8['success']) and int(r8['i']) == 189
    for dim in (2, 3):
        assert sum(int(r['dim']) == dim and int(r['t_max']) == 100 and not bool(r['success']) and r['states'].shape[0] == 101
                   for r in recs.values()) >= 2
        for t_max in (1, 2):
            assert recs['maze%d_t%d_i0' % (dim, t_max)]['states'].shape == (t_max + 1, dim)
    assert any(not bool(r['stop_when_success']) and bool(r['success']) and r['in_goal_region'][:-50].any() for r in recs.values())
    assert any(float(r['first_rand']) < rrtstar.MODEL_EPS for r in recs.values())
    for key in ('direct_steer', 'collided_second_pass', 'goal_rechecks'):
        assert any(int(r[key]) > 0 for r in recs.values()), key
    assert all(int(r['t_max']) <= 300 for r in recs.values())


@pytest.mark.parametrize('name', CASES)
def test_plan_host_equals_reference(name):
    rec = load_case(name)
    got = host_plan(problem_of(rec), int(rec['seed']), int(rec['t_max']), bool(rec['stop_when_success']))
    assert_same_tree(got, rec, name)
    assert got['draws'] == int(rec['draws'])
    for key in ('direct_steer', 'collided_second_pass', 'goal_rechecks'):
        assert got['stats'][key] == int(rec[key]), key
    assert int((got['parents'] != got['rewired_parents']).sum()) == int(rec['rewired'])
    assert got['stats']['rewired'] == int(rec['second_pass_rewires'])


@pytest.mark.parametrize('cls,dim', [(Maze2D, 2), (Maze3D, 3)])
def test_draw_identity(cls, dim):
    """``next_sample`` on the raw doubles of ``RandomState(seed).random_sample`` gives what the reference's calls give on the
    global generator with the same seed: ``rand()``; below model_eps the goal, else ``rand()`` and ``uniform_sample()`` --
    and it consumes as many doubles."""
    env = cls(np.zeros((1, 15, 15)), np.zeros((1, dim)), np.full((1, dim), 0.25))
    env.init_new_problem(0)
    low, ranges = rrtstar.sample_bounds(dim)
    n = 2000
    raw = np.random.RandomState(4321).random_sample(rrtstar.draws_per_problem(n, dim))
    state = np.random.get_state()
    try:
        np.random.seed(4321)
        want, drawn = [], 0
        for _ in range(n):
            drawn += 1
            if np.random.rand() < 0.05:
                want.append(np.array(env.goal_state))
                continue
            assert np.random.rand() < 1.
            want.append(env.uniform_sample())
            drawn += 1 + dim
        tail = np.random.rand()
    finally:
        np.random.set_state(state)
    pos, got = 0, []
    for _ in range(n):
        s, pos = rrtstar.next_sample(raw, pos, env.goal_state, low, ranges)
        got.append(s)
    got, want = np.array(got), np.array(want)
    assert pos == drawn and raw[pos] == tail
    assert got.dtype == want.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    goals = (want == env.goal_state).all(axis=1)
    assert 40 < int(goals.sum()) < 200                              # both branches, about one in twenty the goal


def test_exports():
    assert gnnmp.plan_rrtstar_maze_batch is rrtstar.plan_maze_batch
    assert gnnmp.eval_rrt_device is rrtstar.eval_rrt_device
    assert gnnmp.rrtstar_plan_host is rrtstar.plan_host
