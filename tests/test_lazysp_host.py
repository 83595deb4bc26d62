"""gnnmp.lazysp.plan_host against the recorded runs of the reference's LazySP (tests/golden/lazysp_*.npz, written by
tools/gen_golden_lazysp.py): every field exactly.  No GPU."""
import glob
import os

import numpy as np
import pytest

import gnnmp
from gnnmp import lazysp
from gnnmp.maze2d import Maze2D, Maze3D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# (the lazysp_lattice_* fixtures hold crafted draw blocks, no seed: tests/test_lazysp_ties_host.py)
CASES = sorted(os.path.basename(p)[len('lazysp_'):-len('.npz')] for p in glob.glob(os.path.join(GOLDEN, 'lazysp_*.npz'))
               if not os.path.basename(p).startswith('lazysp_lattice_'))
EXACT_FIELDS = ('checks', 'path_ids', 'T', 'valid_edges', 'invalid_edges', 'dijkstra_runs', 'invalid_order', 'rounds')


def load_case(name):
    with np.load(os.path.join(GOLDEN, 'lazysp_%s.npz' % name)) as f:
        return {k: f[k] for k in f.files}


def assert_same_plan(got, want, what):
    """Field by field: samples bit for bit, everything else exactly."""
    assert np.array_equal(got['samples'], want['samples']), '%s: samples' % what
    assert got['samples'].dtype == np.float64
    for key in EXACT_FIELDS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape and np.array_equal(g, w), '%s: %s differs (%s vs %s)' % (what, key, g.tolist()[:8], w.tolist()[:8])
    assert np.array_equal(got['path'], want['samples'][np.asarray(want['path_ids'], dtype=np.int64)]), '%s: path states' % what


def test_fixture_list():
    """The cases the fixtures must cover between them."""
    assert len(CASES) >= 15
    recs = [load_case(c) for c in CASES]
    first_round = lambda r: len(r['path_ids']) > 0 and len(r['rounds']) == 1      # noqa: E731
    assert any(first_round(r) and int(r['dim']) == 2 for r in recs)
    assert any(first_round(r) and int(r['dim']) == 3 for r in recs)
    assert any(len(r['path_ids']) > 0 and len(r['rounds']) > 1 for r in recs)
    assert any(len(r['path_ids']) == 0 for r in recs)
    assert any(bool(r['first_dist1_inf']) for r in recs)
    assert any(int(r['batch']) == 1 and int(r['rounds'][0, 0]) == 3 for r in recs)


@pytest.mark.parametrize('name', CASES)
def test_plan_host_equals_reference(name):
    rec = load_case(name)
    got = lazysp.plan_host(dict(map=rec['map'], init_state=rec['init_state'], goal_state=rec['goal_state']), int(rec['seed']),
                           batch=int(rec['batch']), t_max=int(rec['t_max']), k=int(rec['k']))
    assert_same_plan(got, rec, name)


def test_full_dijkstra_gives_the_same_plan():
    """The early exit (stop once node 1 is extracted) changes nothing: the full runs of the reference give the same fields."""
    rec = load_case('maze2_b20_t100_i3')
    got = lazysp.plan_host(dict(map=rec['map'], init_state=rec['init_state'], goal_state=rec['goal_state']), int(rec['seed']),
                           batch=int(rec['batch']), t_max=int(rec['t_max']), k=int(rec['k']), early_exit=False)
    assert_same_plan(got, rec, 'full dijkstra')


@pytest.mark.parametrize('cls,dim', [(Maze2D, 2), (Maze3D, 3)])
def test_draw_identity(cls, dim):
    """LazySP's ``bounds[:, 0] + np.random.random(dim) * ranges`` gives the doubles of ``uniform_sample``'s
    ``np.random.uniform(-LIMITS, LIMITS)`` = ``low + (high - low) * d`` from the same generator state."""
    env = cls(np.zeros((1, 15, 15)), np.zeros((1, dim)), np.zeros((1, dim)))
    env.init_new_problem(0)
    low, ranges = lazysp._bounds(env)
    state = np.random.get_state()
    try:
        np.random.seed(77)
        a = np.array([env.uniform_sample() for _ in range(500)])
        np.random.seed(77)
        b = np.array([low + np.random.random(dim) * ranges for _ in range(500)])
    finally:
        np.random.set_state(state)
    assert a.dtype == b.dtype == np.float64 and np.array_equal(a, b)
    rs = np.random.RandomState(77)
    assert np.array_equal(rs.uniform(-cls.SAMPLE_LIMITS, cls.SAMPLE_LIMITS, (500, dim)), a)


def test_exports():
    assert gnnmp.plan_lazysp_maze_batch is lazysp.plan_maze_batch
    assert gnnmp.eval_lazysp_device is lazysp.eval_lazysp_device
    assert gnnmp.lazysp_plan_host is lazysp.plan_host
