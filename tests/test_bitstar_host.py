"""gnnmp.bitstar.plan_host against the recorded runs of the reference's BIT* (tests/golden/bitstar_*.npz, written by
tools/gen_golden_bitstar.py): every field exactly, floats as bit patterns.  No GPU."""
import glob
import os

import numpy as np
import pytest

import gnnmp
from gnnmp import bitstar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(p)[len('bitstar_'):-len('.npz')] for p in glob.glob(os.path.join(GOLDEN, 'bitstar_*.npz')))
BATCH_FIELDS = ('r_by_batch', 'used_by_batch', 'checks_by_batch')
INF = float('inf')
_HOST = {}


def load_case(name):
    with np.load(os.path.join(GOLDEN, 'bitstar_%s.npz' % name)) as f:
        return {k: f[k] for k in f.files}


def problem_of(rec):
    return dict(map=rec['map'], init_state=rec['init_state'], goal_state=rec['goal_state'])


def pool_of(rec):
    return (rec['pool'], rec['r_by_batch']) if bool(rec['crafted']) else None


def host_plan(problem, seed, batch, t_max, pool=None):
    """plan_host once per (problem, settings): the oracle is shared among the tests (the GPU ones too) and left unchanged."""
    key = (problem['map'].tobytes(), np.asarray(problem['init_state']).tobytes(), np.asarray(problem['goal_state']).tobytes(),
           int(seed), int(batch), int(t_max), None if pool is None else np.asarray(pool[0]).tobytes())
    if key not in _HOST:
        _HOST[key] = bitstar.plan_host(problem, seed, batch=batch, t_max=t_max, pool=pool)
    return _HOST[key]


def host_of_case(name):
    rec = load_case(name)
    return rec, host_plan(problem_of(rec), int(rec['seed']), int(rec['batch']), int(rec['t_max']), pool_of(rec))


def assert_same_plan(got, want, what, fields=bitstar.FIELDS + BATCH_FIELDS, stats=None):
    """Field by field: floats bit for bit, everything else exactly, shapes included.  ``want`` is a fixture (counters at the
    top level) or a plan_host result (counters under ``stats``)."""
    for key in fields:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape, '%s: %s has shape %s, expected %s' % (what, key, g.shape, w.shape)
        assert g.dtype.kind == w.dtype.kind or (g.dtype.kind in 'iu' and w.dtype.kind in 'iu'), '%s: %s dtype' % (what, key)
        if g.dtype.kind == 'f':
            g, w = g.astype(np.float64).view(np.uint64), w.astype(np.float64).view(np.uint64)
        assert np.array_equal(g, w), '%s: %s differs at %s' % (what, key, np.flatnonzero((g != w).reshape(-1))[:8].tolist())
    ids = np.asarray(want['path_ids'], dtype=np.int64)
    assert np.array_equal(got['path'], np.asarray(want['points'])[ids]), '%s: path states' % what
    want_stats = want['stats'] if 'stats' in want else want
    for key in (bitstar.STATS if stats is None else stats):
        assert int(got['stats'][key]) == int(want_stats[key]), '%s: %s is %d, expected %d' % (what, key, got['stats'][key], want_stats[key])


def test_fixture_list():
    """The cases the fixtures must cover between them."""
    recs = [load_case(c) for c in CASES]
    solved = lambda r: float(r['g_goal']) < INF      # noqa: E731
    for dim in (2, 3):
        mine = [r for r in recs if int(r['dim']) == dim]
        assert any(solved(r) for r in mine) and any(not solved(r) for r in mine), dim
        assert any(int(r['rewired']) > 0 for r in mine), dim
        assert any(int(r['batch']) == 1 and r['points'].shape[0] == 2 + len(r['r_by_batch']) for r in mine), dim
    assert any(int(r['max_edge_queue']) > 64 for r in recs) and any(0 < int(r['max_edge_queue']) < 64 for r in recs)
    assert any(len(r['vertices']) > 64 for r in recs)
    assert any(int(r['ties_at_pop']) > 0 for r in recs)
    assert any(int(r['T']) > int(r['t_max']) for r in recs)
    assert any(bool(r['never_connected']) and len(r['vertices']) == 1 and len(r['r_by_batch']) > 1 for r in recs)
    for r in recs:
        assert solved(r) == (len(r['path_ids']) > 0)
        assert int(r['T']) == len(r['r_by_batch']) * int(r['batch'])
        assert r['points'].shape[0] == 2 + int(r['T']) == len(r['vertices']) + len(r['samples_left'])


@pytest.mark.parametrize('name', CASES)
def test_plan_host_equals_reference(name):
    rec, got = host_of_case(name)
    assert_same_plan(got, rec, name)


@pytest.mark.parametrize('dim', [2, 3])
def test_radius_table_from_the_attempt_counts(dim):
    """radius_by_batch, which the device path builds its table with, gives the recorded radii bit for bit."""
    for name in CASES:
        rec = load_case(name)
        if int(rec['dim']) != dim or bool(rec['crafted']):
            continue
        got = bitstar.radius_by_batch(dim, int(rec['batch']), rec['used_by_batch'])
        assert np.array_equal(got.view(np.uint64), rec['r_by_batch'].view(np.uint64)), name


def test_plan_host_refuses_what_the_reference_cannot_run():
    rec = load_case(CASES[0])
    pr = problem_of(rec)
    with pytest.raises(ValueError):
        bitstar.plan_host(dict(pr, goal_state=pr['init_state']), 1, batch=5, t_max=5)
    with pytest.raises(ValueError):                              # the pool runs out of batches
        bitstar.plan_host(pr, 1, batch=1, t_max=3, pool=(np.array([[[0.9, 0.9]]]), np.array([1e-9])))


def test_eval_aggregate():
    rows = [dict(g_goal=2.0, checks=100, path=np.zeros((3, 2))), dict(g_goal=INF, checks=50, path=np.zeros((0, 2))),
            dict(g_goal=1.0, checks=30, path=np.zeros((2, 2)))]
    assert bitstar.eval_aggregate(rows) == (2, 60.0, 1.5)
    n, collision, cost = bitstar.eval_aggregate(rows[1:2])
    assert (n, collision) == (0, 50.0) and np.isnan(cost)


def test_exports():
    assert gnnmp.plan_bitstar_maze_batch is bitstar.plan_maze_batch
    assert gnnmp.eval_bit_device is bitstar.eval_bit_device
    assert gnnmp.bitstar_plan_host is bitstar.plan_host
