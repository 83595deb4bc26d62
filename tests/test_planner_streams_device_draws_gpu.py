"""planner.plan_maze_rounds_batch(draws='device'): the per-problem generators run on the device (gnnmp.rng.MTStreams) and every
problem's result equals the host-draws run field by field.  Settings and fixtures of tests/test_planner_streams_gpu.py (which
holds the host-draws path to the reference's loop): maze2 = first 12 problems of the 1000-problem set at batch 50, t_max 150,
k 12 with the shipped smoother; maze3 = first 6 problems of the 40-problem set at batch 60, t_max 180, k 12."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_weights
import gnnmp
from gnnmp import planner
from gnnmp.maze2d import Maze2D, Maze3D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 1234
MAZE2 = dict(batch=50, t_max=150, k=12, idx=list(range(12)))
MAZE3 = dict(batch=60, t_max=180, k=12, idx=list(range(6)))


def _models(dim):
    if dim == 2:
        m = gnnmp.EncoderProcessDecoder(2, 2, 32, 2).eval()
        m.load_state_dict(load_weights('weights_maze'))
        ms = gnnmp.ModelSmoother(workspace_size=2, config_size=2, embed_size=128, obs_size=6).eval()
        ms.load_state_dict(load_weights('smooth_2d_attv3'))
        return m, ms
    m = gnnmp.EncoderProcessDecoder(2, 3, 32, 2).eval()
    m.load_state_dict(load_weights('weights_maze_3'))
    return m, None


def _env(dim):
    name = 'evalset_mazehard_first1000.npz' if dim == 2 else 'evalset_maze3_first40_b200_k12_s9.npz'
    with np.load(os.path.join(GOLDEN, name)) as f:
        return (Maze2D if dim == 2 else Maze3D)(f['maps'], f['init_states'], f['goal_states'])


_CACHE = {}


def _case(dim):
    """Host-draws and device-draws results of the set, computed once per session and left unchanged."""
    if dim in _CACHE:
        return _CACHE[dim]
    cfg = MAZE2 if dim == 2 else MAZE3
    env, (model, model_s) = _env(dim), _models(dim)
    seeds = planner.stream_seeds(SEED, cfg['idx'])
    problems = [dict(map=env.maps[i], init_state=env.init_states[i], goal_state=env.goal_states[i]) for i in cfg['idx']]
    kw = dict(batch=cfg['batch'], t_max=cfg['t_max'], k=cfg['k'], model_s=model_s)
    host = planner.plan_maze_rounds_batch(problems, model, DEV, seeds, draws='host', **kw)
    np.random.seed(99)
    state = np.random.get_state()
    device = planner.plan_maze_rounds_batch(problems, model, DEV, seeds, draws='device', **kw)
    after = np.random.get_state()
    untouched = state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    _CACHE[dim] = dict(cfg=cfg, env=env, model=model, model_s=model_s, seeds=seeds, problems=problems, kw=kw, host=host,
                       device=device, untouched=untouched)
    return _CACHE[dim]


def _assert_same(a, b, smoother, what):
    """Two result dicts of the streams planner, field by field."""
    for key in ('success', 'rounds', 'c_explore', 'n_free') + (('c_smooth',) if smoother else ()):
        assert a[key] == b[key], (what, key, a[key], b[key])
    for key in ('explored', 'explored_edges', 'path') + (('smooth_path',) if smoother else ()):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (what, key)
    assert np.array_equal(a['v'].numpy(), b['v'].numpy()), (what, 'v')


@pytest.mark.parametrize('dim', [2, 3])
def test_device_draws_equal_host_draws(dim):
    c = _case(dim)
    assert any(r['rounds'] >= 2 for r in c['host'])              # on the HOST-draws result: commit-then-continue is exercised
    assert len(c['device']) == len(c['host'])
    for i, (h, d) in enumerate(zip(c['host'], c['device'])):
        _assert_same(d, h, c['model_s'] is not None, (dim, i))


@pytest.mark.parametrize('dim', [2, 3])
def test_global_generator_untouched(dim):
    assert _case(dim)['untouched']


@pytest.mark.parametrize('dim', [2, 3])
def test_short_first_block_retries(dim, monkeypatch):
    """With the draws-per-free estimate at 0 the first block is 64 rows, fewer than ``batch`` free draws for every problem
    (asserted on the CPU from numpy's own first 64 draws): every problem is filled again from its uncommitted state with 128,
    256, ... rows, and the results do not change."""
    c = _case(dim)
    n = c['cfg']['batch']
    lim = np.asarray(type(c['env']).SAMPLE_LIMITS, dtype=np.float64)
    for i, s in zip(c['cfg']['idx'], c['seeds']):
        e = type(c['env'])(c['env'].maps[i][None], c['env'].init_states[i][None], c['env'].goal_states[i][None])
        e.init_new_problem(0)
        free, _ = e.classify_draws(np.random.RandomState(s).uniform(-lim, lim, (64, dim)))
        assert int(np.sum(free)) < n, (i, int(np.sum(free)))
    monkeypatch.setattr(planner, '_DRAWS_PER_FREE', [0.0, 0.0])
    res = planner.plan_maze_rounds_batch(c['problems'], c['model'], DEV, c['seeds'], draws='device', **c['kw'])
    for i, (r, d) in enumerate(zip(res, c['device'])):
        _assert_same(r, d, c['model_s'] is not None, (dim, i))


@pytest.mark.parametrize('dim', [2, 3])
def test_permuted_subset(dim):
    c = _case(dim)
    n = len(c['problems'])
    sel = [int(j) for j in np.random.RandomState(3).permutation(n)[:max(n // 2, 3)]]
    res = planner.plan_maze_rounds_batch([c['problems'][j] for j in sel], c['model'], DEV, [c['seeds'][j] for j in sel],
                                         draws='device', **c['kw'])
    for j, r in zip(sel, res):
        _assert_same(r, c['device'][j], c['model_s'] is not None, (dim, sel, j))


def test_eval_streams_passes_draws_through():
    from gnnmp import dist
    c = _case(2)
    kw = dict(seed=SEED, batch=c['cfg']['batch'], t_max=c['cfg']['t_max'], k=c['cfg']['k'], device=DEV)
    rows = []
    out = planner.eval_gnn_device_streams(c['env'], c['cfg']['idx'], c['model'], c['model_s'], rows_out=rows, chunk=5,
                                          draws='device', **kw)
    assert out['rounds'] == [r['rounds'] for r in c['host']]
    assert [row[3] for row in rows] == [r['c_explore'] for r in c['host']]
    sharded = []
    for rank in range(2):
        dist.eval_streams_shard(c['env'], c['cfg']['idx'], c['model'], c['model_s'], rank, 2, rows_out=sharded, draws='device', **kw)
    assert sharded == rows
    with pytest.raises(ValueError):
        planner.plan_maze_rounds_batch(c['problems'][:1], c['model'], DEV, c['seeds'][:1], draws='gpu', **c['kw'])
