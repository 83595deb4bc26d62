"""The batched resample rounds with one sample stream per problem (planner.plan_maze_rounds_batch / eval_gnn_device_streams)
against the host counterpart of the reference's loop, problem by problem: ``np.random.seed(seeds[i]); planner.explore(...)``
(collision checks and the greedy frontier on the CPU, one explorer forward per round).  Exact equality: success, rounds,
explored list, full pair list, path rows, collision checks, and with the maze2 smoother the smoothed path and its checks."""
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
# settings small enough that rounds happen: test_oracle_takes_rounds asserts the condition on the ORACLE's round counts and
# prints them with the success flags (pytest -s); no list of counts is kept here, since nothing would check it
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
    return m, None                                                # (no maze3 smoother checkpoint is shipped)


def _env(dim):
    name = 'evalset_mazehard_first1000.npz' if dim == 2 else 'evalset_maze3_first40_b200_k12_s9.npz'
    with np.load(os.path.join(GOLDEN, name)) as f:
        return (Maze2D if dim == 2 else Maze3D)(f['maps'], f['init_states'], f['goal_states'])


_CACHE = {}


def _case(dim):
    """Oracle and device results of the set, computed once per session and left unchanged."""
    if dim in _CACHE:
        return _CACHE[dim]
    cfg = MAZE2 if dim == 2 else MAZE3
    env, (model, model_s) = _env(dim), _models(dim)
    seeds = planner.stream_seeds(SEED, cfg['idx'])
    oracle = []
    for i, s in zip(cfg['idx'], seeds):
        e = type(env)(env.maps[i][None], env.init_states[i][None], env.goal_states[i][None])
        e.init_new_problem(0)
        np.random.seed(s)
        oracle.append(planner.explore(e, model, model_s, True, batch=cfg['batch'], t_max=cfg['t_max'], k=cfg['k'],
                                      smoother='model' if model_s is not None else 'none', sparse=True, device=DEV))
    problems = [dict(map=env.maps[i], init_state=env.init_states[i], goal_state=env.goal_states[i]) for i in cfg['idx']]
    np.random.seed(99)
    state = np.random.get_state()
    res = planner.plan_maze_rounds_batch(problems, model, DEV, seeds, batch=cfg['batch'], t_max=cfg['t_max'], k=cfg['k'],
                                         model_s=model_s)
    after = np.random.get_state()
    untouched = state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    _CACHE[dim] = dict(cfg=cfg, env=env, model=model, model_s=model_s, seeds=seeds, oracle=oracle, problems=problems, res=res,
                       untouched=untouched)
    return _CACHE[dim]


def _rows(x, dim):
    return np.asarray(x, dtype=np.float32).reshape(-1, dim)


def _same(a, b, dim, smoother):
    """Two result dicts of the device planner: every figure and array."""
    keys = ('success', 'rounds', 'c_explore', 'n_free') + (('c_smooth',) if smoother else ())
    arrays = ('explored', 'explored_edges', 'path') + (('smooth_path',) if smoother else ())
    return all(a[k] == b[k] for k in keys) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in arrays) and \
        np.array_equal(a['v'].numpy(), b['v'].numpy())


@pytest.mark.parametrize('dim', [2, 3])
def test_oracle_takes_rounds(dim):
    """The condition on the ORACLE's results: the settings make rounds happen."""
    c = _case(dim)
    rounds = [o['forward_split']['calls'] for o in c['oracle']]
    last = c['cfg']['t_max'] // c['cfg']['batch']
    print('\noracle rounds (dim %d):' % dim, rounds, 'solved', [bool(o['success']) for o in c['oracle']])
    assert sum(r >= 2 for r in rounds) >= 3
    assert any(r == last or not o['success'] for r, o in zip(rounds, c['oracle']))


@pytest.mark.parametrize('dim', [2, 3])
def test_every_problem_equals_the_host_loop(dim):
    c = _case(dim)
    assert c['untouched']                                         # the global numpy generator
    for i, (o, r) in enumerate(zip(c['oracle'], c['res'])):
        assert r['success'] == bool(o['success']), i
        assert r['rounds'] == o['forward_split']['calls'], i
        assert np.asarray(r['explored']).tolist() == list(o['explored']), i
        assert np.asarray(r['explored_edges']).tolist() == [list(p) for p in o['explored_edges']], i
        assert r['c_explore'] == o['c_explore'], (i, r['c_explore'], o['c_explore'])
        assert np.array_equal(_rows(r['path'], dim), _rows(o['path'], dim)), i
        if c['model_s'] is not None:
            assert np.array_equal(_rows(r['smooth_path'], dim), _rows(o['smooth_path'], dim)), i
            assert r['c_smooth'] == o['c_smooth'], (i, r['c_smooth'], o['c_smooth'])


@pytest.mark.parametrize('dim', [2, 3])
def test_results_do_not_depend_on_the_batch(dim):
    """A subset, a permuted order and two halves run separately give each problem the full run's result."""
    c = _case(dim)
    n = len(c['problems'])
    kw = dict(batch=c['cfg']['batch'], t_max=c['cfg']['t_max'], k=c['cfg']['k'], model_s=c['model_s'])
    perm = list(np.random.RandomState(3).permutation(n))
    for sel in ([1, n - 2, n // 2], perm, list(range(n // 2)), list(range(n // 2, n))):
        res = planner.plan_maze_rounds_batch([c['problems'][j] for j in sel], c['model'], DEV, [c['seeds'][j] for j in sel], **kw)
        for j, r in zip(sel, res):
            assert _same(r, c['res'][j], dim, c['model_s'] is not None), (sel, j)


def test_eval_streams_rows_and_sharding():
    """eval_gnn_device_streams: rows of the whole index list = rows of two shards (dist.eval_streams_shard), any chunking."""
    from gnnmp import dist
    c = _case(2)
    kw = dict(seed=SEED, batch=c['cfg']['batch'], t_max=c['cfg']['t_max'], k=c['cfg']['k'], device=DEV)
    rows, details = [], []
    out = planner.eval_gnn_device_streams(c['env'], c['cfg']['idx'], c['model'], c['model_s'], rows_out=rows, details_out=details,
                                          chunk=5, **kw)
    assert out['rounds'] == [r['rounds'] for r in c['res']] and out['n_success'] == sum(r['success'] for r in c['res'])
    assert [row[3] for row in rows] == [r['c_explore'] for r in c['res']]
    assert all(np.array_equal(d['smooth_path'], r['smooth_path']) for d, r in zip(details, c['res']) if r['success'])
    sharded = []
    for rank in range(2):
        dist.eval_streams_shard(c['env'], c['cfg']['idx'], c['model'], c['model_s'], rank, 2, rows_out=sharded, **kw)
    assert sharded == rows
