"""The collection and the whole loop of gnnmp.smoother_replay on maze problems (train_smoother.py:91-99, 136-222).

collect_replay: the stored rows must equal, exactly, what plan_maze_rounds_batch's own results, the sample rule of
planner._smooth_maze_batch (the first 500 free / collided rows, one zero row for an empty side) and
oracle_smooth.smoothing_targets under the same generator state give, for maze2 and maze3 problems of the fixtures under
tests/golden, with batch = 100.

train_smoother_maze: data_iter = 2, passes = 2 over the 40 maze3 problems (a dozen samples): finite losses, a best state that
loads into a fresh ModelSmoother, and eval_gnn_device_rounds running its smoothing stage with it."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_weights
import gnnmp
from gnnmp import oracle_smooth, planner
from gnnmp import smoother_replay as sr
from gnnmp.maze2d import Maze2D, Maze3D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BATCH, K, LOOP = 100, 30, 5
# one round of 100 samples solves about one maze3 problem in eight (five of eight on maze2): all 40 problems of the maze3 set
# give 4 samples in the first collection pass and 12 in two, enough for train() to step (it needs more than 8)
N_COLLECT = {2: 8, 3: 40}
N_TRAIN = 40


def _explorer(dim):
    m = gnnmp.EncoderProcessDecoder(2, dim, 32, 2).eval()
    m.load_state_dict(load_weights('weights_maze' if dim == 2 else 'weights_maze_3'))
    return m


def _env(dim):
    name = 'evalset_mazehard_first1000.npz' if dim == 2 else 'evalset_maze3_first40_b200_k12_s9.npz'
    with np.load(os.path.join(GOLDEN, name)) as f:
        return (Maze2D if dim == 2 else Maze3D)(f['maps'], f['init_states'], f['goal_states'])


def _problems(env, n):
    return [dict(map=env.maps[i], init_state=env.init_states[i], goal_state=env.goal_states[i]) for i in range(n)]


@pytest.mark.parametrize('dim', [2, 3])
def test_collect_replay_stores_the_planner_rows_and_the_oracle_targets(dim):
    n = N_COLLECT[dim]
    problems, model = _problems(_env(dim), n), _explorer(dim)
    ids = [40 + i for i in range(n)]
    seeds = sr.pass_seeds(1234, list(range(n)), 0)
    store = sr.SmoothReplayStore(dim, n, n * (BATCH + 2), n * (BATCH + 2), n * 500, DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    stats = sr.collect_replay(model, problems, ids, seeds, store, DEV, batch=BATCH, k=K, loop=LOOP, generator=gen)
    # the same by hand
    res = planner.plan_maze_rounds_batch(problems, model, DEV, seeds, batch=BATCH, t_max=BATCH, k=K, loop=LOOP)
    sel = [b for b in range(n) if res[b]['success']]
    assert all(r['rounds'] == 1 for r in res)
    paths = [np.asarray(res[b]['path'], dtype=np.float32).reshape(-1, dim) for b in sel]
    ptr = np.concatenate([[0], np.cumsum([p.shape[0] for p in paths])])
    gen.manual_seed(5)
    target, status = oracle_smooth.smoothing_targets(torch.from_numpy(np.concatenate(paths)).to(DEV), ptr.tolist(),
                                                     np.array([problems[b]['map'] for b in sel]), generator=gen)
    target, status = target.cpu(), status.cpu().tolist()
    want, want_ids = [], []
    for j, b in enumerate(sel):
        if paths[j].shape[0] > 2 and status[j] == 0:
            v, nf = res[b]['v'].float(), int(res[b]['n_free'])
            side = lambda t: t[:500] if t.shape[0] else torch.zeros(1, dim)      # noqa: E731
            want.append(dict(path=torch.from_numpy(paths[j]), target=target[ptr[j]:ptr[j + 1]], free=side(v[:nf]), coll=side(v[nf:])))
            want_ids.append(ids[b])
    short = sum(1 for p in paths if p.shape[0] <= 2)
    print('\nmaze%d: %s, %d stored' % (dim, stats, len(want)))
    assert stats == {'solved': len(sel), 'taken': len(want), 'short': short, 'failed': n - len(sel)}
    assert len(want) >= 2                                         # the comparison below is about something
    assert len(store) == len(want) and store.host_problem.tolist() == want_ids
    for name, key in (('path', 'path'), ('target', 'target'), ('free', 'free'), ('collided', 'coll')):
        rows = torch.cat([w[key] for w in want])
        assert torch.equal(getattr(store, name)[:rows.shape[0]].cpu(), rows), name
    for host_ptr, key in ((store.host_path_ptr, 'path'), (store.host_free_ptr, 'free'), (store.host_coll_ptr, 'coll')):
        assert host_ptr.tolist() == np.concatenate([[0], np.cumsum([w[key].shape[0] for w in want])]).tolist(), key


def _fresh_smoother():
    """A seeded ModelSmoother whose proposals stay near the waypoints (tests/test_stick_sample_gpu.py's): the stick robot's
    steering raises on a proposal whose orientation is more than 1.2 from its waypoint."""
    torch.manual_seed(0)
    ms = gnnmp.ModelSmoother(3, 3, 6, 128)
    sd = {k: t.clone() for k, t in ms.state_dict().items()}
    sd['smooth_node.weight'] *= 0.05
    sd['smooth_node.bias'] *= 0.05
    ms.load_state_dict(sd)
    return ms


def test_train_smoother_maze_gives_a_checkpoint_the_planner_runs_with():
    env = _env(3)
    problems, model = _problems(env, N_TRAIN), _explorer(3)
    ms = _fresh_smoother().to(DEV)
    before = {k: v.detach().clone() for k, v in ms.state_dict().items()}
    history, best = sr.train_smoother_maze(ms, model, problems, DEV, data_iter=2, passes=2, chunk=8, batch=BATCH)
    print('\ncollect %s, replay %d' % (history['collect'], history['replay']))
    assert len(history['collect']) == 2 and all(sum(c[k] for k in ('solved', 'failed')) == N_TRAIN for c in history['collect'])
    assert history['replay'] == sum(c['taken'] for c in history['collect']) > 8          # enough for train() to step
    assert len(history['train']) == 2
    for entry in history['train']:
        print('mean %.6e lr %g losses %s' % (entry['mean'], entry['lr'], entry['losses']))
        assert len(entry['losses']) == -(-history['replay'] // 8) and np.isfinite(entry['losses']).all()
    assert any(not torch.equal(best[k], before[k]) for k in ('smooth_node.weight', 'process.lin_0.0.weight'))      # it trained
    fresh = gnnmp.ModelSmoother(3, 3, 6, 128)
    fresh.load_state_dict(best)
    rows = []
    out = planner.eval_gnn_device_rounds(env, range(N_TRAIN), model, fresh.eval(), seed=1234, batch=BATCH, t_max=BATCH, k=K,
                                         device=DEV, rows_out=rows)
    rows = np.array(rows, dtype=np.float64)
    print('solved %d of %d, smoothing checks %s' % (int(rows[:, 0].sum()), N_TRAIN, rows[:, 4].tolist()))
    assert out is not None and rows.shape[0] == N_TRAIN and np.isfinite(rows).all()
    assert rows[:, 4].any()                                       # the smoothing stage ran with the trained checkpoint
