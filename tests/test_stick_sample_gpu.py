"""Rejection sampling of the stick robot (MazeEnv(dim=3)) on the device: gnnmp_stick_sample (csrc/maze_kernels.hip) through the C
ABI and through the planner (sample_maze_problems_device, explore_maze_batch, eval_gnn_device with Maze3D environments).

The expectation of the sampling itself is the host's one-by-one classifier Maze3D._state_fp (the reference's
_stick_in_free_space, environment/maze_env.py:279-314) walked over the same draws: sampling is exact, so node rows, row offsets,
draw counts, collision-check counts, the stream cursor and the generator state are compared with no margin.  The planner runs are
held to the rows recorded from the unmodified reference (evalset_maze3_first40_b200_k12_s9.npz) with the bar
tests/test_planner_rounds_gpu.py::test_maze3_40_problems applies to the same rows."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_weights
import gnnmp
from gnnmp import _lib, planner
from gnnmp.maze2d import LIMITS3, Maze3D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIXTURE = os.path.join(GOLDEN, 'evalset_maze3_first40_b200_k12_s9.npz')


def _fixture():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in ('maps', 'init_states', 'goal_states', 'rows', 'seed', 'batch', 'k')}


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ------------------------------------------------------------------------------------------------ the raw entry point
def _expect(att, maps, init, goal, n, cursor=0):
    """Maze3D._state_fp over the draws, problem after problem: node rows, row offsets, draws and checks per problem, cursor."""
    rows, ptr, used, checks = [], [0], [], []
    for b in range(len(maps)):
        e = Maze3D(maps[b][None], init[b][None], goal[b][None])
        e.init_new_problem(0)
        free, rej, start = [], [], cursor
        while len(free) < n:
            p = att[cursor]
            cursor += 1
            (free if e._state_fp(p) else rej).append(p)
        used.append(cursor - start)
        checks.append(e.collision_check_count)
        rows.append(np.concatenate((init[b:b + 1], goal[b:b + 1], np.array(free).reshape(-1, 3),
                                    np.array(rej[:n]).reshape(-1, 3))).astype(np.float32))
        ptr.append(ptr[-1] + rows[-1].shape[0])
    return {'v': np.concatenate(rows), 'node_ptr': ptr, 'used': used, 'checks': checks, 'cursor': cursor}


class _Device:
    """The device arrays of one problem list; :meth:`run` is one gnnmp_stick_sample call and returns what it wrote."""

    def __init__(self, att, maps, init, goal, n):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)      # noqa: E731
        self.B, self.w, self.n = len(maps), int(maps.shape[1]), n
        self.att, self.maps, self.init, self.goal = t(att), t(maps), t(init), t(goal)

    def run(self, n_attempts=None, cursor=0):
        B, n = self.B, self.n
        v = torch.full((B * (2 + 2 * n), 3), float('nan'), dtype=torch.float32, device=DEV)
        nptr = torch.full((B + 1,), -7, dtype=torch.int32, device=DEV)
        used = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        checks = torch.full((B,), -7, dtype=torch.int64, device=DEV)
        state = torch.tensor([cursor, 0], dtype=torch.int64, device=DEV)
        M = int(self.att.shape[0]) if n_attempts is None else n_attempts
        sb = _lib.MazeSampleBatch(B, self.w, n, M, self.att.data_ptr(), self.maps.data_ptr(), self.init.data_ptr(), self.goal.data_ptr())
        rc = _lib.lib().gnnmp_stick_sample(ctypes.byref(sb), state.data_ptr(), v.data_ptr(), nptr.data_ptr(), used.data_ptr(),
                                           checks.data_ptr(), state.data_ptr() + 8, None)
        assert rc == 0
        torch.cuda.synchronize()
        cur, ok = state.cpu().tolist()
        return {'v': v.cpu().numpy(), 'node_ptr': nptr.cpu().tolist(), 'used': used.cpu().tolist(), 'checks': checks.cpu().tolist(),
                'cursor': cur, 'ok': ok & 0xffffffff}


def _assert_equal(got, exp):
    assert got['ok'] == 1 and got['cursor'] == exp['cursor']
    assert got['node_ptr'] == exp['node_ptr']
    assert got['used'] == exp['used']
    assert got['checks'] == exp['checks']
    total = exp['node_ptr'][-1]
    assert got['v'][:total].tobytes() == exp['v'].tobytes()            # float32 rows, bit for bit
    assert np.isnan(got['v'][total:]).all()                            # nothing is written behind the last block


def _synthetic_maps(B, w, share):
    maps = (np.random.default_rng(5).random((B, w, w)) < share).astype(np.float64)
    maps[:, 0, 0] = 0.0
    return maps


@functools.lru_cache(maxsize=None)
def _random_case(w):
    """B = 5 problems with different maps, n_free = 37, one stream of uniform draws; the cursor starts at 3."""
    fx = _fixture()
    B, n = 5, 37
    maps = fx['maps'][:B].astype(np.float64) if w == 15 else _synthetic_maps(B, w, 0.05)      # 70 x 70: read from global memory
    init, goal = fx['init_states'][:B].astype(np.float64), fx['goal_states'][:B].astype(np.float64)
    att = np.random.default_rng(7).uniform(-LIMITS3, LIMITS3, (6000, 3))
    return att, maps, init, goal, n, _expect(att, maps, init, goal, n, cursor=3)


@pytest.mark.parametrize('w', [15, 70], ids=['map_in_lds', 'map_in_global_memory'])
def test_raw_abi_against_the_host_classifier(w):
    att, maps, init, goal, n, exp = _random_case(w)
    assert exp['cursor'] + 1024 < att.shape[0]
    assert max(exp['checks']) > max(exp['used'])                       # a draw is not one check
    _assert_equal(_Device(att, maps, init, goal, n).run(cursor=3), exp)


def test_stream_too_short_consumes_nothing():
    att, maps, init, goal, n, exp = _random_case(15)
    dev = _Device(att, maps, init, goal, n)
    short = 3 + sum(exp['used'][:3]) + 5                               # the stream ends five draws into problem 3
    got = dev.run(n_attempts=short, cursor=3)
    assert got['ok'] == 0 and got['cursor'] == 3
    assert got['node_ptr'][:4] == exp['node_ptr'][:4] and got['node_ptr'][4] == -1
    _assert_equal(dev.run(cursor=3), exp)                              # the same arrays with the whole stream


# ---- crafted streams: z = 0 lays the stick along x (ends at x -+ 0.1), y = 0 is the middle of cell row 7; centres sit mid-cell, so every
# stick end lies a quarter of a cell (0.033) from the nearest cell boundary
def _mid(i):
    return -1.0 + (i + 0.5) * 2.0 / 15.0


def _draw(i):
    return [_mid(i), 0.0, 0.0]


A_OUT, B_OUT = _draw(0), _draw(14)          # end a outside the bounds: no check; end a inside, end b outside: one check
A_OCC, B_OCC, MID_OCC = _draw(6), _draw(4), _draw(5)      # with cell (5, 7) occupied: end a in it (1 check), end b in it (2), the midpoint (3)
FREE_COLUMNS = (1, 2, 3, 8, 9, 10, 11, 12, 13)            # clear of cell (5, 7) on either map


def _crafted_problem(n, pos, rejected_kinds):
    """pos + 1 draws whose n-th free one is the last: the other n - 1 free draws spread over the positions before it, every
    other position a rejected draw (the kinds in turn)."""
    free_at = set(np.linspace(0, pos - 1, n - 1).astype(int).tolist()) if n > 1 else set()
    assert len(free_at) == n - 1 and pos >= n - 1
    draws, r = [], 0
    for j in range(pos):
        if j in free_at:
            draws.append(_draw(FREE_COLUMNS[j % len(FREE_COLUMNS)]))
        else:
            draws.append(rejected_kinds[r % len(rejected_kinds)])
            r += 1
    return draws + [_draw(FREE_COLUMNS[pos % len(FREE_COLUMNS)])]


def test_crafted_draw_kinds_on_the_host():
    """The hand-placed draws are what their names say (host classifier): flag and check count of each kind."""
    one_cell = np.zeros((15, 15))
    one_cell[5, 7] = 1.0
    e = Maze3D(one_cell[None], np.zeros((1, 3)), np.zeros((1, 3)))
    e.init_new_problem(0)
    for draw, checks in ((A_OUT, 0), (B_OUT, 1), (A_OCC, 1), (B_OCC, 2), (MID_OCC, 3)):
        c0 = e.collision_check_count
        assert not e._state_fp(np.array(draw)) and e.collision_check_count - c0 == checks
    for i in range(15):                                               # all-free map: free iff |x| <= 0.9
        e2 = Maze3D(np.zeros((1, 15, 15)), np.zeros((1, 3)), np.zeros((1, 3)))
        e2.init_new_problem(0)
        assert e2._state_fp(np.array(_draw(i))) == (abs(_mid(i)) <= 0.9)
    assert all(e._state_fp(np.array(_draw(i))) for i in FREE_COLUMNS)


# position of the n-th free draw inside its 1024-draw step: first lane, last lane of a wave, first lane of the next wave, last
# thread of the step, first thread of the second step
@pytest.mark.parametrize('n,pos', [(1, 0), (3, 63), (3, 64), (3, 1023), (3, 1024)])
def test_crafted_streams(n, pos):
    free_map, one_cell = np.zeros((15, 15)), np.zeros((15, 15))
    one_cell[5, 7] = 1.0
    maps = np.stack((free_map, one_cell, free_map))
    init = np.array([[0.1, 0.2, 0.3], [-0.4, 0.5, -0.1], [0.7, -0.7, 0.05]])
    goal = -init
    p0 = _crafted_problem(n, pos, [A_OUT, B_OUT])                      # all-free map: only the bounds reject
    p1 = _crafted_problem(n, pos, [A_OCC, B_OUT, B_OCC, A_OUT, MID_OCC])
    # fewer rejected draws than n: a short node block
    p2 = [_draw(8)] if n == 1 else [_draw(8), A_OUT] + [_draw(9 + j) for j in range(n - 1)]
    # free and blocked draws BEHIND the last problem's n-th free one, in the same step: they belong to nobody
    tail = [_draw(2), A_OUT, B_OUT, _draw(3), B_OUT]
    att = np.array(p0 + p1 + p2 + tail, dtype=np.float64)
    exp = _expect(att, maps, init, goal, n)
    # what the layout says by hand
    assert exp['used'] == [pos + 1, pos + 1, len(p2)] and exp['cursor'] == att.shape[0] - len(tail)
    rej = [pos + 1 - n, pos + 1 - n, len(p2) - n]
    assert np.diff(exp['node_ptr']).tolist() == [2 + n + min(r, n) for r in rej]
    assert rej[2] < n                                                  # problem 2: a short node block
    if pos:
        assert rej[0] > n and rej[1] > n                               # problems 0 and 1: only the first n rejected draws are kept
    _assert_equal(_Device(att, maps, init, goal, n).run(), exp)


# ------------------------------------------------------------------------------------------------ through the planner
def _problems(fx, count):
    return [dict(map=fx['maps'][i], init_state=fx['init_states'][i], goal_state=fx['goal_states'][i]) for i in range(count)]


@functools.lru_cache(maxsize=None)
def _host_presampled():
    fx = _fixture()
    np.random.seed(11)
    out = planner.sample_maze_problems(_problems(fx, 40), int(fx['batch']), int(fx['k']))
    return out, np.random.get_state()


@pytest.mark.parametrize('estimate', [8.0, 0.4], ids=['one_block', 'short_first_block'])
def test_device_sampler_equals_host_sampler(estimate):
    fx = _fixture()
    batch, k = int(fx['batch']), int(fx['k'])
    (envs, vs, n_free, k1s), st_host = _host_presampled()
    saved = planner._DRAWS_PER_FREE[1]
    try:
        planner._DRAWS_PER_FREE[1] = estimate                         # 0.4: the first block cannot hold the draws -> repeated launch
        np.random.seed(11)
        d = planner.sample_maze_problems_device(_problems(fx, 40), batch, k, DEV)
        st_dev = np.random.get_state()
    finally:
        planner._DRAWS_PER_FREE[1] = saved
    assert _same_state(st_host, st_dev)
    nptr, v = d['node_ptr_host'], d['v'].cpu()
    assert v.shape[1] == 3 and int(nptr[-1]) == sum(x.shape[0] for x in vs) == v.shape[0]
    for b in range(40):
        assert torch.equal(v[nptr[b]:nptr[b + 1]], vs[b]), b
        assert isinstance(d['envs'][b], Maze3D)
        assert d['envs'][b].collision_check_count == envs[b].collision_check_count, b
    assert d['n_free'] == n_free and d['k1s'] == k1s
    assert d['node_ptr'].cpu().tolist() == [int(x) for x in nptr]
    assert tuple(d['goal64'].shape) == (40, 3)


def _explorer():
    m = gnnmp.EncoderProcessDecoder(2, 3, 32, 2).eval()
    m.load_state_dict(load_weights('weights_maze_3'))
    return m


@functools.lru_cache(maxsize=None)
def _fixture_rows(device_sampling, shard=None):
    fx = _fixture()
    env = Maze3D(fx['maps'], fx['init_states'], fx['goal_states'])
    rows = []
    planner.eval_gnn_device(env, range(fx['rows'].shape[0]), _explorer(), None, seed=int(fx['seed']), batch=int(fx['batch']),
                            k=int(fx['k']), device=DEV, rows_out=rows, device_sampling=device_sampling, shard=shard)
    return np.array(rows, dtype=np.float64).reshape(-1, 7)


@pytest.mark.parametrize('device_sampling', [True, False], ids=['device_sampling', 'host_sampling'])
def test_eval_gnn_device_on_the_maze3_fixture(device_sampling):
    ref = _fixture()['rows']
    rows = _fixture_rows(device_sampling)
    assert rows.shape[0] == ref.shape[0] == 40
    same = (rows[:, 0] == ref[:, 0]) & (rows[:, 3] == ref[:, 3]) & (rows[:, 6] == ref[:, 6]) & (rows[:, 5] == ref[:, 5])
    print('\nmaze3 through eval_gnn_device (device_sampling=%s): solved %d (reference %d) of 40; explore stage identical on %d'
          % (device_sampling, rows[:, 0].sum(), ref[:, 0].sum(), same.sum()))
    assert np.array_equal(rows[:, 0], ref[:, 0])
    assert same.sum() >= 39                                            # the project's margin for one fp32 near-tie of the frontier
    ok = same & (ref[:, 0] > 0)
    assert np.allclose(rows[ok, 1], ref[ok, 1], rtol=0, atol=1e-6)
    # smoother='none': the smoothed path is the path
    assert np.array_equal(rows[:, 2], rows[:, 1]) and not rows[:, 4].any()


def test_shards_partition_the_evaluation():
    whole = _fixture_rows(True)
    parts = np.concatenate((_fixture_rows(True, (0, 2)), _fixture_rows(True, (1, 2))))
    assert np.array_equal(parts, whole)


def _seeded_smoother():
    torch.manual_seed(0)
    ms = gnnmp.ModelSmoother(3, 3, 6, 128)
    sd = {k: t.clone() for k, t in ms.state_dict().items()}
    # the proposals are the last layer's output itself: scaled down they stay inside the map and within 1.2 of any z
    sd['smooth_node.weight'] *= 0.05
    sd['smooth_node.bias'] *= 0.05
    ms.load_state_dict(sd)
    return ms.eval()


def test_with_a_smoother_equals_the_rounds_planner():
    fx = _fixture()
    env = Maze3D(fx['maps'], fx['init_states'], fx['goal_states'])
    seed, batch, k = int(fx['seed']), int(fx['batch']), int(fx['k'])
    m, ms = _explorer(), _seeded_smoother()
    assert fx['rows'][:8, 0].sum() >= 1                                # a solved problem, so that the smoothing stage runs
    rows, ref = [], []
    planner.eval_gnn_device(env, range(8), m, ms, seed=seed, batch=batch, k=k, device=DEV, rows_out=rows, workers=1, chunk=8)
    planner.eval_gnn_device_rounds(env, range(8), m, ms, seed=seed, batch=batch, t_max=batch, k=k, device=DEV, rows_out=ref)
    rows, ref = np.array(rows, dtype=np.float64), np.array(ref, dtype=np.float64)
    print('\nwith a smoother, device planner\n%s\nrounds planner\n%s' % (rows, ref))
    assert rows[:, 4].any()                                            # smoothing checks were spent
    assert np.array_equal(rows, ref)
