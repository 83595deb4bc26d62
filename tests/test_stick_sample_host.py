"""Rejection sampling of the stick robot (MazeEnv(dim=3)) on the host: the vectorised look-ahead sampler
Maze3D.sample_n_points_stream / Maze3D.classify_draws against the one-by-one loop (Maze3D.sample_n_points -> _state_fp), which
restates the reference's _stick_in_free_space (environment/maze_env.py:279-314).  Sampling is exact: every comparison is bit for
bit -- samples, collision-check counts and the state of numpy's global generator."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from gnnmp import planner
from gnnmp.maze2d import LIMITS3, AttemptStream, Maze3D

FIXTURE = os.path.join(GOLDEN, 'evalset_maze3_first40_b200_k12_s9.npz')


def _fixture():
    with np.load(FIXTURE) as f:
        return f['maps'], f['init_states'], f['goal_states']


def _env(maps, init, goal, i):
    e = Maze3D(np.asarray(maps[i])[None], np.asarray(init[i])[None], np.asarray(goal[i])[None])
    e.init_new_problem(0)
    return e


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _one_by_one(maps, init, goal, indexes, n, seed):
    """The reference's loop: (free, rejected, checks) per problem and the generator state it leaves."""
    np.random.seed(seed)
    out = []
    for i in indexes:
        e = _env(maps, init, goal, i)
        free, rej = e.sample_n_points(n, need_negative=True)
        out.append((np.array(free).reshape(-1, 3), np.array(rej).reshape(-1, 3), e.collision_check_count))
    return out, np.random.get_state()


def test_block_draws_equal_single_draws():
    """What AttemptStream rests on for three columns: one (m, 3) draw = m (1, 3) draws, values and generator state."""
    np.random.seed(4)
    one = np.concatenate([np.random.uniform(-LIMITS3, LIMITS3, (1, 3)) for _ in range(257)])
    st = np.random.get_state()
    np.random.seed(4)
    assert np.array_equal(np.random.uniform(-LIMITS3, LIMITS3, (257, 3)), one)
    assert _same_state(st, np.random.get_state())


@pytest.mark.parametrize('n', [200, 37])
def test_stream_sampler_equals_one_by_one_loop(n):
    maps, init, goal = _fixture()
    ref, st_ref = _one_by_one(maps, init, goal, range(6), n, seed=9)
    np.random.seed(9)
    stream = AttemptStream(limits=LIMITS3)
    got = []
    for i in range(6):
        e = _env(maps, init, goal, i)
        free, rej = e.sample_n_points_stream(stream, n)
        got.append((free, rej, e.collision_check_count))
    stream.close()
    assert _same_state(st_ref, np.random.get_state())
    for i, ((f0, r0, c0), (f1, r1, c1)) in enumerate(zip(ref, got)):
        assert f1.shape == (n, 3) and f1.dtype == np.float64
        assert np.array_equal(f0, f1), i
        assert r0.shape == r1.shape and np.array_equal(r0, r1), i
        assert c0 == c1, i


def _synthetic_map(w, share, seed):
    m = (np.random.default_rng(seed).random((w, w)) < share).astype(np.float64)
    m[0, 0] = 0.0
    return m


# 70 x 70 cells with about 5 % of them occupied: a cell is 0.0286 wide, so a quarter of a stick still spans more than one cell and the
# bisection runs to its third level; most sticks are free, so the walk is rarely cut short.  The seeds were chosen on the CPU so that
# the deepest case (two ends + seven midpoints) occurs among the 4000 draws.
@pytest.mark.parametrize('which', ['fixture_w15', 'synthetic_w70'])
def test_classification_of_every_draw(which):
    maps, init, goal = _fixture()
    if which == 'fixture_w15':
        e = _env(maps, init, goal, 0)
    else:
        e = _env(_synthetic_map(70, 0.05, 1)[None], init[:1], goal[:1], 0)
    pts = np.random.default_rng(2).uniform(-LIMITS3, LIMITS3, (4000, 3))
    free, checks = e.classify_draws(pts)
    assert e.collision_check_count == 0                        # classify_draws reports the counts, it does not book them
    exp_free, exp_checks = np.zeros(4000, dtype=bool), np.zeros(4000, dtype=np.int64)
    for j, p in enumerate(pts):
        c0 = e.collision_check_count
        exp_free[j] = e._state_fp(p)
        exp_checks[j] = e.collision_check_count - c0
    assert np.array_equal(free, exp_free)
    assert np.array_equal(checks, exp_checks)
    assert 0 < free.sum() < 4000 and checks.max() <= 9
    if which == 'synthetic_w70':
        assert checks.max() == 9                               # the third level of the bisection is really walked


def test_out_of_bounds_ends_cost_no_check():
    maps, init, goal = _fixture()
    e = _env(np.zeros((1, 15, 15)), init[:1], goal[:1], 0)
    pts = np.array([[0.95, 0.0, 0.0],       # end a = (0.85, 0) is queried, end b = (1.05, 0) is outside: 1 check
                    [-0.95, 0.0, 0.0],      # end a = (-1.05, 0) is outside: nothing is queried
                    [0.5, 0.5, 0.2]])       # free, vertical stick inside one column of cells
    free, checks = e.classify_draws(pts)
    assert free.tolist() == [False, False, True]
    assert checks[:2].tolist() == [1, 0] and checks[2] >= 2


def test_skip_maze_sampling_on_stick_env():
    maps, init, goal = _fixture()
    env = Maze3D(maps, init, goal)
    _, st_ref = _one_by_one(maps, init, goal, [3, 0, 5], 50, seed=21)
    np.random.seed(21)
    planner.skip_maze_sampling(env, [3, 0, 5], 50)
    assert _same_state(st_ref, np.random.get_state())


def test_host_presampling_of_stick_problems():
    maps, init, goal = _fixture()
    n = 60
    ref, st_ref = _one_by_one(maps, init, goal, range(4), n, seed=13)
    pr = [dict(map=maps[i], init_state=init[i], goal_state=goal[i]) for i in range(4)]
    np.random.seed(13)
    envs, vs, n_free, k1s = planner.sample_maze_problems(pr, n, 12)
    assert _same_state(st_ref, np.random.get_state())
    from gnnmp.graph_build import k1_of
    for i, (f0, r0, c0) in enumerate(ref):
        rows = np.concatenate((np.asarray(init[i], dtype=np.float64).reshape(1, 3), np.asarray(goal[i], dtype=np.float64).reshape(1, 3),
                               f0, r0[:n])).astype(np.float32)
        assert isinstance(envs[i], Maze3D) and envs[i].collision_check_count == c0
        assert vs[i].dtype.is_floating_point and tuple(vs[i].shape) == rows.shape and rows.shape[1] == 3
        assert np.array_equal(vs[i].numpy(), rows), i
        assert n_free[i] == n + 2 and k1s[i] == k1_of(12, n + 2)
