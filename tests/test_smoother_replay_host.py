"""Host side of gnnmp.smoother_replay, no GPU: the schedule of train_smoother.py's training passes against a literal
transcription of its loop under ``np.random.seed``, the float64 restatement of the loss against torch's own ``mse_loss`` and
autograd in float64, and ``random_init_goal`` against a transcription of ``MazeEnv.set_random_init_goal`` over the same
environment."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import gnnmp  # noqa: F401
from gnnmp import smoother_replay as sr
from gnnmp.maze2d import Maze2D, Maze3D


def _reference_passes(n, passes, seed):
    """train_smoother.py:198-216 with train() (:33-61) inlined, keeping only what draws: the global generator, seeded."""
    np.random.seed(seed)
    out = []
    for iter_i in range(passes):
        indexes = np.random.permutation(n)
        steps = []
        for index in np.arange(n):
            if index % 8 != 0:
                continue
            batch_idx = indexes[index:(index + 8)]
            if n <= 8:                                            # train(): `if len(replay) <= 8: return 0.`
                continue
            loops = []
            for idx in batch_idx:
                loops.append(np.random.randint(1, 10))
            steps.append((batch_idx, loops, len(batch_idx)))      # the divisor is len(batch_idx)
        out.append(steps)
    return out, np.random.get_state()


@pytest.mark.parametrize('n', [8, 9, 11, 16])
def test_replay_schedule_is_the_reference_loop(n):
    want, state = _reference_passes(n, 3, 77)
    rng = np.random.RandomState(77)
    got = sr.replay_schedule(n, passes=3, group=8, rng=rng)
    assert len(got) == len(want) == 3
    for g_steps, w_steps in zip(got, want):
        assert len(g_steps) == len(w_steps) == (0 if n <= 8 else -(-n // 8))
        for (idx, loops), (w_idx, w_loops, divisor) in zip(g_steps, w_steps):
            assert np.array_equal(idx, w_idx) and loops.tolist() == w_loops and len(idx) == divisor
            assert 1 <= min(w_loops) and max(w_loops) <= 9
    if n > 8:
        assert len(got[0][-1][0]) == (n % 8 or 8)                 # the last group is shorter, its divisor its own length
    mine = rng.get_state()
    assert mine[0] == state[0] and np.array_equal(mine[1], state[1]) and mine[2:] == state[2:]      # the same number of draws


@pytest.mark.parametrize('C,lengths,divisor', [(2, (3,), 1), (3, (2, 3, 4, 65, 130, 5, 7, 9), 8), (14, (4, 2, 66), 3)])
def test_path_loss_reference_is_mse_loss_in_float64(C, lengths, divisor):
    gen = torch.Generator().manual_seed(C * 100 + len(lengths))
    ptr = np.concatenate([[0], np.cumsum(lengths)])
    pred = torch.rand(int(ptr[-1]), C, generator=gen, dtype=torch.float64, requires_grad=True)
    target = torch.rand(int(ptr[-1]), C, generator=gen, dtype=torch.float64)
    terms = [torch.nn.functional.mse_loss(target[a:b][1:-1], pred[a:b][1:-1]) if b - a > 2 else pred.sum() * 0
             for a, b in zip(ptr[:-1], ptr[1:])]
    loss = sum(terms) / divisor
    loss.backward()
    got_terms, got_loss, got_d = sr.path_loss_reference(pred.detach().numpy(), target.numpy(), ptr, divisor)
    want_terms = np.array([float(t.detach()) for t in terms])
    assert np.all(np.abs(got_terms - want_terms) <= 1e-12 * np.abs(want_terms))
    assert abs(got_loss - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    want_d = pred.grad.numpy()
    assert np.all(np.abs(got_d - want_d) <= 1e-12 * np.abs(want_d).max())
    for a, b in zip(ptr[:-1], ptr[1:]):                            # end rows, and all rows of a path without interior
        assert not got_d[a].any() and not got_d[b - 1].any()
        if b - a <= 2:
            assert not got_d[a:b].any() and got_terms[list(ptr[:-1]).index(a)] == 0


def _env(dim):
    name = 'evalset_mazehard_first1000.npz' if dim == 2 else 'evalset_maze3_first40_b200_k12_s9.npz'
    with np.load(os.path.join(GOLDEN, name)) as f:
        return (Maze2D if dim == 2 else Maze3D)(f['maps'], f['init_states'], f['goal_states'])


def _set_random_init_goal(env):
    """maze_env.py:102-117 over the project's environment: uniform_sample draws from the global generator."""
    def sample_empty_points():
        while True:
            point = env.uniform_sample()
            if env._state_fp(point):
                return point
    while True:
        init, goal = sample_empty_points(), sample_empty_points()
        if np.sum(np.abs(init - goal)) != 0:
            break
    return init, goal


@pytest.mark.parametrize('dim', [2, 3])
def test_random_init_goal(dim):
    env = _env(dim)
    for index in range(4):
        problem = env.init_new_problem(index)
        one = type(env)(env.maps[index][None], env.init_states[index][None], env.goal_states[index][None])
        one.init_new_problem(0)
        np.random.seed(500 + index)
        init, goal = _set_random_init_goal(one)
        state = np.random.get_state()
        rng = np.random.RandomState(500 + index)
        new = sr.random_init_goal(problem, rng)
        assert new['map'] is problem['map']
        assert new['init_state'].dtype == np.float64 and new['init_state'].shape == (dim,) and new['goal_state'].shape == (dim,)
        assert np.array_equal(new['init_state'], init) and np.array_equal(new['goal_state'], goal)
        assert one._state_fp(new['init_state']) and one._state_fp(new['goal_state'])          # both free
        assert np.abs(new['init_state'] - new['goal_state']).sum() != 0                        # and distinct
        mine = rng.get_state()
        assert mine[0] == state[0] and np.array_equal(mine[1], state[1]) and mine[2:] == state[2:]      # the same number of draws
