"""NEXT's guided planner on maze problems, restated on the host: ``NEXT_plan(env, model, T=t_max, g_explore_eps=0.1,
stop_when_success=True)`` as the reference's ``eval_next.py`` runs it (``algorithm/tsa.py:12-81, 141-220`` over
``algorithm/search_tree.py:21-28, 83-113``).  It is :func:`gnnmp.rrtstar.plan_host`'s loop -- the same sample stream, nearest
neighbour, steering, ``env.step`` and rewiring, imported from there -- plus the branch a model adds:

  * an iteration draws ``rand()``; below ``model_eps`` the sample is the goal state (1 double).  Otherwise a second ``rand()`` is
    drawn and, with a model, COMPARED against ``g_explore_eps = 0.1``: below it the RRT step with ``uniform_sample()`` (2 + dim
    doubles), else the guided step, which draws nothing more from numpy (2 doubles).
  * ``select``: the non-terminal node with the largest ``Q + c * sqrt(log(w_sum) / w)``, first maximum.
  * ``expand``: ``model.policy(state, k)`` gives k actions; each becomes a candidate through
    ``env.step(state, action, check_collision=False)`` (x, y clipped, the angle wrapped); the candidate with the largest
    ``Q + c * sqrt(log(w_sum) / w(candidate))`` with ``Q = model.pred_value(candidates)`` is stepped to with the counted
    ``env.step``.
  * ``insert_new_state`` with a model: ``pred_value(state)``, the parent's visit, then ``w_sum -= w[parent]``, the parent's
    weight recomputed over the tree INCLUDING the new state, ``w_sum += ``, then the new state's own weight;
    ``w(s) = sum(max(exp(-(dist(states, s) / RRT_EPS)^2), 1e-3))``.

All of it is float64 numpy, one rounded operation at a time; ``model`` is anything with ``pred_value`` and ``policy``
(:class:`gnnmp.next_model.Model2D`, the reference's ``Model2D``, a replay of recorded answers).  The numpy draws come from a
private ``RandomState(seed)``; ``policy`` of the device and reference models draws from the global torch generator, which the
caller seeds (``torch.manual_seed``) as the recorded runs do.
"""
import numpy as np

from . import maze2d
from .rrtstar import (MODEL_EPS, RRT_EPS, _problem_env, distances, draws_per_problem, new_stats, next_sample, rewire_last,
                      sample_bounds)

G_EXPLORE_EPS = 0.1                    # eval_next.py:62 explore_eps


def compute_w(states, state, dim):
    """``compute_w`` over ``state_kernel`` (search_tree.py:100-113)."""
    diff = distances(states, state, dim) / RRT_EPS
    return np.sum(np.maximum(np.exp(-(diff ** 2) * 1.), 1e-3))


def candidate_step(state, action, dim):
    """``env.step(state, action=action, check_collision=False)[0]`` (maze_env.py:181-201)."""
    new_state = state + action
    new_state[:2] = new_state[:2].clip(-maze2d.LIMITS, maze2d.LIMITS)
    if dim == 3:
        maze2d.Maze3D._wrap_orientation(new_state)
    return new_state


def select(non_terminal, state_values, w, w_sum, c):
    """tsa.py:141-165: the index of the non-terminal node to expand."""
    scores = [state_values[idx] + c * np.sqrt(np.log(w_sum) / w[idx]) for idx in non_terminal]
    return non_terminal[int(np.argmax(scores))]


def plan_host(problem, seed, model, t_max=1000, g_explore_eps=G_EXPLORE_EPS, model_eps=MODEL_EPS, stop_when_success=True, c=1.0, k=10):
    """One maze problem (a dict with ``map``, ``init_state``, ``goal_state``).  Returns the tree fields of
    :func:`gnnmp.rrtstar.plan_host` plus ``expanded_by_rrt`` (int8: 1 / 0, -1 for the root's None), ``state_values`` (float32),
    ``w``, ``w_sum``, ``visits`` and in ``stats`` also ``guided`` (guided iterations), ``guided_collided`` (those whose step
    collided), ``guided_success`` (those that reached the goal region) and ``wraps`` (candidate steps that wrapped the angle)."""
    env = _problem_env(problem)
    dim = env.config_dim
    low, ranges = sample_bounds(dim)
    raw = np.random.RandomState(int(seed) & 0xffffffff).random_sample(draws_per_problem(t_max, dim))
    goal = np.asarray(env.goal_state, dtype=np.float64).reshape(dim)
    # SearchTree.__init__ with a model (search_tree.py:5-28)
    states = [np.asarray(env.init_state, dtype=np.float64).reshape(dim).copy()]
    parents, rewired, by_rrt, freesp, in_goal, costs, path_lengths, cum = [-1], [-1], [-1], [True], [False], [0.], [-1.], [0]
    non_terminal = [0]
    visits = [1]
    state_values = [model.pred_value(states[0])]
    w = [compute_w(np.array(states), states[0], dim)]
    w_sum = w[0]
    stats = new_stats()
    stats.update(guided=0, guided_collided=0, guided_success=0, wraps=0)
    pos, success, i = 0, False, -1

    for i in range(int(t_max)):
        guided = raw[pos] >= model_eps and raw[pos + 1] >= g_explore_eps
        if guided:
            pos += 2
            parent = select(non_terminal, state_values, w, w_sum, c)
            state = np.array(states[parent])
            actions = model.policy(state=state, k=k)[0]
            candidates = []
            for a in actions[:k]:
                if dim == 3 and np.abs((state + a)[2]) > maze2d.Maze3D.ORIENT_HALF:
                    stats['wraps'] += 1
                candidates.append(candidate_step(state, a, dim))
            if k > 1:
                qs = model.pred_value(np.array(candidates))
                tree = np.array(states)
                scores = [qs[j] + c * np.sqrt(np.log(w_sum) / compute_w(tree, candidates[j], dim)) for j in range(k)]
                new_state = candidates[int(np.argmax(scores))]
            else:
                new_state = candidates[0]
            new_state, free, done = env.step(state, new_state)
            stats['guided'] += 1
            stats['guided_collided'] += not free
            stats['guided_success'] += bool(done)
        else:
            if raw[pos] < model_eps:
                sample, pos = np.array(goal, dtype=np.float64), pos + 1
            elif model_eps == MODEL_EPS:     # the second rand() (compared above) is skipped, then the uniform draw
                sample, pos = next_sample(raw, pos, goal, low, ranges)
            else:
                sample, pos = low + raw[pos + 2:pos + 2 + dim] * ranges, pos + 2 + dim
            # global_explore (tsa.py:121-139)
            idx = np.array(non_terminal)
            d = distances(np.array(states)[idx], sample, dim)
            j = int(np.argmin(d))
            parent = int(idx[j])
            if d[j] < RRT_EPS:
                new_state = sample
                stats['direct_steer'] += 1
            else:
                new_state = env.interpolate(states[parent], sample, RRT_EPS / d[j])
            new_state, free, done = env.step(states[parent], new_state)
        success = success or done
        # insert_new_state (search_tree.py:65-98)
        states.append(new_state)
        parents.append(parent)
        rewired.append(parent)
        by_rrt.append(0 if guided else 1)
        freesp.append(bool(free))
        in_goal.append(bool(done))
        path_lengths.append(path_lengths[-1])
        costs.append(-1.)
        if free and not done:
            non_terminal.append(len(states) - 1)
        value = model.pred_value(new_state)
        visits[parent] += 1
        visits.append(0)
        state_values.append(value)
        tree = np.array(states)
        w_sum -= w[parent]
        w[parent] = compute_w(tree, states[parent], dim)
        w_sum += w[parent]
        w.append(compute_w(tree, new_state, dim))
        w_sum += w[-1]
        rewire_last(env, goal, states, rewired, freesp, in_goal, costs, path_lengths, parent, stats)
        cum.append(int(env.collision_check_count))
        if success and stop_when_success:
            break
    # search_tree.path() (search_tree.py:30-47), as node ids
    path = []
    if in_goal[-1]:
        cur = len(states) - 1
        while True:
            path.append(cur)
            if cur == 0:
                break
            if len(path) > len(states):
                raise RuntimeError('next_plan.plan_host: rewired_parents hold a cycle (the reference would not return)')
            cur = rewired[cur]
        path.reverse()
    pts = np.array(states).reshape(-1, dim)
    ids = np.array(path, dtype=np.int64)
    return {'states': pts, 'parents': np.array(parents, dtype=np.int64), 'rewired_parents': np.array(rewired, dtype=np.int64),
            'freesp': np.array(freesp, dtype=bool), 'in_goal_region': np.array(in_goal, dtype=bool),
            'costs': np.array(costs, dtype=np.float64), 'path_lengths': np.array(path_lengths, dtype=np.float64),
            'cumulated_collision_checks': np.array(cum, dtype=np.int64), 'success': bool(success), 'i': int(i), 'path_ids': ids,
            'path': pts[ids], 'draws': int(pos), 'expanded_by_rrt': np.array(by_rrt, dtype=np.int8),
            'state_values': np.array(state_values, dtype=np.float32).reshape(-1), 'w': np.array(w, dtype=np.float64),
            'w_sum': float(w_sum), 'visits': np.array(visits, dtype=np.int64), 'stats': stats}
