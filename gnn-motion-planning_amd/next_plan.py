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

The device path (:func:`plan_maze_batch`, :func:`eval_next_device`; ``csrc/next_plan_kernels.hip``) runs the whole ``t_max`` loop
of a batch of problems in one launch, every problem on its own streams: the numpy doubles of ``RandomState(seed)`` and a block
of standard normal draws ``eps`` that replaces the global torch generator (:class:`NoiseModel` feeds the same block to
:func:`plan_host`).  No fallback: without the library the device calls raise.
"""
import numpy as np

from . import maze2d
from .rrtstar import (MODEL_EPS, RRT_EPS, TREE_TENSORS, distances, draws_per_problem, eval_aggregate, nearest_index, new_stats,
                      next_sample, rewire_last, sample_bounds, tied_minimum, tree_results)
from .streams_batch import RawDoubles, StageClock, check_stream_args, eval_chunks, problem_env, problem_tensors

G_EXPLORE_EPS = 0.1                    # eval_next.py:62 explore_eps
POLICY_STD = RRT_EPS * 0.3             # next_model/model2D.py: Model2D's std
K_MAX = 16                             # candidates of a guided step the device loop takes (include/gnnmp.h)

# status bits of a device problem (include/gnnmp.h, gnnmp_next_plan): those of gnnmp_rrtstar_plan plus
STATUS_EPS_SHORT, STATUS_SCORE_NOT_FINITE = 4, 8

TREE_FIELDS = ('states', 'parents', 'rewired_parents', 'expanded_by_rrt', 'freesp', 'in_goal_region', 'costs', 'path_lengths',
               'cumulated_collision_checks', 'visits', 'state_values', 'w', 'w_sum', 'success', 'i', 'path_ids', 'draws', 'guided')


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


def select_scores(non_terminal, state_values, w, w_sum, c):
    """tsa.py:141-165: the score of every non-terminal node."""
    return [state_values[idx] + c * np.sqrt(np.log(w_sum) / w[idx]) for idx in non_terminal]


def select(non_terminal, state_values, w, w_sum, c):
    """tsa.py:141-165: the index of the non-terminal node to expand."""
    return non_terminal[int(np.argmax(select_scores(non_terminal, state_values, w, w_sum, c)))]


def argmax_margin(scores):
    """The gap between the best and the second-best of ``scores`` (inf for a single one): how far an arg-max is from a tie."""
    if len(scores) < 2:
        return float('inf')
    top = np.partition(np.asarray(scores, dtype=np.float64), len(scores) - 2)[-2:]
    return float(top[1] - top[0])


def policy_scale(std=None, dim=2):
    """The float32 diagonal of the Cholesky factor of ``eye(dim) * std ** 2`` as ``MultivariateNormal`` forms it: what an
    action adds per unit of noise (0.015f at the default std)."""
    import torch
    std = POLICY_STD if std is None else std
    return np.float32(torch.linalg.cholesky(torch.eye(int(dim)) * std ** 2)[0, 0].item())


class NoiseModel:
    """``pred_value`` / ``policy`` over any ``Model2D`` (``net_forward``, ``pred_value``, ``std`` or ``var``) with the policy's
    noise GIVEN instead of drawn: call g of :meth:`policy` forms its k actions from row g of ``eps`` [rows, k, dim] as
    ``a_j = fl32(mean + fl32(scale * eps[g, j]))`` -- two float32 roundings, bit for bit what
    ``MultivariateNormal(mean, eye * std ** 2).sample()`` returns when ``eps[g, j]`` is that call's ``torch.randn(dim)``.  This
    is what lets :func:`plan_host` and the device loop consume the same noise.  ``priors`` are not formed (None)."""

    def __init__(self, model, eps):
        self.model = model
        self.eps = np.ascontiguousarray(np.asarray(eps.detach().cpu().numpy() if hasattr(eps, 'detach') else eps, dtype=np.float32))
        if self.eps.ndim != 3:
            raise ValueError('NoiseModel: eps is [rows, k, dim]')
        self.dim = int(self.eps.shape[2])
        var = getattr(model, 'var', None)
        if var is not None:
            import torch
            self.scale = np.float32(torch.linalg.cholesky(torch.as_tensor(var, dtype=torch.float32))[0, 0].item())
        else:
            self.scale = policy_scale(getattr(model, 'std', None), self.dim)
        self.row = 0

    def pred_value(self, states):
        return self.model.pred_value(states)

    def policy(self, state, k=1):
        if self.row >= self.eps.shape[0]:
            raise IndexError('NoiseModel: the eps block has %d rows, guided iteration %d asks for one more' % (self.eps.shape[0], self.row))
        if k > self.eps.shape[1]:
            raise ValueError('NoiseModel: k = %d, the eps block holds %d draws a row' % (k, self.eps.shape[1]))
        mean = np.asarray(self.model.net_forward(state)[0], dtype=np.float32).reshape(self.dim)
        noise = self.eps[self.row, :k]
        self.row += 1
        step = (self.scale * noise).astype(np.float32)
        actions = (mean[None, :] + step).astype(np.float32)
        return [a for a in actions], [None] * k


def plan_host(problem, seed, model, t_max=1000, g_explore_eps=G_EXPLORE_EPS, model_eps=MODEL_EPS, stop_when_success=True, c=1.0, k=10,
              raw=None):
    """One maze problem (a dict with ``map``, ``init_state``, ``goal_state``).  Returns the tree fields of
    :func:`gnnmp.rrtstar.plan_host` plus ``expanded_by_rrt`` (int8: 1 / 0, -1 for the root's None), ``state_values`` (float32),
    ``w``, ``w_sum``, ``visits`` and in ``stats`` also ``guided`` (guided iterations), ``guided_collided`` (those whose step
    collided), ``guided_success`` (those that reached the goal region), ``wraps`` (candidate steps that wrapped the angle) and
    ``min_margin`` (the smallest gap between the best and the second-best score over all ``select`` and ``expand`` arg-maxes:
    how far the run came to a tie that a last-bit difference in ``w`` could flip; inf when no arg-max had two entries).
    ``raw``: the problem's block of raw doubles instead of ``RandomState(seed).random_sample(...)``, as
    :func:`gnnmp.rrtstar.plan_host` takes it; the RRT branch counts the same exact ties."""
    env = problem_env(problem, 'rrtstar')
    dim = env.config_dim
    low, ranges = sample_bounds(dim)
    if raw is None:
        raw = np.random.RandomState(int(seed) & 0xffffffff).random_sample(draws_per_problem(t_max, dim))
    raw = np.asarray(raw, dtype=np.float64).reshape(-1)
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
    stats.update(guided=0, guided_collided=0, guided_success=0, wraps=0, min_margin=float('inf'))
    pos, success, i = 0, False, -1

    for i in range(int(t_max)):
        guided = raw[pos] >= model_eps and raw[pos + 1] >= g_explore_eps
        if guided:
            pos += 2
            scores = select_scores(non_terminal, state_values, w, w_sum, c)
            stats['min_margin'] = min(stats['min_margin'], argmax_margin(scores))
            parent = non_terminal[int(np.argmax(scores))]
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
                stats['min_margin'] = min(stats['min_margin'], argmax_margin(scores))
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
            j = nearest_index(d)
            parent = int(idx[j])
            tied, far = tied_minimum(d, idx)
            stats['nearest_ties'] += tied
            stats['nearest_ties_far'] += far
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


# --------------------------------------------------------------------------------------------------
# device path (libgnnmp.so, csrc/next_plan_kernels.hip).  No fallback: without the library every call raises.
# --------------------------------------------------------------------------------------------------
def max_nodes():
    """Trees of the device loop are capped at this many nodes (``t_max + 1``)."""
    from . import _lib
    return int(_lib.lib().gnnmp_next_plan_max_nodes())


def next_plan_device(maps, init64, goal64, draws, pb_rep, weights, eps, t_max, stop_when_success=True, g_explore_eps=G_EXPLORE_EPS,
                     c=1.0, k=None, scale=None):
    """``gnnmp_next_plan`` on device tensors: ``maps`` [B, 15, 15], ``init64`` / ``goal64`` [B, dim], ``draws``
    [B, draws_per_problem] raw doubles, all float64; ``pb_rep`` [B, 64, 15, 15], the packed ``weights`` and ``eps``
    [B, eps_rows, k, dim] float32.  One launch on the current stream; returns the device tensors of ``gnnmp_next_plan_tree`` as a
    dict (the six per-problem words of RRT* as rows of ``small``, then ``guided`` as row 6).  Nothing is read back."""
    import ctypes
    import torch
    from . import _lib
    dev = maps.device
    B, dim, T1 = int(maps.shape[0]), int(init64.shape[1]), int(t_max) + 1
    if eps.dim() != 4 or int(eps.shape[0]) != B or int(eps.shape[3]) != dim:
        raise ValueError('next_plan_device: eps is [B, eps_rows, k, dim]')
    k = int(eps.shape[2]) if k is None else int(k)
    if k != int(eps.shape[2]):
        raise ValueError('next_plan_device: eps holds %d draws a row, k = %d' % (int(eps.shape[2]), k))
    if tuple(pb_rep.shape) != (B, 64, 15, 15):
        raise ValueError('next_plan_device: pb_rep is [B, 64, 15, 15]')
    scale = policy_scale(None, dim) if scale is None else scale
    maps, init64, goal64, draws = maps.contiguous(), init64.contiguous(), goal64.contiguous(), draws.contiguous()
    pb_rep, weights, eps = pb_rep.contiguous(), weights.contiguous(), eps.contiguous()
    for name, t, dt in (('maps', maps, torch.float64), ('init64', init64, torch.float64), ('goal64', goal64, torch.float64),
                        ('draws', draws, torch.float64), ('pb_rep', pb_rep, torch.float32), ('weights', weights, torch.float32),
                        ('eps', eps, torch.float32)):
        if t.dtype != dt or t.device != dev:
            raise ValueError('next_plan_device: %s must be %s on %s' % (name, dt, dev))
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=dev)      # noqa: E731
    out = {'states': new(torch.float64, B, T1, dim), 'parents': new(torch.int32, B, T1), 'rewired_parents': new(torch.int32, B, T1),
           'flags': new(torch.uint8, B, T1), 'costs': new(torch.float64, B, T1), 'path_lengths': new(torch.float64, B, T1),
           'cumulated_checks': new(torch.int64, B, T1), 'path': new(torch.int32, B, T1), 'small': new(torch.int32, 7, B),
           'expanded_by_rrt': new(torch.int8, B, T1), 'state_values': new(torch.float32, B, T1), 'w': new(torch.float64, B, T1),
           'visits': new(torch.int32, B, T1), 'w_sum': new(torch.float64, B)}
    batch = _lib.NextPlanBatch(B, dim, int(maps.shape[1]), int(t_max), 1 if stop_when_success else 0, int(draws.shape[1]),
                               maps.data_ptr(), init64.data_ptr(), goal64.data_ptr(), draws.data_ptr(), float(g_explore_eps), float(c), k,
                               int(eps.shape[1]), float(scale), pb_rep.data_ptr(), weights.data_ptr(), eps.data_ptr() or None)
    tree = _lib.NextPlanTree(*(out[key].data_ptr() for key in TREE_TENSORS), *(out['small'][r].data_ptr() for r in range(6)),
                             *(out[key].data_ptr() for key in ('expanded_by_rrt', 'state_values', 'w', 'visits', 'w_sum')),
                             out['small'][6].data_ptr())
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gnnmp_next_plan(ctypes.byref(batch), ctypes.byref(tree), torch.cuda.current_stream(dev).cuda_stream),
                   'gnnmp_next_plan')
    return out


def default_eps(seeds, t_max, k, dim):
    """The project's per-problem noise stream: ``eps[i] = torch.randn(t_max, k, dim, generator=Generator().manual_seed(seeds[i]))``
    on the CPU generator."""
    import torch
    return torch.stack([torch.randn(int(t_max), int(k), int(dim), generator=torch.Generator().manual_seed(int(s) & 0xffffffff))
                        for s in seeds])


def plan_maze_batch(problems, device, seeds, net, t_max=1000, stop_when_success=True, draws='host', eps=None, timings=None,
                    g_explore_eps=G_EXPLORE_EPS, c=1.0, k=10, std=None, check=True, streams_out=None):
    """NEXT's guided planner for many maze problems at once (point robot or stick robot, by the width of ``init_state``), every
    problem on its OWN streams: problem i computes what ``plan_host(problems[i], seeds[i], NoiseModel(model, eps[i]), ...)``
    computes with ``model`` the device ``Model2D`` of ``net`` (a loaded :class:`gnnmp.next_model.NextNet`) -- whatever other
    problems are in the batch, in whatever order or chunks.  ``pb_forward`` runs for the batch, then the whole ``t_max`` loop of
    all problems is one launch (``gnnmp_next_plan``); the host only sets up and reads the trees back.

    ``draws``: ``'host'`` -- one ``RandomState(seed).random_sample`` block of ``t_max * (2 + dim)`` raw doubles per problem,
    copied once; ``'device'`` -- :class:`gnnmp.rng.MTStreams` fills the blocks and the streams are then advanced by the
    kernel's ``used`` counts, so their state afterwards is numpy's after the plan (``streams_out`` receives the object).
    ``eps`` [B, rows, k, dim]: the standard normal draws of the policy, row g for a problem's g-th guided iteration; default
    :func:`default_eps`, ``torch.randn(t_max, k, dim)`` from a generator seeded with ``seeds[i]``.  This is the PROJECT's
    per-problem stream: it is NOT ``eval_next``'s global torch generator, which runs through all problems and depends on their
    order (other draws of the same distribution).

    Returns one dict per problem with :func:`plan_host`'s fields (``guided`` at the top level instead of ``stats``) plus
    ``status``.  ``net.check_status()`` and, with ``check``, a non-zero status word raise."""
    import torch
    from .next_model import NextNet
    who = 'next_plan.plan_maze_batch'
    B, t_max = len(problems), int(t_max)
    if B == 0:
        return []
    check_stream_args(B, seeds, draws, who)
    if t_max < 1 or t_max + 1 > max_nodes():
        raise ValueError('next_plan.plan_maze_batch: t_max is 1 .. %d (the device loop keeps the tree in LDS)' % (max_nodes() - 1))
    if not isinstance(net, NextNet):
        raise TypeError('next_plan.plan_maze_batch: net is a loaded gnnmp.next_model.NextNet')
    dev = torch.device(device)
    with torch.cuda.device(dev):
        dim, maps, init64, goal64 = problem_tensors(problems, dev, who)
    if dim != net.dim:
        raise ValueError('next_plan.plan_maze_batch: dim %d problems, a dim %d network' % (dim, net.dim))
    if eps is None:
        eps = default_eps(seeds, t_max, k, dim)
    eps = torch.as_tensor(eps, dtype=torch.float32)
    if eps.dim() != 4 or int(eps.shape[0]) != B or int(eps.shape[2]) != int(k) or int(eps.shape[3]) != dim:
        raise ValueError('next_plan.plan_maze_batch: eps is [B, rows, k, dim]')
    clock = StageClock(timings)
    with torch.cuda.device(dev):
        eps_dev = eps.to(dev).contiguous()
        pb_rep = net.pb_forward(maps.to(torch.float32), goal64.to(torch.float32))
        clock.mark('pb_forward')
        block = RawDoubles(seeds, draws_per_problem(t_max, dim), dev, draws)
        clock.mark('draws')
        out = next_plan_device(maps, init64, goal64, block.raw, pb_rep, net._weights(dev), eps_dev, t_max, stop_when_success,
                               g_explore_eps, c, int(k), policy_scale(std, dim))
        block.finish(out['small'][3], streams_out)                       # by the doubles each problem consumed
        clock.mark('plan')
        small = out['small'].cpu().numpy()
        status, guided = small[5], small[6]
        net.check_status()
        if check and status.any():
            bad = np.flatnonzero(status)
            raise RuntimeError('gnnmp_next_plan: status %s for problem(s) %s (1 = draw block too short, 2 = cycle in rewired_parents, '
                               '4 = eps block too short, 8 = a score was not finite)' % (status[bad].tolist(), bad.tolist()))
        host = {key: out[key].cpu().numpy() for key in TREE_TENSORS + ('expanded_by_rrt', 'state_values', 'w', 'visits', 'w_sum')}
    res = tree_results(host, small)
    for b, r in enumerate(res):
        n = r['states'].shape[0]
        r.update(expanded_by_rrt=host['expanded_by_rrt'][b, :n].copy(), state_values=host['state_values'][b, :n].copy(),
                 w=host['w'][b, :n].copy(), w_sum=float(host['w_sum'][b]), visits=host['visits'][b, :n].astype(np.int64),
                 guided=int(guided[b]))
    clock.mark('results')
    return res


def eval_next_device(env, indexes, net, seed=1234, seeds=None, t_max=1000, device='cuda', chunk=1024, rows_out=None, timings=None,
                     draws='host'):
    """The tuple of the reference's ``eval_next`` (eval_next.py:47-88) without its wall-clock entries, from
    :func:`plan_maze_batch` with ``stop_when_success=True``, ``chunk`` problems per launch: ``(n_success, collision,
    solution_cost, paths)`` through :func:`gnnmp.rrtstar.eval_aggregate`, with the same first-iteration quirk of ``collision``;
    ``paths`` are the float64 states of ``search_tree.path()``.  Problem ``indexes[i]`` draws from ``RandomState(seeds[i])`` and
    from :func:`default_eps` of ``seeds[i]``; default :func:`gnnmp.streams_batch.stream_seeds`.  The numbers DIFFER from
    ``eval_next``'s, which walks ONE global numpy stream and ONE global torch stream problem after problem -- other samples of
    the same distributions -- and in exchange they do not depend on the order of ``indexes`` or on ``chunk``.  ``rows_out``: a
    list that receives per problem (success, checks with the quirk, path_lengths[-1], nodes, last iteration, guided)."""
    results = []
    for pr, chunk_seeds in eval_chunks(env, indexes, seed, seeds, chunk):
        results.extend(plan_maze_batch(pr, device, chunk_seeds, net, t_max=t_max, stop_when_success=True, draws=draws, timings=timings))
    if rows_out is not None:
        rows_out.extend((int(r['success']), int(r['cumulated_collision_checks'][-1]) - int(r['cumulated_collision_checks'][1]),
                         float(r['path_lengths'][-1]), r['states'].shape[0], r['i'], r['guided']) for r in results)
    return eval_aggregate(results) + ([r['path'] for r in results],)
