"""RRT* on maze problems: the sampling-based comparison baseline of the GNN explorer -- the reference's ``eval_rrt.py`` row, which
calls ``NEXT_plan(env, model=None, T=t_max, g_explore_eps=1., stop_when_success=True)`` (``algorithm/tsa.py:12-139, 222-281`` over
``algorithm/search_tree.py:5-98`` and ``environment/maze_env.py:127-208, 266-347``): a goal-biased RRT with RRT*-style rewiring
of the newest node.  Restated on the host (:func:`plan_host`, numpy only) and run for whole batches on the device
(:func:`plan_maze_batch`, :func:`eval_rrt_device`; ``csrc/rrtstar_kernels.hip``, the whole ``t_max`` loop in one launch).

Semantics.  Problem i behaves as ``np.random.seed(seeds[i]); env.init_new_problem(idx_i); NEXT_plan(env, model=None, ...)`` does:
one sample stream PER PROBLEM, the convention of :mod:`gnnmp.lazysp` and :func:`gnnmp.planner.plan_maze_rounds_batch`.  The
reference's ``eval_rrt`` seeds once globally and runs the problems one after another through that one stream; that form is NOT
reproduced (other samples of the same distribution), in exchange a problem's result does not depend on the other problems, on
their order or on how a batch is cut.

  * an iteration draws one ``rand()``; below ``model_eps = 0.05`` the sample is the goal state and nothing else is drawn,
    otherwise a second ``rand()`` is drawn and dropped (``< g_explore_eps = 1.`` always holds) and ``uniform_sample()`` draws
    ``dim`` doubles as ``low + (high - low) * d``: 1 or 2 + dim doubles an iteration (tsa.py:47-56, maze_env.py:127-135).
  * nearest neighbour over the NON-TERMINAL nodes (free and not in the goal region), first minimum = lowest index; the new state
    is the sample itself within RRT_EPS, else ``interpolate(nearest, sample, RRT_EPS / dist)`` (tsa.py:83-139).
  * ``env.step``: clip / wrap, the counted edge query, and only for a free edge the goal test, which counts one more
    ``_state_fp`` within RRT_EPS of the goal (maze_env.py:181-208).  EVERY new state joins the tree, collided ones too.
  * ``RRTS_rewire_last``: a collided newest node gets cost 2; otherwise the cheapest free neighbour within 3 RRT_EPS whose edge
    is free becomes its parent (running minimum, index order), then every neighbour -- collided ones included, their cost is 2
    -- that the new node would improve is checked and rewired; descendants' costs are not updated (tsa.py:222-281).
"""
import numpy as np

from . import maze2d
from .streams_batch import RawDoubles, StageClock, check_stream_args, eval_chunks, maze_class, problem_env, problem_tensors, sample_limits

MODEL_EPS = 0.05                       # tsa.py:13 model_eps: the goal bias
RRT_EPS = maze2d.RRT_EPS               # steering step and goal radius
NEIGHBOR_R = RRT_EPS * 3               # tsa.py:234 (0.15000000000000002, as the reference computes it)
OBS_COST = 2                           # tsa.py:222 obs_cost

# status bits of a device problem (include/gnnmp.h, gnnmp_rrtstar_plan)
STATUS_DRAWS_SHORT, STATUS_PATH_BOUND = 1, 2

TREE_FIELDS = ('states', 'parents', 'rewired_parents', 'freesp', 'in_goal_region', 'costs', 'path_lengths',
               'cumulated_collision_checks', 'success', 'i', 'path_ids', 'draws')
# the per-node arrays of a device tree (include/gnnmp.h, gnnmp_rrtstar_tree), in the struct's order
TREE_TENSORS = ('states', 'parents', 'rewired_parents', 'flags', 'costs', 'path_lengths', 'cumulated_checks', 'path')


def draws_per_problem(t_max, dim):
    """Doubles that ``t_max`` iterations can consume at most: 2 + dim each."""
    return int(t_max) * (2 + int(dim))


def sample_bounds(dim):
    """(low, high - low) of ``uniform_sample`` (maze_env.py:131)."""
    limits = sample_limits(dim, 'rrtstar')
    return -limits, limits - (-limits)


def next_sample(raw, pos, goal_state, low, ranges):
    """The sample of one iteration from the raw doubles ``raw[pos:]`` of the problem's stream -> (sample, new pos):
    ``rand() < model_eps`` -> the goal state, 1 double; else one more ``rand()`` dropped and ``uniform_sample()``'s
    ``low + (high - low) * d`` (tsa.py:47-56)."""
    if raw[pos] < MODEL_EPS:
        return np.array(goal_state, dtype=np.float64), pos + 1
    dim = low.shape[0]
    return low + raw[pos + 2:pos + 2 + dim] * ranges, pos + 2 + dim


def distances(states, to_state, dim):
    """``env.distance(states, to_state)`` for rows of states (maze_env.py:137-149): the orientation gap the short way round,
    ``sqrt((dx^2 + dy^2) + dz^2)``."""
    gap = np.abs(to_state - np.atleast_2d(states))
    if dim == 3:
        gap[:, 2] = np.minimum(gap[:, 2], np.abs(gap[:, 2] - maze2d.Maze3D.ORIENT_PERIOD))
    return np.sqrt(np.sum(gap ** 2, axis=-1))


def nearest_index(d):
    """``np.argmin(dists)`` of ``global_explore`` (tsa.py:129): the FIRST minimum, so among equidistant non-terminal nodes the
    lowest id.  (Module level, like the two tests below, so that a test can swap in another rule.)"""
    return int(np.argmin(d))


def parent_improves(cost_new, min_cost):
    """Pass 1 of ``RRTS_rewire_last`` (tsa.py:256): a STRICT ``cost_new < min_cost`` against the running minimum -- of two
    equally cheap parents the earlier one stays, and the later one's edge is not even checked."""
    return cost_new < min_cost


def neighbor_improves(cost_new, cost_j):
    """Pass 2 of ``RRTS_rewire_last`` (tsa.py:271): a STRICT ``cost_new < costs[j]`` -- a neighbour the new node would reach at
    exactly its present cost keeps its parent, unchecked."""
    return cost_new < cost_j


def tied_minimum(d, ids):
    """(tied, far) for the distances ``d`` of the nodes ``ids`` (ascending): more than one node holds the minimum; two of
    them have ids 64 or more apart (they belong to different strides of a 64-lane scan)."""
    tied = np.asarray(ids)[np.asarray(d) == np.min(d)]
    return len(tied) > 1, bool(len(tied) > 1 and tied[-1] - tied[0] >= 64)


def rewire_last(env, goal, states, rewired, freesp, in_goal, costs, path_lengths, nearest, stats):
    """``RRTS_rewire_last`` (tsa.py:222-281) on the tree lists, whose last entries are the node just inserted from ``nearest``:
    sets its cost (and ``path_lengths[-1]`` when it is in the goal region), rewires it and then its neighbours, in place.
    ``stats`` counts as :func:`plan_host` describes."""
    dim = env.config_dim
    new_state, free = states[-1], freesp[-1]

    def rewire_step(j):                      # env.step(cur_tree[j], new_state) inside RRTS_rewire_last
        if dim == 3:
            stats['max_rewire_k'] = max(stats['max_rewire_k'], int(distances(states[j], new_state, dim)[0] / 0.015))
        _, free_j, _ = env.step(states[j], new_state)
        if free_j and distances(new_state, goal, dim)[0] < RRT_EPS:
            stats['goal_rechecks'] += 1
        return free_j

    if not free:
        costs[-1] = float(OBS_COST)
        return
    tree = np.array(states[:-1])
    dists = distances(tree, new_state, dim)
    near = np.flatnonzero(dists < NEIGHBOR_R)
    n_coll = int(sum(not freesp[j] for j in near))
    stats['max_near'] = max(stats['max_near'], len(near))
    if len(near) > 64:
        stats['max_near_collided'] = max(stats['max_near_collided'], n_coll)
    min_cost, min_j = dists[nearest] + costs[nearest], nearest
    first_group = None                       # the group of 64 ids that held the first improvement
    for j in near:
        if not freesp[j]:
            continue
        cost_new = dists[j] + costs[j]
        if cost_new == min_cost and j != min_j:
            stats['parent_ties'] += 1
            stats['parent_ties_late'] += first_group is not None and j // 64 > first_group
        if parent_improves(cost_new, min_cost) and rewire_step(j):
            min_cost, min_j = cost_new, int(j)
            if first_group is None:
                first_group = j // 64
    rewired[-1] = min_j
    costs[-1] = float(min_cost)
    if in_goal[-1] and (path_lengths[-1] < 0 or path_lengths[-1] > min_cost):      # set_cost (search_tree.py:56-63)
        path_lengths[-1] = float(min_cost)
    for j in near:
        cost_new = min_cost + dists[j]
        if cost_new == costs[j]:
            stats['rewire_ties'] += 1
        if neighbor_improves(cost_new, costs[j]):
            if not freesp[j]:
                stats['collided_second_pass'] += 1
            if rewire_step(j):
                costs[j] = float(cost_new)
                rewired[j] = len(states) - 1
                stats['rewired'] += 1


def new_stats():
    return dict(direct_steer=0, collided_second_pass=0, goal_rechecks=0, rewired=0, max_near=0, max_near_collided=0, max_rewire_k=0,
                nearest_ties=0, nearest_ties_far=0, parent_ties=0, parent_ties_late=0, rewire_ties=0)


def plan_host(problem, seed, t_max=1000, stop_when_success=True, raw=None):
    """``np.random.seed(seed); NEXT_plan(env, model=None, T=t_max, g_explore_eps=1., stop_when_success=...)`` for one maze
    problem (a dict with ``map``, ``init_state``, ``goal_state``; 2 coordinates = point robot, 3 = stick robot) on a private
    ``RandomState``.  Returns the whole search tree as a dict: ``states`` [n, dim] float64 (n = iterations run + 1: collided new
    states are stored too), ``parents`` / ``rewired_parents`` int64 (-1 for the root's None), ``freesp`` / ``in_goal_region``
    bool, ``costs`` / ``path_lengths`` float64, ``cumulated_collision_checks`` int64 (all [n]), ``success``, ``i`` (index of
    the last iteration run), ``path_ids`` (``search_tree.path()``: root -> last node along ``rewired_parents``, empty unless
    the last node is in the goal region), ``path`` (their states) and ``draws`` (doubles taken from the stream).  ``stats``
    counts what tests aim at: ``direct_steer`` iterations whose sample was within RRT_EPS of the tree, ``collided_second_pass``
    second-pass checks on collided neighbours, ``goal_rechecks`` goal tests inside rewiring that counted a ``_state_fp``,
    ``rewired`` nodes whose parent was changed, ``max_near`` / ``max_near_collided`` neighbours (collided ones) of one
    iteration and ``max_rewire_k`` interpolated sticks of one rewiring check.  Exact ties, which random doubles never give and
    a lattice of draws gives all the time: ``nearest_ties`` iterations whose least distance is held by more than one
    non-terminal node (``nearest_ties_far``: by nodes with ids 64 or more apart), ``parent_ties`` free near nodes other than
    the present best parent with ``cost_new == min_cost`` in pass 1 (``parent_ties_late``: those in a later group of 64 ids than
    the call's first improvement, where a running minimum and one frozen at the start of the group differ), ``rewire_ties`` near nodes with ``cost_new == costs[j]``
    in pass 2.  ``raw``: the problem's block of raw doubles (``draws_per_problem`` of them) instead of
    ``RandomState(seed).random_sample(...)``; ``seed`` is not used then."""
    env = problem_env(problem, 'rrtstar')
    dim = env.config_dim
    low, ranges = sample_bounds(dim)
    if raw is None:
        raw = np.random.RandomState(int(seed) & 0xffffffff).random_sample(draws_per_problem(t_max, dim))
    else:
        raw = np.asarray(raw, dtype=np.float64).reshape(-1)
        if raw.shape[0] < draws_per_problem(t_max, dim):
            raise ValueError('rrtstar.plan_host: raw holds %d doubles, %d iterations can draw %d'
                             % (raw.shape[0], t_max, draws_per_problem(t_max, dim)))
    goal = np.asarray(env.goal_state, dtype=np.float64).reshape(dim)
    # search_tree.py:5-19
    states = [np.asarray(env.init_state, dtype=np.float64).reshape(dim).copy()]
    parents, rewired, freesp, in_goal, costs, path_lengths, cum = [-1], [-1], [True], [False], [0.], [-1.], [0]
    stats = new_stats()
    pos, success, i = 0, False, -1

    for i in range(int(t_max)):
        sample, pos = next_sample(raw, pos, goal, low, ranges)
        # global_explore (tsa.py:121-139)
        idx = np.flatnonzero(np.array(freesp) & ~np.array(in_goal))
        d = distances(np.array(states)[idx], sample, dim)
        k = nearest_index(d)
        nearest = int(idx[k])
        tied, far = tied_minimum(d, idx)
        stats['nearest_ties'] += tied
        stats['nearest_ties_far'] += far
        if d[k] < RRT_EPS:                   # RRT_steer (tsa.py:97-101)
            new_state = sample
            stats['direct_steer'] += 1
        else:
            new_state = env.interpolate(states[nearest], sample, RRT_EPS / d[k])
        new_state, free, done = env.step(states[nearest], new_state)
        success = success or done
        # insert_new_state (search_tree.py:65-81)
        states.append(new_state)
        parents.append(nearest)
        rewired.append(nearest)
        freesp.append(bool(free))
        in_goal.append(bool(done))
        path_lengths.append(path_lengths[-1])
        costs.append(-1.)
        rewire_last(env, goal, states, rewired, freesp, in_goal, costs, path_lengths, nearest, stats)
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
                raise RuntimeError('rrtstar.plan_host: rewired_parents hold a cycle (the reference would not return)')
            cur = rewired[cur]
        path.reverse()
    pts = np.array(states).reshape(-1, dim)
    ids = np.array(path, dtype=np.int64)
    return {'states': pts, 'parents': np.array(parents, dtype=np.int64), 'rewired_parents': np.array(rewired, dtype=np.int64),
            'freesp': np.array(freesp, dtype=bool), 'in_goal_region': np.array(in_goal, dtype=bool),
            'costs': np.array(costs, dtype=np.float64), 'path_lengths': np.array(path_lengths, dtype=np.float64),
            'cumulated_collision_checks': np.array(cum, dtype=np.int64), 'success': bool(success), 'i': int(i), 'path_ids': ids,
            'path': pts[ids], 'draws': int(pos), 'stats': stats}


# --------------------------------------------------------------------------------------------------
# device path (libgnnmp.so, csrc/rrtstar_kernels.hip).  No fallback: without the library every call raises.
# --------------------------------------------------------------------------------------------------
def lds_nodes():
    """Trees of up to this many nodes (``t_max + 1``) keep their node state in LDS; longer runs use the workspace."""
    from . import _lib
    return int(_lib.lib().gnnmp_rrtstar_lds_nodes())


def rrtstar_plan(maps, init64, goal64, draws, t_max, stop_when_success=True):
    """``gnnmp_rrtstar_plan`` on device tensors: ``maps`` [B, w, w], ``init64`` / ``goal64`` [B, dim], ``draws``
    [B, draws_per_problem] raw doubles, all float64.  One launch on the current stream; returns the device tensors of
    ``gnnmp_rrtstar_tree`` as a dict (the six per-problem words as rows of ``small``: n_nodes, success, last_iter, used,
    path_len, status).  Nothing is read back."""
    import ctypes
    import torch
    from . import _lib
    dev = maps.device
    B, dim, T1 = int(maps.shape[0]), int(init64.shape[1]), int(t_max) + 1
    maps, init64, goal64, draws = maps.contiguous(), init64.contiguous(), goal64.contiguous(), draws.contiguous()
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=dev)      # noqa: E731
    out = {'states': new(torch.float64, B, T1, dim), 'parents': new(torch.int32, B, T1), 'rewired_parents': new(torch.int32, B, T1),
           'flags': new(torch.uint8, B, T1), 'costs': new(torch.float64, B, T1), 'path_lengths': new(torch.float64, B, T1),
           'cumulated_checks': new(torch.int64, B, T1), 'path': new(torch.int32, B, T1), 'small': new(torch.int32, 6, B)}
    L = _lib.lib()
    need = ctypes.c_size_t()
    _lib.check(L.gnnmp_rrtstar_workspace_bytes(B, int(t_max), ctypes.byref(need)), 'gnnmp_rrtstar_workspace_bytes')
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev) if need.value else None
    batch = _lib.RRTStarBatch(B, dim, int(maps.shape[1]), int(t_max), 1 if stop_when_success else 0, int(draws.shape[1]),
                              maps.data_ptr(), init64.data_ptr(), goal64.data_ptr(), draws.data_ptr())
    tree = _lib.RRTStarTree(*(out[k].data_ptr() for k in TREE_TENSORS), *(out['small'][r].data_ptr() for r in range(6)))
    with torch.cuda.device(dev):
        _lib.check(L.gnnmp_rrtstar_plan(ctypes.byref(batch), ctypes.byref(tree), ws.data_ptr() if ws is not None else None,
                                        need.value, torch.cuda.current_stream(dev).cuda_stream), 'gnnmp_rrtstar_plan')
    out['workspace'] = ws
    return out


def plan_maze_batch(problems, device, seeds, t_max=1000, stop_when_success=True, draws='host', timings=None, streams_out=None):
    """RRT* for many maze problems at once (point robot or stick robot, by the width of ``init_state``), every problem on its
    OWN sample stream: problem i computes what :func:`plan_host` -- ``np.random.seed(seeds[i]); NEXT_plan(env, model=None,
    ...)`` of that problem alone -- computes, whatever other problems are in the batch, in whatever order or chunks.  The whole
    ``t_max`` loop of all problems is one launch (``gnnmp_rrtstar_plan``); the host only sets up and reads the trees back.

    ``draws``: ``'host'`` -- one ``RandomState(seed).random_sample`` block of ``t_max * (2 + dim)`` raw doubles per problem,
    copied once; ``'device'`` -- :class:`gnnmp.rng.MTStreams` fills the blocks without a commit and the streams are then
    advanced by the kernel's ``used`` counts, so their state afterwards is numpy's after the plan (``streams_out``: a list
    that receives the :class:`MTStreams` object).  Returns one dict per problem with :func:`plan_host`'s tree fields plus
    ``status`` (0 = fine; a non-zero one raises)."""
    import torch
    who = 'rrtstar.plan_maze_batch'
    B, t_max = len(problems), int(t_max)
    if B == 0:
        return []
    check_stream_args(B, seeds, draws, who)
    if t_max < 1:
        raise ValueError('rrtstar.plan_maze_batch: t_max >= 1')
    dev = torch.device(device)
    clock = StageClock(timings)
    with torch.cuda.device(dev):
        dim, maps, init64, goal64 = problem_tensors(problems, dev, who)
        maze_class(dim, 'rrtstar')
        block = RawDoubles(seeds, draws_per_problem(t_max, dim), dev, draws)
        clock.mark('draws')
        out = rrtstar_plan(maps, init64, goal64, block.raw, t_max, stop_when_success)
        block.finish(out['small'][3], streams_out)                       # by the doubles each problem consumed
        clock.mark('plan')
        small = out['small'].cpu().numpy()
        status = small[5]
        if status.any():
            bad = np.flatnonzero(status)
            raise RuntimeError('gnnmp_rrtstar_plan: status %s for problem(s) %s (1 = draw block too short, 2 = cycle in rewired_parents)'
                               % (status[bad].tolist(), bad.tolist()))
        host = {k: out[k].cpu().numpy() for k in TREE_TENSORS}
    res = tree_results(host, small)
    clock.mark('results')
    return res


def tree_results(host, small):
    """One dict per problem with :func:`plan_host`'s tree fields plus ``status``, from the host copies ``host`` of the device
    tree (:data:`TREE_TENSORS`, ``[B, t_max + 1, ...]``) and its per-problem words ``small`` (rows n_nodes, success,
    last_iter, used, path_len, status)."""
    n_nodes, success, last_i, used, plen, status = small[:6]
    res = []
    for b in range(len(n_nodes)):
        n = int(n_nodes[b])
        pts = host['states'][b, :n].copy()
        ids = host['path'][b, :plen[b]].astype(np.int64)
        flags = host['flags'][b, :n]
        res.append({'states': pts, 'parents': host['parents'][b, :n].astype(np.int64),
                    'rewired_parents': host['rewired_parents'][b, :n].astype(np.int64), 'freesp': (flags & 1).astype(bool),
                    'in_goal_region': (flags & 2).astype(bool), 'costs': host['costs'][b, :n].copy(),
                    'path_lengths': host['path_lengths'][b, :n].copy(),
                    'cumulated_collision_checks': host['cumulated_checks'][b, :n].copy(), 'success': bool(success[b]),
                    'i': int(last_i[b]), 'path_ids': ids, 'path': pts[ids], 'draws': int(used[b]), 'status': int(status[b])})
    return res


def eval_aggregate(results):
    """``eval_rrt``'s aggregates (eval_rrt.py:43-48) of per-problem trees -> (n_success, collision, solution_cost):
    ``collision`` is the mean of ``cumulated_collision_checks[-1] - cumulated_collision_checks[1]`` -- the reference's quirk:
    entry 1 is the count after the FIRST iteration, so that iteration's checks are subtracted (entry 0 is the root's 0);
    ``solution_cost`` the mean ``path_lengths[-1]`` of the solved problems (nan when none is solved)."""
    n_success = int(sum(bool(r['success']) for r in results))
    collision = float(np.mean([int(r['cumulated_collision_checks'][-1]) - int(r['cumulated_collision_checks'][1]) for r in results]))
    solved = [float(r['path_lengths'][-1]) for r in results if r['success']]
    return n_success, collision, float(np.mean(solved)) if solved else float('nan')


def eval_rrt_device(env, indexes, seed=1234, seeds=None, t_max=1000, device='cuda', chunk=1024, rows_out=None, timings=None,
                    draws='host'):
    """The tuple of the reference's ``eval_rrt`` (eval_rrt.py:21-58) without its wall-clock entries, from
    :func:`plan_maze_batch` with ``stop_when_success=True``, ``chunk`` problems per launch: ``(n_success, collision,
    solution_cost, paths)`` -- see :func:`eval_aggregate` for the first-iteration quirk of ``collision``; ``paths`` are the
    float64 states of ``search_tree.path()``.  Problem ``indexes[i]`` draws from ``np.random.RandomState(seeds[i])``; default
    :func:`gnnmp.streams_batch.stream_seeds`.  The numbers DIFFER from ``eval_rrt``'s, which walks ONE global stream problem after
    problem -- other samples of the same distribution -- and in exchange they do not depend on the order of ``indexes`` or on
    ``chunk``.  ``rows_out``: a list that receives per problem (success, checks with the quirk, path_lengths[-1], nodes,
    last iteration).  The global numpy generator is left alone."""
    results = []
    for pr, chunk_seeds in eval_chunks(env, indexes, seed, seeds, chunk):
        results.extend(plan_maze_batch(pr, device, chunk_seeds, t_max=t_max, stop_when_success=True, draws=draws, timings=timings))
    if rows_out is not None:
        rows_out.extend((int(r['success']), int(r['cumulated_collision_checks'][-1]) - int(r['cumulated_collision_checks'][1]),
                         float(r['path_lengths'][-1]), r['states'].shape[0], r['i']) for r in results)
    return eval_aggregate(results) + ([r['path'] for r in results],)
