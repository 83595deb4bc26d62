"""BIT* on maze problems: the fourth row of the reference's evaluation (``eval_bit.eval_bit``), which calls
``BITStar(env, batch_size=batch, T=t_max, sampling=None).plan(INF, time_budget=300, refine_time_budget=0)`` and then
``get_best_path()`` (``algorithm/bit_star.py:18-334`` over ``environment/maze_env.py:236-347``).  Restated on the host
(:func:`plan_host`, numpy only) and run for whole batches on the device (:func:`plan_maze_batch`, :func:`eval_bit_device`;
``csrc/bitstar_kernels.hip``: the sampling of all batches in one launch, the whole search in a second one).

Semantics.  Problem i behaves as ``np.random.seed(seeds[i]); env.init_new_problem(idx_i); BITStar(...).plan(...)`` does: one
sample stream PER PROBLEM, the convention of :mod:`gnnmp.lazysp` and :mod:`gnnmp.rrtstar`.  The reference's ``eval_bit`` seeds
once globally and runs the problems one after another through that one stream; that form is NOT reproduced (other samples of
the same distribution), in exchange a problem's result does not depend on the other problems, on their order or on how a batch
is cut.

What is reproduced is the search for the FIRST solution: ``refine_time_budget=0`` ends the loop at the end of the iteration
that gives the goal a finite cost, so ``c_best`` is infinite at every sampling call, ``prune`` removes nothing and the
ellipsoid sampler is never reached.  Refinement (``refine_time_budget > 0``, pruning with a finite bound, ``sample_unit_ball``)
and the wall-clock budgets (``time_budget=300`` is taken never to bind) are NOT reproduced.

  * points are ids into one array: row 0 the start, row 1 the goal, then the free draws in order.  A draw is ``bounds[:, 0] +
    np.random.random(dim) * ranges`` and goes through ``_state_fp``, whose collision checks count; a rejected draw adds 1 to
    ``n_collision_points``.
  * a batch is drawn only when both queues are empty: ``batch`` free draws, ``T += batch``, every vertex pushed with value
    ``g(v) + d(v, goal)``, ``old_vertices`` = the vertices of that moment, and ``r = radius_init() * (log(q) / q) ** (1 / dim)``
    with ``q = 2 + batches * batch`` (:func:`radius_by_batch`: the host computes it, the device only reads a table).
  * while the best vertex value is ``<=`` the best edge value (``inf`` for an empty queue) the best vertex is expanded: an edge
    ``(v, x)`` with value ``(g(v) + d(v, x)) + d(x, goal)`` for every sample within ``r``, and, unless ``v`` is an old vertex,
    for every vertex ``w`` within ``r`` with ``edges.get(w) != v`` and ``g(v) + d(v, w) < g(w)``.  Both queues empty: the
    reference's ``heappop`` raises, the ``except`` continues, the next batch is drawn.
  * the best edge is popped and checked with ``_edge_fp`` (counted); ``g(v) + c < g(x)`` (strict) sets ``g(x)`` and the parent,
    moves a sample to the end of ``vertices`` and onto the vertex queue, and removes every queued edge whose target is ``x``
    (the filter's second clause, ``g(a) + h(a, b) < g(a)``, never holds).  Descendants' costs are not updated.
  * ``heapq`` compares ``(value, point)`` and ``(value, (point, neighbor))`` tuples: smaller value, then the source's
    coordinates lexicographically, then the target's -- a total order, whatever the heap's layout.
  * the loop test ``T < t_max`` stands at the top of every iteration, so the iteration that draws the last batch still pops
    one edge, and ``T`` may end above ``t_max``.
  * ``distance`` is ``np.linalg.norm(a - b)`` in all ``dim`` coordinates (no wrap of the stick's angle).
"""
import heapq
import math

import numpy as np

from .streams_batch import (AttemptBlocks, StageClock, bounds, check_stream_args, eval_chunks, maze_class, maze_streams_batch,
                            problem_env, problem_tensors, stream_ptr)

INF = float('inf')
_maze_class = maze_class               # the name a test reaches for: the shared definition, not a copy
ETA = 1.1                              # bit_star.py:51
# scipy.special.gamma(dim / 2 + 1) at dim 2 and 3, the values radius_init divides by (math.gamma(2.5) is one ulp above)
UNIT_BALL_GAMMA = {2: 1.0, 3: 1.329340388179137}

# status bits of a device problem (include/gnnmp.h, gnnmp_bitstar_plan)
STATUS_EDGE_QUEUE_FULL, STATUS_LOOP_BOUND, STATUS_SHORT_INPUT = 1, 2, 4

# default edge-queue entries per node of N_max = 2 + n_batches * batch: the census of DESIGN.md (largest max_edge_queue / N_max
# seen: 0.497), times 4, rounded up to a whole number of N_max
DEFAULT_EDGE_CAP_PER_NODE = 2

FIELDS = ('points', 'vertices', 'parents', 'g', 'samples_left', 'checks', 'g_goal', 'T', 'path_ids', 'draws')
STATS = ('vertex_expansions', 'edge_pops', 'edge_checks', 'rewired', 'filtered', 'max_edge_queue', 'ties_at_pop')


def n_batches(batch, t_max):
    """Batches of ``while T < t_max: ... T += batch`` at most."""
    return max(-(-int(t_max) // int(batch)), 1)


def radius_of(dim, ranges, n_free, n_collision, q):
    """``radius_init() * ((math.log(q) / q) ** (1.0 / dim))`` (bit_star.py:86-94, 288) with the reference's own expressions;
    ``special.gamma`` at the two arguments that occur is :data:`UNIT_BALL_GAMMA` (the package does not import scipy)."""
    n = int(dim)
    unit_ball_volume = np.pi ** (n / 2.0) / UNIT_BALL_GAMMA[n]
    volume = np.abs(np.prod(ranges)) * n_free / (n_collision + n_free)
    gamma = (1.0 + 1.0 / n) * volume / unit_ball_volume
    radius_constant = 2 * ETA * (gamma ** (1.0 / n))
    return radius_constant * ((math.log(q) / q) ** (1.0 / n))


def radius_by_batch(dim, batch, used_by_batch):
    """``r`` after every batch from the cumulative attempts of the sampling: after batch k (1-based) ``n_free_points`` is
    ``2 + k * batch``, ``n_collision_points`` the rejected draws so far and ``q`` the same ``2 + k * batch``."""
    _, ranges = bounds(maze_class(dim, 'bitstar')(np.zeros((1, 1, 1)), np.zeros((1, dim)), np.zeros((1, dim))).bound)
    out = np.zeros(len(used_by_batch), dtype=np.float64)
    for k, used in enumerate(used_by_batch, start=1):
        free = 2 + k * int(batch)
        out[k - 1] = radius_of(dim, ranges, free, int(used) - k * int(batch), free)
    return out


def plan_host(problem, seed, batch=50, t_max=1000, pool=None):
    """``np.random.seed(seed); BITStar(env, batch_size=batch, T=t_max, sampling=None).plan(INF, time_budget=300,
    refine_time_budget=0); get_best_path()`` for one maze problem (a dict with ``map``, ``init_state``, ``goal_state``;
    2 coordinates = point robot, 3 = stick robot) on a private ``RandomState``, every distance a scalar ``np.linalg.norm``.
    Returns a dict: ``points`` [N, dim] float64 (row 0 start, row 1 goal, then the free draws in order), ``vertices`` (ids in
    append order), ``parents`` [N] (-1 = none), ``g`` [N] (inf off the tree), ``samples_left`` (ids in list order), ``checks``
    (sampling included), ``g_goal``, ``T``, ``path_ids`` (start -> goal, empty when unsolved) and ``path`` (their states),
    ``draws`` (doubles consumed), per batch ``r_by_batch``, ``used_by_batch`` (cumulative attempts) and ``checks_by_batch``
    (cumulative sampling checks), and ``stats``: ``vertex_expansions``, ``edge_pops``, ``edge_checks``, ``rewired`` (accepted
    edges whose target was a vertex already), ``filtered`` (queued edges the filter removed), ``max_edge_queue`` and
    ``ties_at_pop`` (pops at which another entry of the same queue held the same value).

    ``pool=(points_per_batch, r_by_batch)`` replaces the sampling: batch k appends ``points_per_batch[k]`` unchecked and uses
    ``r_by_batch[k]``.  Raises where the reference would leave the first-solution search (refinement) or could not run."""
    env = problem_env(problem, 'bitstar')
    dim = env.config_dim
    batch, t_max = int(batch), int(t_max)
    low, ranges = bounds(env.bound)                  # bit_star.py:32-34
    rs = np.random.RandomState(int(seed) & 0xffffffff)
    start, goal = tuple(np.asarray(env.init_state, dtype=np.float64).reshape(dim)), tuple(np.asarray(env.goal_state, dtype=np.float64).reshape(dim))
    if start == goal:
        raise ValueError('bitstar.plan_host: start and goal are the same point (the reference keys its tables by point)')
    pts, ids = [start, goal], {start: 0, goal: 1}
    vertices, samples, parents, g = [0], [1], {}, {0: 0.0, 1: INF}
    vq, eq, old = [], [], set()
    stats = dict.fromkeys(STATS, 0)
    r_by_batch, used_by_batch, checks_by_batch = [], [], []
    T, r, attempts, sampling_checks, n_collision = 0, INF, 0, 0, 0

    def d(a, b):
        return np.linalg.norm(np.array(pts[a]) - np.array(pts[b]))

    def get_g(a):                            # get_g_score
        return 0 if a == 0 else (g[a] if a in parents else INF)

    def pop(queue):
        if len(queue) > 1 and sum(item[0] == queue[0][0] for item in queue) > 1:
            stats['ties_at_pop'] += 1
        return heapq.heappop(queue)

    def push_edge(a, b):
        heapq.heappush(eq, (get_g(a) + d(a, b) + d(b, 1), (pts[a], pts[b])))
        stats['max_edge_queue'] = max(stats['max_edge_queue'], len(eq))

    while T < t_max:
        if not vq and not eq:
            if g[1] != INF:
                raise RuntimeError('bitstar.plan_host: a batch with a finite c_best (refinement is not reproduced)')
            k = len(r_by_batch)
            if pool is not None:
                if k >= len(pool[0]):
                    raise ValueError('bitstar.plan_host: the pool holds fewer batches than the run draws')
                new = [tuple(np.asarray(p, dtype=np.float64).reshape(dim)) for p in pool[0][k]]
            else:
                new = []
                while len(new) < batch:
                    p = low + rs.random_sample(dim) * ranges
                    attempts += 1
                    before = env.collision_check_count
                    free = env._state_fp(np.array(tuple(p)))
                    sampling_checks += env.collision_check_count - before
                    if free:
                        new.append(tuple(p))
                    else:
                        n_collision += 1
            for p in new:
                if p in ids:
                    raise ValueError('bitstar.plan_host: the same point twice (the reference keys its tables by point)')
                ids[p] = len(pts)
                samples.append(len(pts))
                g.setdefault(len(pts), INF)
                pts.append(p)
            T += batch
            old = set(vertices)
            vq = [(get_g(v) + d(v, 1), pts[v]) for v in vertices]
            heapq.heapify(vq)
            q = len(vertices) + len(samples)
            if pool is not None:
                r = float(pool[1][k])
            else:
                r = radius_of(dim, ranges, 2 + (k + 1) * batch, n_collision, q)
            r_by_batch.append(r)
            used_by_batch.append(attempts)
            checks_by_batch.append(sampling_checks)
        empty = False
        while (vq[0][0] if vq else INF) <= (eq[0][0] if eq else INF):
            if not vq:                       # heappop raises; both queues are empty (inf <= inf): the next batch
                if eq:
                    raise RuntimeError('bitstar.plan_host: an infinite edge value')
                empty = True
                break
            v = ids[pop(vq)[1]]
            stats['vertex_expansions'] += 1
            for x in [x for x in samples if d(v, x) <= r]:
                push_edge(v, x)              # estimated_f_score < g_scores[goal] = inf
            if v not in old:
                for w in [w for w in vertices if d(v, w) <= r]:
                    if w not in parents or v != parents.get(w):
                        if get_g(v) + d(v, w) < get_g(w):
                            push_edge(v, w)
        if empty:
            continue
        value, (pv, px) = pop(eq)
        stats['edge_pops'] += 1
        v, x = ids[pv], ids[px]
        if not value < g[1]:
            raise RuntimeError('bitstar.plan_host: the best edge cannot improve the solution (refinement is not reproduced)')
        stats['edge_checks'] += 1
        cost = d(v, x) if env._edge_fp(np.array(pv), np.array(px)) else INF
        if d(0, v) + cost + d(x, 1) < g[1]:
            new_g = get_g(v) + cost
            if new_g < get_g(x):
                g[x] = new_g
                parents[x] = v
                if x not in vertices:
                    samples.remove(x)
                    vertices.append(x)
                    heapq.heappush(vq, (get_g(x) + d(x, 1), pts[x]))
                else:
                    stats['rewired'] += 1
                kept = [item for item in eq if item[1][1] != px]
                stats['filtered'] += len(eq) - len(kept)
                eq = kept
                heapq.heapify(eq)
        if g[1] < INF:                       # refine_time_budget = 0: the first solution ends the run
            break
    path = []
    if g[1] != INF:
        path.append(1)
        while path[-1] != 0:
            if len(path) > len(pts):
                raise RuntimeError('bitstar.plan_host: the parents hold a cycle (the reference would not return)')
            path.append(parents[path[-1]])
        path.reverse()
    points = np.array(pts, dtype=np.float64).reshape(-1, dim)
    ids_np = np.array(path, dtype=np.int64)
    n = len(pts)
    return {'points': points, 'vertices': np.array(vertices, dtype=np.int64),
            'parents': np.array([parents.get(i, -1) for i in range(n)], dtype=np.int64),
            'g': np.array([get_g(i) for i in range(n)], dtype=np.float64), 'samples_left': np.array(samples, dtype=np.int64),
            'checks': int(env.collision_check_count), 'g_goal': float(g[1]), 'T': T, 'path_ids': ids_np, 'path': points[ids_np],
            'draws': attempts * dim, 'r_by_batch': np.array(r_by_batch, dtype=np.float64),
            'used_by_batch': np.array(used_by_batch, dtype=np.int64), 'checks_by_batch': np.array(checks_by_batch, dtype=np.int64),
            'stats': stats}


# --------------------------------------------------------------------------------------------------
# device path (libgnnmp.so, csrc/bitstar_kernels.hip).  No fallback: without the library every call raises.
# --------------------------------------------------------------------------------------------------
_DRAWS_PER_FREE = [2.0, 8.0]           # attempts per free draw by dim (point robot, stick robot): sizes the first attempt block
COUNTERS = ('checks',) + STATS         # the columns of gnnmp_bitstar_result.counters


def lds_nodes():
    """Launches of up to this many nodes per problem (``2 + n_batches * batch``) keep their node state in LDS; larger ones use
    the outputs and the workspace (``flags`` bit 0 of :func:`bitstar_plan` forces that path at any size)."""
    from . import _lib
    return int(_lib.lib().gnnmp_bitstar_lds_nodes())


def default_edge_cap(n_nodes):
    """Entries of a problem's edge queue unless the caller says otherwise: :data:`DEFAULT_EDGE_CAP_PER_NODE` per node, at
    most the provable ``n_nodes * (n_nodes - 1)``.  A problem that fills it is run again alone with the full bound."""
    n = int(n_nodes)
    return max(min(DEFAULT_EDGE_CAP_PER_NODE * n, n * (n - 1)), 1)


def bitstar_sample(attempts, att_ptr_host, maps, init64, goal64, batch, nb, pool, used, checks, status, active=None):
    """``gnnmp_bitstar_sample``: the ``nb * batch`` free draws of every active problem from its own block ``[att_ptr[b],
    att_ptr[b + 1])`` of ``attempts`` (float64 ``[M, dim]``, device) into ``pool`` ``[B, rows, dim]`` behind start and goal,
    and per batch the cumulative attempts / sampling checks into ``used`` / ``checks`` (int64 ``[B, nb]``).  One launch;
    ``status`` (int32 ``[B]``) is written for the active problems.  Nothing is read back."""
    import ctypes
    import torch
    from . import _lib
    dev = pool.device
    sb, keep = maze_streams_batch(pool.shape[0], maps.shape[1], batch, pool.shape[1], attempts, att_ptr_host, maps, init64, goal64, active)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gnnmp_bitstar_sample(ctypes.byref(sb), int(pool.shape[2]), int(nb), pool.data_ptr(), used.data_ptr(),
                                                   checks.data_ptr(), status.data_ptr(), stream_ptr(dev)), 'gnnmp_bitstar_sample')


def bitstar_plan(maps, pool, r_by_batch, checks_by_batch, batch, nb, edge_cap=None, flags=0):
    """``gnnmp_bitstar_plan`` on device tensors: ``maps`` [B, w, w], ``pool`` [B, rows, dim], ``r_by_batch`` [B, nb] (all
    float64), ``checks_by_batch`` [B, nb] int64.  One launch on the current stream; returns the device tensors of
    ``gnnmp_bitstar_result`` as a dict (the five per-problem words as rows of ``small``: n_vertices, batches_run, success,
    path_len, status; ``counters`` [B, 8] in the order of :data:`COUNTERS`).  Nothing is read back."""
    import ctypes
    import torch
    from . import _lib
    dev = maps.device
    B, rows, dim = (int(x) for x in pool.shape)
    edge_cap = default_edge_cap(rows) if edge_cap is None else int(edge_cap)
    maps, pool, r_by_batch, checks_by_batch = maps.contiguous(), pool.contiguous(), r_by_batch.contiguous(), checks_by_batch.contiguous()
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=dev)      # noqa: E731
    out = {'g': new(torch.float64, B, rows), 'parents': new(torch.int32, B, rows), 'vertices': new(torch.int32, B, rows),
           'path': new(torch.int32, B, rows), 'small': new(torch.int32, 5, B), 'counters': new(torch.int64, B, 8)}
    L = _lib.lib()
    need = ctypes.c_size_t()
    _lib.check(L.gnnmp_bitstar_workspace_bytes(B, rows, edge_cap, ctypes.byref(need)), 'gnnmp_bitstar_workspace_bytes')
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=dev)
    batch_s = _lib.BITStarBatch(B, dim, int(maps.shape[1]), int(batch), int(nb), rows, int(flags), edge_cap, maps.data_ptr(),
                                pool.data_ptr(), r_by_batch.data_ptr(), checks_by_batch.data_ptr())
    result = _lib.BITStarResult(*(out[k].data_ptr() for k in ('g', 'parents', 'vertices', 'path')),
                                *(out['small'][r].data_ptr() for r in range(5)), out['counters'].data_ptr())
    with torch.cuda.device(dev):
        _lib.check(L.gnnmp_bitstar_plan(ctypes.byref(batch_s), ctypes.byref(result), ws.data_ptr(), ws.numel(), stream_ptr(dev)),
                   'gnnmp_bitstar_plan')
    out['workspace'] = ws
    return out


def _problem_result(b, batch, dim, pool, used, schecks, r_tab, host, small, counters):
    n_vertices, batches_run, success, path_len, status = (int(x) for x in small[:, b])
    n = 2 + batches_run * batch
    pts = pool[b, :n].copy()
    vertices = host['vertices'][b, :n_vertices].astype(np.int64)
    is_vertex = np.zeros(n, dtype=bool)
    is_vertex[vertices] = True
    ids = host['path'][b, :path_len].astype(np.int64)
    g = host['g'][b, :n].copy()
    return {'points': pts, 'vertices': vertices, 'parents': host['parents'][b, :n].astype(np.int64), 'g': g,
            'samples_left': np.flatnonzero(~is_vertex).astype(np.int64), 'checks': int(counters[b, 0]), 'g_goal': float(g[1]),
            'T': batches_run * batch, 'path_ids': ids, 'path': pts[ids], 'draws': int(used[b, batches_run - 1]) * dim if batches_run else 0,
            'r_by_batch': r_tab[b, :batches_run].copy(), 'used_by_batch': used[b, :batches_run].copy(),
            'checks_by_batch': schecks[b, :batches_run].copy(), 'stats': {k: int(counters[b, 1 + i]) for i, k in enumerate(STATS)},
            'success': bool(success), 'status': status}


def plan_maze_batch(problems, device, seeds, batch=50, t_max=1000, draws='host', edge_cap=None, timings=None, streams_out=None):
    """BIT* for many maze problems at once (point robot or stick robot, by the width of ``init_state``), every problem on its
    OWN sample stream: problem i computes what :func:`plan_host` -- ``np.random.seed(seeds[i]); BITStar(...).plan(INF,
    time_budget=300, refine_time_budget=0)`` of that problem alone -- computes, whatever other problems are in the batch, in
    whatever order or chunks.  Two launches: ``gnnmp_bitstar_sample`` classifies the draws of all ``ceil(t_max / batch)``
    batches up front (a problem's stream feeds nothing but the sampling; whoever runs out of attempts gets a longer block),
    one small readback gives the host the attempt counts the radius table is built from (:func:`radius_by_batch`), and
    ``gnnmp_bitstar_plan`` runs the whole search of all problems.

    ``draws``: ``'host'`` -- one ``RandomState`` per problem draws the attempt blocks; ``'device'`` --
    :class:`gnnmp.rng.MTStreams` fills them without a commit and the streams are then advanced by the attempts of the batches
    each problem REACHED, so their state afterwards is numpy's after the plan (``streams_out``: a list that receives the
    :class:`MTStreams` object).  ``edge_cap``: entries of a problem's edge queue (default :func:`default_edge_cap`); a problem
    that fills it is run again, alone, with the provable bound ``N (N - 1)`` -- the same computation, it has its own stream.
    Returns one dict per problem with :func:`plan_host`'s fields plus ``success`` and ``status`` (0 = fine; a loop bound or a
    bad table raises)."""
    import torch
    who = 'bitstar.plan_maze_batch'
    B, batch, t_max = len(problems), int(batch), int(t_max)
    if B == 0:
        return []
    check_stream_args(B, seeds, draws, who)
    if batch < 1 or t_max < 1:
        raise ValueError('bitstar.plan_maze_batch: batch >= 1 and t_max >= 1')
    dev = torch.device(device)
    nb = n_batches(batch, t_max)
    total, rows = nb * batch, 2 + nb * batch
    clock = StageClock(timings)
    with torch.cuda.device(dev):
        dim, maps, init64, goal64 = problem_tensors(problems, dev, who)
        _, ranges = bounds(maze_class(dim, 'bitstar')(np.zeros((1, 1, 1)), np.zeros((1, dim)), np.zeros((1, dim))).bound)
        pool = torch.zeros(B, rows, dim, dtype=torch.float64, device=dev)
        used_d = torch.zeros(B, nb, dtype=torch.int64, device=dev)
        schecks_d = torch.zeros(B, nb, dtype=torch.int64, device=dev)
        status_d = torch.zeros(B, dtype=torch.int32, device=dev)
        blocks = AttemptBlocks(seeds, dim, dev, draws, _DRAWS_PER_FREE)

        def sample(att, att_ptr, mask_d):
            bitstar_sample(att, att_ptr, maps, init64, goal64, batch, nb, pool, used_d, schecks_d, status_d, active=mask_d)
            return (status_d,)
        # ---- sampling: a block per problem from its own generator, longer for whoever ran out.  The sampler starts over on a
        # longer block, so nothing is committed here: the streams move below, by what each problem's search reached
        blocks.run(np.arange(B), total, sample, commit=False,
                   no_room='gnnmp_bitstar_sample: attempt block outside the buffer for problem(s) %s')
        used, schecks = torch.stack((used_d, schecks_d)).cpu().numpy()     # the one readback between the two launches
        blocks.update_estimate(float(used[:, -1].mean()), total)
        clock.mark('sampling')
        cache, r_tab = {}, np.zeros((B, nb), dtype=np.float64)
        for b in range(B):
            for k in range(1, nb + 1):
                key = (k, int(used[b, k - 1]))
                if key not in cache:
                    free = 2 + k * batch
                    cache[key] = radius_of(dim, ranges, free, key[1] - k * batch, free)
                r_tab[b, k - 1] = cache[key]
        r_tab_d = torch.from_numpy(r_tab).to(dev)
        clock.mark('radius')
        out = bitstar_plan(maps, pool, r_tab_d, schecks_d, batch, nb, edge_cap=edge_cap)
        clock.mark('plan')
        small, counters = out['small'].cpu().numpy(), out['counters'].cpu().numpy()
        host = {k: out[k].cpu().numpy() for k in ('g', 'parents', 'vertices', 'path')}
        pool_h = pool.cpu().numpy()
    res = [_problem_result(b, batch, dim, pool_h, used, schecks, r_tab, host, small, counters) for b in range(B)]
    for b in range(B):
        if res[b]['status'] & STATUS_EDGE_QUEUE_FULL and (edge_cap is None or int(edge_cap) < rows * (rows - 1)):
            res[b] = plan_maze_batch([problems[b]], dev, [seeds[b]], batch=batch, t_max=t_max, draws='host', edge_cap=rows * (rows - 1))[0]
    bad = [b for b in range(B) if res[b]['status']]
    if bad:
        raise RuntimeError('gnnmp_bitstar_plan: status %s for problem(s) %s (1 = edge queue full, 2 = loop bound or a cycle in the '
                           'parents, 4 = radius / check tables not filled)' % ([res[b]['status'] for b in bad], bad))
    if draws == 'device':
        with torch.cuda.device(dev):
            reached = np.array([int(used[b, res[b]['T'] // batch - 1]) for b in range(B)], dtype=np.int32)
            blocks.streams.advance(reached, dim)                        # by the attempts of the batches each problem reached
        if streams_out is not None:
            streams_out.append(blocks.streams)
    clock.mark('results')
    return res


def eval_aggregate(results):
    """``eval_bit``'s aggregates of per-problem results -> (n_success, collision, solution_cost): the problems with a finite
    ``g_goal``, the mean of ``checks`` over ALL problems and the sum of ``g_goal`` over the solved ones divided by
    ``n_success`` (nan when none is solved)."""
    solved = [float(r['g_goal']) for r in results if float(r['g_goal']) != INF]
    collision = float(np.mean([int(r['checks']) for r in results]))
    return len(solved), collision, float(sum(solved)) / len(solved) if solved else float('nan')


def eval_bit_device(env, indexes, seed=1234, seeds=None, batch=50, t_max=1000, device='cuda', chunk=1024, rows_out=None, timings=None,
                    draws='host'):
    """The tuple of the reference's ``eval_bit.eval_bit`` without its wall-clock entries, from :func:`plan_maze_batch`, ``chunk``
    problems per launch: ``(n_success, collision, solution_cost, paths)`` -- see :func:`eval_aggregate`; ``paths`` are the
    float64 states of ``get_best_path()``.  Problem ``indexes[i]`` draws from ``np.random.RandomState(seeds[i])``; default
    :func:`gnnmp.streams_batch.stream_seeds`.  The numbers DIFFER from ``eval_bit``'s, which walks ONE global stream problem after
    problem -- other samples of the same distribution -- and in exchange they do not depend on the order of ``indexes`` or on
    ``chunk``.  ``rows_out``: a list that receives per problem (success, checks, g_goal, vertices, N, T).  The global numpy
    generator is left alone."""
    results = []
    for pr, chunk_seeds in eval_chunks(env, indexes, seed, seeds, chunk):
        results.extend(plan_maze_batch(pr, device, chunk_seeds, batch=batch, t_max=t_max, draws=draws, timings=timings))
    if rows_out is not None:
        rows_out.extend((int(r['success']), r['checks'], r['g_goal'], len(r['vertices']), r['points'].shape[0], r['T']) for r in results)
    return eval_aggregate(results) + ([r['path'] for r in results],)
