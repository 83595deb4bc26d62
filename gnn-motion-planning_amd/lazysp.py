"""LazySP on maze problems: the comparison baseline of the GNN explorer (the reference's ``algorithm/lazy_sp.py:147-196`` with
``algorithm/dijkstra.py:34-76``), restated on the host (:func:`plan_host`, numpy only) and run for whole batches on the device
(:func:`plan_maze_batch`, :func:`eval_lazysp_device`; ``csrc/lazysp_kernels.hip``).

Semantics.  Problem i behaves as ``np.random.seed(seeds[i]); env.init_new_problem(idx_i); LazySP(env, batch_size=batch, T=t_max,
k=k).plan()`` does: one sample stream PER PROBLEM, the convention of :func:`gnnmp.planner.plan_maze_rounds_batch`.  The
reference's ``eval_bit.eval_lazysp`` seeds once globally and runs the problems one after another through that one stream; that
form is NOT reproduced (other samples of the same distribution), in exchange a problem's result does not depend on the other
problems, on their order or on how a batch is cut.

  * samples = [goal, start, then the free draws] in float64: node 0 is the GOAL, node 1 the START.  A draw is
    ``bounds[:, 0] + np.random.random(dim) * ranges`` -- the doubles of ``uniform_sample``'s ``low + (high - low) * d`` -- and goes
    through ``_state_fp``, whose collision checks count; rejected draws are dropped.
  * a round: ``batch`` more free draws, ``T += batch``, ``k1 = ceil(k ln(q) / ln(100))`` with q = all samples, the graph
    ``coalesce(knn_graph(float32(points), k1, loop=True) + flipped)`` minus the invalidated edges, edge cost
    ``np.linalg.norm(points[t] - points[s])`` in float64.
  * inner loop: a full Dijkstra from node 0 (least distance first, lowest id among equals, strict ``alt < dist[v]``); ``dist[1]``
    infinite ends the round; otherwise the path is walked from node 1 along ``prev``: known-valid edges are skipped, unknown ones
    checked with ``_edge_fp`` on the float64 states; a free edge joins ``valid_edges`` (both directions), a blocked one joins
    ``invalid_edges`` (both directions), leaves both neighbour lists, ends the walk, and Dijkstra runs again.  A fully valid
    path ends the problem.  Both edge sets carry across rounds by node id.
"""
import numpy as np

from .streams_batch import (AttemptBlocks, StageClock, bounds, check_stream_args, eval_chunks, maze_streams_batch, maze_class,
                            problem_env, problem_tensors, stream_ptr)

INF = float('inf')
_maze_class = maze_class               # names the tests reach for: the shared definitions, not copies


def _bounds(env):
    return bounds(env.bound)

# status bits of a device slot (include/gnnmp.h, gnnmp_lazysp_round)
STATUS_PAIR_OVERFLOW, STATUS_LOOP_BOUND, STATUS_BAD_INPUT = 1, 2, 4


def k1_of(k, q):
    """``int(np.ceil(k0 * np.log(q) / np.log(100)))`` (lazy_sp.py:159), numpy's arithmetic."""
    return int(np.ceil(k * np.log(q) / np.log(100)))


def rounds_pair_cap(batch, t_max, k):
    """Entries a problem's pair list can reach over all its rounds: every checked edge is an unordered non-loop pair of SOME
    round's graph, a pair is checked at most once (valid and invalid pairs are never checked again), and round r's graph --
    k1-NN plus reversed on N_r = 2 + r * batch nodes -- has at most min(k1_r * N_r, N_r (N_r - 1) / 2) such pairs (each node
    contributes at most its k1 neighbours; a kNN list is cut to N when k1 > N).  A derived bound: the sum over the rounds,
    not the edge counts seen."""
    batch, t_max = int(batch), int(t_max)
    cap, T, r = 0, 0, 0
    while T < t_max:
        T += batch
        r += 1
        n = 2 + r * batch
        cap += min(min(k1_of(k, n), n) * n, n * (n - 1) // 2)
    return max(cap, 1)


def graph_edges(points, k1):
    """``construct_graph``'s edge set (lazy_sp.py:125-129): [E, 2] (source, target) rows sorted by (source, target).  The k1
    nearest of a node (itself included) in ascending (squared distance, id) order -- squared distances accumulated coordinate
    by coordinate in float64 from the float32 coordinates, a stable sort -- so that among equidistant candidates the LOWER id
    is taken, the rule of the device's graph builder (csrc/graph_kernels.hip gb_knn); ``topk`` leaves that order open."""
    import torch
    from .graph_build import coalesce
    x = np.asarray(points, dtype=np.float64).astype(np.float32).astype(np.float64)
    n = x.shape[0]
    d = np.zeros((n, n))
    for c in range(x.shape[1]):
        df = x[:, c].reshape(-1, 1) - x[:, c].reshape(1, -1)
        d = d + df * df
    nb = np.argsort(d, axis=1, kind='stable')[:, :min(int(k1), n)]
    centre = np.broadcast_to(np.arange(n).reshape(-1, 1), nb.shape)
    e = torch.from_numpy(np.stack((nb.reshape(-1), centre.reshape(-1)))).long()
    return coalesce(torch.cat((e, e.flip(0)), dim=1), n).numpy().T


def extract_index(key):
    """``min_dist(q, dist)`` (dijkstra.py:34-46) on the keys of the unvisited nodes: the first strict minimum as the reference
    walks its set ``q`` -- ascending ids, as CPython iterates a set of the ints 0 .. n - 1 that were all added before any was
    removed (each hashes to its own slot) -- so the LOWEST id among equal keys; ``np.argmin``'s first minimum.  (Module level,
    like the test below, so that a test can swap in another rule.)"""
    return int(np.argmin(key))


def relax_improves(alt, dist):
    """The relaxation test ``alt < dist[v]`` (dijkstra.py:71), STRICT: of two equally short ways to v the one found first --
    from the node extracted first -- stays in ``prev``."""
    return alt < dist


def _dijkstra(cost, early_exit, stats=None):
    """``dijkstra(nodes, neighbors, edge_cost, 0)`` on the dense cost matrix (inf = no edge): extraction by (distance, lowest
    id), strict improvement.  With ``early_exit`` the run stops once node 1 is extracted, or at the first infinite minimum
    (nodes at infinite distance relax nothing): extraction keys never decrease under non-negative costs, so neither dist[1] nor
    prev along node 1's chain can change afterwards.  ``stats`` (a dict) counts exact ties: ``extract_ties`` extractions
    whose finite key more than one unvisited node holds, ``relax_ties`` relaxations of another node with a finite
    ``alt == dist[v]``."""
    n = cost.shape[0]
    dist = np.full(n, INF)
    prev = np.full(n, -1, dtype=np.int64)
    dist[0] = 0.0
    prev[0] = 0
    key = dist.copy()                      # dist of the unvisited, inf for the visited
    for _ in range(n):
        u = extract_index(key)
        du = key[u]
        if du == INF:
            break
        if stats is not None:
            stats['extract_ties'] += int(np.count_nonzero(key == du) > 1)
        key[u] = INF
        if early_exit and u == 1:
            break
        alt = du + cost[u]
        better = relax_improves(alt, dist)
        better[u] = False                  # (the loop edge: alt = du, never below dist[u])
        if stats is not None:
            ties = (alt == dist) & (alt < INF)
            ties[u] = False
            stats['relax_ties'] += int(ties.sum())
        dist[better] = alt[better]
        prev[better] = u
        key[better] = alt[better]          # an improved node was never visited: alt >= du >= every visited distance
    return dist, prev


def plan_host(problem, seed, batch=50, t_max=1000, k=10, early_exit=True, attempts=None):
    """``np.random.seed(seed); LazySP(env, batch_size=batch, T=t_max, k=k).plan()`` for one maze problem (a dict with ``map``,
    ``init_state``, ``goal_state``; 2 coordinates = point robot, 3 = stick robot), on a private ``RandomState``.  Returns a dict:
    ``samples`` [N, dim] float64; ``checks`` (sampling included); ``path_ids`` (start -> goal, empty when unsolved) and ``path``
    (their float64 states); ``T``; ``valid_edges`` / ``invalid_edges`` as sorted unordered pairs [m, 2] (a < b);
    ``dijkstra_runs``; ``invalid_order`` [m, 2]: the blocked edges (n1, n2) in the order they were found; ``rounds`` [R, 4]:
    N, cumulative checks, unordered valid pairs, unordered invalid pairs after every round.  Two more, for tests that aim at
    a shape: ``walk_edges`` (edges of the path of every Dijkstra run that reached the start) and ``blocked_at`` (position of
    the blocked edge on the path of every run that found one).  ``checked_order`` [m, 3]: every checked edge (n1, n2, 1 = free / 2 = blocked) in
    the order of the checks -- the device's pair list.  ``extract_ties`` / ``relax_ties``: the exact ties of all
    Dijkstra runs, as :func:`_dijkstra` counts them; ``draws``: the draws taken, rejected ones included.  ``attempts``: an ``[n, dim]`` array of raw doubles in [0, 1), one row
    per draw (``low + row * ranges``), instead of ``RandomState(seed).random_sample(dim)``; ``seed`` is not used then and
    running out of rows raises."""
    env = problem_env(problem, 'lazysp')
    dim = env.config_dim
    rs = np.random.RandomState(int(seed) & 0xffffffff)
    low, ranges = bounds(env.bound)                  # lazy_sp.py:37-39
    samples = [np.asarray(env.goal_state, dtype=np.float64).reshape(dim), np.asarray(env.init_state, dtype=np.float64).reshape(dim)]
    valid, invalid, invalid_order, rounds, checked = set(), set(), [], [], []
    runs, T, path = 0, 0, []
    walk_edges, blocked_at = [], []        # per Dijkstra run that reached the start: edges of its path, position of the blocked one
    ties = dict(extract_ties=0, relax_ties=0, draws=0)
    if attempts is not None:
        rows = iter(np.asarray(attempts, dtype=np.float64).reshape(-1, dim))

    def draw():
        ties['draws'] += 1
        if attempts is None:
            return rs.random_sample(dim)
        row = next(rows, None)
        if row is None:
            raise ValueError('lazysp.plan_host: the attempts ran out')
        return row

    def result():
        pts = np.array(samples).reshape(-1, dim)
        un = lambda s: np.array(sorted((a, b) for a, b in s if a < b), dtype=np.int64).reshape(-1, 2)      # noqa: E731
        return {'samples': pts, 'checks': int(env.collision_check_count), 'path_ids': np.array(path, dtype=np.int64),
                'path': pts[np.array(path, dtype=np.int64)], 'T': T, 'valid_edges': un(valid), 'invalid_edges': un(invalid),
                'dijkstra_runs': runs, 'invalid_order': np.array(invalid_order, dtype=np.int64).reshape(-1, 2),
                'rounds': np.array(rounds, dtype=np.int64).reshape(-1, 4),
                'walk_edges': np.array(walk_edges, dtype=np.int64), 'blocked_at': np.array(blocked_at, dtype=np.int64),
                'checked_order': np.array(checked, dtype=np.int64).reshape(-1, 3), **ties}

    while T < t_max:
        got = 0
        while got < batch:
            p = low + draw() * ranges
            if env._state_fp(p):
                samples.append(p)
                got += 1
        T += batch
        pts = np.array(samples)
        n = len(samples)
        cost = np.full((n, n), INF)
        for s, t in graph_edges(pts, k1_of(k, n)):
            if (int(s), int(t)) not in invalid:
                cost[t, s] = np.linalg.norm(pts[t] - pts[s])
        while True:
            dist, prev = _dijkstra(cost, early_exit, ties)
            runs += 1
            if dist[1] == INF:
                break
            walk = [1]
            while walk[-1] != 0:
                walk.append(int(prev[walk[-1]]))
                if len(walk) > n:
                    raise RuntimeError('lazysp.plan_host: prev holds a cycle (the reference would not return)')
            feasible = True
            walk_edges.append(len(walk) - 1)
            for pos, (n1, n2) in enumerate(zip(walk[:-1], walk[1:])):
                if (n1, n2) in valid:
                    continue
                if env._edge_fp(pts[n1], pts[n2]):
                    valid.update(((n1, n2), (n2, n1)))
                    checked.append((n1, n2, 1))
                else:
                    invalid.update(((n1, n2), (n2, n1)))
                    invalid_order.append((n1, n2))
                    checked.append((n1, n2, 2))
                    cost[n1, n2] = cost[n2, n1] = INF
                    blocked_at.append(pos)
                    feasible = False
                    break
            if feasible:
                path = walk
                rounds.append((n, env.collision_check_count, len(valid) // 2, len(invalid) // 2))
                return result()
        rounds.append((n, env.collision_check_count, len(valid) // 2, len(invalid) // 2))
    return result()


# --------------------------------------------------------------------------------------------------
# device path (libgnnmp.so, csrc/lazysp_kernels.hip).  No fallback: without the library every call raises.
# --------------------------------------------------------------------------------------------------
_DRAWS_PER_FREE = [2.0, 8.0]           # running estimate per dim (point robot, stick robot): sizes the first block of a round


def n_rounds(batch, t_max):
    """Rounds of ``while T < t_max: T += batch``."""
    return max(-(-int(t_max) // int(batch)), 1)


class LazySPStore:
    """The device arrays of ``gnnmp_lazysp_state`` for B problems, all zeros = fresh.  A slot is ``9 * pair_cap`` bytes of pair
    list plus ``(cap + 2) * (8 * dim + 4)`` bytes of pool and path; with :func:`rounds_pair_cap`'s derived bound the pair list
    dominates (about 1.4 MB per problem at batch = 50, t_max = 1000, k = 10)."""

    def __init__(self, B, cap, pair_cap, dim, device):
        import torch
        from . import _lib
        dev = torch.device(device)
        self.B, self.cap, self.pair_cap, self.dim, self.device = int(B), int(cap), int(pair_cap), int(dim), dev
        i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)      # noqa: E731
        self.pool = torch.zeros(B, self.cap + 2, dim, dtype=torch.float64, device=dev)
        self.n_nodes, self.n_pairs, self.dijkstra_runs, self.path_len, self.solved, self.status = (i32(B) for _ in range(6))
        self.pairs = i32(B, self.pair_cap, 2)
        self.pair_state = torch.zeros(B, self.pair_cap, dtype=torch.uint8, device=dev)
        self.checks = torch.zeros(B, dtype=torch.int64, device=dev)
        self.path = i32(B, self.cap + 2)
        self.struct = _lib.LazySPState(self.B, self.cap, self.pair_cap, *(t.data_ptr() for t in (
            self.pool, self.n_nodes, self.pairs, self.pair_state, self.n_pairs, self.checks, self.dijkstra_runs, self.path_len,
            self.path, self.solved, self.status)))


def lazysp_sample(store, attempts, att_ptr_host, maps, init64, goal64, n, active=None):
    """``gnnmp_lazysp_sample``: append ``n`` free draws to every active problem's float64 pool from its own block
    ``[att_ptr[b], att_ptr[b + 1])`` of ``attempts`` (float64 ``[M, dim]``, device).  One launch; returns device tensors
    ``(used, checks, status)``; the store's running check total is incremented."""
    import ctypes
    import torch
    from . import _lib
    dev = store.device
    sb, keep = maze_streams_batch(store.B, maps.shape[1], n, store.cap, attempts, att_ptr_host, maps, init64, goal64, active)
    used = torch.zeros(store.B, dtype=torch.int32, device=dev)
    checks = torch.zeros(store.B, dtype=torch.int64, device=dev)
    status = torch.zeros(store.B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gnnmp_lazysp_sample(ctypes.byref(sb), store.dim, ctypes.byref(store.struct), used.data_ptr(),
                                                  checks.data_ptr(), status.data_ptr(), stream_ptr(dev)), 'gnnmp_lazysp_sample')
    return used, checks, status


def lazysp_gather(store, slot_of, k1_table, v_rows):
    """``gnnmp_lazysp_gather``: float32 node rows, node_ptr, n_free and k1 of the problems ``slot_of`` (int32, device) in the
    layout the graph builder reads.  ``k1_table``: int32 ``[cap + 3]`` (device), k1 by node count.  Nothing is read back."""
    import ctypes
    import torch
    from . import _lib
    dev = store.device
    A = int(slot_of.shape[0])
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)      # noqa: E731
    out = {'v': torch.zeros(max(int(v_rows), 1), store.dim, dtype=torch.float32, device=dev)[:int(v_rows)], 'node_ptr': i32(A + 1),
           'n_free': i32(A), 'k1': i32(A)}
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gnnmp_lazysp_gather(ctypes.byref(store.struct), store.dim, A, slot_of.data_ptr(), k1_table.data_ptr(),
                                                  int(v_rows), out['v'].data_ptr(), out['node_ptr'].data_ptr(),
                                                  out['n_free'].data_ptr(), out['k1'].data_ptr(), stream_ptr(dev)), 'gnnmp_lazysp_gather')
    return out


def lazysp_round(store, slot_of, ei, edge_ptr, maps):
    """``gnnmp_lazysp_round`` for the problems ``slot_of`` (int32 device tensor, or None = slot j for graph j) on their
    coalesced graphs ``ei`` [2, E] / ``edge_ptr``; ``maps`` [B, w, w] float64 by slot.  The store is updated in place."""
    import ctypes
    import torch
    from . import _lib
    dev = store.device
    A = int(edge_ptr.shape[0]) - 1
    ei = ei.contiguous()
    total = int(ei.shape[1])
    need = ctypes.c_size_t()
    L = _lib.lib()
    _lib.check(L.gnnmp_lazysp_workspace_bytes(A, store.cap, total, ctypes.byref(need)), 'gnnmp_lazysp_workspace_bytes')
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.gnnmp_lazysp_round(ctypes.byref(store.struct), store.dim, A, slot_of.data_ptr() if slot_of is not None else None,
                                        ei.data_ptr(), total, edge_ptr.data_ptr(), maps.data_ptr(), int(maps.shape[1]), ws.data_ptr(),
                                        ws.numel(), stream_ptr(dev)), 'gnnmp_lazysp_round')
    return ws


def _unordered(pairs):
    p = np.sort(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), axis=1)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def plan_maze_batch(problems, device, seeds, batch=50, t_max=1000, k=10, draws='host', timings=None, pair_cap=None,
                    raise_on_status=True):
    """LazySP for many maze problems at once (point robot or stick robot, by the width of ``init_state``), every problem on its
    OWN sample stream: problem i computes what :func:`plan_host` -- ``np.random.seed(seeds[i]); LazySP(...).plan()`` of that
    problem alone -- computes, whatever other problems are in the batch, in whatever order or chunks.

    Round r of ALL unfinished problems is one batch: ``gnnmp_lazysp_sample`` -> ``gnnmp_lazysp_gather`` ->
    ``gnnmp_graph_build`` -> ``gnnmp_lazysp_round``; there is no Python loop over problems after the set-up.  Between rounds the
    host reads the sampler's status / used words (they size a longer block for whoever ran out), the graph builder's edge count
    and the per-problem solved / status flags that decide who continues; samples, pairs, paths and counts stay on the device
    until the end.  ``draws``: ``'host'`` -- one ``RandomState`` per problem draws the blocks; ``'device'`` -- the same generators
    run on the device (:class:`gnnmp.rng.MTStreams`) the way :func:`gnnmp.planner.plan_maze_rounds_batch` uses them.

    Returns one dict per problem with :func:`plan_host`'s fields plus ``success`` and ``status`` (the slot's status bits,
    0 = fine; with ``raise_on_status`` a non-zero one raises).  ``pair_cap``: override the derived pair-list capacity."""
    import torch
    from .graph_build import build_edges_gpu
    who = 'lazysp.plan_maze_batch'
    B, n, t_max = len(problems), int(batch), int(t_max)
    if B == 0:
        return []
    check_stream_args(B, seeds, draws, who)
    if n < 1 or t_max < 1:
        raise ValueError('lazysp.plan_maze_batch: batch >= 1 and t_max >= 1')
    dev = torch.device(device)
    dim, maps, init64, goal64 = problem_tensors(problems, dev, who)
    maze_class(dim, 'lazysp')
    R = n_rounds(n, t_max)
    cap = R * n
    store = LazySPStore(B, cap, rounds_pair_cap(n, t_max, k) if pair_cap is None else pair_cap, dim, dev)
    k1_np = np.ones(cap + 3, dtype=np.int32)
    k1_np[2:] = [k1_of(k, q) for q in range(2, cap + 3)]
    k1_table = torch.from_numpy(k1_np).to(dev)
    blocks = AttemptBlocks(seeds, dim, dev, draws, _DRAWS_PER_FREE)

    def sample(att, att_ptr, mask_d):
        used, _, status = lazysp_sample(store, att, att_ptr, maps, init64, goal64, n, active=mask_d)
        return status, used
    act = np.arange(B)
    rounds_done = np.zeros(B, dtype=np.int64)
    snaps = []
    clock = StageClock(timings)
    with torch.cuda.device(dev):
        for r in range(1, R + 1):
            # ---- sampling: a block per active problem from its own generator, longer for whoever ran out
            blocks.run(act, n, sample, no_room='gnnmp_lazysp_sample: no room in the pool of problem(s) %s')
            clock.mark('sampling')
            # ---- this round's graphs
            A, N = int(act.size), 2 + r * n
            slot_of = torch.from_numpy(act.astype(np.int32)).to(dev)
            g = lazysp_gather(store, slot_of, k1_table, A * N)
            clock.mark('gather')
            ei, edge_ptr = build_edges_gpu(g['v'], g['node_ptr'], g['n_free'], g['k1'])
            clock.mark('graph_build')
            ws = lazysp_round(store, slot_of, ei, edge_ptr, maps)
            snaps.append(torch.stack((store.n_nodes.to(torch.int64), store.checks, store.n_pairs.to(torch.int64))))
            solved_h, status_h = torch.stack((store.solved, store.status)).cpu().numpy()      # the read that decides who continues
            del ws
            clock.mark('lazy_round')
            rounds_done[act] = r
            if raise_on_status and status_h[act].any():
                bad = act[status_h[act] != 0]
                raise RuntimeError('gnnmp_lazysp_round: status %s for problem(s) %s (1 = pair list full, 2 = loop bound, 4 = bad graph)'
                                   % (status_h[bad].tolist(), bad.tolist()))
            act = act[(solved_h[act] == 0) & (status_h[act] == 0)]
            if not act.size:
                break
        # ---- results: the store comes back in one go
        small = torch.stack((store.n_nodes, store.n_pairs, store.dijkstra_runs, store.path_len, store.solved, store.status)).cpu().numpy()
        n_nodes, n_pairs, runs, plen, solved, status = (small[i] for i in range(6))
        checks = store.checks.cpu().numpy()
        live = torch.arange(store.pair_cap, device=dev)[None, :] < store.n_pairs[:, None]
        pairs, pstate = store.pairs[live].cpu().numpy(), store.pair_state[live].cpu().numpy()
        pool, paths = store.pool.cpu().numpy(), store.path.cpu().numpy()
        snaps_h = torch.stack(snaps).cpu().numpy()                       # [rounds, 3, B]
    out, po = [], 0
    for b in range(B):
        pr_, st_ = pairs[po:po + n_pairs[b]], pstate[po:po + n_pairs[b]]
        po += n_pairs[b]
        ids = paths[b, :plen[b]].astype(np.int64)
        pts = pool[b, :n_nodes[b]].copy()
        rows = []
        for rr in range(int(rounds_done[b])):
            npr = int(snaps_h[rr, 2, b])
            nv = int((st_[:npr] == 1).sum())
            rows.append((int(snaps_h[rr, 0, b]), int(snaps_h[rr, 1, b]), nv, npr - nv))
        out.append({'samples': pts, 'checks': int(checks[b]), 'path_ids': ids, 'path': pts[ids], 'T': int(rounds_done[b]) * n,
                    'valid_edges': _unordered(pr_[st_ == 1]), 'invalid_edges': _unordered(pr_[st_ == 2]),
                    'dijkstra_runs': int(runs[b]), 'invalid_order': pr_[st_ == 2].astype(np.int64).reshape(-1, 2),
                    'rounds': np.array(rows, dtype=np.int64).reshape(-1, 4), 'success': bool(solved[b]), 'status': int(status[b])})
    clock.mark('results')
    return out


def eval_lazysp_device(env, indexes, seed=1234, seeds=None, batch=50, t_max=1000, k=10, device='cuda', chunk=256, rows_out=None,
                       timings=None, draws='host'):
    """The aggregates of the reference's ``eval_bit.eval_lazysp`` (eval_bit.py:138-151) with :func:`plan_maze_batch`, ``chunk``
    problems per batch: ``n_success``, ``collision`` (mean collision checks, sampling included), ``solution_cost`` (mean
    :func:`gnnmp.planner.path_cost` of the solved problems' float64 paths), ``paths`` and per-problem ``rows`` (success, checks,
    path cost, path nodes, N, dijkstra runs, T).  Problem ``indexes[i]`` draws from ``np.random.RandomState(seeds[i])``; default
    :func:`gnnmp.streams_batch.stream_seeds`.  The numbers DIFFER from ``eval_lazysp``'s, which walks ONE global stream problem after
    problem -- other samples of the same distribution -- and in exchange they do not depend on the order of ``indexes`` or on
    ``chunk``.  The global numpy generator is left alone."""
    from .planner import path_cost
    rows, paths = [], []
    for pr, chunk_seeds in eval_chunks(env, indexes, seed, seeds, chunk):
        for res in plan_maze_batch(pr, device, chunk_seeds, batch=batch, t_max=t_max, k=k, draws=draws, timings=timings):
            paths.append(res['path'])
            rows.append((int(res['success']), res['checks'], path_cost(res['path']) if res['success'] else 0.0, len(res['path_ids']),
                         res['samples'].shape[0], res['dijkstra_runs'], res['T']))
    if rows_out is not None:
        rows_out.extend(rows)
    n_success = sum(r[0] for r in rows)
    return {'n_success': n_success, 'collision': float(np.mean([r[1] for r in rows])),
            'solution_cost': float(sum(r[2] for r in rows if r[0])) / max(n_success, 1), 'paths': paths, 'rows': rows}
