"""Plain-Python restatement of the explorer's training supervision (train_explorer.py:124-176): the yardstick the device
pipeline (gnnmp.episodes, csrc/train_episode_kernels.hip) is held to on random batches.  Test infrastructure only.

Graphs are given as the batch arrays of gnnmp.episodes: edge_index [2, E] (graph-local, coalesced, symmetric), per-edge
float64 costs / free flags, per-edge float32 scores.  Cell (a, c) of the reference's dense P[target][source] is edge (c -> a).
"""
import heapq
import math
from fractions import Fraction

import numpy as np

RRT_EPS = 0.05
INF = float('inf')


# ---- (a) MazeEnv._edge_fp on float64 states (environment/maze_env.py:236-347)
def _cell(x, w):
    c = int((x + 1.0) * w / 2.0)
    return w - 1 if c > w - 1 else c


def _valid2(p):
    return -1.0 <= p[0] <= 1.0 and -1.0 <= p[1] <= 1.0


def _point_fp(m, p):
    if not _valid2(p):
        return False
    w = m.shape[0]
    return m[_cell(p[0], w), _cell(p[1], w)] == 0


def _segment_fp(m, l, r):
    w = m.shape[0]
    dc = abs(_cell(l[0], w) - _cell(r[0], w)) + abs(_cell(l[1], w) - _cell(r[1], w))
    if dc > 1 and abs(l[0] - r[0]) + abs(l[1] - r[1]) > RRT_EPS:
        mid = ((l[0] + r[0]) / 2.0, (l[1] + r[1]) / 2.0)
        if not _point_fp(m, mid):
            return False
        return _segment_fp(m, l, mid) and _segment_fp(m, mid, r)
    return True


def _edge_fp2(m, a, b):
    return _valid2(a) and _valid2(b) and _point_fp(m, a) and _point_fp(m, b) and _segment_fp(m, a, b)


def _valid3(s):
    return _valid2(s) and -0.4 <= s[2] <= 0.4


def _ends(x, y, z):
    theta = z / 0.4 * math.pi
    ox, oy = 0.1 * math.cos(theta), 0.1 * math.sin(theta)
    return (x - ox, y - oy), (x + ox, y + oy)


def _stick_fp(m, s):
    if not _valid3(s):
        return False
    a, b = _ends(s[0], s[1], s[2])
    return _point_fp(m, a) and _point_fp(m, b) and _segment_fp(m, a, b)


def _edge_fp3(m, s, t):
    if not (_valid3(s) and _valid3(t)) or not (_stick_fp(m, s) and _stick_fp(m, t)):
        return False
    d0, d1, d2 = t[0] - s[0], t[1] - s[1], t[2] - s[2]
    if abs(d2) > 0.4:
        d2 = d2 - 0.8 if d2 > 0 else d2 + 0.8
    a0, a1, a2 = abs(t[0] - s[0]), abs(t[1] - s[1]), abs(t[2] - s[2])
    a2 = min(a2, abs(a2 - 0.8))
    K = int(math.sqrt((a0 * a0 + a1 * a1) + a2 * a2) / 0.015)
    for k in range(1, K):
        r = k * 1. / K
        a, b = _ends(s[0] + r * d0, s[1] + r * d1, s[2] + r * d2)
        if not _edge_fp2(m, a, b):
            return False
    return True


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def norm64(d):
    """np.linalg.norm of a 2- or 3-vector: sqrt of a left-to-right dot with fused multiply-adds (numpy's BLAS dot)."""
    acc = d[0] * d[0]
    for x in d[1:]:
        acc = _fma(x, x, acc)
    return math.sqrt(acc)


def label_edges(points, edge_index, maze_map):
    """construct_graph's per-edge (free, cost) for one maze problem: points float64 [N, dim]."""
    dim = points.shape[1]
    pts = [tuple(float(x) for x in row) for row in points]
    E = edge_index.shape[1]
    free = np.zeros(E, dtype=np.uint8)
    cost = np.full(E, INF)
    memo = {}
    for e in range(E):
        s, t = int(edge_index[0, e]), int(edge_index[1, e])
        ok = _edge_fp2(maze_map, pts[s], pts[t]) if dim == 2 else _edge_fp3(maze_map, pts[s], pts[t])
        if ok:
            free[e] = 1
            key = (min(s, t), max(s, t))          # the norm of -d equals the norm of d
            if key not in memo:
                memo[key] = norm64([pts[t][i] - pts[s][i] for i in range(dim)])
            cost[e] = memo[key]
    return free, cost


# ---- (b) dijkstra (algorithm/dijkstra.py:49-76): extraction key (dist, id), strict relaxation over edges (v -> u)
def shortest_paths(N, edge_index, cost, goal):
    incoming = [[] for _ in range(N)]
    for e in range(edge_index.shape[1]):
        incoming[int(edge_index[1, e])].append((int(edge_index[0, e]), float(cost[e])))
    dist = [INF] * N
    prev = [-1] * N
    dist[goal] = 0.0
    prev[goal] = goal
    done = [False] * N
    heap = [(0.0, goal)]
    while heap:
        d, u = heapq.heappop(heap)
        if done[u] or d != dist[u]:
            continue
        done[u] = True
        for v, c in incoming[u]:
            alt = dist[u] + c
            if alt < dist[v]:
                dist[v] = alt
                prev[v] = u
                heapq.heappush(heap, (alt, v))
    dist = np.array(dist)
    return dist, np.array(prev, dtype=np.int64), int(np.isfinite(dist).sum())


# ---- (c) explore / policy_data (train_explorer.py:42-93) on per-edge scores
class _Clone:
    """The dense clone of the policy, sparse: row a = cells (a, c) for edges (c -> a), columns ascending."""

    def __init__(self, N, edge_index, scores, goal):
        self.goal = goal
        eid = {}
        for e in range(edge_index.shape[1]):
            eid[(int(edge_index[1, e]), int(edge_index[0, e]))] = e        # cell (target, source) -> edge id
        self.rows = [[] for _ in range(N)]
        for (a, c), e in sorted(eid.items()):
            self.rows[a].append((c, e))
        self.val = {}
        for (a, c), e in eid.items():
            self.val[(a, c)] = np.float32(1.0 if a == c == goal else (0.0 if a == c else scores[e]))
        self.eid = eid
        self.killed = set()            # columns of explored nodes (P[:, c] = 0)
        self.restored = False          # P[goal, goal] = 1 set again (policy_data, before the frontier is read)

    def present(self, a, c):
        if self.restored and a == c == self.goal:
            return True
        return c not in self.killed and self.val[(a, c)] != 0


def _row_best(cl, a):
    best = None
    for c, _ in cl.rows[a]:
        if cl.present(a, c) and (best is None or cl.val[(a, c)] > cl.val[(a, best)]):
            best = c
    return best


def _rollout(cl, edge_free, start, goal, steps, stop_at_goal):
    explored = [start]
    bests = [_row_best(cl, start)]
    step_i = None
    for step_i in range(steps):
        bp = None
        for i, c in enumerate(bests):
            if c is not None and (bp is None or cl.val[(explored[i], c)] > cl.val[(explored[bp], bests[bp])]):
                bp = i
        if bp is None:
            raise RuntimeError('empty frontier')
        a, c = explored[bp], bests[bp]
        if edge_free[cl.eid[(a, c)]]:
            explored.append(c)
            cl.killed.add(c)
            if c == goal:
                return explored, step_i, True
            bests = [_row_best(cl, r) if bests[i] == c else bests[i] for i, r in enumerate(explored[:-1])]
            bests.append(_row_best(cl, c))
        else:
            cl.val[(a, c)] = np.float32(0)
            if (c, a) in cl.val:
                cl.val[(c, a)] = np.float32(0)
            bests = [_row_best(cl, r) if r in (a, c) else bests[i] for i, r in enumerate(explored)]
    return explored, step_i, False


def explore(N, edge_index, edge_free, scores, start, goal, max_steps=1000):
    """(step, status): status 2 when the frontier empties (the reference's exception)."""
    cl = _Clone(N, edge_index, scores, goal)
    try:
        _, step_i, _ = _rollout(cl, edge_free, start, goal, max_steps, True)
    except RuntimeError:
        return -1, 2
    if step_i is None:
        return -1, 2
    return step_i, 0


def policy_frontier(N, edge_index, edge_free, scores, dist, prev, start, goal, step):
    """(frontier edge ids in the reference's order, next_edge_idx)."""
    cl = _Clone(N, edge_index, scores, goal)
    explored, _, _ = _rollout(cl, edge_free, start, goal, step, True)
    nn = explored[int(np.argmin([dist[x] for x in explored]))]
    cl.restored = True
    ids, rows, cols = [], [], []
    for a in explored:
        for c, e in cl.rows[a]:
            if cl.present(a, c):
                ids.append(e)
                rows.append(a)
                cols.append(c)
    pn = float(prev[nn]) if prev[nn] >= 0 else INF
    dr = np.float32(rows) - np.float32(nn)
    dc = np.float32(cols) - np.float32(pn)
    # torch's two-row norm: fmaf(dc, dc, dr * dr) in float32, sqrt in double.  Every value is an integer (or inf), so the
    # float64 sum below is exact and its one rounding to float32 is the fused one
    acc = (dc.astype(np.float64) * dc.astype(np.float64) + (dr * dr).astype(np.float64)).astype(np.float32)
    nrm = np.sqrt(acc.astype(np.float64)).astype(np.float32)
    return np.array(ids, dtype=np.int64), int(np.argmin(nrm)) if len(ids) else -1


def episode(N, edge_index, edge_free, cost, scores, goal, start, step_draw, max_steps=1000):
    """One sample: dist / prev, n_valid, explore step and status, and -- with ``step_draw(step)`` giving s in [0, step] --
    the frontier and label of policy_data."""
    dist, prev, nv = shortest_paths(N, edge_index, cost, goal)
    out = {'dist': dist, 'prev': prev, 'n_valid': nv, 'status': 0, 'step': -1, 'replay_step': -1,
           'frontier': np.zeros(0, dtype=np.int64), 'label': -1}
    if nv == 1:
        out['status'] = 1
        return out
    step, status = explore(N, edge_index, edge_free, scores, start, goal, max_steps)
    out['status'], out['step'] = status, step
    if status:
        return out
    s = step_draw(step)
    out['replay_step'] = s
    out['frontier'], out['label'] = policy_frontier(N, edge_index, edge_free, scores, dist, prev, start, goal, s)
    return out
