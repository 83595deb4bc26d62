"""Host restatement of the oracle path smoother for 2-D maze problems (the reference's smoother.py:67-151 over
environment/maze_env.py:236-326 and algorithm/dijkstra.py:34-76), index-based where the reference hashes waypoints.

It is the CPU anchor of ``gnnmp.oracle_smooth`` (tests/test_oracle_smooth_host.py holds it to the recorded reference runs
bit for bit) and the timing yardstick of tools/oracle_smooth_bench.py.  A waypoint is a numpy array of shape (2,) whose
dtype is float32 (an untouched input row, ``np.array(tuple of np.float32)``) or float64 (a perturbed or re-spaced one);
numpy's promotion then decides the arithmetic of every expression exactly as it does in the reference.

Where the reference follows Python's hashing this file (and the device) define an order: among queue entries of exactly
equal finite distance dijkstra pops the lowest index (STATUS_TIE is set, the result may differ from a reference run), and
paths with two identical waypoints are refused (STATUS_DUPLICATE: the reference would merge them as dictionary keys).
"""
import glob
import os

import numpy as np

RRT_EPS = 5e-2
CAP = 128                       # waypoints per path the device kernel holds

STATUS_DUPLICATE = 1            # two waypoints with identical coordinates: path returned unchanged
STATUS_CAP = 2                  # more than CAP waypoints: path returned unchanged
STATUS_UNREACHABLE = 4          # a prune round could not reach path[next]: the reference's except, path as before that round
STATUS_ORDER = 8                # the pruned path is not a subsequence of the input (the reference's re-spacing would raise)
STATUS_STACK = 16               # bisection stack overflow on the device (cannot happen for states in [-1, 1]^2)
STATUS_NODE_IDX = 32            # a replayed node_idx outside [1, len - 2]: trial skipped
STATUS_TIE = 64                 # dijkstra met two unvisited waypoints of equal finite distance (lowest index taken)
STOP_NONE, STOP_RANDOM, STOP_PRUNE = 0, 1, 2


class Maze:
    """MazeEnv's checker for dim = 2, collision_check_count included."""

    def __init__(self, maze_map):
        self.map = np.asarray(maze_map)
        self.w = int(self.map.shape[0])
        self.count = 0

    def transform(self, state):
        coord = ((state + 1.0) * self.w / 2.0).astype(int)
        coord[coord > self.w - 1] = self.w - 1
        return coord

    @staticmethod
    def valid(state):
        return bool((state >= -1.0).all() and (state <= 1.0).all())

    def state_fp(self, state):
        if not self.valid(state):
            return False
        self.count += 1
        c = self.transform(state)
        return self.map[c[0], c[1]] == 0

    def segment(self, left, right):
        if np.sum(np.abs(self.transform(left) - self.transform(right))) > 1 and np.sum(np.abs(left - right)) > RRT_EPS:
            mid = (left + right) / 2.0
            if not self.state_fp(mid):
                return False
            return self.segment(left, mid) and self.segment(mid, right)
        return True

    def edge_fp(self, a, b):
        if not self.valid(a) or not self.valid(b):
            return False
        if not self.state_fp(a) or not self.state_fp(b):
            return False
        return self.segment(a, b)


def to_waypoints(xy, is32):
    """[P, 2] float64 coordinates + per-waypoint float32 flags -> list of (2,) arrays of that dtype."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    is32 = np.broadcast_to(np.asarray(is32, dtype=bool), (len(xy),))
    return [np.array(p, dtype=np.float32 if f else np.float64) for p, f in zip(xy, is32)]


def from_waypoints(path):
    xy = np.array([p.astype(np.float64) for p in path], dtype=np.float64).reshape(-1, 2)
    return xy, np.array([p.dtype == np.float32 for p in path], dtype=bool)


def has_duplicates(path):
    seen = set()
    for p in path:
        k = (float(p[0]), float(p[1]))
        if k in seen:
            return True
        seen.add(k)
    return False


def node_index(u, length):
    """The device form of np.random.randint(1, len - 1): 1 + min(floor(u (len - 2)), len - 3)."""
    return 1 + min(int(np.floor(u * (length - 2))), length - 3)


def random_stage(path, env, action, node_idx, u, status):
    """random_path_smoother (smoother.py:67-82) with the draws supplied: action [R, 2], node_idx [R] or u [R]."""
    path = list(path)
    if len(path) <= 2:
        return path, status
    for t in range(len(action)):
        i = int(node_idx[t]) if node_idx is not None else node_index(float(u[t]), len(path))
        if i < 1 or i > len(path) - 2:
            status |= STATUS_NODE_IDX
            continue
        old = path[i]
        new = old + np.asarray(action[t], dtype=np.float64)
        if env.state_fp(new) and env.edge_fp(new, path[i - 1]) and env.edge_fp(new, path[i + 1]):
            if (np.linalg.norm(path[i + 1] - new) + np.linalg.norm(path[i - 1] - new)) < \
                    (np.linalg.norm(path[i + 1] - old) + np.linalg.norm(path[i - 1] - old)):
                path[i] = new
    return path, status


def _dijkstra(pts, free, status):
    """dijkstra() over the waypoints pts from pts[0]: free[a][b] = _edge_fp(pts[a], pts[b]); neighbours in index order,
    strict relaxation, lowest index among equal minima.  Returns prev (None = unreached) and the status."""
    m = len(pts)
    dist, prev, todo = [np.inf] * m, [None] * m, set(range(m))
    dist[0], prev[0] = 0, 0
    while todo:
        u = min(todo, key=lambda k: (dist[k], k))
        if np.isfinite(dist[u]) and sum(1 for k in todo if dist[k] == dist[u]) > 1:
            status |= STATUS_TIE
        todo.remove(u)
        for v in range(m):
            if free[u][v]:
                alt = dist[u] + np.linalg.norm(pts[u] - pts[v])
                if alt < dist[v]:
                    dist[v], prev[v] = alt, u
    return prev, status


def prune_stage(path, src, env, prune_iter, status):
    """prune_path (smoother.py:97-126).  ``src``: for every waypoint its index in the path the stage started from."""
    for _ in range(prune_iter):
        n = len(path)
        crit = [i for i in range(n) if i == 0 or i == n - 1 or not env.edge_fp(path[i - 1], path[i + 1])]
        new_path, new_src, failed = [path[0]], [src[0]], False
        for a, b in zip(crit[:-1], crit[1:]):
            pts = path[a:b + 1]
            free = [[env.edge_fp(p1, p2) for p2 in pts] for p1 in pts]
            prev, status = _dijkstra(pts, free, status)
            part, cur = [], b - a
            while cur != 0:
                if prev[cur] is None:
                    failed = True
                    break
                part.append(cur)
                cur = prev[cur]
            if failed:
                break
            for k in reversed(part):
                new_path.append(pts[k])
                new_src.append(src[a + k])
        if failed:
            return path, src, status | STATUS_UNREACHABLE
        path, src = new_path, new_src
        if len(path) == n:
            break
    return path, src, status


def respace(path, short_src):
    """joint_smoother_ratio's tail (smoother.py:140-150): dropped waypoints go back on the segment between kept ones."""
    path = list(path)
    a = 0
    for b in short_src:
        seg_a, seg_b = path[a], path[b]
        for i in range(a + 1, b):
            path[i] = (seg_b - seg_a) * (i - a) / (b - a) + seg_a
        a = b
    return path


def smooth(xy, is32, maze_map, action, node_idx=None, u=None, iters=5, random_iter=100, prune_iter=100, ratio=True,
           stop=STOP_NONE, trace=None):
    """One path.  action [>= iters, >= random_iter, 2]; node_idx / u [>= iters, >= random_iter].  ``stop``: end after the
    last iteration's random stage (STOP_RANDOM) or prune stage (STOP_PRUNE, before any re-spacing).  ``trace``: a list that
    receives (kind, xy, is32, checks so far) after every stage.  Returns (xy float64 [len, 2], is32, checks, status)."""
    path = to_waypoints(xy, is32)
    env = Maze(maze_map)
    status = 0
    if len(path) > CAP:
        status = STATUS_CAP
    elif has_duplicates(path):
        status = STATUS_DUPLICATE
    if status:
        return (*from_waypoints(path), 0, status)

    def note(kind, p):
        if trace is not None:
            trace.append((kind, *from_waypoints(p), env.count))

    for it in range(iters):
        last = it == iters - 1
        path, status = random_stage(path, env, action[it][:random_iter], None if node_idx is None else node_idx[it],
                                    None if u is None else u[it], status)
        note('random', path)
        if last and stop == STOP_RANDOM:
            break
        if has_duplicates(path):
            status |= STATUS_DUPLICATE
            break
        short, src, status = prune_stage(path, list(range(len(path))), env, prune_iter, status)
        note('prune', short)
        if (last and stop == STOP_PRUNE) or not ratio:
            path = short
        elif any(y <= x for x, y in zip(src[:-1], src[1:])):
            status |= STATUS_ORDER
            break
        else:
            path = respace(path, src)
        note('iter', path)
    return (*from_waypoints(path), env.count, status)


def smooth_batch(xy, path_ptr, is32, maps, action, node_idx=None, u=None, **kw):
    """The batch form the device call has: ragged paths [sumP, 2] with path_ptr [B + 1], maps [B, w, w], draws [B, ...]."""
    out_xy, out32, out_len, checks, status = [], [], [], [], []
    for b in range(len(path_ptr) - 1):
        lo, hi = int(path_ptr[b]), int(path_ptr[b + 1])
        r = smooth(xy[lo:hi], is32[lo:hi], maps[b], action[b], None if node_idx is None else node_idx[b],
                   None if u is None else u[b], **kw)
        out_xy.append(r[0]); out32.append(r[1]); out_len.append(len(r[0])); checks.append(r[2]); status.append(r[3])
    return (np.concatenate(out_xy).reshape(-1, 2), np.concatenate(out32), np.array(out_len, np.int32),
            np.array(checks, np.int64), np.array(status, np.int32))


KINDS = ('random', 'prune', 'iter')


def fixtures():
    """{name: dict of arrays} of every tests/golden/oracle_smooth_*.npz (recorded by tools/gen_golden_oracle_smooth.py)."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    out = {}
    for path in sorted(glob.glob(os.path.join(here, 'oracle_smooth_*.npz'))):
        with np.load(path) as f:
            out[os.path.basename(path)[len('oracle_smooth_'):-4]] = {k: f[k] for k in f.files}
    return out


def fixture_stages(fx):
    """[(kind, iteration, xy, is32, checks so far)] of a fixture, in order."""
    out = []
    for s, kind in enumerate(fx['stage_kind']):
        lo, hi = int(fx['stage_ptr'][s]), int(fx['stage_ptr'][s + 1])
        out.append((KINDS[int(kind)], s // 3, fx['stage_xy'][lo:hi], fx['stage_is32'][lo:hi], int(fx['stage_checks'][s])))
    return out
