"""Host restatement of the oracle path smoother for 3-D maze problems, the stick robot of MazeEnv(dim=3) (the reference's
smoother.py:67-151 over environment/maze_env.py:137-149, 245-347 and algorithm/dijkstra.py:34-76).  It is the dim = 3
companion of tests/oracle_smooth_host.py, whose stages (random_stage, prune_stage, respace, _dijkstra) it reuses: they are
written over ``env.state_fp`` / ``env.edge_fp`` and ``np.linalg.norm`` and do not care about the waypoints' width.

A waypoint is a numpy array of shape (3,), (x, y, z), of dtype float32 (an untouched input row) or float64 (perturbed or
re-spaced); numpy's promotion decides every expression as it does in the reference.  The norms are numpy's own
(``np.linalg.norm`` of a 3-vector is the host BLAS's dot, whose rounding the device kernel restates as: float64
fma(d2, d2, fma(d1, d1, d0 * d0)); float32 the three float32 squares summed left to right in double, rounded once;
tests/test_oracle_smooth3_host.py holds those two formulas to numpy on the recorded vectors).

The two hashing-dependent places are defined as in the 2-D file: lowest index among equal distances (STATUS_TIE), paths
with identical waypoints refused (STATUS_DUPLICATE).
"""
import glob
import os

import numpy as np

import oracle_smooth_host as H

LIMITS = np.array([1.0, 1.0, 8.0 * H.RRT_EPS])          # |x|, |y| and |z| (the orientation coordinate) of a valid state
Z_MAX = LIMITS[2]                                       # np.float64: a float32 z met with it is promoted, not the other way
FULL_TURN = 2 * Z_MAX                                   # z is periodic with this period in distances and displacements
STICK_LENGTH = 1.5 * 2 / 15
HALF_STICK = STICK_LENGTH / 2.
STEP = 0.015                                            # spacing of the interpolated sticks along an edge
CAP = H.CAP


class Maze3(H.Maze):
    """MazeEnv's checker for dim = 3.  state_fp / edge_fp look at the state's size, so the 2-D queries of a stick's two
    ends (size 2) fall through to the parent's point / segment code and sizes of 3 are handled here."""

    @staticmethod
    def valid(state):
        bound = LIMITS[:state.size]
        return bool(np.all(state <= bound) and np.all(-bound <= state))

    @staticmethod
    def ends(state):
        """The stick's two tips, float64 whatever the state's dtype: z / Z_MAX is already a float64."""
        angle = (state[2] / Z_MAX) * np.pi
        reach = HALF_STICK * np.array([np.cos(angle), np.sin(angle)])
        middle = np.asarray(state[:2])
        return middle - reach, middle + reach

    def state_fp(self, state):
        if state.size == 2:
            return super().state_fp(state)
        if not self.valid(state):
            return False                                 # before anything is counted
        tip0, tip1 = self.ends(state)
        return bool(super().state_fp(tip0) and super().state_fp(tip1) and self.segment(tip0, tip1))

    @staticmethod
    def distance(a, b):
        """The metric with z taken the short way round.  The shorter of the two z gaps goes back into the gap vector, i.e.
        is rounded to the states' common dtype, before squaring."""
        gap = np.abs(b - a)
        other_way = np.abs(gap[2] - FULL_TURN)           # float64 even for a float32 gap
        gap[2] = min(gap[2], other_way)
        return np.sqrt(np.square(gap).sum())

    def edge_fp(self, a, b):
        if a.size == 2:
            return super().edge_fp(a, b)
        if not (self.valid(a) and self.valid(b)):
            return False
        if not (self.state_fp(a) and self.state_fp(b)):
            return False
        move = b - a
        if abs(move[2]) > Z_MAX:                         # go round the short way; the result is stored in move's dtype
            move[2] -= np.copysign(FULL_TURN, move[2])
        n_steps = int(self.distance(a, b) / STEP)
        for k in range(1, n_steps):
            if not super().edge_fp(*self.ends(a + k * 1. / n_steps * move)):
                return False
        return True


def to_waypoints(xyz, is32):
    """[P, 3] float64 coordinates + per-waypoint float32 flags -> list of (3,) arrays of that dtype."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    is32 = np.broadcast_to(np.asarray(is32, dtype=bool), (len(xyz),))
    return [np.array(p, dtype=np.float32 if f else np.float64) for p, f in zip(xyz, is32)]


def from_waypoints(path):
    xyz = np.array([p.astype(np.float64) for p in path], dtype=np.float64).reshape(-1, 3)
    return xyz, np.array([p.dtype == np.float32 for p in path], dtype=bool)


def has_duplicates(path):
    return len({(float(p[0]), float(p[1]), float(p[2])) for p in path}) != len(path)


def _random_stage(path, env, action, node_idx, u, status, hook, it):
    """H.random_stage, trial by trial when a hook wants to see the perturbed waypoints."""
    if hook is None:
        return H.random_stage(path, env, action, node_idx, u, status)
    for t in range(len(action)):
        if len(path) > 2:
            i = int(node_idx[t]) if node_idx is not None else H.node_index(float(u[t]), len(path))
            if 1 <= i <= len(path) - 2:
                hook(it, t, path[i] + np.asarray(action[t], dtype=np.float64))
        path, status = H.random_stage(path, env, action[t:t + 1], None if node_idx is None else node_idx[t:t + 1],
                                      None if u is None else u[t:t + 1], status)
    return path, status


def smooth(xyz, is32, maze_map, action, node_idx=None, u=None, iters=5, random_iter=100, prune_iter=100, ratio=True,
           stop=H.STOP_NONE, trace=None, trial_hook=None):
    """One path, as tests/oracle_smooth_host.py's smooth: action [>= iters, >= random_iter, 3].  ``trial_hook(iteration,
    trial, perturbed waypoint)`` is called before every trial that has a valid index.  Returns (xyz float64 [len, 3], is32,
    checks, status)."""
    path = to_waypoints(xyz, is32)
    env = Maze3(maze_map)
    status = 0
    if len(path) > CAP:
        status = H.STATUS_CAP
    elif has_duplicates(path):
        status = H.STATUS_DUPLICATE
    if status:
        return (*from_waypoints(path), 0, status)

    def note(kind, p):
        if trace is not None:
            trace.append((kind, *from_waypoints(p), env.count))

    for it in range(iters):
        last = it == iters - 1
        path, status = _random_stage(path, env, action[it][:random_iter], None if node_idx is None else node_idx[it],
                                     None if u is None else u[it], status, trial_hook, it)
        note('random', path)
        if last and stop == H.STOP_RANDOM:
            break
        if has_duplicates(path):
            status |= H.STATUS_DUPLICATE
            break
        short, src, status = H.prune_stage(path, list(range(len(path))), env, prune_iter, status)
        note('prune', short)
        if (last and stop == H.STOP_PRUNE) or not ratio:
            path = short
        elif any(y <= x for x, y in zip(src[:-1], src[1:])):
            status |= H.STATUS_ORDER
            break
        else:
            path = H.respace(path, src)
        note('iter', path)
    return (*from_waypoints(path), env.count, status)


def smooth_batch(xyz, path_ptr, is32, maps, action, node_idx=None, u=None, **kw):
    """The batch form the device call has: ragged paths [sumP, 3] with path_ptr [B + 1], maps [B, w, w], draws [B, ...]."""
    out_xyz, out32, out_len, checks, status = [], [], [], [], []
    for b in range(len(path_ptr) - 1):
        lo, hi = int(path_ptr[b]), int(path_ptr[b + 1])
        r = smooth(xyz[lo:hi], is32[lo:hi], maps[b], action[b], None if node_idx is None else node_idx[b],
                   None if u is None else u[b], **kw)
        out_xyz.append(r[0]); out32.append(r[1]); out_len.append(len(r[0])); checks.append(r[2]); status.append(r[3])
    return (np.concatenate(out_xyz).reshape(-1, 3), np.concatenate(out32), np.array(out_len, np.int32),
            np.array(checks, np.int64), np.array(status, np.int32))


def z_rejected_trials(xyz, is32, maze_map, action, node_idx, **kw):
    """[(iteration, trial)] of the trials whose perturbed waypoint stays inside the map but leaves |z| <= LIMITS[2]: the ones
    _valid_state rejects for the orientation alone, before any check is counted."""
    hits = []

    def hook(it, t, new):
        if (np.abs(new[:2]) <= LIMITS[:2]).all() and np.abs(new[2]) > LIMITS[2]:
            hits.append((it, t))
    smooth(xyz, is32, maze_map, action, node_idx=node_idx, trial_hook=hook, **kw)
    return hits


def fixtures():
    """{name: dict of arrays} of every tests/golden/oracle_smooth3_*.npz (recorded by tools/gen_golden_oracle_smooth3.py)."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    out = {}
    for path in sorted(glob.glob(os.path.join(here, 'oracle_smooth3_*.npz'))):
        with np.load(path) as f:
            out[os.path.basename(path)[len('oracle_smooth3_'):-4]] = {k: f[k] for k in f.files}
    return out


def fixture_stages(fx):
    """[(kind, iteration, xyz, is32, checks so far)] of a fixture, in order."""
    out = []
    for s, kind in enumerate(fx['stage_kind']):
        lo, hi = int(fx['stage_ptr'][s]), int(fx['stage_ptr'][s + 1])
        out.append((H.KINDS[int(kind)], s // 3, fx['stage_xy'][lo:hi], fx['stage_is32'][lo:hi], int(fx['stage_checks'][s])))
    return out
