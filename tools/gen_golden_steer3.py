#!/usr/bin/env python
"""Record tests/golden/steer3_*.npz: the collision-checked steering of the smoothing stage for the stick robot, computed
by the UNMODIFIED reference function proposed_path_smootherv2 (smoother.py:194-216) over MazeEnv(dim=3) on maps of
maze_files/mazes_hard_3.npz.

The dim = 3 steering companion of tools/gen_golden_oracle_smooth3.py (same stand-ins, same way of importing the
reference; runs only in the authoring container).  What is written is data: the map, old_path / new_path (float32 [P, 3]),
the returned path, the collision checks spent, whether the reference raised, and small annotations saying which behaviour
the case shows.  Every case is CHECKED here to show the behaviour its name promises: a second MazeEnv on the same map (so
the recorded count is not disturbed) replays the rounds through the reference's own interpolate / _edge_fp, must arrive at
the recorded path and count, and reports per round and waypoint what happened.

The hard maps are walled on all four sides and their corridors are one cell (0.133) wide and at most 13 cells long, so a
free edge has K = int(d / 0.015) <= ~110: the K >= 150 case of ``long_edge`` is an edge between two free configurations
that is blocked on its way (the one with the farthest first blocked k that the search finds: the wave stops in its first
pass), and the waypoint of ``out_of_map`` starts inside the wall next to the border.  ``long_edge_2pass`` is the longest
FREE edge the search finds, K > 66 asserted: the wave finishes its first pass and runs a second to the end.  Three free passes
(K >= 130) are covered by tests/test_stick_steer_gpu.py on a map of its own against the host steering these cases pin.
"""
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
os.environ.setdefault('CUDA_VISIBLE_DEVICES', '')
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, 'tools', 'standins'))
sys.modules.setdefault('tensorboardX', types.SimpleNamespace(SummaryWriter=None))

import numpy as np  # noqa: E402

os.chdir(REF)
from environment import MazeEnv  # noqa: E402
import smoother as ref  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
MAP_FILE = 'maze_files/mazes_hard_3.npz'
EPS = MazeEnv.RRT_EPS
f32 = np.float32


def row(*x):
    return np.array(x, dtype=np.float32)


def edge_info(probe, s, t):
    """(free, K, first blocked k or 0, checks) of probe._edge_fp(s, t).  The interior configurations are checked through
    nested two-element _edge_fp calls, one per k: counting them tells where the edge stopped."""
    inner = []
    orig = MazeEnv._edge_fp

    def counted(state, new_state):
        if state.size == 2:
            inner.append(1)
        return orig(probe, state, new_state)

    c0 = probe.collision_check_count
    probe._edge_fp = counted
    try:
        free = bool(orig(probe, s, t))
    finally:
        del probe._edge_fp
    K = int(probe.distance(s, t)[0] / 0.015) if probe._valid_state(s) and probe._valid_state(t) else 0
    return free, K, (len(inner) if not free and inner else 0), probe.collision_check_count - c0


def replay(probe, old, new):
    """The rounds of the steering through the reference's own interpolate / _edge_fp on ``probe``.  Returns the path, the
    checks spent and one record per (round, waypoint)."""
    probe.collision_check_count = 0
    K = int(np.ceil((np.linalg.norm(old - new, axis=-1) / EPS).max()))
    path = [r.copy() for r in old]
    log = []
    for rnd in range(K):
        left_over = 0
        nxt = [r.copy() for r in path]
        for i in range(1, len(path) - 1):
            gap = np.linalg.norm(path[i] - new[i])
            near = bool(gap < EPS)
            rec = dict(round=rnd, i=i, near=near, wrap_disp=False, wrap_state=False)
            if near:
                cand = new[i]
            else:
                step = new[i] - path[i]
                rec['wrap_disp'] = bool(abs(float(step[2])) > 0.4)
                if rec['wrap_disp']:
                    step[2] += -0.8 if step[2] > 0 else 0.8
                before_wrap = path[i] + step * (EPS / gap)
                rec['wrap_state'] = bool(abs(float(before_wrap[2])) > 0.4)
                cand = probe.interpolate(path[i], new[i], EPS / gap)
            c0 = probe.collision_check_count
            e_left = edge_info(probe, nxt[i - 1], cand)
            e_right = edge_info(probe, nxt[i + 1], cand) if e_left[0] else None
            ok = e_left[0] and e_right[0]
            rec.update(cand=cand.copy(), valid=bool(probe._valid_state(cand)), left=e_left, right=e_right, accepted=ok,
                       checks=probe.collision_check_count - c0, left_moved=bool((nxt[i - 1] != path[i - 1]).any()),
                       left_old=path[i - 1].copy(), left_new=nxt[i - 1].copy())
            if ok:
                nxt[i] = cand
                left_over += np.linalg.norm(cand - new[i])
            log.append(rec)
        path = nxt
        if left_over < 1e-5:
            break
    return np.array(path, dtype=np.float32).reshape(-1, 3), probe.collision_check_count, log, K


class Recorder:
    def __init__(self):
        self.env = MazeEnv(dim=3, map_file=MAP_FILE)
        self.probe = MazeEnv(dim=3, map_file=MAP_FILE)

    def problem(self, index):
        self.env.init_new_problem(index)
        self.probe.init_new_problem(index)
        self.index = index

    def free(self, c):
        c0 = self.probe.collision_check_count
        ok = bool(self.probe._state_fp(c))
        self.probe.collision_check_count = c0
        return ok

    def run(self, old, new):
        """The reference on one path: (path or None, checks, raised)."""
        old = np.ascontiguousarray(old, dtype=np.float32).reshape(-1, 3)
        new = np.ascontiguousarray(new, dtype=np.float32).reshape(-1, 3)
        self.env.collision_check_count = 0
        try:
            out = ref.proposed_path_smootherv2([r.copy() for r in old], new.copy(), self.env)
        except AssertionError:
            return None, int(self.env.collision_check_count), True
        return np.array(out, dtype=np.float32).reshape(-1, 3), int(self.env.collision_check_count), False

    def record(self, name, old, new, want=None, note=''):
        old = np.ascontiguousarray(old, dtype=np.float32).reshape(-1, 3)
        new = np.ascontiguousarray(new, dtype=np.float32).reshape(-1, 3)
        out, checks, raised = self.run(old, new)
        info = dict(old=old, new=new, out=out, checks=checks, raised=raised, log=[], K=None)
        if not raised:
            again, c2, _ = self.run(old, new)
            assert again.tobytes() == out.tobytes() and c2 == checks, name + ': the reference run does not repeat'
            rp, rc, log, K = replay(self.probe, old, new)
            assert rp.tobytes() == out.tobytes() and rc == checks, (name, 'replay differs', rc, checks)
            info.update(log=log, K=K)
        info['accepted'] = [r['accepted'] for r in info['log']]
        if want is not None and not want(info):
            return None
        log = info['log']
        rounds = (max(r['round'] for r in log) + 1) if log else 0
        edge_k = np.array([[e[1], e[2]] for r in log for e in (r['left'], r['right']) if e is not None],
                          dtype=np.int32).reshape(-1, 2)
        path = os.path.join(OUT, 'steer3_%s.npz' % name)
        np.savez_compressed(
            path, map=self.env.map.astype(np.uint8), problem=np.int32(self.index), old_path=old, new_path=new,
            result=out if out is not None else np.zeros((0, 3), dtype=np.float32), checks=np.int64(0 if raised else checks),
            raised=np.bool_(raised), K=np.int32(-1 if info['K'] is None else info['K']), rounds=np.int32(rounds),
            accepted=np.array([r['accepted'] for r in log], dtype=bool), edge_k=edge_k, note=np.str_(note))
        print('%-16s problem %4d P=%2d K=%3s rounds=%2d checks=%6d raised=%d moved=%d maxedgeK=%3d  %4.1f KB  %s'
              % (name, self.index, len(old), info['K'], rounds, checks, raised,
                 0 if out is None else int((out != old).any(axis=1).sum()), edge_k[:, 0].max() if len(edge_k) else 0,
                 os.path.getsize(path) / 1024, note), flush=True)
        return info

    # ---- material ---------------------------------------------------------------------------------------------------
    def free_configs(self, n, rng):
        out = []
        while len(out) < n:
            c = rng.uniform([-1, -1, -0.4], [1, 1, 0.4]).astype(np.float32)
            if self.free(c):
                out.append(c)
        return out

    def near_free(self, c, rng, z=None):
        """A free configuration beside c whose edge to c is free; ``z``: draws its orientation coordinate."""
        for _ in range(300):
            cnd = (c + row(*rng.normal(0, 0.05, 2), rng.normal(0, 0.02))).astype(np.float32)
            if z is not None:
                cnd[2] = z()
            if self.probe._valid_state(cnd) and self.free(cnd) and edge_info(self.probe, cnd, c)[0]:
                return cnd
        return None

    def triple(self, rng, zcond, left_z=None):
        """[a, c, b]: c a free configuration whose z satisfies zcond, a and b free beside it with free edges to it."""
        while True:
            c = self.free_configs(1, rng)[0]
            if not zcond(float(c[2])):
                continue
            a, b = self.near_free(c, rng, left_z), self.near_free(c, rng)
            if a is not None and b is not None:
                return np.array([a, c, b], dtype=np.float32)

    def graph_path(self, rng, n=250, k=8, lo=10, hi=12):
        """A free path of lo .. hi waypoints between two of n free configurations over their k-nearest free edges."""
        pts = self.free_configs(n, rng)
        arr = np.array(pts)
        nbr = {}
        for a in range(n):
            d = self.probe.distance(arr[a], arr)
            nbr[a] = [int(b) for b in np.argsort(d)[1:k + 1] if edge_info(self.probe, pts[a], pts[int(b)])[0]]
        for start in range(n):
            prev, order = {start: start}, [start]
            for a in order:
                for b in nbr[a]:
                    if b not in prev:
                        prev[b] = a
                        order.append(b)
            for goal in reversed(order):
                p = [goal]
                while p[-1] != start:
                    p.append(prev[p[-1]])
                if lo <= len(p) <= hi:
                    return np.array([pts[a] for a in p], dtype=np.float32)
        return None

    def edge_search(self, rng, want, tries=4000, dmin=0.05, dmax=2.6, target_fk=None):
        """Random pairs of free configurations until ``want(free, K, first blocked k)``; returns the best by want's score.
        ``target_fk``: a blocked edge is tried again with its start moved along the edge so that the blocked place comes
        to lie about target_fk steps from it."""
        best, best_score = None, 0
        for _ in range(tries):
            s = self.free_configs(1, rng)[0]
            d = rng.uniform(dmin, dmax)
            ang = rng.uniform(0, 2 * np.pi)
            t = (s + row(d * np.cos(ang), d * np.sin(ang), rng.uniform(-0.3, 0.3))).astype(np.float32)
            if axis_aligned(rng):
                t = (s + row(d, 0, 0) * rng.choice([-1, 1]) if rng.rand() < 0.5 else s + row(0, d, 0) * rng.choice([-1, 1]))
                t = t.astype(np.float32)
            if not self.probe._valid_state(t) or not self.free(t):
                continue
            free, K, fk, _ = edge_info(self.probe, s, t)
            score = want(free, K, fk)
            if score == 0 and target_fk is not None and fk > 0:
                s2 = (s + (t - s) * f32((fk - target_fk + rng.uniform(-0.4, 0.4)) / K)).astype(np.float32)
                if self.probe._valid_state(s2) and self.free(s2):
                    free, K, fk, _ = edge_info(self.probe, s2, t)
                    s, score = s2, want(free, K, fk)
            if score > best_score:
                best, best_score = (s, t, free, K, fk), score
                if score >= 1000:
                    break
        return best


def axis_aligned(rng):
    return rng.rand() < 0.6


def three(s, t, third, back=0.02):
    """old = [s, t - a little, third], new = [s, t, third]: the proposal of the one interior waypoint is within RRT_EPS, so
    the candidate is t itself and the first edge check is _edge_fp(s, t)."""
    d = (s - t)[:2]
    d = d / max(np.linalg.norm(d), 1e-9) * back
    mid = (t + row(d[0], d[1], 0)).astype(np.float32)
    return np.array([s, mid, third], dtype=np.float32), np.array([s, t, third], dtype=np.float32)


def main():
    R = Recorder()
    rng = np.random.RandomState(20240607)

    # ---- ordinary paths, and the short ones cut from the first
    R.problem(3)
    kept = []
    for j, index in enumerate((3, 41)):
        R.problem(index)
        for attempt in range(20):
            p = R.graph_path(rng)
            if p is None:
                continue
            noise = np.concatenate((rng.normal(0, 0.07, (len(p), 2)), rng.normal(0, 0.05, (len(p), 1))), axis=1)
            new = (p + noise).astype(np.float32)
            new[0], new[-1] = p[0], p[-1]
            ok = R.record('p12_%d' % j, p, new, note='ordinary path',
                          want=lambda c: not c['raised'] and c['K'] >= 3 and sum(c['accepted']) >= 5
                          and not all(c['accepted']))
            if ok:
                kept.append((index, p, new))
                break
        else:
            raise SystemExit('no ordinary path on problem %d' % index)
    index, p, new = kept[0]
    R.problem(index)
    c = R.record('len2', p[:2], new[:2] + row(0.03, 0, 0), note='P = 2: nothing to steer')
    assert c['checks'] == 0 and c['out'].tobytes() == p[:2].tobytes()
    for a in range(len(p) - 2):
        c = R.record('len3', p[a:a + 3], new[a:a + 3], note='one interior waypoint',
                     want=lambda c: any(c['accepted']) and c['K'] >= 2)
        if c:
            break
    assert c, 'len3'
    c = R.record('noop', p, p.copy(), note='proposal equals the path: K = 0')
    assert c['K'] == 0 and c['checks'] == 0 and c['out'].tobytes() == p.tobytes()

    # ---- arrive: every interior proposal within RRT_EPS and free; the end point's proposal is far, so K > 1 and the run
    # ends after round 1 through diff < 1e-5
    for attempt in range(200):
        new = p.copy()
        new[1:-1] += np.concatenate((rng.normal(0, 0.012, (len(p) - 2, 2)), rng.normal(0, 0.01, (len(p) - 2, 1))), axis=1)
        new = new.astype(np.float32)
        new[0] = p[0] + row(0.2, 0, 0)
        c = R.record('arrive', p, new, note='all proposals within RRT_EPS: taken as is, exit after round 1 of K',
                     want=lambda c: c['K'] >= 4 and max(r['round'] for r in c['log']) == 0
                     and all(r['near'] and r['accepted'] for r in c['log']))
        if c:
            assert c['out'][1:-1].tobytes() == new[1:-1].tobytes()
            break
    assert c, 'arrive'

    # ---- revert: a move rejected in a round in which the left neighbour moved, and where the left neighbour's OLD value
    # would have given another verdict or another count for that edge
    def revert(c, verdict):
        for r in c['log']:
            if r['left_moved'] and not r['accepted'] and r['valid']:
                alt = edge_info(R.probe, r['left_old'], r['cand'])
                if alt[0] != r['left'][0] or (not verdict and alt[3] != r['left'][3]):
                    c['revert_at'] = (r['round'], r['i'], alt[0], r['left'][0])
                    return True
        return False
    for attempt in range(1500):
        noise = np.concatenate((rng.normal(0, 0.12, (len(p), 2)), rng.normal(0, 0.08, (len(p), 1))), axis=1)
        new = (p + noise).astype(np.float32)
        c = R.record('revert', p, new, want=lambda c: not c['raised'] and revert(c, attempt < 1200),
                     note='a rejected move beside a left neighbour that moved in the same round')
        if c:
            print('   revert at (round, i, free with old left, free with new left) =', c['revert_at'])
            break
    assert c, 'revert'

    # ---- orientation wraps.  A free configuration with room around it, from the path
    def variant(name, make, want, note, tries=400, zcond=None, left_z=None):
        for attempt in range(tries):
            a = rng.randint(0, len(p) - 2)
            old, new = make(p[a:a + 3].copy() if zcond is None else R.triple(rng, zcond, left_z))
            c = R.record(name, old, new, want=lambda c: not c['raised'] and want(c), note=note)
            if c:
                return c
        raise SystemExit('no case for ' + name)

    def mk_disp(q):
        q[1][2] = rng.uniform(0.25, 0.39) * rng.choice([-1, 1])
        n = q.copy()
        n[1][2] = -q[1][2] + rng.uniform(-0.05, 0.05)
        n[1][:2] += rng.normal(0, 0.02, 2)
        return q, n.astype(np.float32)
    variant('zwrap_disp', mk_disp, lambda c: any(r['wrap_disp'] and r['accepted'] for r in c['log']),
            '|dz| > 0.4 between waypoint and proposal: displacement wrapped')

    def mk_state(q):
        n = q.copy()
        n[1][2] = np.sign(q[1][2]) * rng.uniform(0.55, 0.75)
        return q, n.astype(np.float32)
    variant('zwrap_state', mk_state, lambda c: any(r['wrap_state'] and r['accepted'] for r in c['log']),
            'interpolated z leaves +-0.4 and is wrapped back', zcond=lambda z: abs(z) > 0.365)

    def mk_edge(q):
        n = q.copy()
        n[1][:2] += rng.normal(0, 0.04, 2)
        n[1][2] += rng.normal(0, 0.01)
        return q, n.astype(np.float32)
    variant('zwrap_edge', mk_edge, zcond=lambda z: z > 0.3, left_z=lambda: -rng.uniform(0.3, 0.4),
            want=
            lambda c: any(r['accepted'] and abs(float(r['cand'][2]) - float(r['left_new'][2])) > 0.4 and r['left'][1] >= 3
                          for r in c['log']),
            note='neighbouring waypoints with |dz| > 0.4: the edge check interpolates along the wrapped displacement')

    def mk_invalid(q):
        n = q.copy()
        n[1][2] = np.sign(q[1][2]) * 0.42
        return q, n.astype(np.float32)
    c = variant('invalid_near', mk_invalid, zcond=lambda z: abs(z) > 0.38, want=
                lambda c: all(r['near'] and not r['valid'] and not r['accepted'] and r['checks'] == 0 for r in c['log'])
                and c['checks'] == 0 and len(c['log']) == 1,
                note='proposal within RRT_EPS with z outside +-0.4: rejected with zero checks')
    assert c['out'].tobytes() == c['old'].tobytes()

    # ---- out_of_map: the waypoint sits in the wall beside the border (the steering does not ask whether the path it is
    # given is free), its proposal beyond x = 1; its neighbour cannot move (the edge to the wall is blocked), the waypoint
    # before that one moves normally
    def mk_out(q):
        old = np.array([q[0], q[1], q[2], row(0.97, q[2][1], q[2][2]), q[0]], dtype=np.float32)
        n = old.copy()
        n[3][0] = 1.3
        n[1][:2] += rng.normal(0, 0.04, 2)
        return old, n.astype(np.float32)
    variant('out_of_map', mk_out,
            lambda c: any(not r['near'] and not r['valid'] and r['checks'] == 0 for r in c['log'])
            and any(r['accepted'] for r in c['log']),
            'proposal outside x = 1: the candidate is invalid, zero checks, rejected')

    # ---- long edges and where they fail: pairs of free configurations from a random search on a map with long corridors
    R.problem(0)

    def edge_case(name, want, note, given=None, **kw):
        best = given if given is not None else R.edge_search(rng, want, **kw)
        assert best is not None, name
        s, t, free, K, fk = best
        # the third waypoint: a free configuration next to t (else any free one)
        third = R.free_configs(1, rng)[0]
        for _ in range(200):
            cnd = (t + row(*rng.normal(0, 0.05, 2), rng.normal(0, 0.03))).astype(np.float32)
            if R.probe._valid_state(cnd) and R.free(cnd) and edge_info(R.probe, cnd, t)[0]:
                third = cnd
                break
        old, new = three(s, t, third)
        c = R.record(name, old, new, note=note + ' (edge K = %d, first blocked k = %d)' % (K, fk),
                     want=lambda c: len(c['log']) == 1 and c['log'][0]['near'] and c['log'][0]['left'][1:3] == (K, fk))
        assert c, name
        return c

    edge_case('long_edge_64', lambda f, K, fk: 1000 if f and K == 64 else 0, 'a free edge of K = 64: one pass of 63 lanes',
              dmin=0.955, dmax=0.98, tries=20000)
    edge_case('long_edge_65', lambda f, K, fk: 1000 if f and K == 65 else 0, 'a free edge of K = 65: one full pass',
              dmin=0.97, dmax=0.995, tries=20000)
    # K >= 150 needs d >= 2.25: only from one corner cell to the opposite one, with a large orientation gap besides
    def corner_pairs(tries):
        lo, hi = -1 + 2 / 15, -1 + 4 / 15
        for _ in range(tries):
            s = row(rng.uniform(lo, hi), rng.uniform(lo, hi), rng.uniform(-0.4, 0.4))
            t = row(-rng.uniform(lo, hi), -rng.uniform(lo, hi), rng.uniform(-0.4, 0.4))
            if rng.rand() < 0.5:
                s[1], t[1] = -s[1], -t[1]
            if R.free(s) and R.free(t):
                yield s, t
    found = None
    for index150 in range(0, 60):
        R.problem(index150)
        for s, t in corner_pairs(300):
            free, K, fk, _ = edge_info(R.probe, s, t)
            if K >= 150 and (found is None or fk > found[5]):
                found = (index150, s, t, free, K, fk)
        if found is not None and found[5] >= 8:
            break
    assert found is not None, 'long_edge_150'
    R.problem(found[0])
    edge_case('long_edge_150', None, 'an edge of K >= 150 between free configurations; no such edge is free on these maps',
              given=found[1:])
    R.problem(0)
    edge_case('fail_first', lambda f, K, fk: 1000 if fk == 1 and K >= 3 else 0, 'an edge blocked at k = 1', dmax=0.6,
              target_fk=1)
    edge_case('fail_lane63', lambda f, K, fk: 1000 if fk == 64 else 0, 'an edge blocked first at k = 64', dmin=0.99,
              tries=40000, target_fk=64)
    edge_case('fail_pass2', lambda f, K, fk: 1000 if fk > 64 else 0, 'an edge blocked first at some k > 64', dmin=1.0,
              tries=40000)

    # ---- assert_z: a proposal more than 1.2 in z from its waypoint
    R.problem(index)
    old = p[:4].copy()
    old[2][2] = -0.35
    new = old.copy()
    new[2][2] = 0.95
    new[1][:2] += row(0.03, 0.02)
    c = R.record('assert_z', old, new, note='proposal z more than 1.2 from its waypoint: interpolate asserts')
    assert c['raised']

    # ---- two passes run to the end: a FREE edge of K > 66 along a long corridor (a generator of its own: the cases above keep theirs)
    rng2 = np.random.RandomState(20240608)
    best = None
    for index2 in range(0, 60):
        R.problem(index2)
        got = R.edge_search(rng2, lambda f, K, fk: K if f and K > 66 else 0, tries=1500, dmin=1.02, dmax=1.7)
        if got is not None and (best is None or got[3] > best[1][3]):
            best = (index2, got)
        if best is not None and best[1][3] >= 80:
            break
    assert best is not None, 'long_edge_2pass'
    R.problem(best[0])
    s, t, free, K, fk = best[1]
    assert free and K > 66 and fk == 0
    c = edge_case('long_edge_2pass', None, 'a free edge of K > 66: the second pass runs to its end', given=best[1])
    left = c['log'][0]['left']
    assert left[0] and left[1] == K and K > 66 and c['log'][0]['accepted'], 'long_edge_2pass is not free'


if __name__ == '__main__':
    main()
