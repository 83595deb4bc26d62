"""Steering of the smoothing stage for the stick robot on the device (maze_kernels.hip: maze_steer_kernel<3>, one
wavefront per problem, the interpolated sticks of every edge check spread over the lanes) through
planner.steer_maze_batch / gnnmp_stick_steer: bit-identical paths and identical check counts against
tests/golden/steer3_*.npz (recorded from the unmodified reference, tools/gen_golden_steer3.py), the status word, and
the smoothing stage of the rounds planner against the host counterpart."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_files, load_weights
import gnnmp
from gnnmp import _lib, planner
from gnnmp.maze2d import Maze3D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _load(path):
    with np.load(path) as f:
        c = {k: f[k] for k in f.files}
    c['name'] = os.path.basename(path)[len('steer3_'):-len('.npz')]
    return c


ALL = [_load(p) for p in golden_files('steer3_')]
CASES = [c for c in ALL if not bool(c['raised'])]
RAISING = [c for c in ALL if bool(c['raised'])]
_singles = {}


def _steer(cases, checks0=None):
    """One launch over the cases as a ragged batch: per case (path, checks, status), all read back."""
    lens = [len(c['old_path']) for c in cases]
    ptr = torch.tensor(np.concatenate(([0], np.cumsum(lens))), dtype=torch.int32, device=DEV)
    old = torch.from_numpy(np.concatenate([c['old_path'] for c in cases])).to(DEV)
    new = torch.from_numpy(np.concatenate([c['new_path'] for c in cases])).to(DEV)
    maps = torch.from_numpy(np.stack([c['map'].astype(np.float64) for c in cases])).to(DEV)
    kw = {} if checks0 is None else {'checks': torch.tensor(checks0, dtype=torch.int64, device=DEV)}
    out, checks, status = planner.steer_maze_batch(old, new, ptr, maps, **kw)
    out, checks, status = out.cpu().numpy(), checks.cpu().tolist(), status.cpu().tolist()
    offs = np.concatenate(([0], np.cumsum(lens)))
    return [(out[offs[i]:offs[i + 1]], int(checks[i]), int(status[i])) for i in range(len(cases))]


def _single(c):
    if c['name'] not in _singles:
        _singles[c['name']] = _steer([c])[0]
    return _singles[c['name']]


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_single_problem_equals_the_reference(c):
    path, checks, status = _single(c)
    print('\n%s: checks device %d reference %d, status %d, waypoints differing %d' % (
        c['name'], checks, int(c['checks']), status, int((path != c['result']).any(axis=1).sum())))
    assert status == 0
    assert path.tobytes() == c['result'].tobytes()
    assert checks == int(c['checks'])


@pytest.mark.parametrize('reverse', [False, True], ids=['fixture_order', 'reversed'])
def test_ragged_batch_equals_the_singles(reverse):
    cases = CASES[::-1] if reverse else CASES
    assert len({c['map'].tobytes() for c in cases}) > 1                   # several maps: per-problem map staging
    for c, (path, checks, status) in zip(cases, _steer(cases)):
        sp, sc, ss = _single(c)
        assert (path.tobytes(), checks, status) == (sp.tobytes(), sc, ss), c['name']
        assert path.tobytes() == c['result'].tobytes() and checks == int(c['checks']) and status == 0, c['name']


def test_assert_case_sets_status_and_leaves_the_others_alone():
    assert RAISING and all(c['name'] == 'assert_z' for c in RAISING)
    bad = RAISING[0]
    cases = [CASES[0], bad, CASES[1], CASES[2]]
    start = [7, 11, 13, 17]
    got = _steer(cases, checks0=start)
    path, checks, status = got[1]
    assert status == 1
    assert path.tobytes() == bad['old_path'].tobytes()
    assert checks == 11                                                    # left as it was
    for i in (0, 2, 3):
        c = cases[i]
        assert got[i][2] == 0 and got[i][0].tobytes() == c['result'].tobytes(), c['name']
        assert got[i][1] == start[i] + int(c['checks']), c['name']         # incremented, not overwritten


def test_two_runs_are_bit_identical():
    a, b = _steer(CASES), _steer(CASES)
    assert all(x[0].tobytes() == y[0].tobytes() and x[1:] == y[1:] for x, y in zip(a, b))


def test_width_two_goes_to_the_point_robot_kernel_unchanged():
    rng = np.random.RandomState(5)
    lens = [8, 2, 11]
    # sparse maps of the test's own (in the fixtures' walled mazes random waypoints sit in walls and nothing would move)
    maps = (rng.rand(3, 15, 15) < 0.08).astype(np.float64)
    # short-stepped walks, so that most edges are free and waypoints do move
    old = np.concatenate([np.clip(rng.uniform(-0.4, 0.4, 2) + np.cumsum(rng.normal(0, 0.08, (n, 2)), axis=0), -0.9, 0.9)
                          for n in lens]).astype(np.float32)
    new = (old + rng.normal(0, 0.1, old.shape)).astype(np.float32)
    ptr = torch.tensor(np.concatenate(([0], np.cumsum(lens))), dtype=torch.int32, device=DEV)
    old_d, new_d, maps_d = torch.from_numpy(old).to(DEV), torch.from_numpy(new).to(DEV), torch.from_numpy(maps).to(DEV)
    out, checks, status = planner.steer_maze_batch(old_d, new_d, ptr, maps_d)
    ref_out, tmp = torch.empty_like(old_d), torch.empty_like(old_d)
    ref_checks = torch.zeros(3, dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().gnnmp_maze_steer(3, sum(lens), 15, maps_d.data_ptr(), ptr.data_ptr(), old_d.data_ptr(),
                                           new_d.data_ptr(), ref_out.data_ptr(), tmp.data_ptr(), ref_checks.data_ptr(), st),
               'gnnmp_maze_steer')
    assert torch.equal(out, ref_out) and torch.equal(checks, ref_checks)
    assert int(checks.sum()) > 0 and not torch.equal(out, old_d)
    assert status.tolist() == [0, 0, 0]


def _host_edge(env, s, t):
    """(free, K, first blocked k or 0) of the host's stick edge check s -> t; the check count is left as it was."""
    c0 = env.collision_check_count
    free = env._edge_fp(s, t)
    K = int((env.distance(s, t) / 0.015)[0])
    step = env._wrap_orientation(t - s)
    first = 0 if free else next((k for k in range(1, K) if not env._edge_fp(*env._ends(s + (k * 1. / K) * step))), 0)
    env.collision_check_count = c0
    return free, K, first


def _own_map_cases():
    """Edges longer than the walled fixture maps can hold, on maps of the test's own: the wave's second and third pass.
    Per case (map index, old_path, new_path, what the host must see on the edge old[0] -> new[1])."""
    f32 = np.float32
    maps = np.zeros((4, 15, 15), dtype=np.float64)
    maps[1, 12, 12] = 1.0                                                  # on the long diagonal, ~0.9 of the way
    maps[2, 8, 8] = 1.0                                                    # ~0.55 of the way
    rng = np.random.RandomState(11)
    maps[3] = rng.rand(15, 15) < 0.04
    maps[3, :2, :2] = maps[3, -2:, :2] = maps[3, :2, -2:] = maps[3, -2:, -2:] = 0
    s, t, third = np.array([-0.85, -0.8, 0.1], f32), np.array([0.85, 0.8, -0.2], f32), np.array([0.8, 0.7, -0.15], f32)
    # the one interior waypoint sits within RRT_EPS of its proposal t: the candidate is t, the first edge check s -> t
    long3 = (np.array([s, t - np.array([0.015, 0.012, 0.0], f32), third], f32), np.array([s, t, third], f32))
    # several rounds over a zigzag of long edges (every edge check of every round is a long one)
    zig = np.array([[-0.85, -0.85, 0.0], [0.85, -0.7, 0.3], [-0.8, 0.0, -0.3], [0.85, 0.7, 0.2], [-0.85, 0.85, 0.0]], f32)
    prop = (zig + np.array([[0, 0, 0], [-0.05, 0.12, -0.1], [0.1, 0.08, -0.2], [-0.1, -0.06, 0.1], [0, 0, 0]], f32)).astype(f32)
    return maps, [(0, *long3, 'free'), (1, *long3, 'pass3'), (2, *long3, 'pass2'), (0, zig, prop, 'rounds'),
                  (3, zig, prop, 'rounds')]


def test_long_edges_on_own_maps_equal_the_host_steering():
    """The fixture maps are walled, so their longest free edge is shorter than three passes of the wave (K <= ~110).  On
    an open map and on maps with single obstacles: a FREE edge of K >= 150 (three passes run to the end), the same edge
    blocked first in the third pass and in the second, and several rounds over a zigzag of long edges.  The yardstick is
    the host's smooth_step over Maze3D, which tests/test_stick_steer_host.py pins to the reference's recorded runs."""
    maps, cases = _own_map_cases()
    env = Maze3D(maps, np.zeros((len(maps), 3)), np.zeros((len(maps), 3)))
    want, batch = [], []
    for mi, old, new, kind in cases:
        env.init_new_problem(mi)
        free, K, first = _host_edge(env, old[0], new[1])
        print('\nmap %d %s: host edge old[0] -> new[1] free %s K %d first blocked k %d' % (mi, kind, free, K, first))
        if kind == 'free':
            assert free and K >= 150                                       # (the bar is K >= 130: a third pass)
        elif kind == 'pass3':
            assert not free and K >= 150 and first > 129                   # k = 1 + 2 * 64 opens the third pass
        elif kind == 'pass2':
            assert not free and K >= 150 and 65 <= first <= 128
        else:
            assert K >= 100
        env.collision_check_count = 0
        out = planner.smooth_step([r.copy() for r in old], new.copy(), env)
        want.append((np.array(out, dtype=np.float32).reshape(-1, 3), int(env.collision_check_count)))
        batch.append({'old_path': old, 'new_path': new, 'map': maps[mi]})
    # the free long edge is accepted, the blocked ones are not; the zigzag moves on the open map
    assert want[0][0].tobytes() == cases[0][2].tobytes()
    assert want[1][0].tobytes() == cases[1][1].tobytes() and want[2][0].tobytes() == cases[2][1].tobytes()
    assert want[3][0].tobytes() != cases[3][1].tobytes() and want[3][1] > 2000
    got = _steer(batch)
    for (mi, old, new, kind), (hp, hc), (path, checks, status) in zip(cases, want, got):
        print('map %d %s: checks device %d host %d, status %d' % (mi, kind, checks, hc, status))
        assert status == 0 and path.tobytes() == hp.tobytes() and checks == hc, (mi, kind)
    for c, g in zip(batch, got):                                           # and alone
        assert _steer([c])[0][0].tobytes() == g[0].tobytes() and _steer([c])[0][1:] == g[1:]


def test_maps_beyond_the_lds_copy_equal_the_host_steering():
    """Width 65 is 4225 cells, more than the 4096 bytes of the LDS copy: every query reads the map in global memory.  Two
    paths of four waypoints on sparse maps of the test's own, against the host's smooth_step over Maze3D."""
    rng = np.random.RandomState(23)
    maps = (rng.rand(2, 65, 65) < 0.004).astype(np.float64)
    env = Maze3D(maps, np.zeros((2, 3)), np.zeros((2, 3)))
    want, batch = [], []
    for mi in range(2):
        old = np.concatenate([np.clip(rng.uniform(-0.4, 0.4, 2) + np.cumsum(rng.normal(0, 0.15, (4, 2)), axis=0), -0.85, 0.85),
                              rng.uniform(-0.3, 0.3, (4, 1))], axis=1).astype(np.float32)
        new = (old + rng.normal(0, 0.06, old.shape) * [[0], [1], [1], [0]]).astype(np.float32)
        env.init_new_problem(mi)
        env.collision_check_count = 0
        out = planner.smooth_step([r.copy() for r in old], new.copy(), env)
        want.append((np.array(out, dtype=np.float32).reshape(-1, 3), int(env.collision_check_count)))
        batch.append({'old_path': old, 'new_path': new, 'map': maps[mi]})
    # waypoints move on one path at least, and one edge at least is blocked (a fully accepted path ends on its proposal)
    assert any(w[0].tobytes() != c['old_path'].tobytes() for w, c in zip(want, batch))
    assert any(w[0].tobytes() != c['new_path'].tobytes() for w, c in zip(want, batch))
    for mi, ((hp, hc), (path, checks, status)) in enumerate(zip(want, _steer(batch))):
        print('\nmap %d: checks device %d host %d, status %d' % (mi, checks, hc, status))
        assert status == 0 and path.tobytes() == hp.tobytes() and checks == hc and hc > 0, mi


class _TrippingSmoother:
    """Stands in for the network: proposes the path itself, except one waypoint turned by more than 1.2."""

    def __init__(self, row):
        self.row = row

    def forward_batch(self, sb, loop):
        new = sb.path.clone()
        new[self.row, 2] += 1.5
        return new


def test_smoothing_stage_raises_on_the_assert_case():
    cases = [CASES[0], CASES[1]]
    # node rows per problem: the path's waypoints, one more free row, one collided row
    vs, nptr, n_free, plen = [], [0], [], []
    for c in cases:
        P = len(c['old_path'])
        vs.append(np.concatenate((c['old_path'], np.zeros((2, 3), dtype=np.float32))))
        nptr.append(nptr[-1] + P + 2)
        n_free.append(P + 1)
        plen.append(P)
    path = np.zeros(nptr[-1], dtype=np.int32)
    for b, P in enumerate(plen):
        path[nptr[b]:nptr[b] + P] = np.arange(P)
    v = torch.from_numpy(np.concatenate(vs)).to(DEV)
    maps = torch.from_numpy(np.stack([c['map'].astype(np.float64) for c in cases])).to(DEV)
    with pytest.raises(RuntimeError, match=r'problem\(s\) \[1\]'):
        planner._smooth_maze_batch(_TrippingSmoother(plen[0] + 1), [0, 1], v, nptr, n_free, path, plen, maps, 2, DEV)


def _seeded_smoother():
    torch.manual_seed(0)
    ms = gnnmp.ModelSmoother(3, 3, 6, 128)
    sd = {k: t.clone() for k, t in ms.state_dict().items()}
    # the proposals are the last layer's output itself: scaled down they stay inside the map and within 1.2 of any z
    sd['smooth_node.weight'] *= 0.05
    sd['smooth_node.bias'] *= 0.05
    ms.load_state_dict(sd)
    return ms.eval()


def test_rounds_planner_smooths_maze3_like_the_host():
    """eval_gnn_device_rounds with a smoother on the first maze3 fixture problems: per solved problem the smoothed path
    and c_smooth equal planner.model_smooth on the host (Maze3D checker, same GPU network, same samples) bit for bit; the
    explore-stage figures stay the fixture's.  The fixture's first 6 problems are all recorded as unsolved (its solved ones
    are 6, 8, 10, 11, ...), so "at least 4 solved" needs the first 12: they contain the first 6 and exactly 4 solved ones."""
    with np.load(os.path.join(GOLDEN, 'evalset_maze3_first40_b200_k12_s9.npz')) as f:
        env = Maze3D(f['maps'], f['init_states'], f['goal_states'])
        ref, seed, batch, k = f['rows'], int(f['seed']), int(f['batch']), int(f['k'])
    m = gnnmp.EncoderProcessDecoder(2, 3, 32, 2).eval()
    m.load_state_dict(load_weights('weights_maze_3'))
    ms = _seeded_smoother()
    rows, det = [], []
    n = 12
    assert int(ref[:n, 0].sum()) >= 4
    planner.eval_gnn_device_rounds(env, range(n), m, ms, seed=seed, batch=batch, t_max=batch, k=k, device=DEV, rows_out=rows,
                                   details_out=det)              # (a non-zero status word would have raised)
    rows = np.array(rows, dtype=np.float64)
    print('\nexplore rows device\n%s\nfixture\n%s' % (rows[:, [0, 3, 5, 6]], ref[:n][:, [0, 3, 5, 6]]))
    assert np.array_equal(rows[:, [0, 3, 5, 6]], ref[:n][:, [0, 3, 5, 6]])
    assert np.allclose(rows[:, 1], ref[:n, 1], rtol=0, atol=1e-6)
    solved = [d for d in det if d['success']]
    assert len(solved) >= 4
    changed = 0
    for d in solved:
        e, v, n_free = d['env'], d['v'], d['n_free']
        c0 = e.collision_check_count
        host = planner.model_smooth(ms, [x for x in v[:n_free]], [x for x in v[n_free:]], [p.copy() for p in d['path']], e, DEV)
        c_host = e.collision_check_count - c0
        host = np.array(host, dtype=np.float32).reshape(-1, 3)
        print('P=%d c_smooth device %d host %d, waypoints moved %d' % (len(host), d['c_smooth'], c_host,
                                                                       int((host != d['path']).any(axis=1).sum())))
        assert host.tobytes() == np.ascontiguousarray(d['smooth_path'], dtype=np.float32).tobytes()
        assert d['c_smooth'] == c_host and d['c_smooth'] > 0
        changed += int(not np.array_equal(d['smooth_path'], d['path']))
    assert changed >= 1
