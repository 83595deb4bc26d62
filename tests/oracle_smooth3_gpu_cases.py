"""The cases of tests/test_oracle_smooth3_gpu.py (which runs each test function of this file in a process of its own).

gnnmp.oracle_smooth on [sumP, 3] paths (the stick robot, gnnmp_stick_oracle_smooth) against the recorded runs of the
unmodified reference over MazeEnv(dim=3) (tests/golden/oracle_smooth3_*.npz): float64 bit patterns, float32 flags, lengths,
collision-check counts and status, final and after every recorded stage; batches against single paths; the device form of
the draws; random paths on synthetic maps against the host restatement (tests/oracle_smooth3_host.py); the per-path error
statuses; the public wrappers.  Exactness everywhere: no tolerance."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import oracle_smooth as OS

import oracle_smooth3_host as H3
import oracle_smooth_host as H

pytestmark = pytest.mark.gpu
FIX = H3.fixtures()
NAMES = sorted(FIX)
DEV = 'cuda:0'


def shape_of(fx):
    return int(fx['iters']), int(fx['random_iter'])


def pack(names):
    """The fixtures ``names`` (all of one iters / random_iter shape) as one ragged batch, per-waypoint flags explicit."""
    assert len({shape_of(FIX[n]) for n in names}) == 1
    paths = [FIX[n]['path'].astype(np.float64) for n in names]
    ptr = np.cumsum([0] + [len(p) for p in paths])
    is32 = np.concatenate([np.full(len(FIX[n]['path']), bool(FIX[n]['in32'])) for n in names])
    maps = np.stack([FIX[n]['map'] for n in names])
    draws = {'action': np.stack([FIX[n]['action'] for n in names]), 'node_idx': np.stack([FIX[n]['node_idx'] for n in names])}
    return torch.from_numpy(np.concatenate(paths)).to(DEV), ptr, torch.from_numpy(is32).to(DEV), maps, draws


def unpack(r, ptr):
    out = []
    for b in range(len(ptr) - 1):
        n, lo = int(r['out_len'][b]), int(ptr[b])
        out.append((r['path'][lo:lo + n].cpu().numpy(), r['is32'][lo:lo + n].cpu().numpy(), int(r['checks'][b]), int(r['status'][b])))
    return out


def run(names, ratio, stop=None, iters=None, draws=None, **kw):
    paths, ptr, is32, maps, d = pack(names)
    it, ri = shape_of(FIX[names[0]])
    r = OS.smooth(paths, ptr, maps, draws or d, iters=it if iters is None else iters, random_iter=ri, ratio=ratio, stop=stop,
                  is32=is32, **kw)
    torch.cuda.synchronize()
    assert r['path'].shape == (int(ptr[-1]), 3)
    return unpack(r, ptr)


def assert_same(got, xyz, is32, checks, status, what):
    gxyz, g32, gchecks, gstatus = got
    print('%s: len %d/%d checks %d/%d status %d/%d' % (what, len(gxyz), len(xyz), gchecks, checks, gstatus, status))
    assert gstatus == status, what
    assert gxyz.shape == xyz.shape, what
    assert gxyz.tobytes() == np.ascontiguousarray(xyz).tobytes(), what
    assert (g32 == is32).all() and gchecks == checks, what


def full_shape(ratio=True):
    return [n for n in NAMES if shape_of(FIX[n]) == (5, 100) and bool(FIX[n]['ratio']) == ratio]


@pytest.mark.parametrize('name', NAMES)
def test_every_fixture_alone_final_and_every_stage(name):
    fx = FIX[name]
    ratio = bool(fx['ratio'])
    assert_same(run([name], ratio)[0], fx['result'], fx['result_is32'], int(fx['checks']), int(fx['status']), name)
    for kind, it, sxyz, s32, schecks in H3.fixture_stages(fx):
        # no fixture collects a status bit (asserted by the host test), so every stage ends with status 0
        stop = {'random': 'random', 'prune': 'prune', 'iter': None}[kind]
        assert_same(run([name], ratio, stop=stop, iters=it + 1)[0], sxyz, s32, schecks, 0, '%s %s %d' % (name, kind, it))


@pytest.mark.parametrize('ratio', [True, False])
def test_all_fixtures_as_one_ragged_batch(ratio):
    names = full_shape(ratio)
    assert len(names) >= 1
    for got, n in zip(run(names, ratio), names):
        fx = FIX[n]
        assert_same(got, fx['result'], fx['result_is32'], int(fx['checks']), int(fx['status']), n)


def test_batch_of_1024_equals_one_by_one_and_repeats():
    names = full_shape()
    single = {n: run([n], True)[0] for n in names}
    rng = np.random.RandomState(5)
    order = [names[i] for i in np.concatenate([rng.permutation(len(names)) for _ in range(1024 // len(names) + 1)])[:1024]]
    a = run(order, True)
    b = run(order, True)
    assert len(a) == len(b) == 1024
    for n, ga, gb in zip(order, a, b):
        for g in (ga, gb):
            assert g[0].tobytes() == single[n][0].tobytes() and (g[1] == single[n][1]).all() and g[2:] == single[n][2:], n
    assert all(single[n][0].tobytes() == FIX[n]['result'].tobytes() for n in names)


def test_device_form_draws_reproduce_the_replay_and_draw_device():
    names = full_shape()
    _, _, _, _, d = pack(names)
    # ratio mode keeps the length, so u = (idx - 1 + 0.5) / (len - 2) gives back the recorded index
    lens = np.array([len(FIX[n]['path']) for n in names], dtype=np.float64)[:, None, None]
    u = np.where(lens > 2, (d['node_idx'] - 0.5) / np.maximum(lens - 2, 1), 0.0)
    # node_index applied on the host gives the recorded indices back
    for b, n in enumerate(names):
        if len(FIX[n]['path']) > 2:
            idx = OS.node_index(torch.from_numpy(u[b]), len(FIX[n]['path'])).numpy()
            assert (idx == d['node_idx'][b]).all(), n
    got = run(names, True, draws={'action': d['action'], 'u': u})
    for g, n in zip(got, names):
        fx = FIX[n]
        assert_same(g, fx['result'], fx['result_is32'], int(fx['checks']), int(fx['status']), n + ' (u)')
    d3 = OS.draw_device(64, generator=torch.Generator(device=DEV).manual_seed(11), dim=3)
    d3b = OS.draw_device(64, generator=torch.Generator(device=DEV).manual_seed(11), dim=3)
    assert torch.equal(d3['action'], d3b['action']) and torch.equal(d3['u'], d3b['u'])
    assert d3['action'].shape == (64, 5, 100, 3) and float(d3['action'].abs().max()) <= OS.RRT_EPS
    assert float(d3['u'].min()) >= 0.0 and float(d3['u'].max()) < 1.0
    # the default is the 2-D draw it always was
    d2 = OS.draw_device(64, generator=torch.Generator(device=DEV).manual_seed(11))
    d2b = OS.draw_device(64, generator=torch.Generator(device=DEV).manual_seed(11), dim=2)
    assert d2['action'].shape == (64, 5, 100, 2) and torch.equal(d2['action'], d2b['action']) and torch.equal(d2['u'], d2b['u'])


def synthetic(seed, B, w=15, fill=0.08):
    """B random problems: a map with ``fill`` of its cells blocked and a path of 4 - 9 float32 waypoints, a random walk in
    (x, y) with steps up to 0.3 and any orientation (so |dz| > 0.4 between neighbours is common), every stick free; the
    edges between them may be blocked: the smoother has to cope."""
    rng = np.random.RandomState(seed)
    maps, paths, ptr = [], [], [0]
    for _ in range(B):
        m = (rng.rand(w, w) < fill).astype(np.uint8)
        env = H3.Maze3(m)
        pts = []
        want = rng.randint(4, 10)
        while len(pts) < want:
            p = rng.uniform(-1, 1, 3) * H3.LIMITS
            if pts:
                p[:2] = np.clip(pts[-1][:2] + rng.uniform(-0.3, 0.3, 2), -0.95, 0.95)
            p = p.astype(np.float32)
            if env.state_fp(p):
                pts.append(p)
        maps.append(m); paths.append(np.array(pts)); ptr.append(ptr[-1] + want)
    return np.stack(maps), np.concatenate(paths), np.array(ptr)


def test_random_paths_on_synthetic_maps_equal_the_host_restatement():
    B, iters, ri = 12, 2, 30
    maps, paths, ptr = synthetic(7, B)
    rng = np.random.RandomState(8)
    action = rng.uniform(-H.RRT_EPS, H.RRT_EPS, (B, iters, ri, 3))
    u = rng.uniform(0, 1, (B, iters, ri))
    for ratio in (True, False):
        for dtype in (np.float32, np.float64):
            is32 = np.full(len(paths), dtype == np.float32)
            want = H3.smooth_batch(paths.astype(np.float64), ptr, is32, maps, action, u=u, iters=iters, random_iter=ri, ratio=ratio)
            r = OS.smooth(torch.from_numpy(paths.astype(dtype)).to(DEV), ptr, maps, {'action': action, 'u': u}, iters=iters,
                          random_iter=ri, ratio=ratio)
            torch.cuda.synchronize()
            got = unpack(r, ptr)
            lo = 0
            for b in range(B):
                n = int(want[2][b])
                assert_same(got[b], want[0][lo:lo + n], want[1][lo:lo + n], int(want[3][b]), int(want[4][b]),
                            'synthetic %d ratio=%d %s' % (b, ratio, dtype.__name__))
                lo += n


def norm_rounding_trials(seed, count):
    """Three float32 waypoints on an empty map and one perturbation of the middle one, built so that the trial's decision
    ``lhs < rhs`` hangs on the LAST BIT of the float32 3-norms on its right side: rhs as numpy rounds it (the three float32
    squares summed in double, rounded once) and rhs from a plain float32 sum differ, and the float64 lhs lies strictly
    between them.  Found by bisection along the direction towards the chord, where lhs falls monotonically."""
    rng = np.random.RandomState(seed)

    def plain(d):
        q = (d * d).astype(np.float32)
        return np.sqrt(np.float32(np.float32(q[0] + q[1]) + q[2]))

    out = []
    while len(out) < count:
        pts = (rng.uniform(-0.5, 0.5, (3, 3)) * np.array([1.0, 1.0, 0.5])).astype(np.float32)
        pv, old, nx = pts
        rhs = np.linalg.norm(nx - old) + np.linalg.norm(pv - old)
        rhs_plain = plain(nx - old) + plain(pv - old)
        if rhs == rhs_plain:
            continue
        lo_v, hi_v = sorted((float(rhs), float(rhs_plain)))
        old64 = old.astype(np.float64)
        dirn = (pv.astype(np.float64) + nx.astype(np.float64)) / 2 - old64

        def lhs(t):
            new = old64 + t * dirn
            return float(np.linalg.norm(nx - new) + np.linalg.norm(pv - new))
        t_lo, t_hi = -0.1, 0.1                                               # lhs(t_lo) > lhs(t_hi)
        if not lhs(t_lo) > hi_v > lo_v > lhs(t_hi):
            continue
        for _ in range(80):
            t = (t_lo + t_hi) / 2
            if lhs(t) > (lo_v + hi_v) / 2:
                t_lo = t
            else:
                t_hi = t
        if lo_v < lhs(t) < hi_v:
            out.append((pts, t * dirn))
    return out


def test_float32_norm_rounding_decides_a_trial():
    """A wrong float32 3-norm in the kernel changes no value directly, only decisions; these trials turn on its last bit."""
    trials = norm_rounding_trials(21, 16)
    B = len(trials)
    paths = np.concatenate([p for p, _ in trials])
    ptr = np.arange(B + 1) * 3
    maps = np.zeros((B, 15, 15), np.uint8)
    action = np.array([a for _, a in trials]).reshape(B, 1, 1, 3)
    node_idx = np.ones((B, 1, 1), np.int32)
    want = H3.smooth_batch(paths.astype(np.float64), ptr, np.ones(len(paths), bool), maps, action, node_idx=node_idx, iters=1,
                           random_iter=1, stop=H.STOP_RANDOM)
    moved = ~want[1].reshape(B, 3)[:, 1]                                     # accepted: the middle waypoint is float64 now
    print('accepted %d of %d' % (moved.sum(), B))
    assert 0 < moved.sum() < B                                               # both outcomes occur
    r = OS.smooth(torch.from_numpy(paths).to(DEV), ptr, maps, {'action': action, 'node_idx': node_idx}, iters=1,
                  random_iter=1, stop='random')
    torch.cuda.synchronize()
    for b, g in enumerate(unpack(r, ptr)):
        assert_same(g, want[0][3 * b:3 * b + 3], want[1][3 * b:3 * b + 3], int(want[3][b]), int(want[4][b]), 'norm trial %d' % b)


def test_bad_paths_get_a_status_and_leave_the_others_alone():
    names = ['drop3', 'keepall', 'p2', 'len3']
    good = run(names, True)
    paths, ptr, is32, maps, d = pack(names)
    cap = OS.limits()[0]
    b_dup = next(b for b, n in enumerate(names) if len(FIX[n]['path']) >= 3)
    # path b_dup <- identical waypoints; a new path beyond the cap appended
    p = paths.clone()
    p[int(ptr[b_dup]) + 2] = p[int(ptr[b_dup])]
    lin = torch.linspace(-0.3, 0.3, cap + 1)
    long = torch.stack((lin, lin, lin), 1).double().to(DEV)
    p = torch.cat((p, long))
    ptr2 = np.append(ptr, ptr[-1] + cap + 1)
    is32b = torch.cat((is32, torch.ones(cap + 1, dtype=torch.bool, device=DEV)))
    maps2 = np.concatenate((maps, maps[:1]))
    d2 = {k: np.concatenate((v, v[:1])) for k, v in d.items()}
    r = OS.smooth(p, ptr2, maps2, d2, is32=is32b)
    torch.cuda.synchronize()
    st = r['status'].cpu().tolist()
    B = len(names)
    assert st[b_dup] == OS.STATUS_DUPLICATE and st[B] == OS.STATUS_CAP
    assert int(r['checks'][b_dup]) == 0 and int(r['checks'][B]) == 0 and int(r['out_len'][B]) == cap + 1
    assert torch.equal(r['path'][int(ptr[b_dup]):int(ptr[b_dup + 1])], p[int(ptr[b_dup]):int(ptr[b_dup + 1])])     # handed through
    assert torch.equal(r['path'][int(ptr[B]):], long)
    for b in range(B):
        if b == b_dup:
            continue
        lo, n = int(ptr[b]), int(r['out_len'][b])
        assert r['path'][lo:lo + n].cpu().numpy().tobytes() == good[b][0].tobytes() and int(r['checks'][b]) == good[b][2]
        assert st[b] == good[b][3]
    # a path_ptr that does not describe a range inside the batch: that path alone is refused
    bad = np.array(ptr).copy()
    bad[2] = int(ptr[-1]) + 5                              # path 1 ends, and path 2 starts, beyond total_points
    r = OS.smooth(paths, torch.from_numpy(bad.astype(np.int32)), maps, d, is32=is32)
    torch.cuda.synchronize()
    st = r['status'].cpu().tolist()
    assert st[1] == OS.STATUS_BAD_PTR and st[2] == OS.STATUS_BAD_PTR and int(r['out_len'][1]) == 0 and int(r['checks'][1]) == 0
    for b in (0, 3):
        lo, n = int(ptr[b]), int(r['out_len'][b])
        assert st[b] == good[b][3] and int(r['checks'][b]) == good[b][2]
        assert r['path'][lo:lo + n].cpu().numpy().tobytes() == good[b][0].tobytes()
    assert float(r['path'][int(ptr[1]):int(ptr[3])].abs().max()) == 0.0      # nothing written for the refused paths
    # a map of the wrong size, a map batch of the wrong length, CPU tensors: errors, not results
    with pytest.raises(ValueError):
        OS.smooth(paths, ptr, maps[:, :, :14], d, is32=is32)
    with pytest.raises(ValueError):
        OS.smooth(paths, ptr, maps[:2], d, is32=is32)
    with pytest.raises(RuntimeError):
        OS.smooth(paths, ptr, np.zeros((len(names), 65, 65)), d, is32=is32)    # the library's GNNMP_ERR_DIMS
    with pytest.raises(RuntimeError):
        OS.smooth(paths.cpu(), ptr, maps, d)
    # 2-D draws with 3-D paths, and a width that is neither robot's
    with pytest.raises(ValueError):
        OS.smooth(paths, ptr, maps, {'action': d['action'][..., :2], 'node_idx': d['node_idx']}, is32=is32)
    four = torch.cat((paths, paths[:, :1]), 1)
    for fn in (lambda: OS.smooth(four, ptr, maps, d), lambda: OS.joint_smoother_ratio(four, ptr, maps, d),
               lambda: OS.joint_smoother(four, ptr, maps, d), lambda: OS.smoothing_targets(four.float(), ptr, maps)):
        with pytest.raises(ValueError):
            fn()


def test_public_wrappers_and_dtype_routes():
    n32 = [n for n in full_shape() if bool(FIX[n]['in32'])]
    n64 = [n for n in full_shape() if not bool(FIX[n]['in32'])]
    nj = full_shape(False)
    assert n32 and n64 and nj
    for names, dtype, fn in ((n32, torch.float32, OS.joint_smoother_ratio), (n64, torch.float64, OS.joint_smoother_ratio),
                             (nj, torch.float32, OS.joint_smoother)):
        paths, ptr, _, maps, d = pack(names)
        out = fn(paths.to(dtype), ptr, maps, d)
        torch.cuda.synchronize()
        assert out[0].shape == (int(ptr[-1]), 3)
        for b, n in enumerate(names):
            fx = FIX[n]
            ln = int(out[4][b]) if len(out) == 5 else len(fx['path'])
            lo = int(ptr[b])
            assert_same((out[0][lo:lo + ln].cpu().numpy(), out[1][lo:lo + ln].cpu().numpy(), int(out[2][b]), int(out[3][b])),
                        fx['result'], fx['result_is32'], int(fx['checks']), int(fx['status']), n + ' ' + fn.__name__)


def test_smoothing_targets_are_float32_rows_of_three():
    names = [n for n in full_shape() if bool(FIX[n]['in32'])]
    assert any(len(FIX[n]['path']) <= 2 for n in names) and any(len(FIX[n]['path']) > 2 for n in names)
    paths, ptr, _, maps, _ = pack(names)
    target, status = OS.smoothing_targets(paths.float(), ptr, maps, torch.Generator(device=DEV).manual_seed(3))
    t2, s2 = OS.smoothing_targets(paths.float(), ptr, maps, torch.Generator(device=DEV).manual_seed(3))
    torch.cuda.synchronize()
    assert target.dtype == torch.float32 and target.shape == (int(ptr[-1]), 3)
    assert torch.equal(target, t2) and torch.equal(status, s2)
    st = status.cpu().tolist()
    assert [bool(s & OS.STATUS_SKIPPED) for s in st] == [len(FIX[n]['path']) <= 2 for n in names]
    # fresh draws may meet a prune round that gives up, or a distance tie, as the reference may; nothing else
    assert all(s & ~(OS.STATUS_SKIPPED | OS.STATUS_TIE | OS.STATUS_UNREACHABLE) == 0 for s in st)
    for b in range(len(names)):                                              # the end points stay where they were
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        assert torch.equal(target[lo], paths[lo].float()) and torch.equal(target[hi - 1], paths[hi - 1].float())
    assert not torch.equal(target, paths.float())                           # and something moved
    assert float(target[:, 2].abs().max()) <= float(np.float32(0.4)) and float(target[:, :2].abs().max()) <= 1.0
