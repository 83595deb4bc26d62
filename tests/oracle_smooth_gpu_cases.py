"""The cases of tests/test_oracle_smooth_gpu.py (which runs each test function of this file in a process of its own).

gnnmp.oracle_smooth on the device against the recorded runs of the unmodified reference
(tests/golden/oracle_smooth_*.npz): float64 bit patterns, float32 flags, lengths, collision-check counts and status,
final and after every recorded stage; batches against single paths; the device form of the draws; the per-path error
statuses; targets into the smoother's training loss.  Exactness everywhere: no tolerance."""
import numpy as np
import pytest
import torch

import gnnmp
from gnnmp import oracle_smooth as OS

import oracle_smooth_host as H

pytestmark = pytest.mark.gpu
FIX = H.fixtures()
NAMES = sorted(FIX)
DEV = 'cuda:0'


def pack(names, dtype=None):
    """The fixtures ``names`` as one ragged batch (all float32-input or all float64-input unless ``dtype`` is forced; the
    per-waypoint flags go in explicitly so that mixed batches work)."""
    paths = [FIX[n]['path'].astype(np.float64) for n in names]
    ptr = np.cumsum([0] + [len(p) for p in paths])
    is32 = np.concatenate([np.full(len(FIX[n]['path']), bool(FIX[n]['in32'])) for n in names])
    maps = np.stack([FIX[n]['map'] for n in names])
    draws = {'action': np.stack([FIX[n]['action'] for n in names]), 'node_idx': np.stack([FIX[n]['node_idx'] for n in names])}
    return torch.from_numpy(np.concatenate(paths)).to(DEV), ptr, torch.from_numpy(is32).to(DEV), maps, draws


def run(names, ratio, stop=None, iters=5, draws=None, **kw):
    paths, ptr, is32, maps, d = pack(names)
    r = OS.smooth(paths, ptr, maps, draws or d, iters=iters, ratio=ratio, stop=stop, is32=is32, **kw)
    torch.cuda.synchronize()
    out = []
    for b in range(len(names)):
        n = int(r['out_len'][b])
        lo = int(ptr[b])
        out.append((r['path'][lo:lo + n].cpu().numpy(), r['is32'][lo:lo + n].cpu().numpy(), int(r['checks'][b]), int(r['status'][b])))
    return out


def assert_same(got, xy, is32, checks, status, what):
    gxy, g32, gchecks, gstatus = got
    print('%s: len %d/%d checks %d/%d status %d/%d' % (what, len(gxy), len(xy), gchecks, checks, gstatus, status))
    assert gstatus == status, what
    assert gxy.shape == xy.shape, what
    assert gxy.tobytes() == np.ascontiguousarray(xy).tobytes(), what
    assert (g32 == is32).all() and gchecks == checks, what


@pytest.mark.parametrize('name', NAMES)
def test_every_fixture_alone_final_and_every_stage(name):
    fx = FIX[name]
    ratio = bool(fx['ratio'])
    assert_same(run([name], ratio)[0], fx['result'], fx['result_is32'], int(fx['checks']), int(fx['status']), name)
    for kind, it, sxy, s32, schecks in H.fixture_stages(fx):
        # the status bits a run has collected by the end of a stage are not recorded: take them from the host restatement
        stop = {'random': 'random', 'prune': 'prune', 'iter': None}[kind]
        hs = H.smooth(fx['path'].astype(np.float64), bool(fx['in32']), fx['map'], fx['action'], node_idx=fx['node_idx'],
                      iters=it + 1, ratio=ratio, stop=H.STOP_RANDOM if kind == 'random' else H.STOP_PRUNE if kind == 'prune' else 0)[3]
        assert_same(run([name], ratio, stop=stop, iters=it + 1)[0], sxy, s32, schecks, hs, '%s %s %d' % (name, kind, it))


@pytest.mark.parametrize('ratio', [True, False])
def test_all_fixtures_as_one_ragged_batch(ratio):
    names = [n for n in NAMES if bool(FIX[n]['ratio']) == ratio]
    for got, n in zip(run(names, ratio), names):
        fx = FIX[n]
        assert_same(got, fx['result'], fx['result_is32'], int(fx['checks']), int(fx['status']), n)


def test_batch_of_2048_equals_one_by_one_and_repeats():
    names = [n for n in NAMES if bool(FIX[n]['ratio'])]
    single = {n: run([n], True)[0] for n in names}
    rng = np.random.RandomState(5)
    order = [names[i] for i in np.concatenate([rng.permutation(len(names)) for _ in range(2048 // len(names) + 1)])[:2048]]
    a = run(order, True)
    b = run(order, True)
    for n, ga, gb in zip(order, a, b):
        for g in (ga, gb):
            assert g[0].tobytes() == single[n][0].tobytes() and (g[1] == single[n][1]).all() and g[2:] == single[n][2:], n
    fx_ok = [n for n in names if int(FIX[n]['status']) == 0]
    assert all(single[n][0].tobytes() == FIX[n]['result'].tobytes() for n in fx_ok)


def test_device_form_draws_reproduce_the_replay_and_draw_device():
    names = [n for n in NAMES if bool(FIX[n]['ratio'])]
    _, _, _, _, d = pack(names)
    # ratio mode keeps the length, so u = (idx - 1 + 0.5) / (len - 2) gives back the recorded index
    lens = np.array([len(FIX[n]['path']) for n in names], dtype=np.float64)[:, None, None]
    u = np.where(lens > 2, (d['node_idx'] - 0.5) / np.maximum(lens - 2, 1), 0.0)
    got = run(names, True, draws={'action': d['action'], 'u': u})
    for g, n in zip(got, names):
        fx = FIX[n]
        assert_same(g, fx['result'], fx['result_is32'], int(fx['checks']), int(fx['status']), n + ' (u)')
    gen = torch.Generator(device=DEV).manual_seed(11)
    d1 = OS.draw_device(64, generator=gen)
    d2 = OS.draw_device(64, generator=torch.Generator(device=DEV).manual_seed(11))
    assert torch.equal(d1['action'], d2['action']) and torch.equal(d1['u'], d2['u'])
    assert d1['action'].shape == (64, 5, 100, 2) and float(d1['action'].abs().max()) <= OS.RRT_EPS
    assert float(d1['u'].min()) >= 0.0 and float(d1['u'].max()) < 1.0
    cap = OS.limits()[0]
    uu = torch.cat((d1['u'].reshape(-1), torch.tensor([0.0, np.nextafter(1.0, 0.0)], dtype=torch.float64, device=DEV)))
    for n in range(3, cap + 1):
        idx = OS.node_index(uu, n)
        assert int(idx.min()) >= 1 and int(idx.max()) <= n - 2


def test_bad_paths_get_a_status_and_leave_the_others_alone():
    names = ['drop3', 'f64end', 'keepall', 'len3']
    good = run(names, True)
    paths, ptr, is32, maps, d = pack(names)
    cap = OS.limits()[0]
    # path 1 <- identical waypoints; a new path beyond the cap appended
    p = paths.clone()
    p[int(ptr[1]) + 2] = p[int(ptr[1])]
    long = torch.stack((torch.linspace(-0.9, 0.9, cap + 1), torch.linspace(-0.9, 0.9, cap + 1)), 1).double().to(DEV)
    p = torch.cat((p, long))
    ptr2 = np.append(ptr, ptr[-1] + cap + 1)
    is32b = torch.cat((is32, torch.ones(cap + 1, dtype=torch.bool, device=DEV)))
    maps2 = np.concatenate((maps, maps[:1]))
    d2 = {k: np.concatenate((v, v[:1])) for k, v in d.items()}
    r = OS.smooth(p, ptr2, maps2, d2, is32=is32b)
    torch.cuda.synchronize()
    st = r['status'].cpu().tolist()
    assert st[1] == OS.STATUS_DUPLICATE and st[4] == OS.STATUS_CAP
    assert int(r['checks'][1]) == 0 and int(r['checks'][4]) == 0 and int(r['out_len'][4]) == cap + 1
    assert torch.equal(r['path'][int(ptr[1]):int(ptr[2])], p[int(ptr[1]):int(ptr[2])])     # handed through
    assert torch.equal(r['path'][int(ptr[4]):], long)
    for b in (0, 2, 3):
        lo, n = int(ptr[b]), int(r['out_len'][b])
        assert r['path'][lo:lo + n].cpu().numpy().tobytes() == good[b][0].tobytes() and int(r['checks'][b]) == good[b][2]
        assert st[b] == good[b][3]
    # a map of the wrong size, a map batch of the wrong length, CPU tensors: errors, not results
    with pytest.raises(ValueError):
        OS.smooth(paths, ptr, maps[:, :, :14], d, is32=is32)
    with pytest.raises(ValueError):
        OS.smooth(paths, ptr, maps[:2], d, is32=is32)
    with pytest.raises(RuntimeError):
        OS.smooth(paths, ptr, np.zeros((len(names), 65, 65)), d, is32=is32)    # the library's GNNMP_ERR_DIMS
    with pytest.raises(RuntimeError):
        OS.smooth(paths.cpu(), ptr, maps, d)


def test_public_wrappers_and_dtype_routes():
    n32 = [n for n in NAMES if bool(FIX[n]['ratio']) and bool(FIX[n]['in32'])]
    n64 = [n for n in NAMES if bool(FIX[n]['ratio']) and not bool(FIX[n]['in32'])]
    nj = [n for n in NAMES if not bool(FIX[n]['ratio'])]
    for names, dtype, fn in ((n32, torch.float32, OS.joint_smoother_ratio), (n64, torch.float64, OS.joint_smoother_ratio),
                             (nj, torch.float32, OS.joint_smoother)):
        paths, ptr, _, maps, d = pack(names)
        out = fn(paths.to(dtype), ptr, maps, d)
        torch.cuda.synchronize()
        for b, n in enumerate(names):
            fx = FIX[n]
            ln = int(out[4][b]) if len(out) == 5 else len(fx['path'])
            lo = int(ptr[b])
            assert_same((out[0][lo:lo + ln].cpu().numpy(), out[1][lo:lo + ln].cpu().numpy(), int(out[2][b]), int(out[3][b])),
                        fx['result'], fx['result_is32'], int(fx['checks']), int(fx['status']), n + ' ' + fn.__name__)


def test_smoothing_targets_feed_the_training_loss():
    # constructing a module draws its initial parameters from torch's global generator: leave that stream as it was found,
    # other tests' random inputs come from it
    with torch.random.fork_rng(devices=[0]):
        _smoothing_targets_body()


def _smoothing_targets_body():
    from conftest import load_weights
    from gnnmp.planner import chain_edge_index
    names = [n for n in NAMES if bool(FIX[n]['ratio']) and bool(FIX[n]['in32'])]
    paths, ptr, _, maps, _ = pack(names)
    gen = torch.Generator(device=DEV).manual_seed(3)
    target, status = OS.smoothing_targets(paths.float(), ptr, maps, gen)
    t2, s2 = OS.smoothing_targets(paths.float(), ptr, maps, torch.Generator(device=DEV).manual_seed(3))
    assert target.dtype == torch.float32 and target.shape == paths.shape and torch.equal(target, t2) and torch.equal(status, s2)
    skipped = [bool(s & OS.STATUS_SKIPPED) for s in status.cpu().tolist()]
    assert skipped == [len(FIX[n]['path']) <= 2 for n in names]
    model = gnnmp.ModelSmoother(workspace_size=2, config_size=2, embed_size=128, obs_size=6)
    model.load_state_dict(load_weights('smooth_2d_attv3'))
    model.train()
    b = next(i for i, n in enumerate(names) if len(FIX[n]['path']) >= 8)
    lo, hi = int(ptr[b]), int(ptr[b + 1])
    path = paths[lo:hi].float()
    g = torch.Generator().manual_seed(1)
    free, coll = (torch.rand(k, 2, generator=g) * 2 - 1 for k in (60, 40))
    pred = model.forward_train(path=path, free=free.to(DEV), collided=coll.to(DEV),
                               edge_index=chain_edge_index(hi - lo).to(DEV), loop=2)
    loss = torch.nn.MSELoss()(target[lo:hi][1:-1], pred[1:-1])
    loss.backward()
    assert torch.isfinite(loss)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert len(grads) >= 10 and all(torch.isfinite(gr).all() for gr in grads) and any(float(gr.abs().max()) > 0 for gr in grads)
