"""The smoother's training targets on the device: ``joint_smoother_ratio`` / ``joint_smoother`` (smoother.py:67-151) for a
batch of maze paths, bit for bit what the reference computes, its ``collision_check_count`` included.  The width of
``paths`` picks the robot: [sumP, 2] is the point robot (MazeEnv(dim=2), ``gnnmp_oracle_smooth``), [sumP, 3] the stick robot
(MazeEnv(dim=3), ``gnnmp_stick_oracle_smooth``): rows (x, y, z), z the stick's orientation coordinate in [-0.4, 0.4].  One
launch (csrc/oracle_smooth_kernels.hip, one wave per path) runs the whole ``iters x [random_path_smoother -> prune_path ->
re-spacing]`` loop; nothing is read back.

The stick robot's rules (maze_env.py:137-149, 245-347): a state is valid inside (1, 1, 0.4); a perturbed waypoint whose z
leaves +-0.4 is rejected before any check is counted (random_path_smoother neither wraps nor clips); the stick's ends and
their bisection are float64 whatever the waypoint's dtype; an edge is both sticks, then ``int(distance / 0.015)``
interpolated sticks along the displacement whose third coordinate is wrapped by 0.8, float32 arithmetic between two float32
rows and float64 otherwise.  The norms that decide a trial and weigh the prune's graph do not wrap.

Paths are ragged: ``paths`` [sumP, dim] with ``path_ptr`` [B + 1] (host ints or a tensor), ``maps`` [B, w, w] (0 = free).
float32 ``paths`` are the reference's ``[tuple(node) for node in path]`` of float32 rows (train_smoother.py:98): every
waypoint starts as a float32 one and becomes float64 when a perturbation or the re-spacing replaces it; float64 ``paths``
are the all-float64 route (``tuple(float(x) ...)``).  Results come back as float64 values plus the per-waypoint ``is32``.

The random draws are the caller's, ``draws`` = dict with
  ``action``   [B, iters, random_iter, dim] float64: np.random.uniform(-eps, eps, dim) of every trial (smoother.py:71), and
  ``node_idx`` [B, iters, random_iter] int32: the reference's np.random.randint(1, len - 1) (:72), replayed, or
  ``u``        [B, iters, random_iter] float64 in [0, 1): node_idx = 1 + min(floor(u (len - 2)), len - 3) on the device,
               at the path's current length (:func:`draw_device` makes these without synchronising).

Per-path status bits (``STATUS_*``, include/gnnmp.h): identical waypoints, waypoint cap exceeded (both: the path is handed
through unchanged), a prune round that gave up like the reference's ``except`` does, and the informational ones.
"""
import ctypes

import numpy as np
import torch

from . import _lib

RRT_EPS = 5e-2
STATUS_DUPLICATE, STATUS_CAP, STATUS_UNREACHABLE, STATUS_ORDER, STATUS_STACK = 1, 2, 4, 8, 16
STATUS_NODE_IDX, STATUS_TIE, STATUS_BAD_PTR = 32, 64, 128
STATUS_SKIPPED = 256            # smoothing_targets only: len(path) <= 2, no training sample (train_smoother.py:97)
_STOP = {None: 0, 'random': 1, 'prune': 2}


def limits():
    """(waypoints per path, map cells per side) the kernel holds."""
    a, b = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.lib().gnnmp_oracle_smooth_limits(ctypes.byref(a), ctypes.byref(b)), 'gnnmp_oracle_smooth_limits')
    return a.value, b.value


def _ptr(path_ptr, dev):
    if torch.is_tensor(path_ptr):
        return path_ptr.to(device=dev, dtype=torch.int32).contiguous()
    return torch.tensor([int(x) for x in path_ptr], dtype=torch.int32).to(dev)


def smooth(paths, path_ptr, maps, draws, iters=5, random_iter=100, prune_iter=100, ratio=True, stop=None, is32=None):
    """The general call.  ``stop``: None, or 'random' / 'prune' to end after that stage of the last iteration (the stages a
    reference run can be recorded at).  ``is32`` [sumP] bool overrides the per-waypoint flags that ``paths.dtype`` implies.
    Returns dict(path [sumP, dim] float64, is32 [sumP] bool, out_len [B] int32, checks [B] int64, status [B] int32); path b
    owns rows path_ptr[b] : path_ptr[b] + out_len[b], the rows behind them are zero."""
    dev = paths.device
    if dev.type != 'cuda':
        raise RuntimeError('gnnmp.oracle_smooth runs on the GPU only (got %s tensors); there is no CPU fallback' % dev)
    if paths.dim() != 2 or paths.shape[1] not in (2, 3):
        raise ValueError('oracle smoothing is for maze paths [sumP, 2] (point robot) or [sumP, 3] (stick robot), got %s'
                         % (tuple(paths.shape),))
    dim = int(paths.shape[1])
    if paths.dtype not in (torch.float32, torch.float64):
        raise ValueError('paths must be float32 (the planner\'s rows) or float64, got %s' % paths.dtype)
    if stop not in _STOP:
        raise ValueError('stop must be None, "random" or "prune"')
    ptr = _ptr(path_ptr, dev)
    B, total = int(ptr.numel()) - 1, int(paths.shape[0])
    maps_d = torch.as_tensor(maps)
    if maps_d.dim() != 3 or maps_d.shape[0] != B or maps_d.shape[1] != maps_d.shape[2]:
        raise ValueError('maps must be [B = %d, w, w], got %s' % (B, tuple(maps_d.shape)))
    maps_d = (maps_d != 0).to(device=dev, dtype=torch.uint8).contiguous()
    shape = (B, int(iters), int(random_iter))
    action = torch.as_tensor(draws['action']).to(device=dev, dtype=torch.float64)
    if tuple(action.shape[:3]) != shape:                      # a longer recording: its leading iterations / trials
        action = action[:, :shape[1], :shape[2]]
    action = action.contiguous()
    if tuple(action.shape) != shape + (dim,):
        raise ValueError('draws["action"] must be [B, iters, random_iter, %d] = %s, got %s'
                         % (dim, shape + (dim,), tuple(action.shape)))
    idx = u = None
    if draws.get('node_idx') is not None:
        idx = torch.as_tensor(draws['node_idx']).to(device=dev, dtype=torch.int32)[:, :shape[1], :shape[2]].contiguous()
        sel = idx
    elif draws.get('u') is not None:
        u = torch.as_tensor(draws['u']).to(device=dev, dtype=torch.float64)[:, :shape[1], :shape[2]].contiguous()
        sel = u
    else:
        raise ValueError('draws needs "node_idx" (replay form) or "u" (device form)')
    if tuple(sel.shape) != shape:
        raise ValueError('draws["node_idx" / "u"] must be [B, iters, random_iter] = %s, got %s' % (shape, tuple(sel.shape)))
    p64 = paths.to(torch.float64).contiguous()
    if is32 is None:
        flags = torch.full((total,), 1 if paths.dtype == torch.float32 else 0, dtype=torch.uint8, device=dev)
    else:
        flags = torch.as_tensor(is32).to(device=dev, dtype=torch.uint8).contiguous()
        if flags.numel() != total:
            raise ValueError('is32 must have one flag per waypoint')
    out = torch.zeros(total, dim, dtype=torch.float64, device=dev)
    out32 = torch.zeros(total, dtype=torch.uint8, device=dev)
    out_len = torch.zeros(B, dtype=torch.int32, device=dev)
    checks = torch.zeros(B, dtype=torch.int64, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    cb = _lib.OracleSmoothBatch(B, total, dim, int(maps_d.shape[1]), shape[1], shape[2], int(prune_iter), 1 if ratio else 0,
                                _STOP[stop], ptr.data_ptr(), p64.data_ptr(), flags.data_ptr(), maps_d.data_ptr(),
                                action.data_ptr(), idx.data_ptr() if idx is not None else None,
                                u.data_ptr() if u is not None else None)
    name = 'gnnmp_oracle_smooth' if dim == 2 else 'gnnmp_stick_oracle_smooth'
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.lib(), name)(ctypes.byref(cb), out.data_ptr(), out32.data_ptr(), out_len.data_ptr(),
                                             checks.data_ptr(), status.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream), name)
    for t in (ptr, p64, flags, maps_d, action, idx, u):       # inputs made here stay alive until the stream has used them
        if t is not None:
            t.record_stream(torch.cuda.current_stream(dev))
    return {'path': out, 'is32': out32.bool(), 'out_len': out_len, 'checks': checks, 'status': status, 'path_ptr': ptr}


def joint_smoother_ratio(paths, path_ptr, maps, draws, iters=5, random_iter=100, prune_iter=100):
    """smoother.joint_smoother_ratio per path: (smoothed [sumP, dim] float64, is32 [sumP] bool, checks [B] int64,
    status [B] int32).  Every path keeps its waypoint count."""
    r = smooth(paths, path_ptr, maps, draws, iters, random_iter, prune_iter, ratio=True)
    return r['path'], r['is32'], r['checks'], r['status']


def joint_smoother(paths, path_ptr, maps, draws, iters=5, random_iter=100, prune_iter=100):
    """smoother.joint_smoother per path (no re-spacing, paths shrink): (smoothed, is32, checks, status, out_len [B]);
    path b is rows path_ptr[b] : path_ptr[b] + out_len[b] of ``smoothed``."""
    r = smooth(paths, path_ptr, maps, draws, iters, random_iter, prune_iter, ratio=False)
    return r['path'], r['is32'], r['checks'], r['status'], r['out_len']


def draw_device(B, eps=RRT_EPS, generator=None, iters=5, random_iter=100, device=None, dim=2):
    """Device-form draws for B paths without synchronisation: action [B, iters, random_iter, dim] uniform in [-eps, eps), u
    uniform in [0, 1).  ``generator``: a torch.Generator on the device (its device is used when ``device`` is None)."""
    dev = torch.device(device) if device is not None else (generator.device if generator is not None else torch.device('cuda'))
    action = (torch.rand(B, iters, random_iter, int(dim), dtype=torch.float64, device=dev, generator=generator) * 2.0 - 1.0) * eps
    u = torch.rand(B, iters, random_iter, dtype=torch.float64, device=dev, generator=generator)
    return {'action': action, 'u': u}


def node_index(u, length):
    """The device form's index rule as tensors: 1 + min(floor(u (len - 2)), len - 3)."""
    n = torch.as_tensor(length, device=u.device).to(torch.float64)
    return (1 + torch.minimum((u * (n - 2)).floor(), n - 3)).to(torch.int64)


def smoothing_targets(paths, path_ptr, maps, generator=None, iters=5, random_iter=100, prune_iter=100):
    """``path_smooth`` of train_smoother.py:98 for a batch: float32 targets [sumP, dim] aligned with ``paths``, ready for
    ``MSELoss(target[1:-1], pred[1:-1])`` per path (:55), and status [B] with ``STATUS_SKIPPED`` set for the paths of
    length <= 2 the reference makes no sample of (:97).  Draws come from ``generator`` in device form."""
    ptr = _ptr(path_ptr, paths.device)
    B = int(ptr.numel()) - 1
    if paths.dim() != 2 or paths.shape[1] not in (2, 3):
        raise ValueError('oracle smoothing is for maze paths [sumP, 2] (point robot) or [sumP, 3] (stick robot), got %s'
                         % (tuple(paths.shape),))
    draws = draw_device(B, RRT_EPS, generator, iters, random_iter, device=paths.device, dim=paths.shape[1])
    smoothed, _, _, status = joint_smoother_ratio(paths.float(), ptr, maps, draws, iters, random_iter, prune_iter)
    short = (ptr[1:] - ptr[:-1]) <= 2
    return smoothed.float(), torch.where(short, status | STATUS_SKIPPED, status)
