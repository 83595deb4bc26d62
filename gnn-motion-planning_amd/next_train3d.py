"""Training the NEXT planning network of the arm families (``Model3D`` / the ``PPN`` of ``next_model/model3D.py``: kuka7, ur5,
kuka13, kuka14 -- state size ``dim`` 1 .. 15, point size ``point_dim`` 3 or 6).  The step of the reference's
``train_next.py:41-69`` is the loss of :mod:`gnnmp.next_train`, differentiated through the 3-D network.  Here:

  * :func:`path_labels`          ``train_next.get_label`` for a batch of arm paths (host, float64 as the reference; the arms'
    ``interpolate`` is ``from + diff * ratio`` clipped to ``pose_range``).
  * :func:`training_loss`        the loss ``train()`` differentiates, on the device through the inference kernels of
    :class:`gnnmp.next_model3d.NextNet3D` (``next_train.loss_from_outputs`` unchanged).
  * :func:`param_shapes`, :func:`unpack_weight_grads`  a gradient in the packed weight layout of the kernels -> a dict under the
    reference's parameter names (the exact adjoint of :func:`gnnmp.next_model3d.pack_weights`).
  * :func:`device_pack`, :func:`pack_weights_t`, :func:`device_pack_t`   the packed weights, and the transposed packing the
    backward streams, built on the device from the parameter tensors.
  * :class:`NextNet3DTrain`      the trainable network: torch Parameters on the device, ``forward`` through one
    ``torch.autograd.Function`` over ``gnnmp_next3d_train_forward`` / ``gnnmp_next3d_state_backward`` /
    ``gnnmp_next3d_pb_backward`` (``csrc/next3d_train_kernels.hip``), and ``train_step``, one optimizer step of ``train()``.

A network input row is ``[point (point_dim), state (dim)]``; the point part is the caller's (in the reference it is
``env.get_robot_points``, PyBullet's forward kinematics on the host).  The kernels are the only implementation: on a CPU tensor
``forward`` raises.  An empty call (no rows) never reaches the library: Python hands back the empty ``y``
and zero gradients itself.
"""
import ctypes

import numpy as np
import torch

from .next_model import _mfma_pack, _np_weights
from .next_model3d import DEFAULT_ITERS, LATENT, MAX_DIM, POINT_DIMS, WIDTH, _conv_pack, pack_weights
from .next_train import loss_from_outputs

_SHARE = (0, 2, 4, 6, 8, 10)


def _check_dims(dim, point_dim, who):
    dim, point_dim = int(dim), int(point_dim)
    if not 1 <= dim <= MAX_DIM or point_dim not in POINT_DIMS:
        raise ValueError('%s: 1 <= dim <= %d and point_dim is 3 or 6' % (who, MAX_DIM))
    return dim, point_dim


def param_shapes(dim, point_dim):
    """The reference's trainable parameters (``PPN.named_parameters()``: ``attention_s`` is ``attention_g``, listed once)."""
    dim, point_dim = _check_dims(dim, point_dim, 'next_train3d')
    shapes = {}
    for name, cin in (('hidden', 9), ('h0', 64), ('c0', 64), ('conv', 64)):
        shapes[name + '.weight'], shapes[name + '.bias'] = (64, cin, 3, 3, 3), (64,)
    shapes.update({'lstm.weight_ih': (256, 64), 'lstm.weight_hh': (256, 64), 'lstm.bias_ih': (256,), 'lstm.bias_hh': (256,)})
    for layer, (co, ci) in zip(_SHARE, ((16, point_dim + 3), (16, 16), (32, 16), (32, 32), (64, 32), (1, 64))):
        shapes['attention_g.mlp_share.%d.weight' % layer], shapes['attention_g.mlp_share.%d.bias' % layer] = (co, ci, 1, 1, 1), (co,)
    shapes.update({'attention_g.mlp.0.weight': (64, dim), 'attention_g.mlp.0.bias': (64,),
                   'attention_g.mlp.2.weight': (8, 64), 'attention_g.mlp.2.bias': (8,)})
    for layer, (co, ci) in zip((0, 2, 4), ((128, 8), (64, 128), (dim + 1, 64))):
        shapes['policy.%d.weight' % layer], shapes['policy.%d.bias' % layer] = (co, ci), (co,)
    return shapes


def pack_weights_t(weights, dim=None, point_dim=None):
    """The transposed packing the backward streams (``gnnmp_next3d_weights_t_floats`` floats, the same count for every
    ``(dim, point_dim)``): ``conv``, ``h0`` and ``c0`` with the taps flipped on all three axes and the channel matrix
    transposed, in the convolution packing of ``pack_weights`` (so the forward's convolution routine computes the transposed
    convolution), the LSTM's ``[256 gate rows][x 64 | h 64]`` in the MFMA packing, and 64 zeros (the bias the transposed
    convolutions read).  ``dim`` and ``point_dim`` are accepted so that it is called like ``pack_weights``; the layout does not
    depend on them."""
    w = _np_weights(weights, np.float32)
    parts = [_conv_pack(np.ascontiguousarray(np.flip(w[name + '.weight'].transpose(1, 0, 2, 3, 4), (2, 3, 4))))
             for name in ('conv', 'h0', 'c0')]
    parts.append(_mfma_pack(np.ascontiguousarray(np.concatenate([w['lstm.weight_ih'], w['lstm.weight_hh']], axis=1))))
    parts.append(np.zeros(64, dtype=np.float32))
    return np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in parts]))


_INDEX = {}
_T_NAMES = ('conv.weight', 'h0.weight', 'c0.weight', 'lstm.weight_ih', 'lstm.weight_hh')


def _index_of(packer, dim, point_dim, names):
    shapes = param_shapes(dim, point_dim)
    zeros = {k: np.zeros(s, dtype=np.float32) for k, s in shapes.items()}
    index, total = {}, None
    for name in names:
        shape = shapes[name]
        w = dict(zeros)
        n = int(np.prod(shape))
        w[name] = np.arange(1, n + 1, dtype=np.float32).reshape(shape)             # n = 110592 at most, < 2^24: exact in float32
        packed = packer(w, dim, point_dim)
        total = packed.shape[0]
        pos = np.flatnonzero(packed)
        if pos.size != n:
            raise RuntimeError('next_train3d: the packing is not a permutation of %s' % name)
        idx = np.empty(n, dtype=np.int64)
        idx[packed[pos].astype(np.int64) - 1] = pos
        index[name] = idx.reshape(shape)
    return index, total


def _pack_index(dim, point_dim):
    """name -> int64 array of the parameter's shape: where each element lands in the packed vector.  Read off
    ``next_model3d.pack_weights`` itself (one parameter at a time set to 1, 2, 3, ...), so the two cannot drift apart."""
    key = (dim, point_dim)
    if key not in _INDEX:
        _INDEX[key], _INDEX[key + ('n',)] = _index_of(pack_weights, dim, point_dim, list(param_shapes(dim, point_dim)))
    return _INDEX[key]


def _pack_t_index(dim, point_dim):
    key = (dim, point_dim, 't')
    if key not in _INDEX:
        _INDEX[key], _INDEX[key + ('n',)] = _index_of(pack_weights_t, dim, point_dim, _T_NAMES)
    return _INDEX[key]


_DEV_INDEX = {}


def _dev_index(which, dim, point_dim, device):
    """The index arrays as flat int64 tensors on ``device``, uploaded once."""
    key = (which, dim, point_dim, str(device))
    if key not in _DEV_INDEX:
        index = _pack_t_index(dim, point_dim) if which == 't' else _pack_index(dim, point_dim)
        _DEV_INDEX[key] = {k: torch.from_numpy(v.reshape(-1)).to(device) for k, v in index.items()}
    return _DEV_INDEX[key]


def _scatter(which, params, dim, point_dim):
    device = next(iter(params.values())).device
    index = _dev_index(which, dim, point_dim, device)       # fills the packed lengths too
    total = _INDEX[(dim, point_dim, 't', 'n') if which == 't' else (dim, point_dim, 'n')]
    out = torch.zeros(total, dtype=torch.float32, device=device)
    for name, idx in index.items():
        out.index_add_(0, idx, params[name].detach().to(torch.float32).reshape(-1))
    return out


def device_pack(params, dim, point_dim):
    """:func:`gnnmp.next_model3d.pack_weights` on the tensors' own device: every reference-named parameter scattered through
    :func:`_pack_index` with ``index_add_`` into zeros.  ``lstm.bias_ih`` and ``lstm.bias_hh`` land on the same positions, so
    the one packed bias is ``(0 + bias_ih) + bias_hh``: the host packer's single rounding.  Bit-equal to ``pack_weights``."""
    dim, point_dim = _check_dims(dim, point_dim, 'next_train3d.device_pack')
    return _scatter('w', params, dim, point_dim)


def device_pack_t(params, dim, point_dim):
    """:func:`pack_weights_t` on the tensors' own device."""
    dim, point_dim = _check_dims(dim, point_dim, 'next_train3d.device_pack_t')
    return _scatter('t', params, dim, point_dim)


def unpack_weight_grads(packed, dim, point_dim):
    """The gradient with respect to the packed weights -> the gradient with respect to the reference's parameters, as a dict of
    arrays (numpy in, numpy out; a torch tensor in, tensors on its device out).  The adjoint of ``pack_weights``: the MFMA and
    convolution permutations inverted, the padding lanes dropped (the first attention layer's 12, the a3 MLP's 16, the policy's
    16 output rows, the last bias's 3 zeros, the hidden convolution's channels 9 .. 15), and the one packed LSTM bias
    (``bias_ih + bias_hh``) giving the same gradient to both."""
    dim, point_dim = _check_dims(dim, point_dim, 'next_train3d.unpack_weight_grads')
    index = _pack_index(dim, point_dim)
    n = max(int(v.max()) for v in index.values()) + 1
    if hasattr(packed, 'detach'):
        flat = packed.reshape(-1)
        if flat.shape[0] < n:
            raise ValueError('unpack_weight_grads: %d packed floats, need at least %d' % (flat.shape[0], n))
        dev = _dev_index('w', dim, point_dim, flat.device)
        return {k: flat[dev[k]].reshape(v.shape) for k, v in index.items()}
    flat = np.asarray(packed).reshape(-1)
    if flat.shape[0] < n:
        raise ValueError('unpack_weight_grads: %d packed floats, need at least %d' % (flat.shape[0], n))
    return {k: flat[v] for k, v in index.items()}


# --------------------------------------------------------------------------------------------------
# labels (train_next.get_label) and the loss
# --------------------------------------------------------------------------------------------------
def path_labels(paths, path_ptr, rrt_eps, lo=None, hi=None):
    """``train_next.get_label`` for a batch of arm paths: ``paths`` [N, dim] holds the paths one after another, path ``i`` is rows
    ``path_ptr[i] : path_ptr[i + 1]``.  Returns ``(actions [N, dim], values [N])`` in float32, computed in float64 as the
    reference does: the value of a state is minus the cost to go along the path, the action is the step to the next state, cut to
    length ``rrt_eps`` (0.5 for the kukas, 0.1 for ur5) by the arms' ``interpolate`` -- ``from + diff * ratio`` clipped to the
    joint limits ``lo`` / ``hi`` (``pose_range``; None: not clipped) -- and zero for the last state."""
    paths = np.asarray(paths, dtype=np.float64)
    if paths.ndim != 2:
        raise ValueError('path_labels: paths is [N, dim]')
    dim = paths.shape[1]
    eps = float(rrt_eps)
    lo = None if lo is None else np.asarray(lo, dtype=np.float64).reshape(dim)
    hi = None if hi is None else np.asarray(hi, dtype=np.float64).reshape(dim)
    ptr = np.asarray(path_ptr, dtype=np.int64).reshape(-1)
    if ptr.size < 1 or ptr[0] != 0 or ptr[-1] != paths.shape[0] or (np.diff(ptr) < 1).any():
        raise ValueError('path_labels: path_ptr runs from 0 to the number of states, every path has a state')
    actions = np.zeros_like(paths)
    values = np.zeros(paths.shape[0], dtype=np.float64)
    for a, b in zip(ptr[:-1], ptr[1:]):
        cost = [0.]
        for k in range(a, b - 1):
            prev, nxt = paths[k], paths[k + 1]
            edge = np.linalg.norm(nxt - prev)
            cost.append(cost[-1] + edge)
            if edge > eps:
                new = prev + (nxt - prev) * (eps / edge)
                if lo is not None:
                    new = np.maximum(new, lo)
                if hi is not None:
                    new = np.minimum(new, hi)
                actions[k] = new - prev
            else:
                actions[k] = nxt - prev
        values[a:b] = np.array(cost) - cost[-1]
    return actions.astype(np.float32), values.astype(np.float32)


def _rows(points, paths, point_dim, dim):
    points = np.asarray(points, dtype=np.float64).reshape(-1, point_dim)
    if points.shape[0] != paths.shape[0]:
        raise ValueError('next_train3d: one point part per path state')
    return np.concatenate([points, paths], axis=1).astype(np.float32)


def training_loss(net, maps, goal_rows, points, paths, path_ptr, rrt_eps, lo=None, hi=None, iters=DEFAULT_ITERS):
    """The value of the reference's training loss for a batch of ``(problem, path)`` samples on the device: problem ``i`` is
    ``maps[i]``, ``goal_rows[i]`` (device tensors; a goal row is ``[point, state]``) with the path
    ``paths[path_ptr[i] : path_ptr[i + 1]]`` (host array, float64) whose point parts are ``points`` (host array, one row per
    path state).  ``net`` is a :class:`gnnmp.next_model3d.NextNet3D`.  Evaluation only: the inference kernels keep no gradient
    history."""
    ptr = np.asarray(path_ptr, dtype=np.int64).reshape(-1)
    paths = np.asarray(paths, dtype=np.float64).reshape(-1, net.dim)
    actions, values = path_labels(paths, ptr, rrt_eps, lo, hi)
    dev = maps.device
    of = torch.from_numpy(np.repeat(np.arange(ptr.size - 1, dtype=np.int32), np.diff(ptr))).to(dev)
    rows = torch.from_numpy(_rows(points, paths, net.point_dim, net.dim)).to(dev)
    y = net.state_forward(rows, of, net.pb_forward(maps, goal_rows, iters))
    return loss_from_outputs(y, torch.from_numpy(actions).to(dev), torch.from_numpy(values).to(dev), ptr)


# --------------------------------------------------------------------------------------------------
# the trainable network on the device
# --------------------------------------------------------------------------------------------------
class _Next3dTrainFn(torch.autograd.Function):
    """``y`` of :meth:`NextNet3DTrain.forward`.  The forward packs the parameters on the device and calls
    ``gnnmp_next3d_train_forward``; the backward calls ``gnnmp_next3d_state_backward``, then ``gnnmp_next3d_pb_backward`` (which
    completes the shared attention's gradient: DESIGN.md section 7), then :func:`unpack_weight_grads`."""

    @staticmethod
    def forward(ctx, net, maps, goals, rows, of, iters, *params):
        from . import _lib
        dim, pd, dev = net.dim, net.point_dim, maps.device
        B, S = int(maps.shape[0]), int(rows.shape[0])
        named = dict(zip(net._names, params))
        ctx.net, ctx.meta = net, (B, S, int(iters))
        y = torch.empty(S, dim + 1, dtype=torch.float32, device=dev)
        if S == 0:                              # nothing to read out: the library is not called, the gradients are zero
            ctx.empty = True
            return y
        ctx.empty = False
        packed, packed_t = device_pack(named, dim, pd), device_pack_t(named, dim, pd)
        pb_rep = torch.empty(B, LATENT, WIDTH, WIDTH, WIDTH, dtype=torch.float32, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        ws = net._workspace(B, int(iters), S, dev)
        d = _lib.Next3dTrain(B, S, dim, pd, WIDTH, int(iters), maps.data_ptr(), goals.data_ptr(), rows.data_ptr(), of.data_ptr(),
                             packed.data_ptr(), pb_rep.data_ptr(), y.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel())
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().gnnmp_next3d_train_forward(ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream),
                       'gnnmp_next3d_train_forward')
        net._pending.append(status)
        net._generation += 1
        ctx.generation = net._generation
        ctx.held = (goals, rows, of, packed, packed_t, pb_rep, ws)
        net.pb_rep = pb_rep
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import _lib
        net = ctx.net
        none = (None,) * 6
        if ctx.empty:
            return none + tuple(torch.zeros_like(p) for p in net._params.values())
        if ctx.generation != net._generation:
            raise RuntimeError('NextNet3DTrain: backward after a later forward -- the workspace holds one forward at a time')
        B, S, iters = ctx.meta
        goals, rows, of, packed, packed_t, pb_rep, ws = ctx.held
        dev = pb_rep.device
        dy = dy.to(torch.float32).contiguous()
        dpb = torch.empty_like(pb_rep)
        dw = torch.empty_like(packed)
        d = _lib.Next3dTrainBwd(B, S, net.dim, net.point_dim, WIDTH, iters, goals.data_ptr(), rows.data_ptr(), of.data_ptr(),
                                packed.data_ptr(), packed_t.data_ptr(), pb_rep.data_ptr(), dy.data_ptr(), dpb.data_ptr(),
                                dw.data_ptr(), ws.data_ptr(), ws.numel())
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(_lib.lib().gnnmp_next3d_state_backward(ctypes.byref(d), stream), 'gnnmp_next3d_state_backward')
            _lib.check(_lib.lib().gnnmp_next3d_pb_backward(ctypes.byref(d), stream), 'gnnmp_next3d_pb_backward')
        net.last_dweights = dw
        grads = unpack_weight_grads(dw, net.dim, net.point_dim)
        return none + tuple(grads[k].to(p.dtype) for k, p in net._params.items())


class NextNet3DTrain:
    """The 3-D NEXT network with trainable parameters on the device.  ``load_state_dict`` / ``state_dict`` speak the reference's
    names (``attention_s.*`` is written as copies of ``attention_g.*``, so :class:`gnnmp.next_model3d.NextNet3D` and ``Model3D``
    load the result); ``parameters()`` / ``named_parameters()`` are torch Parameters an optimizer takes.  The workspace of the
    saved activations (about 55 MB a problem at 20 rounds) belongs to the object and is reused across steps: run a forward's
    backward before the next forward."""

    def __init__(self, dim, point_dim=3, device='cuda'):
        self.dim, self.point_dim = _check_dims(dim, point_dim, 'NextNet3DTrain')
        self.row = self.dim + self.point_dim
        self.device = torch.device(device)
        self._names = list(param_shapes(self.dim, self.point_dim))
        self._params = {}
        self._pending = []
        self._ws = None
        self._generation = 0
        self.pb_rep = None
        self.last_dweights = None

    def load_state_dict(self, state_dict):
        w = _np_weights(state_dict, np.float32)
        pack_weights(w, self.dim, self.point_dim)       # its checks: a checkpoint of these sizes, attention_s equal to attention_g
        shapes = param_shapes(self.dim, self.point_dim)
        params = {}
        for name in self._names:
            if tuple(w[name].shape) != tuple(shapes[name]):
                raise ValueError('NextNet3DTrain: %s has shape %s, expected %s' % (name, w[name].shape, shapes[name]))
            params[name] = torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(w[name])).to(self.device))
        self._params = params
        return self

    def state_dict(self):
        if not self._params:
            raise RuntimeError('NextNet3DTrain: load_state_dict first')
        out = {k: p.detach().clone() for k, p in self._params.items()}
        for k in list(out):
            if k.startswith('attention_g.'):
                out['attention_s.' + k[len('attention_g.'):]] = out[k].clone()
        return out

    def named_parameters(self):
        return list(self._params.items())

    def parameters(self):
        return list(self._params.values())

    def _workspace(self, B, iters, S, dev):
        from . import _lib
        n = ctypes.c_size_t()
        _lib.check(_lib.lib().gnnmp_next3d_train_workspace_bytes(B, iters, S, ctypes.byref(n)), 'gnnmp_next3d_train_workspace_bytes')
        if self._ws is None or self._ws.numel() < n.value or self._ws.device != dev:
            self._ws = None                     # let go of the old block first
            self._ws = torch.empty(int(n.value), dtype=torch.uint8, device=dev)          # the allocator's blocks are 512-byte aligned
        return self._ws

    def forward(self, maps, goal_rows, rows, problem_of_state, iters=DEFAULT_ITERS):
        """``maps`` [B, 15, 15, 15], ``goal_rows`` [B, point_dim + dim], ``rows`` [S, point_dim + dim], ``problem_of_state`` [S]
        (any order, repeats) -> ``y`` [S, dim + 1] with a gradient history to the parameters."""
        if not self._params:
            raise RuntimeError('NextNet3DTrain: load_state_dict first')
        dev = maps.device
        if dev.type != 'cuda':
            raise RuntimeError('NextNet3DTrain.forward: device tensors only (the kernels are the only implementation)')
        maps = maps.to(torch.float32).reshape(-1, WIDTH, WIDTH, WIDTH).contiguous()
        goals = goal_rows.to(device=dev, dtype=torch.float32).reshape(-1, self.row).contiguous()
        rows = rows.to(device=dev, dtype=torch.float32).reshape(-1, self.row).contiguous()
        of = problem_of_state.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if int(goals.shape[0]) != int(maps.shape[0]):
            raise ValueError('NextNet3DTrain.forward: one goal row per map')
        if int(of.shape[0]) != int(rows.shape[0]):
            raise ValueError('NextNet3DTrain.forward: one problem_of_state per row')
        if int(iters) < 0:
            raise ValueError('NextNet3DTrain.forward: iters >= 0')
        if int(rows.shape[0]) > 0 and int(maps.shape[0]) == 0:
            raise ValueError('NextNet3DTrain.forward: rows without problems')
        return _Next3dTrainFn.apply(self, maps, goals, rows, of, int(iters), *self._params.values())

    __call__ = forward

    def check_status(self):
        """Read the status words of the forwards issued so far (this waits for them).  Raises RuntimeError when a
        ``problem_of_state`` entry was outside ``[0, B)``."""
        pending, self._pending = self._pending, []
        if not pending:
            return
        words = torch.stack(pending).cpu().numpy()
        bad = np.flatnonzero(words[:, 0])
        if bad.size:
            raise RuntimeError('gnnmp_next3d_train_forward: %d row(s) with problem_of_state outside [0, B) (last offending row %d, '
                               'call %d of %d checked); their rows of y are NaN and they take no part in the backward'
                               % (int(words[bad, 0].sum()), int(words[bad[0], 1]) - 1, int(bad[0]), len(pending)))

    def train_step(self, optimizer, maps, goal_rows, points, paths, path_ptr, rrt_eps, lo=None, hi=None, iters=DEFAULT_ITERS):
        """One step of ``train_next.py:41-69`` on a batch of ``(problem, path)`` samples (as :func:`training_loss` takes them):
        the labels on the host, then forward, loss, backward and ``optimizer.step()`` on the device.  Returns the loss as a
        device scalar; nothing is copied back."""
        ptr = np.asarray(path_ptr, dtype=np.int64).reshape(-1)
        paths = np.asarray(paths, dtype=np.float64).reshape(-1, self.dim)
        if ptr.size < 2 or paths.shape[0] == 0:
            raise ValueError('NextNet3DTrain.train_step: no paths')
        actions, values = path_labels(paths, ptr, rrt_eps, lo, hi)
        dev = maps.device
        of = torch.from_numpy(np.repeat(np.arange(ptr.size - 1, dtype=np.int32), np.diff(ptr))).to(dev)
        rows = torch.from_numpy(_rows(points, paths, self.point_dim, self.dim)).to(dev)
        y = self.forward(maps, goal_rows, rows, of, iters)
        loss = loss_from_outputs(y, torch.from_numpy(actions).to(dev), torch.from_numpy(values).to(dev), ptr)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        return loss.detach()
