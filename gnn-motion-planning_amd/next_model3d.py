"""The NEXT planning network of the arm families: the ``PPN`` of the reference's ``next_model/model3D.py:87-213`` (a
convolutional LSTM over the 15 x 15 x 15 voxel map followed by an attention read-out per queried state), batched over problems and
over states on the device (``csrc/next3d_kernels.hip``: ``gnnmp_next3d_pb_forward`` / ``gnnmp_next3d_state_forward``), behind the
reference's own ``Model3D`` interface, plus a float64 numpy restatement that serves as the oracle for shapes no fixture covers.

The mathematics, for a checkpoint of state size ``dim`` and point size ``point_dim`` (``next_7``: 7 / 3, ``next_ur5``: 6 / 3,
``next_13``: 13 / 3, ``next_14``: 14 / 6), map width 15 (3375 voxels), cap = g = 8.  A network input row is
``[point (point_dim), state (dim)]``; unlike ``Model2D`` no coordinate is scaled.

  * ``attention(inp)``: at voxel ``(i, j, k)`` the input ``[inp[:point_dim], j, i, k]`` (coords channel 0 is the SECOND index, then
    the first, then the third) goes through the 1 x 1 x 1-conv MLP (point_dim + 3)-16-16-32-32-64-1 (ReLU between); softmax over
    the 3375 voxels gives ``a123``; ``softmax(mlp(inp[point_dim:]))`` with ``mlp`` = dim-64-8 gives ``a3``; the attention is
    ``a3[cap] * a123[voxel]``.
  * ``pb_forward``: ``x9 = [map, attention(goal)]`` (9 channels); ``hl = hidden(x9)``; ``h = h0(hl)``, ``c = c0(hl)`` (3 x 3 x 3
    convolutions, padding 1, no activation); ``iters`` rounds of ``x = conv(h)``; ``h, c = LSTMCell(x, (h, c))`` per voxel (the
    reference's transposes around the cell cancel).  ``pb_rep[c, i, j, k]`` is the final ``h``; channel ``c = g * 8 + cap``.
  * ``state_forward``: ``x[g] = sum_cap a3[cap] * sum_voxel a123[voxel] * pb_rep[g * 8 + cap, voxel]`` with the state's attention,
    then the policy MLP 8-128-64-(dim + 1): the action mean and the value.

No fallback: without the library :class:`NextNet3D` raises.
"""
import ctypes

import numpy as np

from .next_model import PlannerModel, _mfma_pack, _np_weights, _sigmoid, raise_bad_status

WIDTH, VOXELS, CAP, G, LATENT = 15, 3375, 8, 8, 64
DEFAULT_ITERS = 20
MAX_DIM = 15
POINT_DIMS = (3, 6)

_SHARE = (0, 2, 4, 6, 8, 10)               # attention.mlp_share's convolutions
_IN1, _MIN, _POUT = 12, 16, 16             # padded widths of the packed first attention layer, the a3 MLP and the policy's last layer


def load_npz_weights(*paths):
    """One state dict out of one or more ``.npz`` files (a checkpoint split by parameter name)."""
    out = {}
    for path in paths:
        with np.load(path) as f:
            out.update({k: f[k] for k in f.files})
    return out


def _dims_of(w):
    return w['attention_g.mlp.0.weight'].shape[1], w['attention_g.mlp_share.0.weight'].shape[1] - 3


# --------------------------------------------------------------------------------------------------
# host restatement (numpy; float64 by default)
# --------------------------------------------------------------------------------------------------
def _attention_host(w, inp):
    """``inp`` [n, point_dim + dim] -> (a123 [n, 3375] in (i, j, k) order, a3 [n, 8])."""
    dim, pd = _dims_of(w)
    n = inp.shape[0]
    v = np.arange(VOXELS)
    i, j, k = v // (WIDTH * WIDTH), (v // WIDTH) % WIDTH, v % WIDTH
    x = np.empty((n, VOXELS, pd + 3), dtype=inp.dtype)
    x[:, :, :pd] = inp[:, None, :pd]
    x[:, :, pd], x[:, :, pd + 1], x[:, :, pd + 2] = j, i, k
    for li, layer in enumerate(_SHARE):
        wt = w['attention_g.mlp_share.%d.weight' % layer].reshape(-1, x.shape[-1])
        x = x @ wt.T + w['attention_g.mlp_share.%d.bias' % layer]
        if li + 1 < len(_SHARE):
            x = np.maximum(x, 0)
    logits = x[:, :, 0]
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    a123 = e / e.sum(axis=1, keepdims=True)
    z = np.maximum(inp[:, pd:] @ w['attention_g.mlp.0.weight'].T + w['attention_g.mlp.0.bias'], 0)
    z = z @ w['attention_g.mlp.2.weight'].T + w['attention_g.mlp.2.bias']
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return a123, e / e.sum(axis=1, keepdims=True)


def _conv27_host(x, weight, bias):
    """3 x 3 x 3 convolution with padding 1 (cross-correlation, as torch) on channel-last maps: x [n, 15, 15, 15, cin] ->
    [n, 15, 15, 15, cout], as 27 shifted matmuls."""
    n, cin = x.shape[0], x.shape[-1]
    pad = np.zeros((n, WIDTH + 2, WIDTH + 2, WIDTH + 2, cin), dtype=x.dtype)
    pad[:, 1:-1, 1:-1, 1:-1] = x
    out = np.zeros((n, WIDTH, WIDTH, WIDTH, weight.shape[0]), dtype=x.dtype)
    for di in range(3):
        for dj in range(3):
            for dk in range(3):
                out += pad[:, di:di + WIDTH, dj:dj + WIDTH, dk:dk + WIDTH] @ weight[:, :, di, dj, dk].T
    return out + bias


def pb_forward_host(weights, maps, goals, iters=DEFAULT_ITERS, dtype=np.float64):
    """The problem representation of B problems, ``[B, 64, 15, 15, 15]``: ``maps`` [B, 15, 15, 15], ``goals`` [B, point_dim + dim];
    ``weights`` under the reference's parameter names.  All arithmetic in ``dtype``."""
    w = _np_weights(weights, dtype)
    dim, pd = _dims_of(w)
    maps = np.asarray(maps, dtype=dtype).reshape(-1, WIDTH, WIDTH, WIDTH)
    B = maps.shape[0]
    a123, a3 = _attention_host(w, np.asarray(goals, dtype=dtype).reshape(B, pd + dim))
    x9 = np.empty((B, WIDTH, WIDTH, WIDTH, CAP + 1), dtype=dtype)
    x9[..., 0] = maps
    x9[..., 1:] = (a123[:, :, None] * a3[:, None, :]).reshape(B, WIDTH, WIDTH, WIDTH, CAP)
    hl = _conv27_host(x9, w['hidden.weight'], w['hidden.bias'])
    h = _conv27_host(hl, w['h0.weight'], w['h0.bias'])
    c = _conv27_host(hl, w['c0.weight'], w['c0.bias'])
    wih, whh, bias = w['lstm.weight_ih'].T, w['lstm.weight_hh'].T, w['lstm.bias_ih'] + w['lstm.bias_hh']
    for _ in range(int(iters)):
        x = _conv27_host(h, w['conv.weight'], w['conv.bias'])
        gates = x @ wih + h @ whh + bias
        gi, gf, gg, go = (gates[..., k * LATENT:(k + 1) * LATENT] for k in range(4))
        with np.errstate(over='ignore'):       # exp(-gate) of a saturated gate: the sigmoid is 0 then, as it should be
            c = _sigmoid(gf) * c + _sigmoid(gi) * np.tanh(gg)
            h = _sigmoid(go) * np.tanh(c)
    return np.ascontiguousarray(h.transpose(0, 4, 1, 2, 3))


def state_forward_host(weights, inputs, problem_of_state, pb_rep, dtype=np.float64):
    """``y`` [S, dim + 1] (action mean, value) of S input rows [point, state], row s read out of ``pb_rep[problem_of_state[s]]``."""
    w = _np_weights(weights, dtype)
    dim, pd = _dims_of(w)
    pb = np.asarray(pb_rep, dtype=dtype).reshape(-1, G, CAP, VOXELS)
    a123, a3 = _attention_host(w, np.asarray(inputs, dtype=dtype).reshape(-1, pd + dim))
    of = np.asarray(problem_of_state, dtype=np.int64).reshape(-1)
    if of.shape[0] != a123.shape[0] or (of.size and (of.min() < 0 or of.max() >= pb.shape[0])):
        raise ValueError('state_forward_host: problem_of_state needs one entry per state, each in [0, B)')
    x = np.einsum('sgcp,sp,sc->sg', pb[of], a123, a3) if of.size else np.zeros((0, G), dtype=dtype)
    for layer in (0, 2, 4):
        x = x @ w['policy.%d.weight' % layer].T + w['policy.%d.bias' % layer]
        if layer != 4:
            x = np.maximum(x, 0)
    return x


# --------------------------------------------------------------------------------------------------
# packed weights of the device kernels (layout: include/gnnmp.h, gnnmp_next3d_weights_floats)
# --------------------------------------------------------------------------------------------------
def _conv_pack(weight):
    """A 3 x 3 x 3 convolution [64, cin, 3, 3, 3] as [K = 27 taps x cin padded to 16s, 64]: ``next_model._conv_pack`` with 27 taps."""
    cout, cin = weight.shape[:2]
    cpad = -(-cin // 16) * 16
    m = np.zeros((27, cpad, cout), dtype=np.float32)
    m[:, :cin] = weight.reshape(cout, cin, 27).transpose(2, 1, 0)
    return _mfma_pack(m.reshape(27 * cpad, cout))


def _padded(a, shape):
    out = np.zeros(shape, dtype=np.float32)
    out[tuple(slice(0, n) for n in a.shape)] = a
    return out


def pack_weights(weights, dim, point_dim):
    """The reference's state dict (tensors or arrays under its parameter names) -> one float32 array for the kernels."""
    w = _np_weights(weights, np.float32)
    if not 1 <= dim <= MAX_DIM or point_dim not in POINT_DIMS:
        raise ValueError('next_model3d: 1 <= dim <= %d and point_dim is 3 or 6' % MAX_DIM)
    first = w['attention_g.mlp_share.0.weight']
    if first.ndim != 5:
        raise ValueError('next_model3d: a 2-D checkpoint (mlp_share.0.weight %s); gnnmp.next_model loads those' % (first.shape,))
    for k in list(w):
        if k.startswith('attention_s.'):       # one module stored twice
            if not np.array_equal(w[k], w['attention_g.' + k[len('attention_s.'):]]):
                raise ValueError('next_model3d: attention_s and attention_g differ (%s); they are one module' % k)
    if (first.shape != (16, point_dim + 3, 1, 1, 1) or w['attention_g.mlp.0.weight'].shape != (64, dim)
            or w['policy.4.weight'].shape != (dim + 1, 64)):
        raise ValueError('next_model3d: this state dict is not a dim = %d, point_dim = %d checkpoint' % (dim, point_dim))
    parts = [_padded(first.reshape(16, point_dim + 3), (16, _IN1)), w['attention_g.mlp_share.0.bias']]
    for layer in _SHARE[1:]:
        parts += [w['attention_g.mlp_share.%d.weight' % layer].reshape(-1), w['attention_g.mlp_share.%d.bias' % layer]]
    parts.append(np.zeros(3, dtype=np.float32))                       # the last bias padded to 4
    parts += [_padded(w['attention_g.mlp.0.weight'], (64, _MIN)), w['attention_g.mlp.0.bias'], w['attention_g.mlp.2.weight'],
              w['attention_g.mlp.2.bias']]
    parts += [w['policy.0.weight'], w['policy.0.bias'], w['policy.2.weight'], w['policy.2.bias'],
              _padded(w['policy.4.weight'], (_POUT, 64)), _padded(w['policy.4.bias'], (_POUT,))]
    for name in ('hidden', 'h0', 'c0', 'conv'):
        parts += [_conv_pack(w[name + '.weight']), w[name + '.bias']]
    lstm = np.concatenate([w['lstm.weight_ih'], w['lstm.weight_hh']], axis=1).T         # [128, 256]: k < 64 the input, then h
    parts += [_mfma_pack(np.ascontiguousarray(lstm)), w['lstm.bias_ih'] + w['lstm.bias_hh']]
    return np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in parts]))


def weights_floats(dim, point_dim):
    from . import _lib
    n = ctypes.c_size_t()
    _lib.check(_lib.lib().gnnmp_next3d_weights_floats(int(dim), int(point_dim), ctypes.byref(n)), 'gnnmp_next3d_weights_floats')
    return int(n.value)


def workspace_bytes(n_problems):
    from . import _lib
    n = ctypes.c_size_t()
    _lib.check(_lib.lib().gnnmp_next3d_workspace_bytes(int(n_problems), ctypes.byref(n)), 'gnnmp_next3d_workspace_bytes')
    return int(n.value)


# --------------------------------------------------------------------------------------------------
# device path
# --------------------------------------------------------------------------------------------------
class NextNet3D:
    """The batched network on the device.  ``load_state_dict`` packs the reference's parameters once; ``pb_forward`` and
    ``state_forward`` are stream-ordered, return device tensors and do not synchronise.  The workspace of ``pb_forward`` (h, c and
    the hidden layer of every problem) is a tensor this object owns and grows; calls of one object are meant for one stream.  A
    ``problem_of_state`` outside ``[0, B)`` is found by the kernel: the row is neither read nor clamped (its ``y`` is NaN) and
    :meth:`check_status` raises."""

    def __init__(self, dim, point_dim=3):
        if not 1 <= dim <= MAX_DIM or point_dim not in POINT_DIMS:
            raise ValueError('NextNet3D: 1 <= dim <= %d and point_dim is 3 or 6' % MAX_DIM)
        self.dim, self.point_dim = int(dim), int(point_dim)
        self.row = self.dim + self.point_dim
        self._packed = None
        self._dev = {}
        self._ws = {}
        self._pending = []

    def load_state_dict(self, state_dict):
        packed = pack_weights(state_dict, self.dim, self.point_dim)
        want = weights_floats(self.dim, self.point_dim)
        if packed.shape[0] != want:
            raise RuntimeError('NextNet3D: packed %d floats, the library expects %d' % (packed.shape[0], want))
        self._packed, self._dev = packed, {}
        return self

    def _weights(self, dev):
        import torch
        if self._packed is None:
            raise RuntimeError('NextNet3D: load_state_dict first')
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self._packed).to(dev)
        return self._dev[key]

    def _workspace(self, dev, B):
        import torch
        need = workspace_bytes(B)
        ws = self._ws.get(str(dev))
        if ws is None or ws.numel() < need:
            ws = self._ws[str(dev)] = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        return ws

    def pb_forward(self, maps, goals, iters=DEFAULT_ITERS):
        """``maps`` [B, 15, 15, 15], ``goals`` [B, point_dim + dim] float32 device tensors -> ``pb_rep`` [B, 64, 15, 15, 15]."""
        import torch
        from . import _lib
        dev = maps.device
        if dev.type != 'cuda':
            raise RuntimeError('NextNet3D.pb_forward: device tensors only (the kernels are the only implementation)')
        maps = maps.to(torch.float32).reshape(-1, WIDTH, WIDTH, WIDTH).contiguous()
        goals = goals.to(device=dev, dtype=torch.float32).reshape(-1, self.row).contiguous()
        B = int(maps.shape[0])
        if int(goals.shape[0]) != B:
            raise ValueError('NextNet3D.pb_forward: one goal row per map')
        out = torch.empty(B, LATENT, WIDTH, WIDTH, WIDTH, dtype=torch.float32, device=dev)
        wts = self._weights(dev)
        ws = self._workspace(dev, B)
        d = _lib.Next3dPbForward(B, self.dim, self.point_dim, WIDTH, int(iters), maps.data_ptr() or None, goals.data_ptr() or None,
                                 wts.data_ptr(), out.data_ptr() or None, ws.data_ptr(), ws.numel())
        if B == 0:                              # empty tensors have no storage: the call is a no-op the library accepts
            d.maps = d.goals = d.pb_rep = wts.data_ptr()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().gnnmp_next3d_pb_forward(ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream),
                       'gnnmp_next3d_pb_forward')
        return out

    def state_forward(self, inputs, problem_of_state, pb_rep):
        """``inputs`` [S, point_dim + dim] float32, ``problem_of_state`` [S] int32 (any order, repeats), ``pb_rep``
        [B, 64, 15, 15, 15] -> ``y`` [S, dim + 1]: the action mean in the first ``dim`` columns, the value in the last."""
        import torch
        from . import _lib
        dev = pb_rep.device
        if dev.type != 'cuda':
            raise RuntimeError('NextNet3D.state_forward: device tensors only (the kernels are the only implementation)')
        inputs = inputs.to(device=dev, dtype=torch.float32).reshape(-1, self.row).contiguous()
        of = problem_of_state.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        pb = pb_rep.to(torch.float32).reshape(-1, LATENT, WIDTH, WIDTH, WIDTH).contiguous()
        S, B = int(inputs.shape[0]), int(pb.shape[0])
        if int(of.shape[0]) != S:
            raise ValueError('NextNet3D.state_forward: one problem_of_state per state')
        y = torch.empty(S, self.dim + 1, dtype=torch.float32, device=dev)
        if S == 0:
            return y
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        wts = self._weights(dev)
        d = _lib.Next3dStateForward(S, B, self.dim, self.point_dim, WIDTH, inputs.data_ptr(), of.data_ptr(),
                                    pb.data_ptr() or wts.data_ptr(), wts.data_ptr(), y.data_ptr(), status.data_ptr())
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().gnnmp_next3d_state_forward(ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream),
                       'gnnmp_next3d_state_forward')
        self._pending.append(status)
        if len(self._pending) > 4096:           # a long planner run: fold the old words so the list stays short
            self.check_status()
        return y

    def check_status(self):
        """Read the status words of the ``state_forward`` calls issued so far (this waits for them).  Raises RuntimeError when
        a ``problem_of_state`` entry was outside ``[0, B)``."""
        pending, self._pending = self._pending, []
        raise_bad_status(pending, 'gnnmp_next3d_state_forward')


class Model3D(PlannerModel):
    """The reference's ``Model3D`` interface (next_model/model3D.py:216-306) over :class:`NextNet3D`, so the reference's
    ``NEXT_plan`` runs on it unchanged: ``set_problem``, ``net_forward``, ``pred_value``, ``policy``
    (:class:`gnnmp.next_model.PlannerModel`).  ``env`` supplies ``RRT_EPS`` and ``get_robot_points(state)`` (the point part of
    every input row, computed on the host as the reference does)."""

    def __init__(self, env, dim, point_dim=3, std=None, device='cuda', UCB_type='kde'):
        import torch
        if std is None:
            std = env.RRT_EPS * 0.3
        self.env = env
        self.dim, self.point_dim = int(dim), int(point_dim)
        self.std = std
        self.var = torch.eye(self.dim) * self.std ** 2
        self.env_width = WIDTH
        self.UCB_type = UCB_type
        self.device = torch.device(device)
        self.net = NextNet3D(self.dim, self.point_dim)
        self.problem = None
        self.pb_rep = None
        self.iters = DEFAULT_ITERS

    def load_state_dict(self, state_dict):
        self.net.load_state_dict(state_dict)
        return self

    def set_problem(self, problem):
        import torch
        self.problem = problem
        maze_map = np.asarray(problem['map']).reshape(1, WIDTH, WIDTH, WIDTH)
        goal = np.asarray(problem['goal_state']).reshape(1, self.dim)
        goal = np.concatenate(([self.env.get_robot_points(goal[0, :])], goal), axis=-1)
        self.maze_map = torch.FloatTensor(maze_map).to(self.device)
        self.goal_state = torch.FloatTensor(goal).to(self.device)
        self.pb_rep = self.net.pb_forward(self.maze_map, self.goal_state, self.iters)

    def _rows(self, states):
        import torch
        positions = [np.concatenate((self.env.get_robot_points(state), state), axis=-1) for state in states]
        return torch.FloatTensor(np.array(positions)).to(self.device)
