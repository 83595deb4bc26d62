"""The NEXT planning network on maze problems: the ``PPN`` of the reference's ``next_model/model2D.py:84-210`` (a convolutional LSTM
over the 15 x 15 maze map followed by an attention read-out per queried state), batched over problems and over states on the
device (``csrc/next_kernels.hip``: ``gnnmp_next_pb_forward`` / ``gnnmp_next_state_forward``), behind the reference's own
``Model2D`` interface, plus a float64 numpy restatement that serves as the oracle for shapes no fixture covers.

The mathematics, for ``dim`` = 2 (point robot, ``next_2``) or 3 (stick robot, ``next_3``), map width 15, cap = g = 8:

  * the LAST coordinate of every goal and state is divided by ``LIMITS[2] = 0.4`` first -- for ``dim = 2`` that is y, and the
    2-D attention then sees the divided y.
  * ``attention(s)``: per cell (row i, column j) the input ``[s0, s1, j, i]`` (coords channel 0 is the COLUMN index) goes through
    the 1 x 1-conv MLP 4-16-16-32-32-64-1 (ReLU between); softmax over the 225 cells gives ``a12``; ``softmax(mlp(s))`` with
    ``mlp`` = dim-64-8 gives ``a3``; the attention is ``a3[cap] * a12[cell]``.
  * ``pb_forward``: ``x9 = [map, attention(goal)]`` (9 channels); ``hl = hidden(x9)``; ``h = h0(hl)``, ``c = c0(hl)`` (3 x 3
    convolutions, padding 1, no activation); ``iters`` rounds of ``x = conv(h)``; ``h, c = LSTMCell(x, (h, c))`` per cell (the
    reference's transposes around the cell cancel: the cell only ever sees one map cell's 64 channels).  ``pb_rep[c, i, j]`` is the
    final ``h``; channel ``c = g * 8 + cap``.
  * ``state_forward``: ``x[g] = sum_cap a3[cap] * sum_cell a12[cell] * pb_rep[g * 8 + cap, cell]`` with the state's attention, then
    the policy MLP 8-128-64-(dim + 1): the action mean and the value.

No fallback: without the library :class:`NextNet` raises.
"""
import ctypes

import numpy as np

WIDTH, CELLS, CAP, G, LATENT = 15, 225, 8, 8, 64
LAST_COORD_SCALE = 0.4                     # environment/env_config.py LIMITS[2]
DEFAULT_ITERS = 20

_SHARE = (0, 2, 4, 6, 8, 10)               # attention.mlp_share's convolutions


# --------------------------------------------------------------------------------------------------
# host restatement (numpy; float64 by default)
# --------------------------------------------------------------------------------------------------
def _np_weights(weights, dtype):
    out = {}
    for k, v in weights.items():
        if hasattr(v, 'detach'):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v).astype(dtype)
    return out


def _attention_host(w, s):
    """``s`` [n, dim], last coordinate already divided -> (a12 [n, 225] in (row, column) order, a3 [n, 8])."""
    n = s.shape[0]
    rows, cols = np.divmod(np.arange(CELLS), WIDTH)
    x = np.empty((n, CELLS, 4), dtype=s.dtype)
    x[:, :, 0], x[:, :, 1] = s[:, 0:1], s[:, 1:2]
    x[:, :, 2], x[:, :, 3] = cols, rows
    for li, layer in enumerate(_SHARE):
        wt = w['attention_g.mlp_share.%d.weight' % layer].reshape(-1, x.shape[-1])
        x = x @ wt.T + w['attention_g.mlp_share.%d.bias' % layer]
        if li + 1 < len(_SHARE):
            x = np.maximum(x, 0)
    logits = x[:, :, 0]
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    a12 = e / e.sum(axis=1, keepdims=True)
    z = np.maximum(s @ w['attention_g.mlp.0.weight'].T + w['attention_g.mlp.0.bias'], 0)
    z = z @ w['attention_g.mlp.2.weight'].T + w['attention_g.mlp.2.bias']
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return a12, e / e.sum(axis=1, keepdims=True)


def _conv3_host(x, weight, bias):
    """3 x 3 convolution with padding 1 (cross-correlation, as torch): x [n, cin, 15, 15] -> [n, cout, 15, 15]."""
    n, cin = x.shape[:2]
    pad = np.zeros((n, cin, WIDTH + 2, WIDTH + 2), dtype=x.dtype)
    pad[:, :, 1:-1, 1:-1] = x
    out = np.zeros((n, weight.shape[0], WIDTH, WIDTH), dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            out += np.einsum('oc,nchw->nohw', weight[:, :, ky, kx], pad[:, :, ky:ky + WIDTH, kx:kx + WIDTH])
    return out + bias[None, :, None, None]


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _scaled(states, dim, dtype):
    s = np.array(states, dtype=dtype).reshape(-1, dim)
    s[:, -1] = s[:, -1] / dtype(LAST_COORD_SCALE)
    return s


def pb_forward_host(weights, maps, goals, iters=DEFAULT_ITERS, dtype=np.float64):
    """The problem representation of B problems, ``[B, 64, 15, 15]``: ``maps`` [B, 15, 15], ``goals`` [B, dim]; ``weights`` under
    the reference's parameter names.  All arithmetic in ``dtype``."""
    w = _np_weights(weights, dtype)
    dim = w['attention_g.mlp.0.weight'].shape[1]
    maps = np.asarray(maps, dtype=dtype).reshape(-1, WIDTH, WIDTH)
    B = maps.shape[0]
    a12, a3 = _attention_host(w, _scaled(goals, dim, dtype))
    x9 = np.empty((B, CAP + 1, WIDTH, WIDTH), dtype=dtype)
    x9[:, 0] = maps
    x9[:, 1:] = (a3[:, :, None] * a12[:, None, :]).reshape(B, CAP, WIDTH, WIDTH)
    hl = _conv3_host(x9, w['hidden.weight'], w['hidden.bias'])
    h = _conv3_host(hl, w['h0.weight'], w['h0.bias'])
    c = _conv3_host(hl, w['c0.weight'], w['c0.bias'])
    wih, whh = w['lstm.weight_ih'], w['lstm.weight_hh']
    for _ in range(int(iters)):
        x = _conv3_host(h, w['conv.weight'], w['conv.bias'])
        gates = (np.einsum('gc,nchw->nghw', wih, x) + w['lstm.bias_ih'][None, :, None, None]
                 + np.einsum('gc,nchw->nghw', whh, h) + w['lstm.bias_hh'][None, :, None, None])
        gi, gf, gg, go = (gates[:, k * LATENT:(k + 1) * LATENT] for k in range(4))
        c = _sigmoid(gf) * c + _sigmoid(gi) * np.tanh(gg)
        h = _sigmoid(go) * np.tanh(c)
    return h


def state_forward_host(weights, states, problem_of_state, pb_rep, dtype=np.float64):
    """``y`` [S, dim + 1] (action mean, value) of S states, state s read out of ``pb_rep[problem_of_state[s]]``."""
    w = _np_weights(weights, dtype)
    dim = w['attention_g.mlp.0.weight'].shape[1]
    pb = np.asarray(pb_rep, dtype=dtype).reshape(-1, G, CAP, CELLS)
    a12, a3 = _attention_host(w, _scaled(states, dim, dtype))
    of = np.asarray(problem_of_state, dtype=np.int64).reshape(-1)
    if of.shape[0] != a12.shape[0] or (of.size and (of.min() < 0 or of.max() >= pb.shape[0])):
        raise ValueError('state_forward_host: problem_of_state needs one entry per state, each in [0, B)')
    x = np.einsum('sgcp,sp,sc->sg', pb[of], a12, a3) if of.size else np.zeros((0, G), dtype=dtype)
    for layer in (0, 2, 4):
        x = x @ w['policy.%d.weight' % layer].T + w['policy.%d.bias' % layer]
        if layer != 4:
            x = np.maximum(x, 0)
    return x


# --------------------------------------------------------------------------------------------------
# packed weights of the device kernels (layout: include/gnnmp.h, gnnmp_next_weights_floats)
# --------------------------------------------------------------------------------------------------
def _mfma_pack(mat):
    """``mat`` [K, N] (K a multiple of 16, N of 16) -> the B operands of v_mfma_f32_16x16x4_f32 in the order the kernels stream
    them: [K / 16][N / 16][lane 64][step 4], lane = (k quarter) * 16 + column, element k = 16 kg + 4 (lane / 16) + step."""
    K, N = mat.shape
    return np.ascontiguousarray(mat.reshape(K // 16, 4, 4, N // 16, 16).transpose(0, 3, 1, 4, 2)).reshape(-1)


def _conv_pack(weight):
    """A 3 x 3 convolution [64, cin, 3, 3] as [K = 9 taps x cin padded to 16s, 64]."""
    cout, cin = weight.shape[:2]
    cpad = -(-cin // 16) * 16
    m = np.zeros((9, cpad, cout), dtype=np.float32)
    m[:, :cin] = weight.reshape(cout, cin, 9).transpose(2, 1, 0)
    return _mfma_pack(m.reshape(9 * cpad, cout))


def pack_weights(weights, dim):
    """The reference's state dict (tensors or arrays under its parameter names) -> one float32 array for the kernels."""
    w = _np_weights(weights, np.float32)
    if dim not in (2, 3):
        raise ValueError('next_model: dim is 2 (point robot) or 3 (stick robot)')
    for k in list(w):
        if k.startswith('attention_s.'):       # one module stored twice
            if not np.array_equal(w[k], w['attention_g.' + k[len('attention_s.'):]]):
                raise ValueError('next_model: attention_s and attention_g differ (%s); they are one module' % k)
    if w['attention_g.mlp.0.weight'].shape != (64, dim) or w['policy.4.weight'].shape != (dim + 1, 64):
        raise ValueError('next_model: this state dict is not a dim = %d checkpoint' % dim)
    parts = []
    for layer in _SHARE:
        parts += [w['attention_g.mlp_share.%d.weight' % layer].reshape(-1), w['attention_g.mlp_share.%d.bias' % layer]]
    parts.append(np.zeros(3, dtype=np.float32))                       # the last bias padded to 4
    m1 = np.zeros((64, 3), dtype=np.float32)
    m1[:, :dim] = w['attention_g.mlp.0.weight']
    parts += [m1.reshape(-1), w['attention_g.mlp.0.bias'], w['attention_g.mlp.2.weight'].reshape(-1), w['attention_g.mlp.2.bias']]
    p3, b3 = np.zeros((4, 64), dtype=np.float32), np.zeros(4, dtype=np.float32)
    p3[:dim + 1], b3[:dim + 1] = w['policy.4.weight'], w['policy.4.bias']
    parts += [w['policy.0.weight'].reshape(-1), w['policy.0.bias'], w['policy.2.weight'].reshape(-1), w['policy.2.bias'],
              p3.reshape(-1), b3]
    for name in ('hidden', 'h0', 'c0', 'conv'):
        parts += [_conv_pack(w[name + '.weight']), w[name + '.bias']]
    lstm = np.concatenate([w['lstm.weight_ih'], w['lstm.weight_hh']], axis=1).T         # [128, 256]: k < 64 the input, then h
    parts += [_mfma_pack(np.ascontiguousarray(lstm)), w['lstm.bias_ih'] + w['lstm.bias_hh']]
    return np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in parts]))


def weights_floats(dim):
    from . import _lib
    n = ctypes.c_size_t()
    _lib.check(_lib.lib().gnnmp_next_weights_floats(int(dim), ctypes.byref(n)), 'gnnmp_next_weights_floats')
    return int(n.value)


# --------------------------------------------------------------------------------------------------
# device path
# --------------------------------------------------------------------------------------------------
class NextNet:
    """The batched network on the device.  ``load_state_dict`` packs the reference's parameters once; ``pb_forward`` and
    ``state_forward`` are stream-ordered, return device tensors and do not synchronise.  A ``problem_of_state`` outside
    ``[0, B)`` is found by the kernel: the row is neither read nor clamped (its ``y`` is NaN) and :meth:`check_status` raises."""

    def __init__(self, dim):
        if dim not in (2, 3):
            raise ValueError('NextNet: dim is 2 (point robot) or 3 (stick robot)')
        self.dim = int(dim)
        self._packed = None
        self._dev = {}
        self._pending = []

    def load_state_dict(self, state_dict):
        packed = pack_weights(state_dict, self.dim)
        if packed.shape[0] != weights_floats(self.dim):
            raise RuntimeError('NextNet: packed %d floats, the library expects %d' % (packed.shape[0], weights_floats(self.dim)))
        self._packed, self._dev = packed, {}
        return self

    def _weights(self, dev):
        import torch
        if self._packed is None:
            raise RuntimeError('NextNet: load_state_dict first')
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self._packed).to(dev)
        return self._dev[key]

    def pb_forward(self, maps, goals, iters=DEFAULT_ITERS):
        """``maps`` [B, 15, 15], ``goals`` [B, dim] float32 device tensors -> ``pb_rep`` [B, 64, 15, 15] float32."""
        import torch
        from . import _lib
        dev = maps.device
        if dev.type != 'cuda':
            raise RuntimeError('NextNet.pb_forward: device tensors only (the kernels are the only implementation)')
        maps = maps.to(torch.float32).reshape(-1, WIDTH, WIDTH).contiguous()
        goals = goals.to(torch.float32).reshape(-1, self.dim).contiguous()
        B = int(maps.shape[0])
        if int(goals.shape[0]) != B:
            raise ValueError('NextNet.pb_forward: one goal per map')
        out = torch.empty(B, LATENT, WIDTH, WIDTH, dtype=torch.float32, device=dev)
        wts = self._weights(dev)
        d = _lib.NextPbForward(B, self.dim, WIDTH, int(iters), maps.data_ptr() or None, goals.data_ptr() or None, wts.data_ptr(),
                               out.data_ptr() or None)
        if B == 0:                              # empty tensors have no storage: the call is a no-op the library accepts
            d.maps = d.goals = d.pb_rep = wts.data_ptr()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().gnnmp_next_pb_forward(ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream),
                       'gnnmp_next_pb_forward')
        return out

    def state_forward(self, states, problem_of_state, pb_rep):
        """``states`` [S, dim] float32, ``problem_of_state`` [S] int32 (any order, repeats), ``pb_rep`` [B, 64, 15, 15] ->
        ``y`` [S, dim + 1]: the action mean in the first ``dim`` columns, the value in the last."""
        import torch
        from . import _lib
        dev = pb_rep.device
        if dev.type != 'cuda':
            raise RuntimeError('NextNet.state_forward: device tensors only (the kernels are the only implementation)')
        states = states.to(device=dev, dtype=torch.float32).reshape(-1, self.dim).contiguous()
        of = problem_of_state.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        pb = pb_rep.to(torch.float32).reshape(-1, LATENT, WIDTH, WIDTH).contiguous()
        S, B = int(states.shape[0]), int(pb.shape[0])
        if int(of.shape[0]) != S:
            raise ValueError('NextNet.state_forward: one problem_of_state per state')
        y = torch.empty(S, self.dim + 1, dtype=torch.float32, device=dev)
        if S == 0:
            return y
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        wts = self._weights(dev)
        d = _lib.NextStateForward(S, B, self.dim, WIDTH, states.data_ptr(), of.data_ptr(), pb.data_ptr() or wts.data_ptr(),
                                  wts.data_ptr(), y.data_ptr(), status.data_ptr())
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().gnnmp_next_state_forward(ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream),
                       'gnnmp_next_state_forward')
        self._pending.append(status)
        if len(self._pending) > 4096:           # a long planner run: fold the old words so the list stays short
            self.check_status()
        return y

    def check_status(self):
        """Read the status words of the ``state_forward`` calls issued so far (this waits for them).  Raises RuntimeError when
        a ``problem_of_state`` entry was outside ``[0, B)``."""
        pending, self._pending = self._pending, []
        raise_bad_status(pending, 'gnnmp_next_state_forward')


def raise_bad_status(pending, entry, noun='state', tail=''):
    """The status words ``[count, last row + 1]`` that the calls of ``entry`` left, one device tensor a call (reading them
    waits for the calls): RuntimeError when any counted a ``problem_of_state`` outside ``[0, B)``.  Shared by the inference
    and the training networks of both families; ``noun`` is what they call a row, ``tail`` what else follows from one."""
    import torch
    if not pending:
        return
    words = torch.stack(pending).cpu().numpy()
    bad = np.flatnonzero(words[:, 0])
    if bad.size:
        raise RuntimeError('%s: %d %s(s) with problem_of_state outside [0, B) (last offending row %d, call %d of %d checked); '
                           'their rows of y are NaN%s'
                           % (entry, int(words[bad, 0].sum()), noun, int(words[bad[0], 1]) - 1, int(bad[0]), len(pending), tail))


class PlannerModel:
    """What ``Model2D`` and ``Model3D`` share behind the reference's interface: ``net_forward`` once a class has built its input
    rows (:meth:`_rows`), ``pred_value``, ``policy`` and ``check_status``.  ``policy`` samples on the host with torch's
    ``MultivariateNormal`` from the global torch generator, call for call what the reference does, so the draw stream is the
    reference's.  A subclass sets ``dim``, ``var``, ``device``, ``net`` and, in ``set_problem``, ``pb_rep``."""

    def net_forward(self, states, use_np=True):
        import torch
        if self.pb_rep is None:
            raise RuntimeError('%s: set_problem first' % type(self).__name__)
        states = np.asarray(states)
        if states.ndim == 1:
            states = states.reshape(1, -1)
        cur = self._rows(states)
        of = torch.zeros(cur.shape[0], dtype=torch.int32, device=self.device)
        y = self.net.state_forward(cur, of, self.pb_rep)
        if not use_np:
            return y[:, :self.dim], y[:, -1]
        y = y.cpu().numpy()
        actions, values = y[:, :self.dim], y[:, -1]
        if actions.shape[0] == 1:
            actions, values = actions[0], values[0]
        return actions, values

    def pred_value(self, states):
        return self.net_forward(states)[1]

    def policy(self, state, k=1):
        import torch
        from torch.distributions.multivariate_normal import MultivariateNormal
        mean, _ = self.net_forward(state)
        m = MultivariateNormal(torch.FloatTensor(mean), self.var)
        actions, priors = [], []
        for _ in range(k):
            a = m.sample()
            priors.append(torch.exp(m.log_prob(a)).item())
            actions.append(a.cpu().numpy())
        return actions, priors

    def check_status(self):
        self.net.check_status()


class Model2D(PlannerModel):
    """The reference's ``Model2D`` interface (next_model/model2D.py:213-294) over :class:`NextNet`, so the reference's
    ``NEXT_plan`` and :func:`gnnmp.next_plan.plan_host` run on it unchanged: ``set_problem``, ``net_forward``, ``pred_value``,
    ``policy`` (:class:`PlannerModel`)."""

    def __init__(self, env_or_problem=None, dim=2, std=None, device='cuda'):
        import torch
        if std is None:
            rrt_eps = getattr(env_or_problem, 'RRT_EPS', None)
            std = (0.05 if rrt_eps is None else rrt_eps) * 0.3
        self.dim = int(dim)
        self.std = std
        self.var = torch.eye(self.dim) * self.std ** 2
        self.env_width = WIDTH
        self.device = torch.device(device)
        self.net = NextNet(self.dim)
        self.problem = None
        self.pb_rep = None
        self.iters = DEFAULT_ITERS
        if isinstance(env_or_problem, dict):
            self._first_problem = env_or_problem
        else:
            self._first_problem = None

    def load_state_dict(self, state_dict):
        self.net.load_state_dict(state_dict)
        if self._first_problem is not None:
            self.set_problem(self._first_problem)
        return self

    def set_problem(self, problem):
        import torch
        self.problem = problem
        maps = torch.from_numpy(np.asarray(problem['map'], dtype=np.float32).reshape(1, WIDTH, WIDTH)).to(self.device)
        goal = torch.from_numpy(np.asarray(problem['goal_state'], dtype=np.float32).reshape(1, self.dim)).to(self.device)
        self.pb_rep = self.net.pb_forward(maps, goal, self.iters)

    def _rows(self, states):
        import torch
        return torch.from_numpy(np.ascontiguousarray(states, dtype=np.float32)).to(self.device)
