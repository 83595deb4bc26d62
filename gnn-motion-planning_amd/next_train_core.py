"""The body of NEXT training that no network family owns: the Python between torch and the C ABI of
``gnnmp_next_train_*`` (mazes, :mod:`gnnmp.next_train`) and ``gnnmp_next3d_train_*`` (arms, :mod:`gnnmp.next_train3d`).  A
family hands in a :class:`Family` -- data, no code path here asks which family called:

  * :func:`pack_index`, :func:`scatter`, :func:`unpack`   the permutation read off a family's packer and its adjoint.
  * :func:`path_labels`, :func:`loss_from_outputs`, :func:`sample_loss`   ``train_next.get_label`` with the family's step, the
    loss ``train()`` differentiates, and the tail every ``training_loss`` / ``train_step`` shares.
  * :class:`TrainNet`            the trainable network: torch Parameters on the device, ``forward`` through one
    ``torch.autograd.Function`` over the family's forward / state-backward / pb-backward entry points.

The kernels are the only implementation: on a CPU tensor ``forward`` raises.  An empty call (no rows) never reaches the
library: the library's own no-work calls return before any HIP call and write nothing, so Python hands
back the empty ``y`` and zero gradients itself.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from .next_model import DEFAULT_ITERS, LATENT, WIDTH, _np_weights, raise_bad_status

# What differs between the families.  ``dims`` below is a family's key: ``(dim,)`` for the mazes, ``(dim, point_dim)`` for the
# arms; ``dims[0]`` is the state size, and a goal / input row holds ``sum(dims)`` floats.
Family = collections.namedtuple('Family', [
    'module',           # the family module's name, in front of its messages
    'cls', 'noun', 'goal',      # the class name and the words for an input row and a goal row in error messages
    'check',            # check(dims, who) -> dims as ints, or ValueError
    'param_shapes', 'pack', 'pack_t', 't_names',        # called with *dims; t_names: the parameters pack_t holds
    'structs',          # the _lib struct classes of the forward and of the two backwards
    'entries',          # *_train_workspace_bytes, *_train_forward, *_state_backward, *_pb_backward
    'map_shape'])       # one problem's map; pb_rep is [B, 64, *map_shape]


# --------------------------------------------------------------------------------------------------
# the packing as an index, and its adjoint
# --------------------------------------------------------------------------------------------------
_INDEX = {}             # (module, 'w' / 't', dims) -> (name -> int64 array of the parameter's shape, packed length)
_DEV_INDEX = {}         # (module, 'w' / 't', dims, device) -> name -> flat int64 tensor


def pack_index(fam, dims, which='w'):
    """``(index, n)``: name -> where each element of the parameter lands in the packed vector of ``n`` floats.  Read off the
    packer itself (``fam.pack``, or ``fam.pack_t`` for ``which = 't'``; one parameter at a time set to 1, 2, 3, ...), so the
    two cannot drift apart."""
    key = (fam.module, which, dims)
    if key not in _INDEX:
        packer, names = (fam.pack_t, fam.t_names) if which == 't' else (fam.pack, None)
        shapes = fam.param_shapes(*dims)
        zeros = {k: np.zeros(s, dtype=np.float32) for k, s in shapes.items()}
        index, total = {}, None
        for name in names or list(shapes):
            shape = shapes[name]
            w = dict(zeros)
            n = int(np.prod(shape))
            w[name] = np.arange(1, n + 1, dtype=np.float32).reshape(shape)         # n = 110592 at most, < 2^24: exact in float32
            packed = packer(w, *dims)
            total = packed.shape[0]
            pos = np.flatnonzero(packed)
            if pos.size != n:
                raise RuntimeError('%s: the packing is not a permutation of %s' % (fam.module, name))
            idx = np.empty(n, dtype=np.int64)
            idx[packed[pos].astype(np.int64) - 1] = pos
            index[name] = idx.reshape(shape)
        _INDEX[key] = index, total
    return _INDEX[key]


def _dev_index(fam, dims, which, device):
    """The index arrays as flat int64 tensors on ``device``, uploaded once."""
    key = (fam.module, which, dims, str(device))
    if key not in _DEV_INDEX:
        _DEV_INDEX[key] = {k: torch.from_numpy(v.reshape(-1)).to(device) for k, v in pack_index(fam, dims, which)[0].items()}
    return _DEV_INDEX[key]


def scatter(fam, dims, which, params):
    """The packer (``which = 'w'``) or the transposed packer (``'t'``) on the tensors' own device: every parameter added
    through its index into zeros.  ``lstm.bias_ih`` and ``lstm.bias_hh`` land on the same positions, in that order, so the
    one packed bias is ``(0 + bias_ih) + bias_hh``: the host packer's single rounding.  Bit-equal to the host packer."""
    device = next(iter(params.values())).device
    out = torch.zeros(pack_index(fam, dims, which)[1], dtype=torch.float32, device=device)
    for name, idx in _dev_index(fam, dims, which, device).items():
        out.index_add_(0, idx, params[name].detach().to(torch.float32).reshape(-1))
    return out


def unpack(fam, dims, packed):
    """The adjoint of ``fam.pack``: a gradient in the packed layout -> a dict under the parameter names (numpy in, numpy out;
    a torch tensor in, tensors on its device out).  Padding lanes are dropped and the one packed LSTM bias
    (``bias_ih + bias_hh``) gives the same gradient to both."""
    index = pack_index(fam, dims)[0]
    n = max(int(v.max()) for v in index.values()) + 1
    tensor = hasattr(packed, 'detach')
    flat = packed.reshape(-1) if tensor else np.asarray(packed).reshape(-1)
    if flat.shape[0] < n:
        raise ValueError('unpack_weight_grads: %d packed floats, need at least %d' % (flat.shape[0], n))
    if tensor:
        dev = _dev_index(fam, dims, 'w', flat.device)
        return {k: flat[dev[k]].reshape(v.shape) for k, v in index.items()}
    return {k: flat[v] for k, v in index.items()}


# --------------------------------------------------------------------------------------------------
# labels (train_next.get_label) and the loss of train()
# --------------------------------------------------------------------------------------------------
def path_labels(paths, path_ptr, eps, step):
    """``train_next.get_label`` for a batch of paths: ``paths`` [N, dim] float64 holds the paths one after another, path ``i``
    is rows ``path_ptr[i] : path_ptr[i + 1]``.  Returns ``(actions [N, dim], values [N])`` in float32, computed in float64 as
    the reference does: the value of a state is minus the cost to go along the path (plain Euclidean edge costs), the action
    is the step to the next state, cut to length ``eps`` by ``step(prev, nxt, ratio)`` (the environment's ``interpolate``),
    and zero for the last state."""
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
                actions[k] = step(prev, nxt, eps / edge) - prev
            else:
                actions[k] = nxt - prev
        values[a:b] = np.array(cost) - cost[-1]
    return actions.astype(np.float32), values.astype(np.float32)


def loss_from_outputs(y, actions, values, ptr):
    """The mean over the paths of ``MSE(value) + MSE(action)`` from ``y`` [N, dim + 1]: what ``train()`` calls ``.backward()``
    on when a step holds 8 paths.  Differentiable in ``y``; shared with the tests' host oracle."""
    total = 0.
    for a, b in zip(ptr[:-1], ptr[1:]):
        a, b = int(a), int(b)
        total = total + ((values[a:b] - y[a:b, -1]) ** 2).mean() + ((actions[a:b] - y[a:b, :-1]) ** 2).mean()
    return total / (len(ptr) - 1)


def sample_arrays(paths, path_ptr, dim, who=None):
    """``(paths [N, dim] float64, ptr int64)`` of a batch of ``(problem, path)`` samples; with ``who``, no paths is an error."""
    ptr = np.asarray(path_ptr, dtype=np.int64).reshape(-1)
    paths = np.asarray(paths, dtype=np.float64).reshape(-1, dim)
    if who and (ptr.size < 2 or paths.shape[0] == 0):
        raise ValueError('%s: no paths' % who)
    return paths, ptr


def sample_loss(forward, rows, ptr, labels, dev):
    """The tail of every ``training_loss`` / ``train_step``: path ``i`` belongs to problem ``i``, ``y = forward(rows,
    problem_of_state)`` on the device, then :func:`loss_from_outputs` against ``labels = (actions, values)``."""
    of = torch.from_numpy(np.repeat(np.arange(ptr.size - 1, dtype=np.int32), np.diff(ptr))).to(dev)
    y = forward(torch.from_numpy(rows).to(dev), of)
    return loss_from_outputs(y, torch.from_numpy(labels[0]).to(dev), torch.from_numpy(labels[1]).to(dev), ptr)


# --------------------------------------------------------------------------------------------------
# the trainable network on the device
# --------------------------------------------------------------------------------------------------
class _TrainFn(torch.autograd.Function):
    """``y`` of :meth:`TrainNet.forward`.  The forward packs the parameters on the device and calls the family's
    ``*_train_forward``; the backward calls ``*_state_backward``, then ``*_pb_backward`` (which completes the shared
    attention's gradient: DESIGN.md section 7), then :func:`unpack`."""

    @staticmethod
    def forward(ctx, net, maps, goals, rows, of, iters, *params):
        fam, dims, dev = net.family, net.dims, maps.device
        B, S = int(maps.shape[0]), int(rows.shape[0])
        named = dict(zip(net._names, params))
        ctx.net, ctx.meta = net, (B, S, int(iters))
        y = torch.empty(S, dims[0] + 1, dtype=torch.float32, device=dev)
        if S == 0:                              # nothing to read out: the library is not called, the gradients are zero
            ctx.empty = True
            return y
        ctx.empty = False
        packed, packed_t = scatter(fam, dims, 'w', named), scatter(fam, dims, 't', named)
        pb_rep = torch.empty(B, LATENT, *fam.map_shape, dtype=torch.float32, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        ws = net._workspace(B, int(iters), S, dev)
        d = fam.structs[0](B, S, *dims, WIDTH, int(iters), maps.data_ptr(), goals.data_ptr(), rows.data_ptr(), of.data_ptr(),
                           packed.data_ptr(), pb_rep.data_ptr(), y.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel())
        with torch.cuda.device(dev):
            _lib.check(getattr(_lib.lib(), fam.entries[1])(ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream), fam.entries[1])
        net._pending.append(status)
        net._generation += 1
        ctx.generation = net._generation
        ctx.held = (goals, rows, of, packed, packed_t, pb_rep, ws)
        net.pb_rep = pb_rep
        return y

    @staticmethod
    def backward(ctx, dy):
        net = ctx.net
        fam = net.family
        none = (None,) * 6
        if ctx.empty:
            return none + tuple(torch.zeros_like(p) for p in net._params.values())
        if ctx.generation != net._generation:
            raise RuntimeError('%s: backward after a later forward -- the workspace holds one forward at a time' % fam.cls)
        B, S, iters = ctx.meta
        goals, rows, of, packed, packed_t, pb_rep, ws = ctx.held
        dev = pb_rep.device
        dy = dy.to(torch.float32).contiguous()
        dpb = torch.empty_like(pb_rep)
        dw = torch.empty_like(packed)
        d = fam.structs[1](B, S, *net.dims, WIDTH, iters, goals.data_ptr(), rows.data_ptr(), of.data_ptr(), packed.data_ptr(),
                           packed_t.data_ptr(), pb_rep.data_ptr(), dy.data_ptr(), dpb.data_ptr(), dw.data_ptr(), ws.data_ptr(),
                           ws.numel())
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for entry in fam.entries[2:]:       # the states' backward, then the problems'
                _lib.check(getattr(_lib.lib(), entry)(ctypes.byref(d), stream), entry)
        net.last_dweights = dw
        grads = unpack(fam, net.dims, dw)
        return none + tuple(grads[k].to(p.dtype) for k, p in net._params.items())


class TrainNet:
    """A NEXT network with trainable parameters on the device; a subclass names its ``family``.  ``load_state_dict`` /
    ``state_dict`` speak the reference's names (``attention_s.*`` is written as copies of ``attention_g.*``, so the inference
    classes load the result); ``parameters()`` / ``named_parameters()`` are torch Parameters an optimizer takes.  The workspace
    of the saved activations belongs to the object and is reused across steps: run a forward's backward before the next
    forward."""
    family = None

    def __init__(self, dims, device):
        self.dims = self.family.check(dims, self.family.cls)
        self.device = torch.device(device)
        self._names = list(self.family.param_shapes(*self.dims))
        self._params = {}
        self._pending = []
        self._ws = None
        self._generation = 0
        self.pb_rep = None
        self.last_dweights = None

    def load_state_dict(self, state_dict):
        w = _np_weights(state_dict, np.float32)
        self.family.pack(w, *self.dims)         # its checks: a checkpoint of these sizes, attention_s equal to attention_g
        shapes = self.family.param_shapes(*self.dims)
        params = {}
        for name in self._names:
            if tuple(w[name].shape) != tuple(shapes[name]):
                raise ValueError('%s: %s has shape %s, expected %s' % (self.family.cls, name, w[name].shape, shapes[name]))
            params[name] = torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(w[name])).to(self.device))
        self._params = params
        return self

    def state_dict(self):
        if not self._params:
            raise RuntimeError('%s: load_state_dict first' % self.family.cls)
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
        entry = self.family.entries[0]
        n = ctypes.c_size_t()
        _lib.check(getattr(_lib.lib(), entry)(B, iters, S, ctypes.byref(n)), entry)
        if self._ws is None or self._ws.numel() < n.value or self._ws.device != dev:
            self._ws = None                     # let go of the old block first
            self._ws = torch.empty(int(n.value), dtype=torch.uint8, device=dev)          # the allocator's blocks are 512-byte aligned
        return self._ws

    def forward(self, maps, goals, rows, problem_of_state, iters=DEFAULT_ITERS):
        """``maps`` [B, *map_shape], ``goals`` [B, row], ``rows`` [S, row], ``problem_of_state`` [S] (any order, repeats) ->
        ``y`` [S, dim + 1] with a gradient history to the parameters.  The subclass says what a row is."""
        fam, who = self.family, self.family.cls + '.forward'
        if not self._params:
            raise RuntimeError('%s: load_state_dict first' % fam.cls)
        dev = maps.device
        if dev.type != 'cuda':
            raise RuntimeError('%s: device tensors only (the kernels are the only implementation)' % who)
        maps = maps.to(torch.float32).reshape(-1, *fam.map_shape).contiguous()
        goals = goals.to(device=dev, dtype=torch.float32).reshape(-1, sum(self.dims)).contiguous()
        rows = rows.to(device=dev, dtype=torch.float32).reshape(-1, sum(self.dims)).contiguous()
        of = problem_of_state.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if int(goals.shape[0]) != int(maps.shape[0]):
            raise ValueError('%s: one %s per map' % (who, fam.goal))
        if int(of.shape[0]) != int(rows.shape[0]):
            raise ValueError('%s: one problem_of_state per %s' % (who, fam.noun))
        if int(iters) < 0:
            raise ValueError('%s: iters >= 0' % who)
        if int(rows.shape[0]) > 0 and int(maps.shape[0]) == 0:
            raise ValueError('%s: %ss without problems' % (who, fam.noun))
        return _TrainFn.apply(self, maps, goals, rows, of, int(iters), *self._params.values())

    __call__ = forward

    def check_status(self):
        """Read the status words of the forwards issued so far (this waits for them).  Raises RuntimeError when a
        ``problem_of_state`` entry was outside ``[0, B)``."""
        pending, self._pending = self._pending, []
        raise_bad_status(pending, self.family.entries[1], self.family.noun, ' and they take no part in the backward')

    def _step(self, optimizer, maps, goals, rows, ptr, labels, iters):
        """One optimizer step on a batch of samples (:func:`sample_loss` through :meth:`forward`); the loss as a device scalar,
        nothing is copied back."""
        loss = sample_loss(lambda r, of: self.forward(maps, goals, r, of, iters), rows, ptr, labels, maps.device)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        return loss.detach()
