"""The host side of training the NEXT planning network on maze problems (``Model2D`` / ``PPN``, dim 2 and 3).  The step of the
reference's ``train_next.py:41-69`` is, per ``(problem, path)`` sample, an MSE on the value column plus an MSE on the action
columns, averaged over the problems of a step, with the gradient through the whole network.  Built here:

  * :func:`path_labels`          ``train_next.get_label`` for a batch of paths.
  * :func:`loss_from_outputs`, :func:`training_loss`   the loss ``train()`` differentiates, from any ``y``, and its value on the
    device through the inference kernels of :class:`gnnmp.next_model.NextNet`.
  * :func:`param_shapes`, :func:`unpack_weight_grads`  a gradient in the packed weight layout of the kernels -> a dict under the
    reference's parameter names (the exact adjoint of :func:`gnnmp.next_model.pack_weights`).

NOT built: the device forward that saves its activations and the backward (DESIGN.md section 7 says why), so nothing here
takes an optimizer step.
"""
import numpy as np
import torch

from .next_model import DEFAULT_ITERS, pack_weights

RRT_EPS = 5e-2                              # environment/env_config.py
_SHARE = (0, 2, 4, 6, 8, 10)


def param_shapes(dim):
    """The reference's trainable parameters (``PPN.named_parameters()``: ``attention_s`` is ``attention_g``, listed once)."""
    dim = int(dim)
    if dim not in (2, 3):
        raise ValueError('next_train: dim is 2 (point robot) or 3 (stick robot)')
    shapes = {}
    for name, cin in (('hidden', 9), ('h0', 64), ('c0', 64), ('conv', 64)):
        shapes[name + '.weight'], shapes[name + '.bias'] = (64, cin, 3, 3), (64,)
    shapes.update({'lstm.weight_ih': (256, 64), 'lstm.weight_hh': (256, 64), 'lstm.bias_ih': (256,), 'lstm.bias_hh': (256,)})
    for layer, (co, ci) in zip(_SHARE, ((16, 4), (16, 16), (32, 16), (32, 32), (64, 32), (1, 64))):
        shapes['attention_g.mlp_share.%d.weight' % layer], shapes['attention_g.mlp_share.%d.bias' % layer] = (co, ci, 1, 1), (co,)
    shapes.update({'attention_g.mlp.0.weight': (64, dim), 'attention_g.mlp.0.bias': (64,),
                   'attention_g.mlp.2.weight': (8, 64), 'attention_g.mlp.2.bias': (8,)})
    for layer, (co, ci) in zip((0, 2, 4), ((128, 8), (64, 128), (dim + 1, 64))):
        shapes['policy.%d.weight' % layer], shapes['policy.%d.bias' % layer] = (co, ci), (co,)
    return shapes


_INDEX = {}


def _pack_index(dim):
    """name -> int64 array of the parameter's shape: where each element lands in the packed vector.  Read off
    ``pack_weights`` itself (one parameter at a time set to 1, 2, 3, ...), so the two cannot drift apart."""
    if dim not in _INDEX:
        shapes = param_shapes(dim)
        zeros = {k: np.zeros(s, dtype=np.float32) for k, s in shapes.items()}
        index = {}
        for name, shape in shapes.items():
            w = dict(zeros)
            n = int(np.prod(shape))
            w[name] = np.arange(1, n + 1, dtype=np.float32).reshape(shape)         # n < 2^24: exact in float32
            packed = pack_weights(w, dim)
            pos = np.flatnonzero(packed)
            idx = np.empty(n, dtype=np.int64)
            idx[packed[pos].astype(np.int64) - 1] = pos
            if pos.size != n:
                raise RuntimeError('next_train: pack_weights is not a permutation of %s' % name)
            index[name] = idx.reshape(shape)
        _INDEX[dim] = index
    return _INDEX[dim]


def unpack_weight_grads(packed, dim):
    """The gradient with respect to the packed weights -> the gradient with respect to the reference's parameters, as a dict of
    arrays (numpy in, numpy out; a torch tensor in, tensors on its device out).  The adjoint of ``pack_weights``: the MFMA and
    convolution permutations inverted, padding lanes dropped, and the one packed LSTM bias (``bias_ih + bias_hh``) giving the
    same gradient to both."""
    index = _pack_index(int(dim))
    n = (max(int(v.max()) for v in index.values()) + 1)
    if hasattr(packed, 'detach'):
        flat = packed.reshape(-1)
        if flat.shape[0] < n:
            raise ValueError('unpack_weight_grads: %d packed floats, need at least %d' % (flat.shape[0], n))
        return {k: flat[torch.from_numpy(v.reshape(-1)).to(flat.device)].reshape(v.shape) for k, v in index.items()}
    flat = np.asarray(packed).reshape(-1)
    if flat.shape[0] < n:
        raise ValueError('unpack_weight_grads: %d packed floats, need at least %d' % (flat.shape[0], n))
    return {k: flat[v] for k, v in index.items()}


# --------------------------------------------------------------------------------------------------
# labels (train_next.get_label)
# --------------------------------------------------------------------------------------------------
def _interpolate(prev, nxt, ratio, dim):
    if dim == 3:
        from .maze2d import Maze3D
        return Maze3D.interpolate(Maze3D, prev.copy(), nxt.copy(), ratio)
    return prev + (nxt - prev) * ratio


def path_labels(paths, path_ptr, env_or_dim):
    """``train_next.get_label`` for a batch of paths: ``paths`` [N, dim] holds the paths one after another, path ``i`` is rows
    ``path_ptr[i] : path_ptr[i + 1]``.  Returns ``(actions [N, dim], values [N])`` in float32, computed in float64 as the
    reference does: the value of a state is minus the cost to go along the path (plain Euclidean edge costs), the action is the
    step to the next state, cut to length ``RRT_EPS`` by the environment's ``interpolate`` (the stick robot's wraps its
    orientation), and zero for the last state."""
    dim = int(getattr(env_or_dim, 'dim', env_or_dim))
    eps = float(getattr(env_or_dim, 'RRT_EPS', RRT_EPS))
    paths = np.asarray(paths, dtype=np.float64).reshape(-1, dim)
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
                actions[k] = _interpolate(prev, nxt, eps / edge, dim) - prev
            else:
                actions[k] = nxt - prev
        values[a:b] = np.array(cost) - cost[-1]
    return actions.astype(np.float32), values.astype(np.float32)


# --------------------------------------------------------------------------------------------------
# the loss of train()
# --------------------------------------------------------------------------------------------------
def loss_from_outputs(y, actions, values, ptr):
    """The mean over the paths of ``MSE(value) + MSE(action)`` from ``y`` [N, dim + 1]: what ``train()`` calls ``.backward()``
    on when a step holds 8 paths.  Differentiable in ``y``; shared with the tests' host oracle."""
    total = 0.
    for a, b in zip(ptr[:-1], ptr[1:]):
        a, b = int(a), int(b)
        total = total + ((values[a:b] - y[a:b, -1]) ** 2).mean() + ((actions[a:b] - y[a:b, :-1]) ** 2).mean()
    return total / (len(ptr) - 1)


def training_loss(net, maps, goals, paths, path_ptr, iters=DEFAULT_ITERS):
    """The value of the reference's training loss for a batch of ``(problem, path)`` samples on the device: problem ``i`` is
    ``maps[i]``, ``goals[i]`` (device tensors) with the path ``paths[path_ptr[i] : path_ptr[i + 1]]`` (host array, float64 as
    the planners return it).  ``net`` is a :class:`gnnmp.next_model.NextNet`; the states enter as float32, as in
    ``Model2D.net_forward``.  Evaluation only: the inference kernels keep no gradient history."""
    ptr = np.asarray(path_ptr, dtype=np.int64).reshape(-1)
    paths = np.asarray(paths, dtype=np.float64).reshape(-1, net.dim)
    actions, values = path_labels(paths, ptr, net.dim)
    dev = maps.device
    of = torch.from_numpy(np.repeat(np.arange(ptr.size - 1, dtype=np.int32), np.diff(ptr))).to(dev)
    y = net.state_forward(torch.from_numpy(paths.astype(np.float32)).to(dev), of, net.pb_forward(maps, goals, iters))
    return loss_from_outputs(y, torch.from_numpy(actions).to(dev), torch.from_numpy(values).to(dev), ptr)
