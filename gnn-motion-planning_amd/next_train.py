"""Training the NEXT planning network on maze problems (``Model2D`` / ``PPN``, dim 2 and 3).  The step of the reference's
``train_next.py:41-69`` is, per ``(problem, path)`` sample, an MSE on the value column plus an MSE on the action columns,
averaged over the problems of a step, with the gradient through the whole network.  Here:

  * :func:`path_labels`          ``train_next.get_label`` for a batch of paths (host, float64 as the reference).
  * :func:`loss_from_outputs`, :func:`training_loss`   the loss ``train()`` differentiates, from any ``y``, and its value on the
    device through the inference kernels of :class:`gnnmp.next_model.NextNet`.
  * :func:`param_shapes`, :func:`unpack_weight_grads`  a gradient in the packed weight layout of the kernels -> a dict under the
    reference's parameter names (the exact adjoint of :func:`gnnmp.next_model.pack_weights`).
  * :func:`device_pack`, :func:`pack_weights_t`, :func:`device_pack_t`   the packed weights, and the transposed packing the
    backward streams, built on the device from the parameter tensors.
  * :class:`NextNetTrain`        the trainable network: torch Parameters on the device, ``forward`` through one
    ``torch.autograd.Function`` over ``gnnmp_next_train_forward`` / ``gnnmp_next_state_backward`` / ``gnnmp_next_pb_backward``
    (``csrc/next_train_kernels.hip``), and ``train_step``, one optimizer step of ``train()``.

What is specific to the mazes lives here: the parameter shapes, the transposed packing, the labels' step, :data:`FAMILY`.  The
body it describes the mazes to -- the packing index and its adjoint, the autograd function, the network's base class, the label
loop -- is :mod:`gnnmp.next_train_core`, shared with :mod:`gnnmp.next_train3d`.
"""
import numpy as np

from . import _lib, next_train_core as core
from .next_model import DEFAULT_ITERS, WIDTH, _conv_pack, _mfma_pack, _np_weights, pack_weights
from .next_train_core import loss_from_outputs  # noqa: F401  (one loss for both families; tests and tools take it from here)

RRT_EPS = 5e-2                              # environment/env_config.py
_SHARE = (0, 2, 4, 6, 8, 10)


def _check_dims(dims, who):
    dim, = (int(d) for d in dims)
    if dim not in (2, 3):
        raise ValueError('%s: dim is 2 (point robot) or 3 (stick robot)' % who)
    return (dim,)


def param_shapes(dim):
    """The reference's trainable parameters (``PPN.named_parameters()``: ``attention_s`` is ``attention_g``, listed once)."""
    dim, = _check_dims((dim,), 'next_train')
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


def pack_weights_t(weights, dim):
    """The transposed packing the backward streams (``gnnmp_next_weights_t_floats`` floats): ``conv``, ``h0`` and ``c0`` with
    flipped taps and the channel matrix transposed, in the convolution packing of :func:`pack_weights` (so the forward's
    convolution routine computes the transposed convolution), the LSTM's ``[256 gate rows][x 64 | h 64]`` in the MFMA packing,
    and 64 zeros (the bias the transposed convolutions read)."""
    w = _np_weights(weights, np.float32)
    parts = [_conv_pack(np.ascontiguousarray(np.flip(w[name + '.weight'].transpose(1, 0, 2, 3), (2, 3)))) for name in ('conv', 'h0', 'c0')]
    parts.append(_mfma_pack(np.ascontiguousarray(np.concatenate([w['lstm.weight_ih'], w['lstm.weight_hh']], axis=1))))
    parts.append(np.zeros(64, dtype=np.float32))
    return np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in parts]))


_T_NAMES = ('conv.weight', 'h0.weight', 'c0.weight', 'lstm.weight_ih', 'lstm.weight_hh')

FAMILY = core.Family(
    module='next_train', cls='NextNetTrain', noun='state', goal='goal', check=_check_dims,
    param_shapes=param_shapes, pack=pack_weights, pack_t=pack_weights_t, t_names=_T_NAMES,
    structs=(_lib.NextTrain, _lib.NextTrainBwd),
    entries=('gnnmp_next_train_workspace_bytes', 'gnnmp_next_train_forward', 'gnnmp_next_state_backward', 'gnnmp_next_pb_backward'),
    map_shape=(WIDTH, WIDTH))


def _pack_index(dim):
    """name -> int64 array of the parameter's shape: where each element lands in the packed vector.  Read off
    ``pack_weights`` itself (one parameter at a time set to 1, 2, 3, ...), so the two cannot drift apart."""
    return core.pack_index(FAMILY, (dim,))[0]


def device_pack(params, dim):
    """:func:`gnnmp.next_model.pack_weights` on the tensors' own device: every reference-named parameter scattered through
    :func:`_pack_index` into zeros (:func:`gnnmp.next_train_core.scatter`).  Bit-equal to ``pack_weights``, the one packed
    LSTM bias ``bias_ih + bias_hh`` included."""
    return core.scatter(FAMILY, _check_dims((dim,), 'next_train.device_pack'), 'w', params)


def device_pack_t(params, dim):
    """:func:`pack_weights_t` on the tensors' own device."""
    return core.scatter(FAMILY, _check_dims((dim,), 'next_train.device_pack_t'), 't', params)


def unpack_weight_grads(packed, dim):
    """The gradient with respect to the packed weights -> the gradient with respect to the reference's parameters, as a dict of
    arrays (numpy in, numpy out; a torch tensor in, tensors on its device out).  The adjoint of ``pack_weights``: the MFMA and
    convolution permutations inverted, padding lanes dropped, and the one packed LSTM bias (``bias_ih + bias_hh``) giving the
    same gradient to both."""
    return core.unpack(FAMILY, _check_dims((dim,), 'next_train.unpack_weight_grads'), packed)


# --------------------------------------------------------------------------------------------------
# labels (train_next.get_label) and the loss of train()
# --------------------------------------------------------------------------------------------------
def _interpolate(dim):
    """The environment's ``interpolate`` as the label loop's ``step(prev, nxt, ratio)``."""
    if dim == 3:
        from .maze2d import Maze3D
        return lambda prev, nxt, ratio: Maze3D.interpolate(Maze3D, prev.copy(), nxt.copy(), ratio)
    return lambda prev, nxt, ratio: prev + (nxt - prev) * ratio


def path_labels(paths, path_ptr, env_or_dim):
    """``train_next.get_label`` for a batch of paths: ``paths`` [N, dim] holds the paths one after another, path ``i`` is rows
    ``path_ptr[i] : path_ptr[i + 1]``.  Returns ``(actions [N, dim], values [N])`` in float32, computed in float64 as the
    reference does: the value of a state is minus the cost to go along the path (plain Euclidean edge costs), the action is the
    step to the next state, cut to length ``RRT_EPS`` by the environment's ``interpolate`` (the stick robot's wraps its
    orientation), and zero for the last state."""
    dim = int(getattr(env_or_dim, 'dim', env_or_dim))
    eps = float(getattr(env_or_dim, 'RRT_EPS', RRT_EPS))
    return core.path_labels(np.asarray(paths, dtype=np.float64).reshape(-1, dim), path_ptr, eps, _interpolate(dim))


def training_loss(net, maps, goals, paths, path_ptr, iters=DEFAULT_ITERS):
    """The value of the reference's training loss for a batch of ``(problem, path)`` samples on the device: problem ``i`` is
    ``maps[i]``, ``goals[i]`` (device tensors) with the path ``paths[path_ptr[i] : path_ptr[i + 1]]`` (host array, float64 as
    the planners return it).  ``net`` is a :class:`gnnmp.next_model.NextNet`; the states enter as float32, as in
    ``Model2D.net_forward``.  Evaluation only: the inference kernels keep no gradient history."""
    paths, ptr = core.sample_arrays(paths, path_ptr, net.dim)
    return core.sample_loss(lambda states, of: net.state_forward(states, of, net.pb_forward(maps, goals, iters)),
                            paths.astype(np.float32), ptr, path_labels(paths, ptr, net.dim), maps.device)


# --------------------------------------------------------------------------------------------------
# the trainable network on the device
# --------------------------------------------------------------------------------------------------
class NextNetTrain(core.TrainNet):
    """The NEXT network with trainable parameters on the device (:class:`gnnmp.next_train_core.TrainNet`; its ``state_dict`` is
    what :class:`gnnmp.next_model.NextNet` and ``Model2D`` load).  ``forward(maps, goals, states, problem_of_state, iters)``:
    ``maps`` [B, 15, 15], ``goals`` [B, dim], ``states`` [S, dim], ``problem_of_state`` [S] (any order, repeats) -> ``y``
    [S, dim + 1] with a gradient history to the parameters."""
    family = FAMILY

    def __init__(self, dim, device='cuda'):
        super().__init__((dim,), device)
        self.dim, = self.dims

    def train_step(self, optimizer, maps, goals, paths, path_ptr, iters=DEFAULT_ITERS):
        """One step of ``train_next.py:41-69`` on a batch of ``(problem, path)`` samples (as :func:`training_loss` takes them):
        the labels on the host, then forward, loss, backward and ``optimizer.step()`` on the device.  Returns the loss as a
        device scalar; nothing is copied back."""
        paths, ptr = core.sample_arrays(paths, path_ptr, self.dim, 'NextNetTrain.train_step')
        return self._step(optimizer, maps, goals, paths.astype(np.float32), ptr, path_labels(paths, ptr, self.dim), iters)
