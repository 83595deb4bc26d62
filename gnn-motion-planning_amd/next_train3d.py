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
``env.get_robot_points``, PyBullet's forward kinematics on the host).  What is specific to the arms lives here: the parameter
shapes, the transposed packing, the labels' step, the rows, :data:`FAMILY`.  The body it describes the arms to is
:mod:`gnnmp.next_train_core`, shared with :mod:`gnnmp.next_train`.
"""
import numpy as np

from . import _lib, next_train_core as core
from .next_model import _mfma_pack, _np_weights
from .next_model3d import DEFAULT_ITERS, MAX_DIM, POINT_DIMS, WIDTH, _conv_pack, pack_weights

_SHARE = (0, 2, 4, 6, 8, 10)


def _check_dims(dims, who):
    dim, point_dim = (int(d) for d in dims)
    if not 1 <= dim <= MAX_DIM or point_dim not in POINT_DIMS:
        raise ValueError('%s: 1 <= dim <= %d and point_dim is 3 or 6' % (who, MAX_DIM))
    return dim, point_dim


def param_shapes(dim, point_dim):
    """The reference's trainable parameters (``PPN.named_parameters()``: ``attention_s`` is ``attention_g``, listed once)."""
    dim, point_dim = _check_dims((dim, point_dim), 'next_train3d')
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


_T_NAMES = ('conv.weight', 'h0.weight', 'c0.weight', 'lstm.weight_ih', 'lstm.weight_hh')

FAMILY = core.Family(
    module='next_train3d', cls='NextNet3DTrain', noun='row', goal='goal row', check=_check_dims,
    param_shapes=param_shapes, pack=pack_weights, pack_t=pack_weights_t, t_names=_T_NAMES,
    structs=(_lib.Next3dTrain, _lib.Next3dTrainBwd),
    entries=('gnnmp_next3d_train_workspace_bytes', 'gnnmp_next3d_train_forward', 'gnnmp_next3d_state_backward',
             'gnnmp_next3d_pb_backward'),
    map_shape=(WIDTH, WIDTH, WIDTH))


def _pack_index(dim, point_dim):
    """name -> int64 array of the parameter's shape: where each element lands in the packed vector.  Read off
    ``next_model3d.pack_weights`` itself (one parameter at a time set to 1, 2, 3, ...), so the two cannot drift apart."""
    return core.pack_index(FAMILY, (dim, point_dim))[0]


def device_pack(params, dim, point_dim):
    """:func:`gnnmp.next_model3d.pack_weights` on the tensors' own device: every reference-named parameter scattered through
    :func:`_pack_index` into zeros (:func:`gnnmp.next_train_core.scatter`).  Bit-equal to ``pack_weights``, the one packed
    LSTM bias ``bias_ih + bias_hh`` included."""
    return core.scatter(FAMILY, _check_dims((dim, point_dim), 'next_train3d.device_pack'), 'w', params)


def device_pack_t(params, dim, point_dim):
    """:func:`pack_weights_t` on the tensors' own device."""
    return core.scatter(FAMILY, _check_dims((dim, point_dim), 'next_train3d.device_pack_t'), 't', params)


def unpack_weight_grads(packed, dim, point_dim):
    """The gradient with respect to the packed weights -> the gradient with respect to the reference's parameters, as a dict of
    arrays (numpy in, numpy out; a torch tensor in, tensors on its device out).  The adjoint of ``pack_weights``: the MFMA and
    convolution permutations inverted, the padding lanes dropped (the first attention layer's 12, the a3 MLP's 16, the policy's
    16 output rows, the last bias's 3 zeros, the hidden convolution's channels 9 .. 15), and the one packed LSTM bias
    (``bias_ih + bias_hh``) giving the same gradient to both."""
    return core.unpack(FAMILY, _check_dims((dim, point_dim), 'next_train3d.unpack_weight_grads'), packed)


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
    lo = None if lo is None else np.asarray(lo, dtype=np.float64).reshape(dim)
    hi = None if hi is None else np.asarray(hi, dtype=np.float64).reshape(dim)

    def interpolate(prev, nxt, ratio):
        new = prev + (nxt - prev) * ratio
        if lo is not None:
            new = np.maximum(new, lo)
        if hi is not None:
            new = np.minimum(new, hi)
        return new
    return core.path_labels(paths, path_ptr, float(rrt_eps), interpolate)


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
    paths, ptr = core.sample_arrays(paths, path_ptr, net.dim)
    labels = path_labels(paths, ptr, rrt_eps, lo, hi)
    return core.sample_loss(lambda rows, of: net.state_forward(rows, of, net.pb_forward(maps, goal_rows, iters)),
                            _rows(points, paths, net.point_dim, net.dim), ptr, labels, maps.device)


# --------------------------------------------------------------------------------------------------
# the trainable network on the device
# --------------------------------------------------------------------------------------------------
class NextNet3DTrain(core.TrainNet):
    """The 3-D NEXT network with trainable parameters on the device (:class:`gnnmp.next_train_core.TrainNet`; its
    ``state_dict`` is what :class:`gnnmp.next_model3d.NextNet3D` and ``Model3D`` load).  ``forward(maps, goal_rows, rows,
    problem_of_state, iters)``: ``maps`` [B, 15, 15, 15], ``goal_rows`` [B, point_dim + dim], ``rows`` [S, point_dim + dim],
    ``problem_of_state`` [S] (any order, repeats) -> ``y`` [S, dim + 1] with a gradient history to the parameters.  The
    workspace of the saved activations is about 55 MB a problem at 20 rounds."""
    family = FAMILY

    def __init__(self, dim, point_dim=3, device='cuda'):
        super().__init__((dim, point_dim), device)
        self.dim, self.point_dim = self.dims
        self.row = self.dim + self.point_dim

    def train_step(self, optimizer, maps, goal_rows, points, paths, path_ptr, rrt_eps, lo=None, hi=None, iters=DEFAULT_ITERS):
        """One step of ``train_next.py:41-69`` on a batch of ``(problem, path)`` samples (as :func:`training_loss` takes them):
        the labels on the host, then forward, loss, backward and ``optimizer.step()`` on the device.  Returns the loss as a
        device scalar; nothing is copied back."""
        paths, ptr = core.sample_arrays(paths, path_ptr, self.dim, 'NextNet3DTrain.train_step')
        labels = path_labels(paths, ptr, rrt_eps, lo, hi)
        return self._step(optimizer, maps, goal_rows, _rows(points, paths, self.point_dim, self.dim), ptr, labels, iters)
