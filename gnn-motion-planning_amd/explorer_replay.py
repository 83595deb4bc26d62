"""The explorer's training loop on maze problems with the dataset on the device: what the reference's ``train_explorer.py``
(:96-210) does around one optimizer step, over the labelled graphs of ``algorithm/dijkstra.py:91-97``.  The counterpart of
:mod:`gnnmp.next_replay` and :mod:`gnnmp.smoother_replay` for the project's headline network.

  * :class:`ExplorerDataset`    the ``(points, neighbors, edge_cost, edge_index, edge_free)`` entries of ``dijkstra.py:91-97``
    for any number of maze problems as device arrays with three prefix arrays; :meth:`ExplorerDataset.batch` hands the
    problems of a step to the pipeline as a :class:`gnnmp.episodes.TrainingGraphs` through ``gnnmp_episode_dataset_gather``:
    rows, edges, labels, obstacles and the batch's prefix arrays in one launch after one small upload (the indices).  The host
    keeps a mirror of the prefix arrays only; a step reads nothing back.
  * :func:`build_maze_dataset`  ``dijkstra.py:91-97`` for maze problems: per problem ``randint(100, 400)`` plain uniform points
    (``MazeEnv.uniform_sample(n)``, not rejection-sampled) and ``construct_graph``.
  * :func:`frontier_loss`       the loss of ``:172`` as a ``torch.autograd.Function`` over ``gnnmp_episode_frontier_loss``;
    :func:`frontier_loss_reference` is the same value in float64 torch.
  * :func:`explorer_schedule`   the loop order of ``:120-204``: a permutation per iteration, ``T`` running on across
    iterations, an optimizer step after the sample at which ``T % 8 == 0`` -- so the groups are ``[1, 8, 8, ...]`` -- and the
    samples behind the last step, which are backpropagated but never stepped.
  * :func:`train_dataset`       the loop itself; :func:`train_explorer_maze` builds the dataset, runs Adam and returns the
    history.  ``model.state_dict()`` afterwards is the checkpoint, under the reference's names.

Deviations from the reference, on purpose:
  * the draws of a step (goal, loop count, start, replay step) are per problem and independent, as
    :func:`gnnmp.episodes.draw_device` makes them; the reference draws them from its one global numpy stream, each draw after
    the previous sample's outcome;
  * a skipped sample (only the goal is reachable, or the frontier emptied) still takes its place in its group; in the reference
    ``T`` does not advance for it, so its group takes one more sample.  Knowing this before grouping would need a read-back
    per sample;
  * the points and the permutations come from ``RandomState(1234)`` (``rng``), the reference draws them from the global
    generator (the points in another process, ``dijkstra.py``'s).

The kernels are the only implementation: nothing here falls back to the host.
"""
import ctypes
import time

import numpy as np
import torch

from . import episodes as ep

STATUS_BAD_INDEX, STATUS_BAD_GATHER = 1, 2
LOSS_BAD_ENTRY, LOSS_BAD_RANGE, LOSS_TOO_LARGE = 1, 2, 4
MAX_LOSS_EDGES = 16384                  # edges of one problem gnnmp_episode_frontier_loss counts in LDS
LIMITS = (1.0, 1.0, 0.4)                # environment/env_config.py:5, the box MazeEnv.uniform_sample draws from


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# --------------------------------------------------------------------------------------------------
# the dataset
# --------------------------------------------------------------------------------------------------
class ExplorerDataset:
    """Labelled maze graphs as device arrays (``gnnmp_episode_dataset`` of ``include/gnnmp.h``): ``v`` [sumN, dim] float32,
    ``points64`` [sumN, dim] float64, ``edge_index`` [2, sumE] int64 (graph-local), ``edge_free`` uint8 / ``edge_cost`` float64
    [sumE], ``obstacles`` [sumO, 2] float32 and the int32 prefix arrays ``node_ptr`` / ``edge_ptr`` / ``obs_ptr`` [n + 1], whose
    host mirrors are ``host_node_ptr`` / ``host_edge_ptr`` / ``host_obs_ptr``.  Problem ``i`` is rows ``node_ptr[i] :
    node_ptr[i + 1]`` of ``v`` and ``points64``, columns ``edge_ptr[i] : edge_ptr[i + 1]`` of the edge arrays and rows
    ``obs_ptr[i] : obs_ptr[i + 1]`` of ``obstacles``."""

    OBS_SIZE = 2

    def __init__(self, dim, device='cuda'):
        dim = int(dim)
        if dim not in (2, 3):
            raise ValueError('ExplorerDataset: maze problems are 2-D (point robot) or 3-D (stick robot), got dim %d' % dim)
        self.dim = dim
        self.device = dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError('ExplorerDataset: a device dataset (the kernels are the only implementation)')
        new = lambda dtype, *shape: torch.zeros(*shape, dtype=dtype, device=dev)      # noqa: E731
        self.v, self.points64 = new(torch.float32, 0, dim), new(torch.float64, 0, dim)
        self.edge_index = new(torch.int64, 2, 0)
        self.edge_free, self.edge_cost = new(torch.uint8, 0), new(torch.float64, 0)
        self.obstacles = new(torch.float32, 0, self.OBS_SIZE)
        self.node_ptr, self.edge_ptr, self.obs_ptr = new(torch.int32, 1), new(torch.int32, 1), new(torch.int32, 1)
        self.status = new(torch.int32, 1)
        self.host_node_ptr = np.zeros(1, dtype=np.int64)
        self.host_edge_ptr = np.zeros(1, dtype=np.int64)
        self.host_obs_ptr = np.zeros(1, dtype=np.int64)
        self._pad = new(torch.float64, 2)                        # what the pointer of an empty array is replaced by

    def __len__(self):
        return int(self.host_node_ptr.shape[0]) - 1

    def sizes(self):
        """Nodes per problem, by the host mirror."""
        return np.diff(self.host_node_ptr).tolist()

    def add(self, points64, node_ptr, maps):
        """Label a chunk of maze problems with :func:`gnnmp.episodes.maze_training_graphs` (``construct_graph``) and append
        it: ``points64`` [sumN, dim] float64 on the device, ``node_ptr`` a host sequence [B + 1], ``maps`` [B, w, w].  Returns
        the number of problems appended."""
        return self.add_graphs(ep.maze_training_graphs(points64.to(self.device), node_ptr, maps, self.dim))

    def add_graphs(self, graphs):
        """Append the problems of a labelled :class:`gnnmp.episodes.TrainingGraphs` (with its ``points64``)."""
        if graphs.points64 is None or int(graphs.v.shape[1]) != self.dim:
            raise ValueError('ExplorerDataset.add_graphs: labelled maze graphs of dim %d with their float64 points' % self.dim)
        if int(graphs.obstacles.shape[1]) != self.OBS_SIZE:
            raise ValueError('ExplorerDataset.add_graphs: obstacle rows of %d columns' % self.OBS_SIZE)
        dev = self.device
        grow = lambda ptr, more: np.concatenate([ptr, ptr[-1] + np.asarray(more, dtype=np.int64)[1:]])      # noqa: E731
        node_ptr, edge_ptr = grow(self.host_node_ptr, graphs.node_ptr_host), grow(self.host_edge_ptr, graphs.edge_ptr_host)
        obs_ptr = grow(self.host_obs_ptr, graphs.obs_ptr_host)
        if max(node_ptr[-1], edge_ptr[-1], obs_ptr[-1]) >= 2 ** 31 - 1:
            raise ValueError('ExplorerDataset: more than 2^31 - 2 rows')
        with torch.cuda.device(dev):
            self.v = torch.cat([self.v, graphs.v.to(torch.float32)])
            self.points64 = torch.cat([self.points64, graphs.points64.to(torch.float64)])
            self.edge_index = torch.cat([self.edge_index, graphs.edge_index], dim=1).contiguous()
            self.edge_free = torch.cat([self.edge_free, graphs.edge_free])
            self.edge_cost = torch.cat([self.edge_cost, graphs.edge_cost])
            self.obstacles = torch.cat([self.obstacles, graphs.obstacles.to(torch.float32)])
            up = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)                                     # noqa: E731
            self.node_ptr, self.edge_ptr, self.obs_ptr = up(node_ptr), up(edge_ptr), up(obs_ptr)
        self.host_node_ptr, self.host_edge_ptr, self.host_obs_ptr = node_ptr, edge_ptr, obs_ptr
        return graphs.n_problems

    def _ptr(self, t):
        return t.data_ptr() if t.numel() else self._pad.data_ptr()

    def _struct(self):
        from . import _lib
        return _lib.EpisodeDataset(len(self), int(self.host_node_ptr[-1]), int(self.host_edge_ptr[-1]), int(self.host_obs_ptr[-1]),
                                   self.dim, self.OBS_SIZE, self._ptr(self.v), self._ptr(self.points64), self._ptr(self.edge_index),
                                   self._ptr(self.edge_free), self._ptr(self.edge_cost), self._ptr(self.obstacles),
                                   self.node_ptr.data_ptr(), self.edge_ptr.data_ptr(), self.obs_ptr.data_ptr(),
                                   self.status.data_ptr())

    def check_status(self):
        """Read the status word (a synchronising read), clear it, and raise if a bit was set."""
        status = int(self.status.cpu())
        if status:
            self.status.zero_()
            why = [text for bit, text in (
                (STATUS_BAD_INDEX, 'an index outside [0, %d): that slot of its batch is empty' % len(self)),
                (STATUS_BAD_GATHER, 'prefix entries or totals on the device that differ from the host mirror\'s: that batch was not '
                                    'written')) if status & bit]
            raise RuntimeError('ExplorerDataset: status %d: %s' % (status, '; '.join(why)))

    def batch(self, idx):
        """The problems at the store positions ``idx`` (any order, repeats allowed) as a
        :class:`gnnmp.episodes.TrainingGraphs`: one upload (the indices) and one launch (``gnnmp_episode_dataset_gather``);
        the sizes come from the host mirror and nothing is read back.  A position outside the store is not clamped and does
        not raise here: its slot is an empty problem and :meth:`check_status` reports it."""
        from . import _lib
        dev = self.device
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        G = int(idx.size)
        if G == 0:
            raise ValueError('ExplorerDataset.batch: an empty group')
        inside = (idx >= 0) & (idx < len(self))
        at = np.where(inside, idx, 0)
        count = lambda ptr: np.where(inside, ptr[at + 1] - ptr[at], 0) if len(self) else np.zeros(G, dtype=np.int64)   # noqa: E731
        prefix = lambda c: np.concatenate([[0], np.cumsum(c)]).tolist()                                               # noqa: E731
        node_ptr, edge_ptr, obs_ptr = (prefix(count(p)) for p in (self.host_node_ptr, self.host_edge_ptr, self.host_obs_ptr))
        tn, te, to = node_ptr[-1], edge_ptr[-1], obs_ptr[-1]
        if max(tn, te, to) >= 2 ** 31 - 1:
            raise ValueError('ExplorerDataset.batch: more than 2^31 - 2 rows in one batch')
        with torch.cuda.device(dev):
            idx_d = torch.from_numpy(np.clip(idx, -2 ** 31, 2 ** 31 - 1).astype(np.int32)).to(dev)
            v = torch.empty(tn, self.dim, dtype=torch.float32, device=dev)
            points64 = torch.empty(tn, self.dim, dtype=torch.float64, device=dev)
            edge_index = torch.empty(2, te, dtype=torch.int64, device=dev)
            edge_free = torch.empty(te, dtype=torch.uint8, device=dev)
            edge_cost = torch.empty(te, dtype=torch.float64, device=dev)
            obstacles = torch.empty(to, self.OBS_SIZE, dtype=torch.float32, device=dev)
            ptrs = torch.zeros(3, G + 1, dtype=torch.int32, device=dev)       # a gather that refuses (status bit 2) leaves empty problems
            out = _lib.EpisodeDatasetBatch(G, tn, te, to, self._ptr(v), self._ptr(points64), self._ptr(edge_index),
                                           self._ptr(edge_free), self._ptr(edge_cost), self._ptr(obstacles), ptrs[0].data_ptr(),
                                           ptrs[1].data_ptr(), ptrs[2].data_ptr())
            store = self._struct()
            _lib.check(_lib.lib().gnnmp_episode_dataset_gather(ctypes.byref(store), G, idx_d.data_ptr(), ctypes.byref(out),
                                                               _stream(dev)), 'gnnmp_episode_dataset_gather')
            idx_d.record_stream(torch.cuda.current_stream(dev))
        return ep.TrainingGraphs(v, edge_index, node_ptr, edge_ptr, edge_free, edge_cost, obstacles, obs_ptr, points64=points64,
                                 device_ptrs=(ptrs[0], ptrs[1], ptrs[2]))


def draw_maze_points(n_problems, dim, n_lo=100, n_hi=400, rng=None):
    """The draws of ``dijkstra.py:94`` for ``n_problems`` maze problems in the reference's numpy call order: per problem
    ``rng.randint(n_lo, n_hi)`` and then ``MazeEnv.uniform_sample(n)`` = ``rng.uniform(-LIMITS[:dim], LIMITS[:dim], (n, dim))``
    -- plain uniform points, not rejection-sampled.  Returns a list of float64 arrays [n, dim]."""
    rng = np.random.RandomState(1234) if rng is None else rng
    lim = np.array(LIMITS[:int(dim)], dtype=np.float64)
    out = []
    for _ in range(int(n_problems)):
        n = rng.randint(n_lo, n_hi)
        out.append(rng.uniform(-lim, lim, (n, int(dim))))
    return out


def build_maze_dataset(maps, dim, device, n_lo=100, n_hi=400, rng=None, chunk=256):
    """``dijkstra.py:91-97`` for the maze problems of ``maps`` [n, w, w]: the points of :func:`draw_maze_points` (from
    ``RandomState(1234)`` by default), labelled ``chunk`` problems at a time.  Returns the :class:`ExplorerDataset`."""
    maps = np.asarray(maps)
    points = draw_maze_points(maps.shape[0], dim, n_lo, n_hi, rng)
    dataset = ExplorerDataset(dim, device)
    for c0 in range(0, maps.shape[0], int(chunk)):
        part = points[c0:c0 + int(chunk)]
        node_ptr = np.concatenate([[0], np.cumsum([p.shape[0] for p in part])]).tolist()
        dataset.add(torch.from_numpy(np.concatenate(part)).to(dataset.device), node_ptr, maps[c0:c0 + int(chunk)])
    return dataset


# --------------------------------------------------------------------------------------------------
# the loss of :172
# --------------------------------------------------------------------------------------------------
def frontier_loss_reference(scores, fr, divisor=1.0):
    """``gnnmp_episode_frontier_loss`` in float64 torch: ``(loss, terms [B], counted [B])`` with ``terms[b] =
    -scores[frontier_b].log_softmax(0)[label_b]`` over problem ``b``'s frontier LIST (an edge listed twice counts twice, as
    ``policy[frontier]`` does), 0 for a problem with ``status != 0``, ``frontier_len == 0`` or ``label < 0``, and ``loss =
    terms.sum() / divisor``.  Autograd flows back to ``scores``; ``fr`` as :func:`gnnmp.episodes.policy_frontier` returns it,
    on any device (read back problem by problem: for tests)."""
    s = scores.double()
    eptr = fr['edge_ptr'].cpu().tolist()
    flen, label, status = fr['frontier_len'].cpu().tolist(), fr['label'].cpu().tolist(), fr['status'].cpu().tolist()
    terms, counted = [], []
    for b in range(len(flen)):
        ok = status[b] == 0 and flen[b] > 0 and label[b] >= 0
        counted.append(ok)
        if ok:
            off = 2 * eptr[b] + b
            ids = fr['frontier'][off:off + flen[b]].long().to(s.device)
            terms.append(-s[ids].log_softmax(0)[label[b]])
        else:
            terms.append(s.new_zeros(()))
    terms = torch.stack(terms) if terms else s.new_zeros(0)
    return terms.sum() / float(divisor), terms, torch.tensor(counted, dtype=torch.bool, device=s.device)


def frontier_loss_device(scores, fr, divisor=1.0, bad=None):
    """``gnnmp_episode_frontier_loss`` on device tensors: ``scores`` [sumE] float32 and the dict of
    :func:`gnnmp.episodes.policy_frontier` -> ``(terms [B] float32, counted [B] int32, loss [1] float32, dscores [sumE] float32,
    bad [1] int32)``.  One allocation, the loss launch and its one-lane sum on the current stream; nothing is read back.
    ``bad``: a device word of the caller's that accumulates the launch's complaints (see :func:`check_loss_status`)."""
    from . import _lib
    dev = scores.device
    if dev.type != 'cuda':
        raise RuntimeError('frontier_loss: device tensors only (the kernels are the only implementation)')
    B, E = int(fr['frontier_len'].numel()), int(fr['total_edges'])
    scores = scores.contiguous()
    if scores.dtype != torch.float32 or tuple(scores.shape) != (E,):
        raise ValueError('frontier_loss: scores must be float32 [%d]' % E)
    if not float(divisor) > 0:
        raise ValueError('frontier_loss: divisor is above 0')
    arrays = [fr[k].contiguous() for k in ('frontier', 'frontier_len', 'label', 'status', 'edge_ptr')]
    for name, t, n in zip(('frontier', 'frontier_len', 'label', 'status', 'edge_ptr'), arrays, (2 * E + B, B, B, B, B + 1)):
        if t.dtype != torch.int32 or t.device != dev or int(t.numel()) != n:
            raise ValueError('frontier_loss: %s must be int32 [%d] on %s' % (name, n, dev))
    with torch.cuda.device(dev):
        buf = torch.zeros(2 * B + 2 + max(E, 1), dtype=torch.float32, device=dev)      # edges outside every problem stay zero
        terms, counted, loss = buf[0:B], buf[B:2 * B].view(torch.int32), buf[2 * B:2 * B + 1]
        own_bad, dscores = buf[2 * B + 1:2 * B + 2].view(torch.int32), buf[2 * B + 2:2 * B + 2 + E]
        bad = own_bad if bad is None else bad
        if B > 0:
            desc = _lib.EpisodeFrontierLoss(B, E, float(divisor), *[t.data_ptr() for t in arrays], scores.data_ptr(), terms.data_ptr(),
                                            counted.data_ptr(), loss.data_ptr(), buf[2 * B + 2:].data_ptr(), bad.data_ptr())
            _lib.check(_lib.lib().gnnmp_episode_frontier_loss(ctypes.byref(desc), _stream(dev)), 'gnnmp_episode_frontier_loss')
    return terms, counted, loss, dscores, bad


def check_loss_status(bad):
    """Read a ``bad`` word of :func:`frontier_loss_device` (a synchronising read), clear it, and raise if a bit was set."""
    word = int(bad.cpu())
    if word:
        bad.zero_()
        why = [text for bit, text in (
            (LOSS_BAD_ENTRY, 'a frontier entry, length or label outside its problem (the entry, or the problem, contributed nothing)'),
            (LOSS_BAD_RANGE, 'edge_ptr entries that do not ascend inside the edges'),
            (LOSS_TOO_LARGE, 'a problem of more than %d edges (not counted)' % MAX_LOSS_EDGES)) if word & bit]
        raise RuntimeError('gnnmp_episode_frontier_loss: bad %d: %s' % (word, '; '.join(why)))


class _FrontierLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, fr, divisor, bad):
        terms, counted, loss, dscores, _ = frontier_loss_device(scores.detach(), fr, divisor, bad)
        ctx.save_for_backward(dscores)
        ctx.mark_non_differentiable(terms, counted)
        return loss.reshape(()), terms, counted

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms, _grad_counted):
        dscores, = ctx.saved_tensors
        return dscores * grad_loss.to(torch.float32), None, None, None


def frontier_loss(scores, fr, divisor=1.0, return_terms=False, bad=None):
    """``(sum over the problems of -policy[frontier].log_softmax(0)[next_edge_idx]) / divisor`` (train_explorer.py:172) from the
    per-edge ``scores`` [sumE] of the training forward and the dict of :func:`gnnmp.episodes.policy_frontier`, as a float32
    device scalar with a gradient history to ``scores``: what :func:`gnnmp.episodes.frontier_loss` computes with about twenty
    torch launches, in one (plus the one-lane sum).  The backward scales the kernel's ``dscores`` by the incoming scalar.
    With ``return_terms`` also the per-problem terms [B] (float32, no history) and the mask [B] of the problems that count.
    ``bad``: see :func:`frontier_loss_device`."""
    loss, terms, counted = _FrontierLossFn.apply(scores, fr, float(divisor), bad)
    return (loss, terms, counted != 0) if return_terms else loss


# --------------------------------------------------------------------------------------------------
# train_explorer()
# --------------------------------------------------------------------------------------------------
def _schedule(n, iters, group, rng):
    rng = np.random.RandomState(1234) if rng is None else rng
    n, group = int(n), int(group)
    groups, at_iter, cur, T = [], [], [], 0
    for it in range(int(iters)):
        for index in rng.permutation(n):
            cur.append(int(index))
            if T % group == 0:
                groups.append(np.array(cur, dtype=np.int64))
                at_iter.append(it)
                cur = []
            T += 1
    return groups, np.array(cur, dtype=np.int64), at_iter


def explorer_schedule(n, iters=20, group=8, rng=None):
    """The optimizer steps of ``train_explorer.py:120-204`` over a dataset of ``n`` problems: per iteration one
    ``rng.permutation(n)``; ``T`` counts the samples across iterations and is never reset, and the optimizer steps after the
    sample at which ``T % group == 0`` -- after the very first one, then after every ``group`` more, so the groups are ``[1,
    group, group, ...]`` and one may span two iterations.  Returns ``(groups, dropped)``: the store positions of every step
    (int64 arrays) and those behind the last step, which the reference backpropagates but never steps."""
    groups, dropped, _ = _schedule(n, iters, group, rng)
    return groups, dropped


def train_dataset(model, optimizer, dataset, iters=20, group=8, loop=10, max_steps=1000, rng=None, generator=None,
                  cpu_generator=None, batched=False, log=None):
    """The loop of ``train_explorer.py:120-204`` over ``dataset``: the groups of :func:`explorer_schedule`, each
    ``dataset.batch`` -> the pipeline of :func:`gnnmp.episodes.training_step` (``draw_device``, ``shortest_paths``,
    ``draw_start``, ``forward_scores`` -- ``batched``: ``forward_scores_batched`` --, ``explore_steps``, ``draw_step``,
    ``policy_frontier``) -> :func:`frontier_loss` with divisor 1 (the reference sums undivided per-sample gradients) ->
    backward -> ``optimizer.step()`` -> ``zero_grad()``.  The loss and the counted / skipped numbers of every step stay on the
    device and are read once at the end of an iteration; a step belongs to the iteration its last sample falls in.

    Returns the history, one dict per iteration: ``{'losses': the loss of every step, 'mean': their mean (0.0 without steps),
    'samples': samples in those steps, 'counted' / 'single' / 'empty': samples that gave a loss / were skipped because only the
    goal is reachable / because the frontier emptied, 'steps_per_s'}``.  ``log(iteration, entry)`` is called per iteration."""
    if len(dataset) == 0:
        raise ValueError('train_dataset: an empty dataset')
    groups, _, at_iter = _schedule(len(dataset), iters, group, rng)
    dev = dataset.device
    model.train()
    forward = ep.forward_scores_batched if batched else ep.forward_scores
    history, k = [], 0
    with torch.cuda.device(dev):
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        for it in range(int(iters)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            losses, numbers, samples = [], [], 0
            while k < len(groups) and at_iter[k] == it:
                graphs = dataset.batch(groups[k])
                goal, loops = ep.draw_device(graphs, loop, generator, cpu_generator)
                paths = ep.shortest_paths(graphs, goal)
                start = ep.draw_start(graphs, paths, generator)
                scores = forward(model, graphs, paths['goal'], loops)
                step, status = ep.explore_steps(graphs, scores, start, paths['goal'], paths['n_valid'], max_steps)
                fr = ep.policy_frontier(graphs, scores, paths, start, paths['goal'], ep.draw_step(step, generator), status)
                loss, _, counted = frontier_loss(scores, fr, 1.0, return_terms=True, bad=bad)
                loss.backward()
                optimizer.step()
                optimizer.zero_grad()
                losses.append(loss.detach())
                numbers.append(torch.stack([counted.sum(), (status == ep.STATUS_SINGLE).sum(), (status == ep.STATUS_EMPTY).sum()]))
                samples += len(groups[k])
                k += 1
            if losses:                                           # the iteration's one read-back
                host = torch.stack(losses).cpu().numpy().astype(np.float64)
                nums = torch.stack(numbers).sum(0).cpu().tolist()
            else:
                host, nums = np.zeros(0), [0, 0, 0]
            wall = time.perf_counter() - t0
            entry = {'losses': host.tolist(), 'mean': float(host.mean()) if host.size else 0.0, 'samples': samples,
                     'counted': int(nums[0]), 'single': int(nums[1]), 'empty': int(nums[2]),
                     'steps_per_s': len(losses) / wall if wall > 0 else 0.0}
            history.append(entry)
            if log is not None:
                log(it, entry)
        dataset.check_status()
        check_loss_status(bad)
    return history


def train_explorer_maze(model, maps, dim, device, iters=20, loop=10, lr=1e-3, group=8, seed=1234, n_lo=100, n_hi=400, chunk=256,
                        max_steps=1000, batched=False, log=None):
    """``train_explorer`` of ``train_explorer.py:96-210`` for the maze problems of ``maps`` [n, w, w]:
    :func:`build_maze_dataset` (``dijkstra.py:91-97``), ``model.train()`` on ``device``, Adam at ``lr`` (``config.lr = 1e-3``)
    and :func:`train_dataset`.  ``model`` is a :class:`gnnmp.EncoderProcessDecoder` (trained in place); ``seed`` seeds the
    ``RandomState`` of the points and permutations and the two torch generators of the per-problem draws.  See the module
    docstring for the deviations from the reference.  Returns the history of :func:`train_dataset`; ``model.state_dict()``
    afterwards is the checkpoint, under the reference's names."""
    dev = torch.device(device)
    rng = np.random.RandomState(int(seed))
    dataset = build_maze_dataset(maps, dim, dev, n_lo, n_hi, rng, chunk)
    if len(dataset) == 0:
        raise ValueError('train_explorer_maze: no problems')
    model.to(dev).train()
    optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    optimizer.zero_grad()
    generator = torch.Generator(device=dev)
    generator.manual_seed(int(seed))
    cpu_generator = torch.Generator()
    cpu_generator.manual_seed(int(seed))
    return train_dataset(model, optimizer, dataset, iters=iters, group=group, loop=loop, max_steps=max_steps, rng=rng,
                         generator=generator, cpu_generator=cpu_generator, batched=batched, log=log)
