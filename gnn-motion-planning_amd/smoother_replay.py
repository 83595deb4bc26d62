"""The smoother's training loop on maze problems with the replay on the device: what the reference's ``train_smoother.py``
does around one optimizer step, for ``maze2`` / ``maze3``.  The counterpart of :mod:`gnnmp.next_replay` for the other network.

  * :class:`SmoothReplayStore`  the ``(path, path_smooth, free, collided)`` samples of ``train_smoother.py:96-99`` as device
    arrays, filled by ``gnnmp_smooth_replay_append`` with ``obs_data``'s rule (the first 500 free and 500 collided rows, one
    zero row for an empty side, ``:20-30``); :meth:`SmoothReplayStore.batch` hands the 8 samples of a step to the network as a
    complete :class:`gnnmp.smoother.SmoothBatch` through ``gnnmp_smooth_replay_gather``: rows, chain edges and prefix arrays in
    one launch, already longest loop first.  The host keeps a mirror of the three prefix arrays and ``problem`` only, refreshed
    by one small read-back per append call; a step reads nothing back.
  * :func:`path_loss`           the loss ``train()`` differentiates (``:55-58``) as a ``torch.autograd.Function`` over
    ``gnnmp_smooth_path_loss``; :func:`path_loss_reference` restates it in float64 numpy with the same order of sums.
  * :func:`replay_schedule`     the permutations, groups and loop counts of ``:106-118, 41, 53`` from one ``RandomState``.
  * :func:`train_replay`        the training passes of ``train_env`` (``:198-220``).
  * :func:`random_init_goal`    ``MazeEnv.set_random_init_goal``.
  * :func:`collect_replay`      ``:91-99`` for a chunk of problems; :func:`train_smoother_maze` is ``train_env`` (``:136-222``).

Deviations from the reference, on purpose:
  * every problem draws its samples from its own stream (``streams_batch.stream_seeds``, mixed with the number of the collection
    pass); the reference continues the one global generator from problem to problem;
  * the draws of the smoothing targets come from a torch device generator, as :func:`gnnmp.oracle_smooth.smoothing_targets`
    already does;
  * the problems are collected in ascending chunks, the reference walks a permutation of them; ``train()`` permutes the replay,
    so the order has no effect on the distribution of its steps;
  * the start / goal draws, the permutations and the loop counts come from ``RandomState(1234)`` (``rng``), the reference draws
    them from the global generator.

The kernels are the only implementation: nothing here falls back to the host.
"""
import ctypes

import numpy as np
import torch

STATUS_FULL, STATUS_BAD_SOURCE, STATUS_BAD_GATHER = 1, 2, 4
MAX_SIDE = 500                          # obs_data: free[:500], collided[:500]
PASS_SEED_MIX = 0x85EBCA6B              # seeds of collection pass p: stream_seeds(...) ^ (p * PASS_SEED_MIX)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# --------------------------------------------------------------------------------------------------
# the store
# --------------------------------------------------------------------------------------------------
class SmoothReplayStore:
    """The replay as device arrays (``gnnmp_smooth_replay`` of ``include/gnnmp.h``): ``path`` / ``target`` [cap_path_rows, C],
    ``free`` [cap_free_rows, C], ``collided`` [cap_coll_rows, C], the prefix arrays ``path_ptr`` / ``free_ptr`` / ``coll_ptr``
    [cap_samples + 1] and ``problem`` [cap_samples].  Sample ``i`` is rows ``path_ptr[i] : path_ptr[i + 1]`` of ``path`` and
    ``target`` and the like of the other two.  An append is all or nothing: one that does not fit any of the four capacities,
    or whose source is malformed, leaves the store and its mirror as they were and raises."""

    def __init__(self, C, cap_samples, cap_path_rows, cap_free_rows, cap_coll_rows, device='cuda'):
        C = int(C)
        caps = [int(cap_samples), int(cap_path_rows), int(cap_free_rows), int(cap_coll_rows)]
        if C < 2 or C > 14:
            raise ValueError('SmoothReplayStore: config_size is 2 .. 14')
        if min(caps) < 0 or max(caps) >= 2 ** 31 - 1:
            raise ValueError('SmoothReplayStore: capacities are 0 .. 2^31 - 2')
        self.C = C
        self.cap_samples, self.cap_path_rows, self.cap_free_rows, self.cap_coll_rows = caps
        self.device = dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError('SmoothReplayStore: a device store (the kernels are the only implementation)')
        new = lambda dtype, *shape: torch.zeros(*shape, dtype=dtype, device=dev)      # noqa: E731
        self.path = new(torch.float32, max(caps[1], 1), C)
        self.target = new(torch.float32, max(caps[1], 1), C)
        self.free = new(torch.float32, max(caps[2], 1), C)
        self.collided = new(torch.float32, max(caps[3], 1), C)
        self.path_ptr = new(torch.int32, caps[0] + 1)
        self.free_ptr = new(torch.int32, caps[0] + 1)
        self.coll_ptr = new(torch.int32, caps[0] + 1)
        self.problem = new(torch.int32, max(caps[0], 1))
        self._words = new(torch.int32, 17)                       # counts [2, 4], status [1], pending [8]
        self.counts, self.status, self._pending = self._words[0:8], self._words[8:9], self._words[9:17]
        self.epoch = 0                                           # append launches so far: counts bank (epoch & 1) is current
        self.host_path_ptr = np.zeros(1, dtype=np.int64)         # the mirror: the prefix arrays [: len + 1], problem [: len]
        self.host_free_ptr = np.zeros(1, dtype=np.int64)
        self.host_coll_ptr = np.zeros(1, dtype=np.int64)
        self.host_problem = np.zeros(0, dtype=np.int64)

    def __len__(self):
        return int(self.host_problem.shape[0])

    def rows_in_use(self):
        """(samples, path rows, free rows, collided rows) by the host mirror."""
        return len(self), int(self.host_path_ptr[-1]), int(self.host_free_ptr[-1]), int(self.host_coll_ptr[-1])

    def _struct(self):
        from . import _lib
        return _lib.SmoothReplay(self.C, self.cap_samples, self.cap_path_rows, self.cap_free_rows, self.cap_coll_rows, self.epoch,
                                 self.path.data_ptr(), self.target.data_ptr(), self.free.data_ptr(), self.collided.data_ptr(),
                                 self.path_ptr.data_ptr(), self.free_ptr.data_ptr(), self.coll_ptr.data_ptr(),
                                 self.problem.data_ptr(), self.counts.data_ptr(), self.status.data_ptr(), self._pending.data_ptr())

    def _raise_status(self, status, what):
        use = self.rows_in_use()
        why = [text for bit, text in (
            (STATUS_FULL, 'the samples or rows do not fit in the store (%d of %d samples, %d of %d path rows, %d of %d free rows, '
                          '%d of %d collided rows in use); nothing was appended'
             % (use[0], self.cap_samples, use[1], self.cap_path_rows, use[2], self.cap_free_rows, use[3], self.cap_coll_rows)),
            (STATUS_BAD_SOURCE, 'a malformed source (a taken sample with fewer than three path rows, rows outside the source '
                                'arrays, n_free beyond a sample\'s rows, or more taken samples than take_upper); nothing was '
                                'appended'),
            (STATUS_BAD_GATHER, 'a gather with an index outside the store or sizes other than the mirror\'s; that batch was '
                                'not written')) if status & bit]
        self.status.zero_()
        raise RuntimeError('%s: status %d: %s' % (what, status, '; '.join(why)))

    def _refresh(self, upper, what):
        """The one read-back of an append call: both count banks, status, the call's record, and the slots it can have
        filled."""
        n0 = len(self)
        hi = min(n0 + int(upper), self.cap_samples)
        m = hi + 1 - n0
        back = torch.cat([self._words, self.path_ptr[n0:hi + 1], self.free_ptr[n0:hi + 1], self.coll_ptr[n0:hi + 1],
                          self.problem[n0:hi]]).cpu().numpy().astype(np.int64)
        counts = back[4 * (self.epoch & 1):4 * (self.epoch & 1) + 4]              # the bank the call wrote
        status, before, added = int(back[8]), back[9:13], back[13:17]
        if status & (STATUS_FULL | STATUS_BAD_SOURCE):
            self._raise_status(status, what)
        use = np.array(self.rows_in_use(), dtype=np.int64)
        if (before != use).any() or (counts != use + added).any():
            raise RuntimeError('%s: the store on the device %s and its host mirror %s disagree' % (what, before.tolist(), use.tolist()))
        n_new = int(added[0])
        if n_new:
            o = 17
            self.host_path_ptr = np.concatenate([self.host_path_ptr, back[o + 1:o + 1 + n_new]])
            self.host_free_ptr = np.concatenate([self.host_free_ptr, back[o + m + 1:o + m + 1 + n_new]])
            self.host_coll_ptr = np.concatenate([self.host_coll_ptr, back[o + 2 * m + 1:o + 2 * m + 1 + n_new]])
            self.host_problem = np.concatenate([self.host_problem, back[o + 3 * m:o + 3 * m + n_new]])
        if status:                                               # an earlier gather's bit: the append itself went through
            self._raise_status(status, what)
        return n_new

    def check_status(self):
        """Read the status word (a synchronising read; an append makes it anyway) and raise if a bit is set."""
        status = int(self.status.cpu())
        if status:
            self._raise_status(status, 'SmoothReplayStore')

    def append(self, path, target, path_ptr, v, node_ptr, n_free, take, problem_ids, take_upper=None):
        """Append the taken ones of B candidate samples, in ascending position.  Device tensors: ``path`` / ``target`` [sumP, C]
        float32 with ``path_ptr`` [B + 1]; ``v`` [sumN, C] float32, every sample's free rows first and then its collided rows,
        with ``node_ptr`` [B + 1] and ``n_free`` [B]; ``take`` [B] (non-zero: store it); ``problem_ids`` [B] (what ``problem``
        receives).  ``take_upper``: an upper bound of the number of set flags when the caller knows one without asking the
        device (default B; 0: nothing is launched).  Returns the number of samples appended."""
        from . import _lib
        dev = self.device
        f32 = lambda t: torch.as_tensor(t).to(device=dev, dtype=torch.float32).reshape(-1, self.C).contiguous()      # noqa: E731
        i32 = lambda t: torch.as_tensor(t).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()                # noqa: E731
        path, target, v = f32(path), f32(target), f32(v)
        path_ptr, node_ptr, n_free, take, ids = i32(path_ptr), i32(node_ptr), i32(n_free), i32(take), i32(problem_ids)
        B = int(take.shape[0])
        if path.shape != target.shape:
            raise ValueError('SmoothReplayStore.append: one target row per path row')
        if int(path_ptr.shape[0]) != B + 1 or int(node_ptr.shape[0]) != B + 1 or int(n_free.shape[0]) != B or int(ids.shape[0]) != B:
            raise ValueError('SmoothReplayStore.append: path_ptr and node_ptr [B + 1], n_free, take and problem_ids [B]')
        upper = B if take_upper is None else int(take_upper)
        if upper < 0 or upper > B:
            raise ValueError('SmoothReplayStore.append: take_upper is 0 .. B')
        if B == 0 or upper == 0:
            return 0
        src = _lib.SmoothReplaySrc(B, int(path.shape[0]), int(v.shape[0]), upper, path.data_ptr(), target.data_ptr(), v.data_ptr(),
                                   path_ptr.data_ptr(), node_ptr.data_ptr(), n_free.data_ptr(), take.data_ptr(), ids.data_ptr())
        store = self._struct()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().gnnmp_smooth_replay_append(ctypes.byref(store), ctypes.byref(src), _stream(dev)),
                       'gnnmp_smooth_replay_append')
            self.epoch += 1                                      # the launch wrote the other bank, whatever it decided
            return self._refresh(upper, 'gnnmp_smooth_replay_append')

    def batch(self, idx, loops):
        """The group of replay indices ``idx`` (repeats allowed) with one loop count each -> ``(SmoothBatch, targets, order)``:
        the group in the order ``order`` (positions of ``idx``, longest loop first, ties in the caller's order), which is the
        order ``ModelSmoother.forward_train_batch`` runs in, so it does no reordering of its own; call it with
        ``[loops[b] for b in order]``.  ``targets`` [sum P, C] is aligned with the batch's path rows.  One launch
        (``gnnmp_smooth_replay_gather``) after one small upload (the indices); sizes come from the host mirror and nothing is
        read back."""
        from . import _lib
        from .smoother import SmoothBatch
        dev = self.device
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        loops = [int(x) for x in loops]
        G = int(idx.size)
        if len(loops) != G:
            raise ValueError('SmoothReplayStore.batch: one loop count per index')
        if G == 0:
            raise ValueError('SmoothReplayStore.batch: an empty group')
        if idx.min() < 0 or idx.max() >= len(self):
            raise IndexError('SmoothReplayStore.batch: replay index outside [0, %d)' % len(self))
        order = sorted(range(G), key=lambda b: -loops[b])
        ids = idx[order]
        pc = (self.host_path_ptr[ids + 1] - self.host_path_ptr[ids]).tolist()
        fc = (self.host_free_ptr[ids + 1] - self.host_free_ptr[ids]).tolist()
        cc = (self.host_coll_ptr[ids + 1] - self.host_coll_ptr[ids]).tolist()
        ec = [3 * p - 2 for p in pc]
        tp, tf, tc, te = sum(pc), sum(fc), sum(cc), sum(ec)
        sb = SmoothBatch.__new__(SmoothBatch)
        sb.n = G
        with torch.cuda.device(dev):
            idx_d = torch.from_numpy(ids.astype(np.int32)).to(dev)
            sb.path = torch.empty(tp, self.C, dtype=torch.float32, device=dev)
            targets = torch.empty(tp, self.C, dtype=torch.float32, device=dev)
            sb.free = torch.empty(tf, self.C, dtype=torch.float32, device=dev)
            sb.collided = torch.empty(tc, self.C, dtype=torch.float32, device=dev)
            sb.edge_index = torch.empty(2, te, dtype=torch.int64, device=dev)
            ptrs = torch.zeros(4, G + 1, dtype=torch.int32, device=dev)     # a gather that refuses (status bit 4) leaves empty problems
            sb.path_ptr, sb.free_ptr, sb.coll_ptr, sb.edge_ptr = ptrs[0], ptrs[1], ptrs[2], ptrs[3]
            sb.max_path, sb.max_samples, sb.max_edges = max(pc), max(f + c for f, c in zip(fc, cc)), max(ec)
            sb.path_counts, sb.free_counts, sb.coll_counts, sb.edge_counts = pc, fc, cc, ec
            sb.caps_from_host = True
            out = _lib.SmoothBatch(G, tp, tf, tc, te, sb.max_path, sb.max_samples, sb.max_edges, sb.path.data_ptr(), sb.free.data_ptr(),
                                   sb.collided.data_ptr(), sb.edge_index.data_ptr(), sb.path_ptr.data_ptr(), sb.free_ptr.data_ptr(),
                                   sb.coll_ptr.data_ptr(), sb.edge_ptr.data_ptr())
            store = self._struct()
            _lib.check(_lib.lib().gnnmp_smooth_replay_gather(ctypes.byref(store), G, len(self), idx_d.data_ptr(), ctypes.byref(out),
                                                             targets.data_ptr(), _stream(dev)), 'gnnmp_smooth_replay_gather')
            idx_d.record_stream(torch.cuda.current_stream(dev))
        return sb, targets, order


# --------------------------------------------------------------------------------------------------
# the loss of train()
# --------------------------------------------------------------------------------------------------
def path_loss_reference(pred, target, ptr, divisor):
    """``gnnmp_smooth_path_loss`` restated on the host in float64 numpy: ``(terms [G], loss, d_pred [S, C])`` with ``terms[g]``
    the mean of ``(pred - target)^2`` over the interior rows ``1 .. P - 2`` of path ``g`` (one ascending chain in (row, column)
    order), ``loss = (terms[0] + terms[1] + ...) / divisor`` and ``d_pred`` its gradient with respect to ``pred``; a path with
    ``P <= 2`` has the term 0 and zero rows."""
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    ptr = np.asarray(ptr, dtype=np.int64).reshape(-1)
    C = pred.shape[1]
    terms, d_pred, total = np.zeros(ptr.size - 1), np.zeros_like(pred), 0.
    for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        P = int(b - a)
        if P > 2:
            d = (pred[a + 1:b - 1] - target[a + 1:b - 1]).reshape(-1)
            s = 0.
            for x in (d * d).tolist():
                s = s + x
            terms[g] = s / ((P - 2) * C)
            d_pred[a + 1:b - 1] = (2. * d / (float(P - 2) * float(C) * float(divisor))).reshape(-1, C)
        total = total + terms[g]
    return terms, total / divisor, d_pred


def path_loss_device(pred, target, ptr, divisor):
    """``gnnmp_smooth_path_loss`` on device tensors: ``pred`` / ``target`` [S, C] float32, ``ptr`` [G + 1] int32 ->
    ``(terms [G] float64, loss [1] float32, d_pred [S, C] float32)``.  One launch on the current stream; nothing is read
    back."""
    from . import _lib
    dev = pred.device
    if dev.type != 'cuda':
        raise RuntimeError('path_loss: device tensors only (the kernels are the only implementation)')
    S, C, G = int(pred.shape[0]), int(pred.shape[1]), int(ptr.shape[0]) - 1
    pred, target, ptr = pred.contiguous(), target.contiguous(), ptr.contiguous()
    for name, t, dt, shape in (('pred', pred, torch.float32, (S, C)), ('target', target, torch.float32, (S, C)),
                               ('ptr', ptr, torch.int32, (G + 1,))):
        if t.dtype != dt or t.device != dev or tuple(t.shape) != shape:
            raise ValueError('path_loss: %s must be %s %s on %s' % (name, dt, shape, dev))
    if int(divisor) < 1:
        raise ValueError('path_loss: divisor is at least 1')
    terms = torch.zeros(max(G, 0), dtype=torch.float64, device=dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    d_pred = torch.zeros_like(pred)                              # rows outside every path stay zero
    if G > 0:
        desc = _lib.SmoothPathLoss(G, S, C, int(divisor), ptr.data_ptr(), pred.data_ptr(), target.data_ptr(), terms.data_ptr(),
                                   loss.data_ptr(), d_pred.data_ptr())
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().gnnmp_smooth_path_loss(ctypes.byref(desc), _stream(dev)), 'gnnmp_smooth_path_loss')
    return terms, loss, d_pred


class _PathLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, ptr, divisor):
        terms, loss, d_pred = path_loss_device(pred.detach(), target, ptr, divisor)
        ctx.save_for_backward(d_pred)
        ctx.mark_non_differentiable(terms)
        return loss.reshape(()), terms

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        d_pred, = ctx.saved_tensors
        return d_pred * grad_loss.to(torch.float32), None, None, None


def path_loss(pred, target, ptr, divisor, return_terms=False):
    """``(sum over the paths of MSELoss(target[1:-1], pred[1:-1])) / divisor`` (train_smoother.py:55-58) from ``pred`` [S, C] as
    a float32 device scalar with a gradient history to ``pred``; path ``g`` is rows ``ptr[g] : ptr[g + 1]``.  The backward
    scales the kernel's ``d_pred`` by the incoming scalar on the device.  With ``return_terms`` also the per-path terms [G]
    (float64, no history)."""
    loss, terms = _PathLossFn.apply(pred, target, ptr, int(divisor))
    return (loss, terms) if return_terms else loss


# --------------------------------------------------------------------------------------------------
# train()
# --------------------------------------------------------------------------------------------------
def replay_schedule(n, passes=20, group=8, rng=None):
    """The optimizer steps of the training passes over a replay of ``n`` samples, in the draw order of
    ``train_smoother.py:106-118, 41, 53``: per pass one ``rng.permutation(n)``, the groups ``perm[i : i + group]`` for ``i = 0,
    group, ...`` (the last one may be shorter; its divisor is its own length) and, per sample in group order, one
    ``rng.randint(1, 10)``.  Returns one list per pass of ``(indices, loops)`` pairs (int64 arrays).  With ``n <= group`` the
    reference's ``train()`` returns 0 without drawing or stepping: the permutations are drawn and every pass is empty."""
    rng = np.random.RandomState(1234) if rng is None else rng
    n, group = int(n), int(group)
    out = []
    for _ in range(int(passes)):
        perm = rng.permutation(n)
        steps = []
        if n > group:
            for i in range(0, n, group):
                idx = np.asarray(perm[i:i + group], dtype=np.int64)
                steps.append((idx, np.array([rng.randint(1, 10) for _ in idx], dtype=np.int64)))
        out.append(steps)
    return out


def train_replay(model_s, optimizer, store, passes=20, group=8, rng=None, scheduler=None, log=None):
    """The training passes of ``train_env`` (train_smoother.py:198-220) over ``store``: the steps of :func:`replay_schedule`,
    each ``store.batch`` -> ``model_s.forward_train_batch`` -> :func:`path_loss` with the group's own length as divisor ->
    backward -> ``optimizer.step()``.  The losses stay on the device and are stacked and read once per pass.

    Returns ``(history, best_state)``.  ``history[p]`` = ``{'losses': the differentiated loss of every step, 'sums': what
    train() returns for it (the undivided sum of the group's terms, :61), 'mean': the mean of the sums (what the reference
    hands to the scheduler and compares with loss_min; 0.0 for a pass without steps, :34-35), 'lr': the rate the pass ran at}``;
    ``scheduler.step(mean)`` follows every pass.  ``best_state`` is a copy of ``model_s.state_dict()`` after the first pass
    with the lowest mean: the checkpoint the reference keeps (:218-220).  ``log(pass, history[pass])`` is called per pass."""
    if len(store) == 0:
        raise ValueError('train_replay: an empty replay')
    schedule = replay_schedule(len(store), passes, group, rng)
    model_s.train()
    history, best_state, loss_min = [], None, float('inf')
    for p, steps in enumerate(schedule):
        lr = float(optimizer.param_groups[0]['lr'])
        losses = []
        for idx, loops in steps:
            sb, targets, order = store.batch(idx, loops)
            pred = model_s.forward_train_batch(sb, [int(loops[b]) for b in order])
            loss = path_loss(pred, targets, sb.path_ptr, len(idx))
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            losses.append(loss.detach())
        if losses:
            host = torch.stack(losses).cpu().numpy().astype(np.float64)
            sums = host * np.array([len(idx) for idx, _ in steps], dtype=np.float64)
            mean = float(np.mean(sums))
        else:
            host, sums, mean = np.zeros(0), np.zeros(0), 0.0
        entry = {'losses': host.tolist(), 'sums': sums.tolist(), 'mean': mean, 'lr': lr}
        history.append(entry)
        if scheduler is not None:
            scheduler.step(mean)
        if mean < loss_min:
            loss_min = mean
            best_state = {k: v.detach().clone() for k, v in model_s.state_dict().items()}
        if log is not None:
            log(p, entry)
    store.check_status()
    return history, best_state


# --------------------------------------------------------------------------------------------------
# train_env
# --------------------------------------------------------------------------------------------------
def random_init_goal(problem, rng):
    """``MazeEnv.set_random_init_goal`` (maze_env.py:102-117) for one problem dict over the project's ``Maze2D`` / ``Maze3D``,
    in float64: two free states drawn one ``uniform_sample`` at a time from ``rng`` (a ``RandomState``), again while they
    coincide.  Returns the problem with the new ``init_state`` / ``goal_state`` (the map is shared)."""
    from .streams_batch import problem_env
    env = problem_env(problem, 'smoother_replay.random_init_goal')
    limits = np.asarray(env.SAMPLE_LIMITS, dtype=np.float64)

    def empty_point():
        while True:
            point = rng.uniform(-limits, limits, (1, limits.shape[0])).reshape(-1)
            if env._state_fp(point):
                return point
    while True:
        init, goal = empty_point(), empty_point()
        if np.sum(np.abs(init - goal)) != 0:
            break
    return {'map': problem['map'], 'init_state': init, 'goal_state': goal}


def collect_replay(model_explore, problems, problem_ids, seeds, store, device, batch=500, k=30, loop=5, generator=None, draws='host',
                   timings=None):
    """``train_smoother.py:91-99`` for a chunk of maze problems: :func:`gnnmp.planner.plan_maze_rounds_batch` with ``t_max =
    batch`` and no smoother -- ONE round, because the reference's ``explore(smooth=False)`` returns ``[]`` after a failed first
    round and the problem is skipped --, :func:`gnnmp.oracle_smooth.smoothing_targets` on the solved paths (draws from
    ``generator``, a torch generator on the device), and one append with ``take = solved & (P > 2) & (target status == 0)``.
    ``problem_ids[i]`` is what the store records for ``problems[i]``.

    Returns ``{'solved': n, 'taken': n, 'short': n, 'failed': n}``: problems with a path, samples stored, solved problems the
    reference makes no sample of (``len(path) <= 2``), problems without a path.  ``timings`` receives the wall clock of the
    stages plan, targets, append."""
    from .oracle_smooth import smoothing_targets
    from .planner import plan_maze_rounds_batch
    from .streams_batch import StageClock
    B = len(problems)
    stats = {'solved': 0, 'taken': 0, 'short': 0, 'failed': 0}
    if B == 0:
        return stats
    if len(problem_ids) != B:
        raise ValueError('smoother_replay.collect_replay: one problem id per problem')
    dev = torch.device(device)
    clock = StageClock(timings)
    with torch.cuda.device(dev):
        res = plan_maze_rounds_batch(problems, model_explore, dev, seeds, batch=int(batch), t_max=int(batch), k=k, loop=loop,
                                     model_s=None, draws=draws)
        clock.mark('plan')
        sel = [b for b in range(B) if res[b]['success']]
        stats['solved'], stats['failed'] = len(sel), B - len(sel)
        if not sel:
            return stats
        src = solved_source(res, sel, problems, problem_ids, dev)
        stats['short'] = int((src['lengths'] <= 2).sum())
        target, status = smoothing_targets(src['path'], src['path_ptr'], src['maps'], generator=generator)
        clock.mark('targets')
        take = ((src['path_ptr'][1:] - src['path_ptr'][:-1] > 2) & (status == 0)).to(torch.int32)
        stats['taken'] = store.append(src['path'], target, src['path_ptr'], src['v'], src['node_ptr'], src['n_free'], take,
                                      src['problem_ids'], take_upper=len(sel) - stats['short'])
        clock.mark('append')
    return stats


def solved_source(res, sel, problems, problem_ids, device):
    """The solved problems ``sel`` of a :func:`gnnmp.planner.plan_maze_rounds_batch` result as the device tensors an append
    takes: ``path`` [sumP, dim] float32 (the waypoints' sample rows), ``path_ptr``, ``v`` (free rows, then collided rows, per
    problem), ``node_ptr``, ``n_free``, ``problem_ids``, plus ``maps`` [len(sel), w, w] for the targets and ``lengths`` (host)."""
    dev = torch.device(device)
    lengths = np.array([res[b]['path'].shape[0] for b in sel], dtype=np.int64)
    nodes = np.array([res[b]['v'].shape[0] for b in sel], dtype=np.int64)
    dim = int(res[sel[0]]['v'].shape[1])
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)       # noqa: E731
    return {
        'path': torch.from_numpy(np.concatenate([np.asarray(res[b]['path'], dtype=np.float32).reshape(-1, dim) for b in sel])).to(dev),
        'path_ptr': i32(np.concatenate([[0], np.cumsum(lengths)])),
        'v': torch.cat([res[b]['v'].to(torch.float32).reshape(-1, dim) for b in sel]).to(dev),
        'node_ptr': i32(np.concatenate([[0], np.cumsum(nodes)])),
        'n_free': i32([res[b]['n_free'] for b in sel]),
        'problem_ids': i32([problem_ids[b] for b in sel]),
        'maps': torch.from_numpy(np.ascontiguousarray([np.asarray(problems[b]['map']) != 0 for b in sel]).astype(np.uint8)).to(dev),
        'lengths': lengths,
    }


def pass_seeds(seed, ids, data_pass):
    """The sample-stream seeds of the problems ``ids`` in collection pass ``data_pass``: ``streams_batch.stream_seeds`` mixed
    with the pass number, so a problem draws other samples every time it comes up."""
    from .streams_batch import stream_seeds
    return [(s ^ (int(data_pass) * PASS_SEED_MIX)) & 0xffffffff for s in stream_seeds(seed, ids)]


def train_smoother_maze(model_s, model_explore, problems, device, data_iter=3, passes=20, lr=1e-3, momentum=0.9, weight_decay=1e-4,
                        chunk=256, batch=500, seed=1234, k=30, loop=5, group=8, draws='host', log=None):
    """``train_env`` of ``train_smoother.py:136-222`` for maze problems (dicts with ``map``, ``init_state``, ``goal_state``):
    ``data_iter`` collection passes over all problems through :func:`collect_replay`, ``chunk`` problems at a time, the passes
    after the first with :func:`random_init_goal`; then :func:`train_replay` with ``SGD(lr, momentum, weight_decay)`` and
    ``ReduceLROnPlateau('min', patience=0)``.  ``model_s`` is a :class:`gnnmp.smoother.ModelSmoother` on ``device`` (trained
    in place), ``model_explore`` the loaded explorer.  See the module docstring for the deviations from the reference.

    Returns ``(history, best_state)``: ``history = {'collect': the dict of every collection pass, 'replay': samples stored,
    'train': the per-pass list of`` :func:`train_replay` ``}`` and the state dict of the best pass, which
    ``ModelSmoother.load_state_dict`` takes.  A replay of no more than ``group`` samples trains nothing (:34-35): every mean is 0
    and the state returned is the untrained one, which is what the reference would save."""
    dev = torch.device(device)
    n = len(problems)
    if n == 0:
        raise ValueError('train_smoother_maze: no problems')
    rng = np.random.RandomState(int(seed))
    dim = int(np.asarray(problems[0]['init_state']).reshape(-1).shape[0])
    side = min(MAX_SIDE, int(batch) + 2)
    cap = int(data_iter) * n
    store = SmoothReplayStore(dim, cap, cap * (int(batch) + 2), cap * side, cap * side, dev)
    generator = torch.Generator(device=dev)
    generator.manual_seed(int(seed))
    collect = []
    for it in range(int(data_iter)):
        stats = {'solved': 0, 'taken': 0, 'short': 0, 'failed': 0}
        for c0 in range(0, n, int(chunk)):
            ids = list(range(c0, min(c0 + int(chunk), n)))
            probs = [problems[i] if it == 0 else random_init_goal(problems[i], rng) for i in ids]
            got = collect_replay(model_explore, probs, ids, pass_seeds(seed, ids, it), store, dev, batch=batch, k=k, loop=loop,
                                 generator=generator, draws=draws)
            for key, val in got.items():
                stats[key] += val
        collect.append(stats)
    if len(store) == 0:
        raise RuntimeError('train_smoother_maze: no problem gave a training sample')
    optimizer = torch.optim.SGD(model_s.parameters(), lr=lr, momentum=momentum, weight_decay=weight_decay)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, 'min', patience=0)
    optimizer.zero_grad()
    train, best_state = train_replay(model_s, optimizer, store, passes=passes, group=group, rng=rng, scheduler=scheduler, log=log)
    return {'collect': collect, 'replay': len(store), 'train': train}, best_state
