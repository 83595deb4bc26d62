"""NEXT's training loop on maze problems with the replay on the device: what the reference's ``train_env`` does around one
optimizer step (``train_next.py:71-115``), for ``maze2`` / ``maze3`` (``Model2D`` / ``PPN``, dim 2 and 3).

  * :class:`ReplayStore`      the ``(problem, path)`` samples with ``get_label``'s actions and values as device arrays, filled
    from the trees of ``gnnmp_next_plan`` (``append_trees``) or from packed paths (``append_paths``) by
    ``csrc/next_replay_kernels.hip``; the trees, paths and labels never come back to the host.  The host keeps a mirror of
    ``path_ptr`` and ``problem`` only, refreshed by one small read-back per append call.
  * :func:`path_loss`         the loss ``train()`` differentiates as a ``torch.autograd.Function`` over ``gnnmp_next_path_loss``.
  * :func:`train_replay`      ``train()`` of ``train_next.py:42-68``: ``L`` passes over a fresh permutation, a step after every
    8th sample with the loss ``sum / 8``, and the reference's carry-over (below).  :func:`train_replay_host` is the same
    schedule over host arrays and any differentiable forward: the oracle of the tests.
  * :func:`collect_replay`    the body of ``train_next.py:88-108`` for a chunk of problems that share one network.
  * :func:`train_env_maze`    ``train_env``.

The carry-over.  ``train()`` sets ``loss = 0`` once, before the passes, and again after every step -- not at the end of a
pass.  The ``len(replay) % 8`` trailing samples of pass ``p`` therefore stay in the running loss and join the first step of
pass ``p + 1``, which then sums ``8 + r`` terms and is still divided by 8; the trailing samples of the last pass are dropped.
:func:`replay_schedule` reproduces exactly that.

Two deviations from the reference, both in :func:`collect_replay`: the fallback planner's budget is a sample count
(``fallback_t_max``), not ``T = INF`` under a 60 s wall clock, and the fallback draws from its own stream
(``seeds[i] ^ 0x9E3779B9``) instead of continuing NEXT's numpy stream.  ``train()``'s permutations come from the ``rng`` handed
in (default ``RandomState(1234)``), the project's stream; the reference draws them from the global generator.

The kernels are the only implementation: nothing here falls back to the host.
"""
import ctypes

import numpy as np
import torch

from .next_model import DEFAULT_ITERS
from .next_train import loss_from_outputs, path_labels

FALLBACK_SEED_XOR = 0x9E3779B9
STATUS_FULL, STATUS_BAD_SOURCE, STATUS_BAD_NODE = 1, 2, 4


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# --------------------------------------------------------------------------------------------------
# the store
# --------------------------------------------------------------------------------------------------
class ReplayStore:
    """The replay as device arrays (``gnnmp_next_replay`` of ``include/gnnmp.h``): ``states64`` / ``states32`` / ``actions``
    [cap_states, dim], ``values`` [cap_states], ``path_ptr`` [cap_paths + 1], ``problem`` [cap_paths], ``counts`` [2], ``status``
    [1].  Path ``i`` is rows ``path_ptr[i] : path_ptr[i + 1]`` and belongs to problem ``problem[i]``.  An append is all or
    nothing: one that does not fit, or whose source is malformed, leaves the store as it was and raises."""

    def __init__(self, dim, cap_paths, cap_states, device='cuda'):
        dim, cap_paths, cap_states = int(dim), int(cap_paths), int(cap_states)
        if dim not in (2, 3):
            raise ValueError('ReplayStore: dim is 2 (point robot) or 3 (stick robot)')
        if cap_paths < 0 or cap_states < 0 or cap_paths >= 2 ** 31 - 1 or cap_states >= 2 ** 31 - 1:
            raise ValueError('ReplayStore: capacities are 0 .. 2^31 - 2')
        self.dim, self.cap_paths, self.cap_states = dim, cap_paths, cap_states
        self.device = dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError('ReplayStore: a device store (the kernels are the only implementation)')
        new = lambda dtype, *shape: torch.zeros(*shape, dtype=dtype, device=dev)      # noqa: E731
        self.states64 = new(torch.float64, max(cap_states, 1), dim)
        self.states32 = new(torch.float32, max(cap_states, 1), dim)
        self.actions = new(torch.float32, max(cap_states, 1), dim)
        self.values = new(torch.float32, max(cap_states, 1))
        self.path_ptr = new(torch.int32, cap_paths + 1)
        self.problem = new(torch.int32, max(cap_paths, 1))
        self._words = new(torch.int32, 8)                        # counts [2], status [1], pending [4]
        self.counts, self.status, self._pending = self._words[0:2], self._words[2:3], self._words[3:7]
        self.host_ptr = np.zeros(1, dtype=np.int64)              # the mirror: path_ptr[: len + 1] and problem[: len]
        self.host_problem = np.zeros(0, dtype=np.int64)

    def __len__(self):
        return int(self.host_problem.shape[0])

    @property
    def n_states(self):
        return int(self.host_ptr[-1])

    def _struct(self):
        from . import _lib
        return _lib.NextReplay(self.dim, self.cap_paths, self.cap_states, self.states64.data_ptr(), self.states32.data_ptr(),
                               self.actions.data_ptr(), self.values.data_ptr(), self.path_ptr.data_ptr(), self.problem.data_ptr(),
                               self.counts.data_ptr(), self.status.data_ptr(), self._pending.data_ptr())

    def _refresh(self, n_sources, what):
        """The one read-back of an append call: counts, status, the call's record, and the slots it can have filled."""
        p0 = len(self)
        hi = min(p0 + int(n_sources), self.cap_paths)
        back = torch.cat([self._words, self.path_ptr[p0:hi + 1], self.problem[p0:hi]]).cpu().numpy().astype(np.int64)
        status, (q0, s0, n_new, s_new) = int(back[2]), back[3:7]
        why = [text for bit, text in ((STATUS_FULL, 'the paths or states do not fit in the store (%d of %d paths, %d of %d states '
                                                    'in use); nothing was appended' % (p0, self.cap_paths, self.n_states, self.cap_states)),
                                      (STATUS_BAD_SOURCE, 'a malformed source (a path length outside the tree, path_ptr not from 0 to '
                                                          'the number of states, or a path without a state); nothing was appended'),
                                      (STATUS_BAD_NODE, 'a node id outside the tree; its row was stored as zeros')) if status & bit]
        if status:
            self.status.zero_()
        if status & (STATUS_FULL | STATUS_BAD_SOURCE):
            raise RuntimeError('%s: status %d: %s' % (what, status, '; '.join(why)))
        if int(q0) != p0 or int(s0) != self.n_states or int(back[0]) != p0 + n_new or int(back[1]) != self.n_states + s_new:
            raise RuntimeError('%s: the store on the device (%d paths, %d states) and its host mirror (%d, %d) disagree'
                               % (what, int(back[0]) - int(n_new), int(back[1]) - int(s_new), p0, self.n_states))
        n_new = int(n_new)
        ptr = back[8:8 + (hi + 1 - p0)]
        prob = back[8 + (hi + 1 - p0):]
        if n_new:
            self.host_ptr = np.concatenate([self.host_ptr, ptr[1:n_new + 1]])
            self.host_problem = np.concatenate([self.host_problem, prob[:n_new]])
        if status:
            raise RuntimeError('%s: status %d: %s' % (what, status, '; '.join(why)))
        return n_new

    def append_trees(self, plan_out, problem_ids):
        """Append the path of every successful problem of one :func:`gnnmp.next_plan.next_plan_device` batch (its dict), in
        ascending batch position; ``problem_ids`` [B] (device tensor or host array) is what ``problem`` receives.  Returns the
        number of paths appended."""
        from . import _lib
        dev = self.device
        states, path, small = plan_out['states'], plan_out['path'], plan_out['small']
        B, T1 = int(states.shape[0]), int(states.shape[1])
        if int(states.shape[2]) != self.dim or states.dtype != torch.float64 or tuple(path.shape) != (B, T1) or states.device != dev:
            raise ValueError('ReplayStore.append_trees: the tree of a dim %d plan on %s' % (self.dim, dev))
        ids = torch.as_tensor(problem_ids).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if int(ids.shape[0]) != B:
            raise ValueError('ReplayStore.append_trees: one problem id per problem')
        if B == 0:
            return 0
        states, path = states.contiguous(), path.contiguous()
        success, path_len = small[1].contiguous(), small[4].contiguous()
        trees = _lib.NextReplayTrees(B, T1 - 1, states.data_ptr(), path.data_ptr(), path_len.data_ptr(), success.data_ptr(), ids.data_ptr())
        store = self._struct()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().gnnmp_next_replay_append_trees(ctypes.byref(store), ctypes.byref(trees), _stream(dev)),
                       'gnnmp_next_replay_append_trees')
            return self._refresh(B, 'gnnmp_next_replay_append_trees')

    def append_paths(self, paths, path_ptr, problem_ids):
        """Append packed paths: ``paths`` [N, dim] float64 holds them one after another, path ``i`` is rows
        ``path_ptr[i] : path_ptr[i + 1]`` (as :func:`gnnmp.next_train.path_labels` takes them), ``problem_ids`` [P].  Host
        arrays are copied to the device once.  Returns the number of paths appended."""
        from . import _lib
        dev = self.device
        paths = torch.as_tensor(paths).to(device=dev, dtype=torch.float64).reshape(-1, self.dim).contiguous()
        ptr = torch.as_tensor(path_ptr).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        ids = torch.as_tensor(problem_ids).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        P = int(ids.shape[0])
        if int(ptr.shape[0]) != P + 1:
            raise ValueError('ReplayStore.append_paths: path_ptr has one entry more than there are paths')
        if P == 0:
            return 0
        desc = _lib.NextReplayPaths(P, int(paths.shape[0]), paths.data_ptr(), ptr.data_ptr(), ids.data_ptr())
        store = self._struct()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().gnnmp_next_replay_append_paths(ctypes.byref(store), ctypes.byref(desc), _stream(dev)),
                       'gnnmp_next_replay_append_paths')
            return self._refresh(P, 'gnnmp_next_replay_append_paths')

    def batch(self, idx):
        """The group of replay indices ``idx`` (any order, repeats) as device tensors: ``states32`` [S, dim],
        ``problem_of_state`` [S] (the position within the group), ``actions`` [S, dim], ``values`` [S], ``ptr`` [G + 1], and
        ``problems`` (host, [G]): the problem of every path.  The rows are gathered on the device from an index built out of the
        host mirror: one small upload, nothing is read back."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError('ReplayStore.batch: replay index outside [0, %d)' % len(self))
        a, b = self.host_ptr[idx], self.host_ptr[idx + 1]
        lens = b - a
        ptr = np.concatenate([[0], np.cumsum(lens)])
        S = int(ptr[-1])
        of = np.repeat(np.arange(idx.size, dtype=np.int64), lens)
        rows = np.arange(S, dtype=np.int64) - ptr[:-1][of] + a[of]
        up = torch.from_numpy(np.concatenate([rows, of, ptr])).to(self.device)
        rows_d = up[:S]
        return {'states32': self.states32.index_select(0, rows_d), 'problem_of_state': up[S:2 * S].to(torch.int32),
                'actions': self.actions.index_select(0, rows_d), 'values': self.values.index_select(0, rows_d),
                'ptr': up[2 * S:].to(torch.int32), 'problems': self.host_problem[idx]}


# --------------------------------------------------------------------------------------------------
# the loss of train()
# --------------------------------------------------------------------------------------------------
def path_loss_reference(y, actions, values, ptr, divisor):
    """``gnnmp_next_path_loss`` restated on the host in float64 numpy: ``(terms [G, 2], loss, dy [S, dim + 1])`` with
    ``terms[g] = (mean_s (values - y[:, dim])^2, mean_{s, j} (actions - y[:, :dim])^2)``, ``loss = (sum of all terms) /
    divisor`` and ``dy`` its gradient with respect to ``y``."""
    y = np.asarray(y, dtype=np.float64)
    actions, values = np.asarray(actions, dtype=np.float64), np.asarray(values, dtype=np.float64)
    ptr = np.asarray(ptr, dtype=np.int64).reshape(-1)
    dim = y.shape[1] - 1
    terms, dy, total = np.zeros((ptr.size - 1, 2)), np.zeros_like(y), 0.
    for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        n = b - a
        dv, da = values[a:b] - y[a:b, dim], actions[a:b] - y[a:b, :dim]
        terms[g] = (dv ** 2).sum() / n, (da ** 2).sum() / (n * dim)
        total = (total + terms[g, 0]) + terms[g, 1]
        dy[a:b, dim] = -2. * dv / (n * divisor)
        dy[a:b, :dim] = -2. * da / (n * dim * divisor)
    return terms, total / divisor, dy


def path_loss_device(y, actions, values, ptr, divisor):
    """``gnnmp_next_path_loss`` on device tensors: ``y`` [S, dim + 1], ``actions`` [S, dim], ``values`` [S] float32, ``ptr``
    [G + 1] int32 -> ``(terms [G, 2] float64, loss [1] float64, dy [S, dim + 1] float32)``.  Two launches on the current
    stream; nothing is read back."""
    from . import _lib
    dev = y.device
    if dev.type != 'cuda':
        raise RuntimeError('path_loss: device tensors only (the kernels are the only implementation)')
    S, dim, G = int(y.shape[0]), int(y.shape[1]) - 1, int(ptr.shape[0]) - 1
    y, actions, values, ptr = y.contiguous(), actions.contiguous(), values.contiguous(), ptr.contiguous()
    for name, t, dt, shape in (('y', y, torch.float32, (S, dim + 1)), ('actions', actions, torch.float32, (S, dim)),
                               ('values', values, torch.float32, (S,)), ('ptr', ptr, torch.int32, (G + 1,))):
        if t.dtype != dt or t.device != dev or tuple(t.shape) != shape:
            raise ValueError('path_loss: %s must be %s %s on %s' % (name, dt, shape, dev))
    terms = torch.zeros(max(G, 0), 2, dtype=torch.float64, device=dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    dy = torch.zeros_like(y)
    if G > 0:
        desc = _lib.NextPathLoss(G, S, dim, int(divisor), y.data_ptr(), actions.data_ptr(), values.data_ptr(), ptr.data_ptr(),
                                 terms.data_ptr(), loss.data_ptr(), dy.data_ptr())
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().gnnmp_next_path_loss(ctypes.byref(desc), _stream(dev)), 'gnnmp_next_path_loss')
    return terms, loss, dy


class _PathLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, actions, values, ptr, divisor):
        terms, loss, dy = path_loss_device(y.detach(), actions, values, ptr, divisor)
        ctx.save_for_backward(dy)
        ctx.mark_non_differentiable(terms)
        return loss.reshape(()), terms

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        dy, = ctx.saved_tensors
        return dy * grad_loss.to(torch.float32), None, None, None, None


def path_loss(y, actions, values, ptr, divisor, return_terms=False):
    """``(sum over the paths of MSE(value) + MSE(action)) / divisor`` from ``y`` [S, dim + 1] as a float64 device scalar with a
    gradient history to ``y``: ``train()``'s ``loss / 8.`` for the group ``ptr`` describes, however many paths it holds.  With
    ``return_terms`` also the per-path terms [G, 2] (float64, no history)."""
    loss, terms = _PathLossFn.apply(y, actions, values, ptr, int(divisor))
    return (loss, terms) if return_terms else loss


# --------------------------------------------------------------------------------------------------
# train()
# --------------------------------------------------------------------------------------------------
def replay_schedule(n, L=10, group=8, rng=None):
    """The optimizer steps of ``train()`` over a replay of ``n`` samples: ``(groups, perms)`` with ``perms`` the ``L``
    permutations drawn from ``rng`` (``rng.permutation(n)``; default ``RandomState(1234)``) and ``groups`` one list of replay
    indices per step, in the order their terms enter the loss.  A step follows every sample whose position in its pass is
    ``group - 1`` modulo ``group``; the running list is NOT cleared at the end of a pass (the carry-over of the module
    docstring), and what is left after the last pass is dropped."""
    rng = np.random.RandomState(1234) if rng is None else rng
    groups, perms, running = [], [], []
    for _ in range(int(L)):
        perm = rng.permutation(int(n))
        perms.append(perm)
        for batch_i, index in enumerate(perm):
            running.append(int(index))
            if batch_i % group == group - 1:
                groups.append(running)
                running = []
    return groups, perms


def train_replay(train_net, optimizer, store, maps, goals, L=10, group=8, rng=None, iters=DEFAULT_ITERS, log=None):
    """``train()`` of ``train_next.py:42-68`` over ``store``: the steps of :func:`replay_schedule`, each ``store.batch`` ->
    ``train_net.forward`` -> :func:`path_loss` with divisor ``group`` -> backward -> ``optimizer.step()``.  ``maps`` [n, 15, 15]
    and ``goals`` [n, dim] are the device arrays of ALL problems, indexed by ``store.problem``.  Returns ``(losses, groups)``:
    the per-step losses as device scalars (float64) and the index groups used.  Nothing is read back; ``log(step, loss)`` is
    called after every step with the device scalar."""
    groups, _ = replay_schedule(len(store), L, group, rng)
    dev = store.device
    losses = []
    for step, idx in enumerate(groups):
        b = store.batch(idx)
        pid = torch.from_numpy(np.asarray(b['problems'], dtype=np.int64)).to(dev)
        y = train_net.forward(maps.index_select(0, pid), goals.index_select(0, pid), b['states32'], b['problem_of_state'], iters)
        loss = path_loss(y, b['actions'], b['values'], b['ptr'], group)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        losses.append(loss.detach())
        if log is not None:
            log(step, losses[-1])
    return losses, groups


def train_replay_host(forward, optimizer, paths, path_ptr, problem, maps, goals, dim, L=10, group=8, rng=None, iters=DEFAULT_ITERS,
                      dtype=torch.float64):
    """:func:`train_replay` over host arrays: the replay is ``paths`` [N, dim] float64 / ``path_ptr`` [P + 1] / ``problem``
    [P], the labels are :func:`gnnmp.next_train.path_labels`, and ``forward(maps, goals, states32, problem_of_state, iters)``
    is any differentiable forward returning ``y`` [S, dim + 1] in ``dtype`` (``tests/next_train_host.py``'s, closed over its
    leaves, which ``optimizer`` holds).  Returns ``(losses, groups)`` with host floats."""
    paths = np.asarray(paths, dtype=np.float64).reshape(-1, dim)
    ptr = np.asarray(path_ptr, dtype=np.int64).reshape(-1)
    problem = np.asarray(problem, dtype=np.int64).reshape(-1)
    actions, values = path_labels(paths, ptr, dim)
    states32 = paths.astype(np.float32)
    groups, _ = replay_schedule(problem.shape[0], L, group, rng)
    losses = []
    for idx in groups:
        idx = np.asarray(idx, dtype=np.int64)
        lens = ptr[idx + 1] - ptr[idx]
        gptr = np.concatenate([[0], np.cumsum(lens)])
        rows = np.concatenate([np.arange(ptr[i], ptr[i + 1]) for i in idx])
        of = np.repeat(np.arange(idx.size), lens)
        y = forward(np.asarray(maps)[problem[idx]], np.asarray(goals)[problem[idx]], states32[rows], of, iters)
        loss = loss_from_outputs(y, torch.from_numpy(actions[rows]).to(dtype), torch.from_numpy(values[rows]).to(dtype), gptr) * (idx.size / group)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
    return losses, groups


# --------------------------------------------------------------------------------------------------
# train_env
# --------------------------------------------------------------------------------------------------
def collect_replay(net, problems, problem_ids, seeds, store, device, explore_eps, t_max=1000, fallback_batch=50, fallback_t_max=1000,
                   draws='host', stats=None, timings=None, k=10):
    """The body of ``train_next.py:88-108`` for a chunk of maze problems that share one network ``net`` (a loaded
    :class:`gnnmp.next_model.NextNet`): ``NEXT_plan(g_explore_eps=explore_eps, stop_when_success=True)`` for all of them in
    one launch, on :func:`gnnmp.next_plan.plan_maze_batch`'s streams (``RandomState(seeds[i])`` and
    :func:`gnnmp.next_plan.default_eps`), the successes appended straight from the device trees; then BIT* for the failures
    (``bitstar.plan_maze_batch`` with seeds ``seeds[i] ^ 0x9E3779B9``) and its solved paths appended.  ``problem_ids[i]`` is what
    the store records for ``problems[i]``.

    Deviations from the reference: the fallback's budget is the sample count ``fallback_t_max``, not ``T = INF`` under a 60 s
    wall clock; and the fallback draws from its own stream instead of continuing NEXT's numpy stream.  Within a chunk the store
    receives the NEXT successes in ascending order, then the fallback's; the reference interleaves them by problem.
    ``train()`` permutes the replay uniformly, so the order has no effect on the distribution of its steps.

    Returns (and adds to ``stats``) ``{'next': n, 'fallback': n, 'unsolved': n}``; ``timings`` receives the wall clock of the
    stages pb_forward, plan, append, fallback."""
    from . import bitstar
    from .next_model import NextNet
    from .next_plan import default_eps, max_nodes, next_plan_device, policy_scale
    from .rrtstar import draws_per_problem
    from .streams_batch import RawDoubles, StageClock, check_stream_args, problem_tensors
    who = 'next_replay.collect_replay'
    B, t_max = len(problems), int(t_max)
    out_stats = {'next': 0, 'fallback': 0, 'unsolved': 0}
    if B:
        check_stream_args(B, seeds, draws, who)
        if len(problem_ids) != B:
            raise ValueError('%s: one problem id per problem' % who)
        if t_max < 1 or t_max + 1 > max_nodes():
            raise ValueError('%s: t_max is 1 .. %d (the device loop keeps the tree in LDS)' % (who, max_nodes() - 1))
        if not isinstance(net, NextNet):
            raise TypeError('%s: net is a loaded gnnmp.next_model.NextNet' % who)
        dev = torch.device(device)
        clock = StageClock(timings)
        with torch.cuda.device(dev):
            dim, maps, init64, goal64 = problem_tensors(problems, dev, who)
            if dim != net.dim or dim != store.dim:
                raise ValueError('%s: dim %d problems, a dim %d network, a dim %d store' % (who, dim, net.dim, store.dim))
            eps = default_eps(seeds, t_max, k, dim).to(dev).contiguous()
            pb_rep = net.pb_forward(maps.to(torch.float32), goal64.to(torch.float32))
            clock.mark('pb_forward')
            block = RawDoubles(seeds, draws_per_problem(t_max, dim), dev, draws)
            out = next_plan_device(maps, init64, goal64, block.raw, pb_rep, net._weights(dev), eps, t_max, True, explore_eps, 1.0,
                                   int(k), policy_scale(None, dim))
            block.finish(out['small'][3])
            clock.mark('plan')
            ids = np.asarray(problem_ids, dtype=np.int64).reshape(-1)
            store.append_trees(out, ids)
            small = out['small'].cpu().numpy()
            clock.mark('append')
            net.check_status()
            if small[5].any():
                bad = np.flatnonzero(small[5])
                raise RuntimeError('gnnmp_next_plan: status %s for problem(s) %s (1 = draw block too short, 2 = cycle in '
                                   'rewired_parents, 4 = eps block too short, 8 = a score was not finite)'
                                   % (small[5][bad].tolist(), bad.tolist()))
            solved = (small[1] != 0) & (small[4] > 0)
            failed = np.flatnonzero(~solved)
            out_stats['next'] = int(solved.sum())
            if failed.size:
                res = bitstar.plan_maze_batch([problems[i] for i in failed], dev, [(int(seeds[i]) ^ FALLBACK_SEED_XOR) & 0xffffffff for i in failed],
                                              batch=fallback_batch, t_max=fallback_t_max, draws=draws)
                got = [(i, r['path']) for i, r in zip(failed, res) if r['success']]
                if got:
                    store.append_paths(np.concatenate([p for _, p in got]), np.concatenate([[0], np.cumsum([len(p) for _, p in got])]),
                                       ids[[i for i, _ in got]])
                out_stats['fallback'] = len(got)
                out_stats['unsolved'] = int(failed.size) - len(got)
            clock.mark('fallback')
    if stats is not None:
        for key, v in out_stats.items():
            stats[key] = stats.get(key, 0) + v
    return out_stats


def train_env_maze(train_net, problems, device, chunk=200, eps0=1.0, decay=0.7, L=10, lr=1e-3, t_max=1000, fallback_batch=50,
                   fallback_t_max=1000, group=8, iters=DEFAULT_ITERS, draws='host', rng=None):
    """``train_env`` of ``train_next.py:71-115`` for maze problems: problem ``i`` is planned with seed ``i`` (the reference's
    ``set_random_seed(i)``) by :func:`collect_replay` at the current explore rate with a
    :class:`gnnmp.next_model.NextNet` loaded from ``train_net.state_dict()``; after every ``chunk`` problems the explore rate
    is multiplied by ``decay`` and :func:`train_replay` runs with Adam (``lr``) over the whole replay so far.  As in the
    reference, problems behind the last full chunk are collected but no training follows them.  ``rng`` (default
    ``RandomState(1234)``) draws all permutations.

    ``train_net`` is a loaded :class:`gnnmp.next_train.NextNetTrain`; its ``state_dict()`` afterwards is the checkpoint
    (:class:`gnnmp.next_model.NextNet` and ``Model2D`` load it).  Returns the history: per chunk a dict with ``explore_eps``
    (the rate the chunk was planned at), ``next`` / ``fallback`` / ``unsolved``, ``replay`` (its size after the chunk) and
    ``losses`` (host floats, one per optimizer step; empty for a trailing partial chunk)."""
    from . import bitstar
    from .next_model import NextNet
    n, dim, dev = len(problems), train_net.dim, torch.device(device)
    rng = np.random.RandomState(1234) if rng is None else rng
    longest = max(int(t_max) + 1, 2 + bitstar.n_batches(fallback_batch, fallback_t_max) * int(fallback_batch))
    store = ReplayStore(dim, n, n * longest, dev)                # every problem solved, every path as long as a planner allows
    optimizer = torch.optim.Adam(train_net.parameters(), lr=lr)
    with torch.cuda.device(dev):
        maps = torch.from_numpy(np.ascontiguousarray([np.asarray(p['map'], dtype=np.float32) for p in problems])).to(dev)
        goals = torch.from_numpy(np.ascontiguousarray([np.asarray(p['goal_state'], dtype=np.float32).reshape(-1) for p in problems])).to(dev)
    explore, history = float(eps0), []
    for c0 in range(0, n, int(chunk)):
        ids = list(range(c0, min(c0 + int(chunk), n)))
        net = NextNet(dim).load_state_dict(train_net.state_dict())
        entry = collect_replay(net, [problems[i] for i in ids], ids, ids, store, dev, explore, t_max=t_max, fallback_batch=fallback_batch,
                               fallback_t_max=fallback_t_max, draws=draws)
        entry.update(explore_eps=explore, replay=len(store), losses=[])
        if len(ids) == int(chunk):
            explore = decay * explore
            losses, _ = train_replay(train_net, optimizer, store, maps, goals, L=L, group=group, rng=rng, iters=iters)
            train_net.check_status()
            if losses:
                entry['losses'] = torch.stack(losses).cpu().numpy().tolist()
        history.append(entry)
    return history
