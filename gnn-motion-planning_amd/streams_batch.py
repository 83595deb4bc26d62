"""What the batched maze planners with one sample stream per problem share on the host (:func:`gnnmp.planner.plan_maze_rounds_batch`,
:mod:`gnnmp.lazysp`, :mod:`gnnmp.bitstar`, :mod:`gnnmp.rrtstar`, :mod:`gnnmp.next_plan`): the problem helpers, the stage clock, the
float64 staging of a batch, the attempt-block driver of the rejection samplers (:class:`AttemptBlocks`), the raw-doubles block of
the tree planners (:class:`RawDoubles`), the chunk loop of the ``eval_*_device`` functions and the marshalling of
``gnnmp_maze_streams_batch``.  A new planner brings its own kernels and plugs its sampler in as a ``sample`` callback.  Nothing here
imports torch or the library before a call needs them."""
import time

import numpy as np

from . import maze2d


def maze_class(dim, who=None):
    """Host environment of a maze problem by the width of its configurations: 2 = point robot, 3 = stick robot.  ``who``: the
    module named in the error."""
    if int(dim) in (2, 3):
        return maze2d.Maze3D if int(dim) == 3 else maze2d.Maze2D
    if who is None:
        raise ValueError('maze problems have configurations of width 2 or 3, got %d' % dim)
    raise ValueError('%s: maze problems have 2 (point robot) or 3 (stick robot) coordinates' % who)


def problem_env(problem, who=None):
    """The host environment of one problem (a dict with ``map``, ``init_state``, ``goal_state``), float64 states."""
    init = np.asarray(problem['init_state'], dtype=np.float64).reshape(-1)
    env = maze_class(init.shape[0], who)(np.asarray(problem['map'])[None], init[None],
                                         np.asarray(problem['goal_state'], dtype=np.float64).reshape(1, -1))
    env.init_new_problem(0)
    return env


def bounds(bound):
    """(low, high - low) of an environment's ``bound`` as the reference's planners form them (lazy_sp.py:37-39, bit_star.py:32-34)."""
    b = np.array(bound, dtype=np.float64).reshape((2, -1)).T
    return b[:, 0].copy(), b[:, 1] - b[:, 0]


def sample_limits(dim, who=None):
    """The box ``uniform_sample`` draws from, as float64: ``uniform(-limits, limits)``."""
    return np.asarray(maze_class(dim, who).SAMPLE_LIMITS, dtype=np.float64)


def stream_seeds(seed, indexes):
    """Default per-problem seeds of the ``eval_*_device`` functions: ``(seed + 0x9E3779B1 * (index + 1)) mod 2**32``."""
    return [(int(seed) + 0x9E3779B1 * (int(i) + 1)) % (1 << 32) for i in indexes]


class StageClock:
    """Wall clock per stage into the caller's ``timings`` dict; with ``None`` every :meth:`mark` does nothing."""

    def __init__(self, timings):
        self.timings, self.t = timings, time.perf_counter()

    def mark(self, name):
        """Add the time since the last mark (or the construction) to ``timings[name]``, after a synchronise of the CURRENT
        stream only: other passes may be in flight on theirs."""
        if self.timings is None:
            return
        import torch
        torch.cuda.current_stream().synchronize()
        now = time.perf_counter()
        self.timings[name] = self.timings.get(name, 0.) + now - self.t
        self.t = now


def check_stream_args(n_problems, seeds, draws, who):
    """The argument checks every ``plan_*_batch`` of ``who`` makes: one seed per problem, a known way of drawing."""
    if len(seeds) != n_problems:
        raise ValueError('%s: one seed per problem' % who)
    if draws not in ('host', 'device'):
        raise ValueError("%s: draws is 'host' or 'device'" % who)


def problem_tensors(problems, dev, who):
    """The batch as float64 device tensors -> ``(dim, maps [B, w, w], init64 [B, dim], goal64 [B, dim])``."""
    import torch
    dims = {int(np.asarray(pr['init_state']).reshape(-1).shape[0]) for pr in problems}
    if len(dims) != 1:
        raise ValueError('%s: point-robot and stick-robot problems in one batch' % who)
    f64 = lambda key: torch.from_numpy(np.ascontiguousarray(np.asarray(        # noqa: E731
        [np.asarray(pr[key], dtype=np.float64) if key == 'map' else np.asarray(pr[key], dtype=np.float64).reshape(-1) for pr in problems]))).to(dev)
    return dims.pop(), f64('map'), f64('init_state'), f64('goal_state')


class AttemptBlocks:
    """The sample streams of B problems as blocks of attempts for a rejection sampler on the device: problem i's attempts are
    the rows of ``RandomState(seeds[i]).uniform(-limits, limits, (m, dim))``, drawn on the host (``draws='host'``) or by
    :class:`gnnmp.rng.MTStreams` (``'device'``).  ``estimate``: the calling module's ``[point, stick]`` list of attempts per
    free draw, which sizes the first block.  ``gstat_values``: name the generators' status words in their error too."""

    def __init__(self, seeds, dim, dev, draws, estimate, gstat_values=False):
        self.B, self.dim, self.dev, self.estimate, self.gstat_values = len(seeds), int(dim), dev, estimate, gstat_values
        self.limits = sample_limits(dim)
        self.streams = None
        if draws == 'device':
            from .rng import MTStreams
            self.streams = MTStreams(seeds, dev)
        else:
            self.gens = [np.random.RandomState(int(s) & 0xffffffff) for s in seeds]
            self.bufs = [np.zeros((0, self.dim))] * self.B               # drawn, not yet consumed

    def update_estimate(self, attempts, free):
        e, d = self.estimate, self.dim - 2
        e[d] = max(1.5, 0.5 * e[d] + 0.5 * attempts / free)

    def run(self, pending, n_free, sample, commit=True, no_room='sampler: status above 1 for problem(s) %s'):
        """Give every problem of ``pending`` (ids, ascending) ``n_free`` free draws: a block of ``int(n_free * estimate * 1.25)
        + 64`` attempts each, twice as long for whoever ran out, until nobody is left.

        ``sample(att, att_ptr_host, mask_d)`` launches the planner's sampler on ``att`` (float64 ``[M, dim]``, device; problem
        b's block is ``[att_ptr[b], att_ptr[b + 1])``, empty unless ``mask_d[b]``) and returns int32 ``[B]`` device tensors:
        ``status`` (0 done, 1 ran out, above that ``no_room`` raises) and, with ``commit``, ``used`` (attempts consumed, 0 for
        whoever ran out); any more ride along.  They come back in the ONE read of the attempt, with the generators' status
        words behind them.  Returns ``[rows, B]``: every problem's words of the attempt that finished it.

        ``commit``: a problem that finished leaves its ``used`` attempts behind (the host buffer is trimmed, the device stream
        advanced) and the estimate moves to the mean of ``used / n_free``.  Without it nothing moves: a sampler that starts
        over gets every block from the same stream position, and the caller advances ``self.streams`` when it knows how far."""
        import torch
        B, dim, limits = self.B, self.dim, self.limits
        want = int(n_free * self.estimate[dim - 2] * 1.25) + 64
        drawn = consumed = 0
        at_finish = None
        while pending.size:
            mask = np.zeros(B, dtype=np.uint8)
            mask[pending] = 1
            mask_d = torch.from_numpy(mask).to(self.dev)
            counts = np.zeros(B, dtype=np.int64)
            if self.streams is not None:
                counts[pending] = want
            else:
                for i in pending:
                    short = want - self.bufs[i].shape[0]
                    if short > 0:
                        self.bufs[i] = np.concatenate((self.bufs[i], self.gens[i].uniform(-limits, limits, (short, dim))))
                    counts[i] = self.bufs[i].shape[0]
            att_ptr = np.zeros(B + 1, dtype=np.int64)
            att_ptr[1:] = np.cumsum(counts)
            if self.streams is not None:
                att, gstat = self.streams.uniform(counts, -limits, limits, out_ptr=att_ptr, active=mask_d)      # not committed
            else:
                att = torch.from_numpy(np.concatenate([self.bufs[i] for i in pending])).to(self.dev)
            words = tuple(sample(att, att_ptr, mask_d))
            if self.streams is not None:
                if commit:
                    self.streams.advance(words[1], dim, active=mask_d)   # used is 0 for whoever ran out: those stay put
                words += (gstat,)
            words_h = (torch.stack(words) if len(words) > 1 else words[0][None]).cpu().numpy()
            status_h = words_h[0]
            if self.streams is not None and words_h[-1][pending].any():
                bad = words_h[-1][pending] != 0
                raise RuntimeError('gnnmp_mt19937_uniform: status %sfor problem(s) %s'
                                   % ('%s ' % words_h[-1][pending][bad].tolist() if self.gstat_values else '', pending[bad].tolist()))
            if (status_h[pending] > 1).any():
                raise RuntimeError(no_room % pending[status_h[pending] > 1].tolist())
            fin = pending[status_h[pending] == 0]
            if at_finish is None:
                at_finish = np.zeros(words_h.shape, dtype=words_h.dtype)
            at_finish[:, fin] = words_h[:, fin]
            if commit:
                if self.streams is None:
                    for i in fin:
                        self.bufs[i] = self.bufs[i][words_h[1][i]:]
                drawn += n_free * int(fin.size)
                consumed += int(words_h[1][fin].sum())
            pending = pending[status_h[pending] == 1]
            want *= 2
        if commit:
            self.update_estimate(consumed, max(drawn, 1))
        return at_finish


class RawDoubles:
    """``raw`` [B, n_draws] float64 on the device: problem i's row is ``RandomState(seeds[i]).random_sample(n_draws)``, drawn on
    the host (``draws='host'``) or by uncommitted :class:`gnnmp.rng.MTStreams` (``'device'``; :meth:`finish` commits)."""

    def __init__(self, seeds, n_draws, dev, draws):
        import torch
        self.streams = None
        if draws == 'device':
            from .rng import MTStreams
            self.streams = MTStreams(seeds, dev)
            rows, self.gstat = self.streams.uniform([n_draws] * len(seeds), 0.0, 1.0)      # low 0, range 1: the raw doubles; not committed
            self.raw = rows.reshape(len(seeds), n_draws)
        else:
            self.raw = torch.from_numpy(np.stack([np.random.RandomState(int(s) & 0xffffffff).random_sample(n_draws) for s in seeds])).to(dev)

    def finish(self, used, streams_out=None):
        """After the planner's launch: advance the device streams by the doubles each problem consumed (``used``, int32 device
        tensor), so that their state is numpy's after the plan; ``streams_out`` (a list) receives them."""
        if self.streams is None:
            return
        self.streams.advance(used, 1)
        if self.gstat.cpu().numpy().any():
            raise RuntimeError('gnnmp_mt19937_uniform: a stream reported a status')
        if streams_out is not None:
            streams_out.append(self.streams)


def eval_chunks(env, indexes, seed, seeds, chunk):
    """The problems ``indexes`` of ``env`` in chunks of ``chunk`` -> ``(problems, seeds_of_chunk)`` per chunk; ``seeds`` None:
    :func:`stream_seeds` of ``seed``."""
    indexes, chunk = list(indexes), max(int(chunk), 1)
    seeds = stream_seeds(seed, indexes) if seeds is None else list(seeds)
    for c0 in range(0, len(indexes), chunk):
        part = indexes[c0:c0 + chunk]
        yield ([dict(map=env.maps[i], init_state=env.init_states[i], goal_state=env.goal_states[i]) for i in part],
               seeds[c0:c0 + len(part)])


def stream_ptr(dev):
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


def maze_streams_batch(B, width, n, cap, attempts, att_ptr_host, maps, init64, goal64, active):
    """``gnnmp_maze_streams_batch`` for a sampler launch -> ``(struct, keep)``: the struct holds raw pointers, ``keep`` the
    arrays behind them that the caller must hold until the launch is issued."""
    import torch
    from . import _lib
    att_ptr_host = np.ascontiguousarray(att_ptr_host, dtype=np.int64)
    att_ptr = torch.from_numpy(att_ptr_host).to(maps.device)
    attempts = attempts.contiguous()
    sb = _lib.MazeStreamsBatch(int(B), int(width), int(n), int(cap), int(attempts.shape[0]), attempts.data_ptr(), att_ptr.data_ptr(),
                               att_ptr_host.ctypes.data, maps.data_ptr(), init64.data_ptr(), goal64.data_ptr(),
                               active.data_ptr() if active is not None else None)
    return sb, (attempts, att_ptr, att_ptr_host)
