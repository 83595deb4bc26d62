"""numpy's legacy generator per problem on the device (``gnnmp_mt19937_seed`` / ``gnnmp_mt19937_uniform``,
``csrc/rng_kernels.hip``): stream i of :class:`MTStreams` yields what ``np.random.RandomState(seeds[i])`` yields, bit for bit,
and its state is numpy's (``get_state()`` / ``set_state``), so the streams planner keeps its recorded answers when the draws
move off the host.  No host fallback: without the library every call raises."""
import ctypes

import numpy as np
import torch

from . import _lib

STATE_WORDS = 625                      # uint32 key[624] + int32 pos: RandomState.get_state()[1:3]


def _device(device):
    d = torch.device(device)
    if d.type == 'cuda' and d.index is None:
        d = torch.device('cuda', torch.cuda.current_device())
    return d


def _bounds(low, high):
    """numpy's uniform with array bounds: (low, range = high - low in double, dim)."""
    lo, hi = np.broadcast_arrays(np.atleast_1d(np.asarray(low, dtype=np.float64)), np.atleast_1d(np.asarray(high, dtype=np.float64)))
    if lo.ndim != 1 or not 1 <= lo.shape[0] <= 3:
        raise ValueError('MTStreams.uniform: bounds of 1 to 3 columns')
    return lo, hi - lo, int(lo.shape[0])


class MTStreams:
    """``len(seeds)`` independent ``np.random.RandomState`` streams living on ``device``; seeds are taken ``& 0xffffffff``."""

    def __init__(self, seeds, device):
        self.device = _device(device)
        seeds = np.array([int(s) & 0xffffffff for s in seeds], dtype=np.uint32)
        self.n = int(seeds.shape[0])
        if self.n < 1:
            raise ValueError('MTStreams: at least one stream')
        self._state = torch.empty(self.n, STATE_WORDS, dtype=torch.int32, device=self.device)
        seeds_d = torch.from_numpy(seeds.view(np.int32)).to(self.device)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.lib().gnnmp_mt19937_seed(self.n, seeds_d.data_ptr(), self._state.data_ptr(), st), 'gnnmp_mt19937_seed')

    @classmethod
    def from_states(cls, states, device):
        """Streams that continue numpy generators: ``states`` are ``RandomState.get_state()`` tuples (any ``pos``)."""
        self = cls.__new__(cls)
        self.device = _device(device)
        self.n = len(states)
        if self.n < 1:
            raise ValueError('MTStreams: at least one stream')
        words = np.empty((self.n, STATE_WORDS), dtype=np.uint32)
        for i, s in enumerate(states):
            if s[0] != 'MT19937' or not 0 <= int(s[2]) <= 624:
                raise ValueError('MTStreams.from_states: an MT19937 state with pos in [0, 624]')
            words[i, :624] = np.asarray(s[1], dtype=np.uint32)
            words[i, 624] = int(s[2])
        self._state = torch.from_numpy(words.view(np.int32)).to(self.device)
        return self

    def state(self, i):
        """Stream ``i``'s state as ``np.random.RandomState().set_state`` takes it (reads the device: synchronises)."""
        words = self._state[int(i)].cpu().numpy().view(np.uint32)
        return ('MT19937', words[:624].copy(), int(words[624]), 0, 0.0)

    def _i32(self, counts):
        if isinstance(counts, torch.Tensor):
            c = counts.to(device=self.device, dtype=torch.int32).contiguous()
        else:
            c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).to(self.device)
        if c.shape != (self.n,):
            raise ValueError('MTStreams: one count per stream')
        return c

    def _run(self, counts, dim, low, rng, out, out_ptr, out_rows, commit, active):
        status = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        b = _lib.MtUniformBatch(self.n, dim, out_rows, counts.data_ptr(), out_ptr.data_ptr() if out_ptr is not None else None,
                                active.data_ptr() if active is not None else None)
        for c in range(dim):
            b.low[c], b.range[c] = float(low[c]), float(rng[c])
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.lib().gnnmp_mt19937_uniform(ctypes.byref(b), self._state.data_ptr(), out.data_ptr() if out is not None else None,
                                                        1 if commit else 0, status.data_ptr(), st), 'gnnmp_mt19937_uniform')
        return status

    def uniform(self, counts, low, high, out_ptr=None, commit=False, active=None, out=None):
        """``RandomState.uniform(low, high, (counts[i], dim))`` of every stream in one launch -> ``(rows, status)``: ``rows``
        float64 ``[sum(counts), dim]`` on the device, stream after stream (or, with ``out_ptr`` -- int64 ``[n + 1]``, host or
        device -- stream i's rows at row ``out_ptr[i]`` of ``[out_ptr[-1], dim]``; ``out``: the caller's buffer instead of a new
        one, any rows no stream writes keep their content).  ``status`` (int32 ``[n]``, device): 0 done, 2 a negative count or
        a block outside the buffer (nothing written).  Without ``commit`` the streams do not move: the same rows come again,
        and a longer count continues them.  ``active`` (uint8 ``[n]``, device): streams with 0 are skipped entirely.
        ``counts``: a host sequence or an int32 device tensor.  Nothing is read back."""
        lo, rng, dim = _bounds(low, high)
        if out_ptr is None:
            if isinstance(counts, torch.Tensor):
                raise ValueError('MTStreams.uniform: device counts need out_ptr')
            ptr_h = np.zeros(self.n + 1, dtype=np.int64)
            ptr_h[1:] = np.cumsum(np.maximum(np.asarray(counts, dtype=np.int64), 0))
            out_ptr = ptr_h
        rows = None
        if isinstance(out_ptr, torch.Tensor):
            ptr_d = out_ptr.to(device=self.device, dtype=torch.int64).contiguous()
        else:
            ptr_h = np.ascontiguousarray(out_ptr, dtype=np.int64)
            rows = int(ptr_h[-1])
            ptr_d = torch.from_numpy(ptr_h).to(self.device)
        if ptr_d.shape != (self.n + 1,):
            raise ValueError('MTStreams.uniform: out_ptr holds n + 1 offsets')
        if out is None:
            if rows is None:
                raise ValueError('MTStreams.uniform: a device out_ptr needs out')
            out = torch.empty(max(rows, 1), dim, dtype=torch.float64, device=self.device)[:rows]      # (never a NULL pointer)
        elif out.dtype != torch.float64 or out.dim() != 2 or out.shape[1] != dim or not out.is_contiguous() or out.device != self.device:
            raise ValueError('MTStreams.uniform: out is a contiguous float64 [rows, dim] tensor on the streams\' device')
        status = self._run(self._i32(counts), dim, lo, rng, out, ptr_d, int(out.shape[0]), commit, active)
        return out, status

    def advance(self, counts, dim, active=None):
        """Skip ``counts[i]`` rows of ``dim`` columns in every stream (committed) -> status.  ``counts`` may be the int32
        device tensor a sampler wrote (``maze_sample_streams``' ``used``)."""
        return self._run(self._i32(counts), int(dim), (0.0,) * 3, (0.0,) * 3, None, None, 0, True, active)
