"""Ranked frontier rows for planners whose collision checks stay on the host (device side).

``greedy_expand_sparse`` rebuilds a dict of dicts over all E ~ 56 k scores in Python after every forward.  Here the device that
produced the scores also sorts them: for every node row ``a`` the live cells ``P[a, b]`` by score descending, ties by source id
ascending (``gnnmp_frontier_rank``, csrc/frontier_kernels.hip).  One copy brings the rows to pinned host memory and
``planner.greedy_expand_ranked`` walks only the cells it tries.

A cell ``(a, b)`` is live iff ``a != b``, its score is not zero (+0 and -0 are zero) and both ends are free samples (id below
``n_free``).  Of several columns naming the same ``(a, b)`` the LAST decides, the meaning of the reference's ``index_put`` and of
the dense ``planner._mask_policy`` (``greedy_expand_sparse`` keeps an earlier non-zero duplicate instead; the two never differ on
coalesced input).

``rank_rows_host`` is the same ranking in numpy (lexsort): the oracle of the device tests, and what CPU tensors get.
"""
import ctypes

import numpy as np
import torch

ERR_INDEX = -8                          # GNNMP_ERR_INDEX: the per-graph status of a graph with a node id outside [0, N_g)


def limits():
    """(wave_row_cells, block_tile_cells): the row lengths at which the kernels change path (``gnnmp_frontier_limits``)."""
    from . import _lib
    w, t = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.lib().gnnmp_frontier_limits(ctypes.byref(w), ctypes.byref(t)), 'gnnmp_frontier_limits')
    return int(w.value), int(t.value)


class RankedRows:
    """The ranked rows of one ``rank_rows`` call, and the buffers behind them.  ``row_beg`` / ``row_len`` [sum N] (int32) and
    ``cols`` (int32 source ids) / ``vals`` (float32) [sum E]: row ``a`` of graph ``g`` is
    ``cols[row_beg[node_ptr[g] + a] :][:row_len[node_ptr[g] + a]]``; what follows a row's live prefix is unspecified.  On the
    device the four arrays and the per-graph status are views of ONE int32 block, so ``host()`` is a single copy into one pinned
    buffer.  A holder handed back to ``rank_rows(out=...)`` is reused: its buffers only ever grow, and the arrays an earlier
    ``host()`` returned are overwritten by the next one."""

    def __init__(self):
        self.n = self.e = self.g = 0
        self._dev = self._pin = self._ws = self._np = self._got = None

    # ---- layout of the block, in int32 words: row_beg [n] | row_len [n] | status [g] | cols [e] | vals [e]
    def _words(self):
        return 2 * self.n + self.g + 2 * self.e

    def _split(self, block):
        n, g, e = self.n, self.g, self.e
        o = 2 * n + g
        return block[:n], block[n:2 * n], block[2 * n:o], block[o:o + e], block[o + e:o + 2 * e]

    def _reserve(self, n, e, g, device, ws_bytes):
        self.n, self.e, self.g, self._np, self._got = n, e, g, None, None
        words = max(self._words(), 1)
        if self._dev is None or self._dev.device != device or self._dev.numel() < words:
            self._dev = torch.empty(words + words // 4, dtype=torch.int32, device=device)
            self._pin = torch.empty(words + words // 4, dtype=torch.int32, pin_memory=True)
        if self._ws is None or self._ws.device != device or self._ws.numel() < ws_bytes:
            self._ws = torch.empty(ws_bytes + ws_bytes // 4, dtype=torch.uint8, device=device)

    @property
    def is_device(self):
        return self._np is None

    def _tensors(self):
        if self._np is not None:
            return tuple(torch.from_numpy(x) for x in self._np)
        rb, rl, st, co, va = self._split(self._dev)
        return rb, rl, st, co, va.view(torch.float32)

    row_beg = property(lambda self: self._tensors()[0])
    row_len = property(lambda self: self._tensors()[1])
    status = property(lambda self: self._tensors()[2])
    cols = property(lambda self: self._tensors()[3])
    vals = property(lambda self: self._tensors()[4])

    def host(self, check=True):
        """``(row_beg, row_len, cols, vals)`` as numpy arrays: for device rows, views of the pinned buffer after ONE copy on the
        current stream and a wait for it (done once per ``rank_rows`` call; later calls return the same views).  ``check``: raise
        RuntimeError naming the graphs whose ``edge_index`` holds a node id outside the graph (their columns with such an id
        were dropped; the rows of the other graphs are right)."""
        if self._np is not None:
            rb, rl, st, co, va = self._np
        else:
            if self._got is None:
                words = self._words()
                self._pin[:words].copy_(self._dev[:words], non_blocking=True)
                torch.cuda.current_stream(self._dev.device).synchronize()
                rb, rl, st, co, va = self._split(self._pin.numpy())
                self._got = (rb, rl, st, co, va.view(np.float32))
            rb, rl, st, co, va = self._got
        if check:
            bad = np.nonzero(st)[0]
            if bad.size:
                raise RuntimeError('rank_rows: edge_index holds a node id outside its graph (or a prefix array leaves the batch) '
                                   'in graph%s %s -- the rows of %s are wrong' % ('s' if bad.size > 1 else '',
                                                                                ', '.join(str(int(x)) for x in bad),
                                                                                'those graphs' if bad.size > 1 else 'that graph'))
        return rb, rl, co, va


def _ptr_arrays(n_free, node_ptr, edge_ptr, n_nodes, edge_index, E):
    """Host prefix arrays of the numpy restatement."""
    nf = np.atleast_1d(np.asarray(n_free, dtype=np.int64))
    G = int(nf.shape[0])
    if (node_ptr is None or edge_ptr is None) and G != 1:
        raise ValueError('rank_rows: node_ptr / edge_ptr may be left out for one graph only, got %d' % G)
    if node_ptr is None:
        if n_nodes is None:
            n_nodes = max(int(nf[0]), int(edge_index.max()) + 1 if E else 0)
        node_ptr = [0, int(n_nodes)]
    if edge_ptr is None:
        edge_ptr = [0, E]
    return nf, np.asarray(node_ptr, dtype=np.int64), np.asarray(edge_ptr, dtype=np.int64)


def rank_rows_host(scores, edge_index, n_free, node_ptr=None, edge_ptr=None, n_nodes=None):
    """The ranking in numpy: same arguments (arrays or CPU tensors), same layout and same liveness / duplicate / tie rules as
    the kernels; the unspecified tail of a row holds column -1 and value 0.  Returns a :class:`RankedRows`."""
    scores = np.ascontiguousarray(np.asarray(scores, dtype=np.float32)).reshape(-1)
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    E = int(ei.shape[1])
    nf, nptr, eptr = _ptr_arrays(n_free, node_ptr, edge_ptr, n_nodes, ei, E)
    G, total_n = int(nf.shape[0]), int(nptr[-1])
    row_beg, row_len = np.zeros(total_n, dtype=np.int32), np.zeros(total_n, dtype=np.int32)
    cols, vals = np.full(E, -1, dtype=np.int32), np.zeros(E, dtype=np.float32)
    status = np.zeros(G, dtype=np.int32)
    for g in range(G):
        n0, n1, e0, e1 = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
        if not (0 <= n0 <= n1 <= total_n and 0 <= e0 <= e1 <= E):
            status[g] = ERR_INDEX
            continue
        N = n1 - n0
        src, dst, sc = ei[0, e0:e1], ei[1, e0:e1], scores[e0:e1]
        ok = (src >= 0) & (src < N) & (dst >= 0) & (dst < N)
        if not ok.all():
            status[g] = ERR_INDEX                                           # such a column is dropped
        col = np.nonzero(ok)[0]
        a, b, s = dst[col], src[col], sc[col]
        deg = np.bincount(a, minlength=N)[:N] if N else np.zeros(0, dtype=np.int64)
        beg = e0 + np.cumsum(deg) - deg                                     # the by-target CSR position
        row_beg[n0:n1] = beg
        if not col.size:
            continue
        order = np.lexsort((col, a * N + b))                                # per cell, its columns in ascending order
        key = (a * N + b)[order]
        last = order[np.append(key[1:] != key[:-1], True)]                  # the highest column of a cell decides it
        a, b, s = a[last], b[last], s[last]
        live = (a != b) & (s != 0) & (a < nf[g]) & (b < nf[g])
        a, b, s = a[live], b[live], s[live]
        o = np.lexsort((b, -s, a))                                          # row, score descending, source ascending
        a, b, s = a[o], b[o], s[o]
        ln = np.bincount(a, minlength=N)[:N]
        row_len[n0:n1] = ln
        slot = beg[a] + np.arange(a.shape[0]) - (np.cumsum(ln) - ln)[a]
        cols[slot], vals[slot] = b, s
    out = RankedRows()
    out.n, out.e, out.g = total_n, E, G
    out._np = (row_beg, row_len, status, cols, vals)
    return out


def rank_rows(scores, edge_index, n_free, node_ptr=None, edge_ptr=None, n_nodes=None, out=None):
    """Rank the live cells of every node row.  ``scores`` [sum E] float32 in the column order of ``edge_index`` [2, sum E] (int64,
    graph-local ids; row 0 = source b, row 1 = target a: column e is the dense cell ``P[a, b]``); ``n_free``: per graph, how many
    of its nodes -- a prefix -- are free samples (an int for one graph, a sequence, or an int32 tensor on the scores' device);
    ``node_ptr`` / ``edge_ptr`` [G + 1] int32 (the ``GraphBatch`` convention), both optional for one graph; ``n_nodes``: the total
    node count -- without it it is read from ``node_ptr`` (a device wait), or for one graph taken from the largest id present.
    CUDA tensors go to the kernels: everything is enqueued on the current stream, nothing waits until ``host()``.  CPU tensors go
    to :func:`rank_rows_host`.  ``out``: a :class:`RankedRows` of an earlier call whose buffers are reused."""
    if not scores.is_cuda:
        as_np = lambda t: None if t is None else (t.numpy() if torch.is_tensor(t) else t)      # noqa: E731
        res = rank_rows_host(scores.detach().numpy(), as_np(edge_index), as_np(n_free), as_np(node_ptr), as_np(edge_ptr), n_nodes)
        if out is None:
            return res
        out.n, out.e, out.g, out._np, out._got = res.n, res.e, res.g, res._np, None
        return out
    from . import _lib
    device = scores.device
    scores = scores.detach().to(torch.float32).contiguous().reshape(-1)
    edge_index = edge_index.to(device=device, dtype=torch.int64).contiguous()
    E = int(scores.shape[0])
    if tuple(edge_index.shape) != (2, E):
        raise ValueError('rank_rows: edge_index must be [2, %d], got %s' % (E, tuple(edge_index.shape)))
    if torch.is_tensor(n_free):
        nf = n_free.to(device=device, dtype=torch.int32).contiguous().reshape(-1)
    else:
        nf = torch.tensor(np.atleast_1d(np.asarray(n_free, dtype=np.int32))).to(device)
    G = int(nf.shape[0])
    if (node_ptr is None or edge_ptr is None) and G != 1:
        raise ValueError('rank_rows: node_ptr / edge_ptr may be left out for one graph only, got %d' % G)
    i32 = lambda t: None if t is None else torch.as_tensor(t).to(device=device, dtype=torch.int32).contiguous()   # noqa: E731
    node_ptr, edge_ptr = i32(node_ptr), i32(edge_ptr)
    for name, t in (('node_ptr', node_ptr), ('edge_ptr', edge_ptr)):
        if t is not None and int(t.numel()) != G + 1:
            raise ValueError('rank_rows: %s must have %d entries, got %d' % (name, G + 1, int(t.numel())))
    if n_nodes is None:
        if node_ptr is not None:
            n_nodes = int(node_ptr[-1])
        else:
            n_nodes = max(int(nf[0]), int(edge_index.max()) + 1 if E else 0)
    N = int(n_nodes)
    ptr = lambda t: None if t is None else t.data_ptr()            # noqa: E731
    fb = _lib.FrontierBatch(G, N, E, edge_index.data_ptr(), scores.data_ptr(), ptr(node_ptr), ptr(edge_ptr), nf.data_ptr())
    need = ctypes.c_size_t()
    _lib.check(_lib.lib().gnnmp_frontier_workspace_bytes(ctypes.byref(fb), ctypes.byref(need)), 'gnnmp_frontier_workspace_bytes')
    out = RankedRows() if out is None else out
    out._reserve(N, E, G, device, int(need.value))
    base = out._dev.data_ptr()                                     # (an empty view has no address of its own: offsets of the block)
    rb, rl, st, co, va = (base + 4 * o for o in (0, N, 2 * N, 2 * N + G, 2 * N + G + E))
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().gnnmp_frontier_rank(ctypes.byref(fb), rb, rl, co, va, st, out._ws.data_ptr(), out._ws.numel(),
                                                  stream), 'gnnmp_frontier_rank')
    return out
