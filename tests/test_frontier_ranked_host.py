"""Ranked frontier rows on the host (gnnmp.frontier.rank_rows_host + planner.greedy_expand_ranked): the numpy restatement of
the device ranking and the walk over its rows, against the two frontiers the planner already has -- the heap of
``greedy_expand_sparse`` on duplicate-free columns, the dense ``_mask_policy`` + ``greedy_expand`` where columns repeat (last
column wins) -- and against the recorded reference traces.  CPU only; the argument checks of the C entry points return before
anything touches a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import golden_files
import gnnmp  # noqa: F401
from gnnmp import _lib, planner
from gnnmp.frontier import rank_rows, rank_rows_host
from test_planner_host import ReplayExplorer, ReplaySmoother, _StubEnv, _env, _load


def _random_case(seed, values, duplicates):
    rng = np.random.RandomState(1000 + seed)
    n = int(rng.randint(6, 41))
    v = rng.rand(n, 2).astype(np.float32)
    tgt, src = np.nonzero(rng.rand(n, n) < 0.3)                     # self loops included
    ei = np.stack((src, tgt))                                       # column e: edge src -> tgt = cell P[tgt, src]
    scores = rng.choice(np.array(values, dtype=np.float32), size=ei.shape[1])
    if duplicates:
        m = max(2, ei.shape[1] // 4)
        again = rng.randint(0, ei.shape[1], size=m)                 # some cells two or three times
        ei = np.concatenate((ei, ei[:, again], ei[:, again[:m // 2]]), axis=1)
        extra = rng.choice(np.array(values, dtype=np.float32), size=m + m // 2)
        extra[::3] = 0.0                                            # a duplicate whose LAST value is 0 kills the cell
        scores = np.concatenate((scores, extra))
    perm = rng.permutation(ei.shape[1])                             # unsorted columns
    ei, scores = np.ascontiguousarray(ei[:, perm]), scores[perm]
    n_free = n - int(rng.randint(0, n // 4 + 1))                    # collided suffix
    labels = np.zeros((n, 2), dtype=np.int64)
    labels[n_free:, 1] = 1
    blocked = set()
    for _ in range(int(rng.randint(0, n))):
        i, j = sorted(rng.randint(0, n, 2).tolist())
        blocked.add((i, j))
    goal = int(rng.randint(1, n))
    start_explored = [0] + [int(x) for x in rng.permutation(np.arange(1, n))[:int(rng.randint(0, 3))]]
    hist = [[0, 0]]
    for _ in range(int(rng.randint(0, 3))):
        a, b = rng.randint(0, n, 2).tolist()
        hist.extend([[a, b], [b, a]])

    def fresh():
        return {'explored': list(start_explored), 'explored_edges': [list(x) for x in hist],
                'costs': {k: 0. for k in start_explored}, 'prev': {k: 0 for k in start_explored}}
    return n, v, ei, scores, n_free, labels, blocked, goal, fresh


def _same(path_x, sx, env_x, path_y, sy, env_y):
    assert path_x == path_y
    assert sx['explored'] == sy['explored']
    assert sx['explored_edges'] == sy['explored_edges']
    assert env_x.collision_check_count == env_y.collision_check_count


@pytest.mark.parametrize('seed', range(30))
def test_ranked_walk_equals_the_heap_on_random_ties(seed):
    """Duplicate-free columns, few distinct score values (ties everywhere), +0 and -0, negatives, self loops, a collided
    suffix, a non-trivial starting tree and an explored-edge history that goes through the legacy-index quirk."""
    n, v, ei, scores, n_free, labels, blocked, goal, fresh = _random_case(
        seed, [-2.1, -1.3, 0.0, -0.0, 0.5, 0.5, 1.7], duplicates=False)
    sh, sr = fresh(), fresh()
    env_h, env_r = _StubEnv(v, blocked, goal), _StubEnv(v, blocked, goal)
    path_h = planner.greedy_expand_sparse(scores, ei, labels, v, env_h, sh)
    ranked = rank_rows_host(scores, ei, n_free, n_nodes=n)
    path_r = planner.greedy_expand_ranked(ranked, n, v, env_r, sr)
    _same(path_h, sh, env_h, path_r, sr, env_r)


@pytest.mark.parametrize('seed', range(30))
def test_ranked_walk_equals_the_dense_matrix_with_duplicate_columns(seed):
    """Columns that repeat a cell: the last one decides, a last value of 0 kills the cell -- the dense matrix's behaviour.
    All scores are >= 0, so the dense loop's float32 sum test cannot cancel while live cells remain."""
    n, v, ei, scores, n_free, labels, blocked, goal, fresh = _random_case(
        seed, [0.0, 0.25, 0.5, 0.5, 1.75, 3.0], duplicates=True)
    P = np.zeros((n, n), dtype=np.float32)
    for e in range(ei.shape[1]):                                    # index_put, column after column
        P[ei[1, e], ei[0, e]] = scores[e]
    sd, sr = fresh(), fresh()
    env_d, env_r = _StubEnv(v, blocked, goal), _StubEnv(v, blocked, goal)
    Pm = planner._mask_policy(P.copy(), labels, sd['explored'], sd['explored_edges'])
    path_d = planner.greedy_expand(Pm, v, env_d, sd)
    # through the public entry: CPU tensors take the numpy restatement
    ranked = rank_rows(torch.from_numpy(scores), torch.from_numpy(ei), n_free, n_nodes=n)
    path_r = planner.greedy_expand_ranked(ranked, n, v, env_r, sr)
    _same(path_d, sd, env_d, path_r, sr, env_r)


@pytest.mark.parametrize('path', golden_files('planner_'), ids=os.path.basename)
def test_planner_replay_ranked_matches_reference_trace(path):
    r = _load(path)
    env = _env(r)
    np.random.seed(int(r['seed']))
    torch.manual_seed(int(r['seed']))
    ex, sm = ReplayExplorer(r), ReplaySmoother(r)
    res = planner.explore(env, ex, sm, True, batch=int(r['batch']), t_max=int(r['t_max']), k=int(r['k']), device='cpu',
                          frontier='ranked')
    assert ex.i == int(r['n_forward']) and sm.i == int(r['n_smooth'])
    assert res['success'] == bool(r['success'])
    assert res['explored'] == r['explored'].tolist()
    assert res['explored_edges'] == r['explored_edges'].tolist()
    assert res['c_explore'] == int(r['c_explore'])
    assert res['c_smooth'] == int(r['c_smooth'])
    assert np.array_equal(np.array(res['path'], dtype=np.float32), r['path'])
    assert np.array_equal(np.array(res['smooth_path'], dtype=np.float64), r['smooth_path'])


def test_replay_goldens_are_all_there():
    assert len(golden_files('planner_mazehard_')) == 5


def test_explore_refuses_an_unknown_frontier():
    with pytest.raises(ValueError, match='frontier'):
        planner.explore(None, None, None, frontier='sorted')


@pytest.mark.parametrize('seed', range(8))
def test_rank_rows_host_invariants(seed):
    """Two graphs side by side: rows sorted by (-score, source), row_len = number of live cells of the dense matrix, every
    cell of a prefix live, every row inside its own in-degree range."""
    parts, nptr, eptr, nfs = [], [0], [0], []
    for g in range(2):
        n, _, ei, scores, n_free, *_ = _random_case(50 * seed + g, [-2.1, -1.3, 0.0, -0.0, 0.5, 0.5, 1.7], duplicates=bool(g))
        parts.append((n, ei, scores, n_free))
        nptr.append(nptr[-1] + n)
        eptr.append(eptr[-1] + ei.shape[1])
        nfs.append(n_free)
    ei_all = np.concatenate([p[1] for p in parts], axis=1)
    sc_all = np.concatenate([p[2] for p in parts])
    row_beg, row_len, cols, vals = rank_rows_host(sc_all, ei_all, nfs, nptr, eptr).host()
    assert row_beg.dtype == np.int32 and row_len.dtype == np.int32 and cols.dtype == np.int32 and vals.dtype == np.float32
    for g, (n, ei, scores, n_free) in enumerate(parts):
        P = np.zeros((n, n), dtype=np.float32)
        for e in range(ei.shape[1]):
            P[ei[1, e], ei[0, e]] = scores[e]
        P[np.arange(n), np.arange(n)] = 0
        P[n_free:, :] = 0
        P[:, n_free:] = 0
        deg = np.bincount(ei[1], minlength=n)
        beg = eptr[g] + np.cumsum(deg) - deg
        assert np.array_equal(row_beg[nptr[g]:nptr[g + 1]], beg)
        for a in range(n):
            lo, ln = int(row_beg[nptr[g] + a]), int(row_len[nptr[g] + a])
            assert ln == int(np.count_nonzero(P[a])) and ln <= deg[a]
            b, s = cols[lo:lo + ln], vals[lo:lo + ln]
            assert np.array_equal(P[a, b], s) and np.all(s != 0)               # no dead cell in the prefix, bitwise values
            assert len(set(b.tolist())) == ln
            keys = list(zip((-s).tolist(), b.tolist()))
            assert keys == sorted(keys)


def test_rank_rows_host_names_the_graph_with_a_bad_node_id():
    ei = np.array([[0, 1, 2, 1], [1, 0, 1, 2]], dtype=np.int64)
    sc = np.array([1., 2., 3., 4.], dtype=np.float32)
    both = np.concatenate((ei, ei), axis=1)
    both[0, 6] = 3                                                   # graph 1 has three nodes
    rr = rank_rows_host(np.concatenate((sc, sc)), both, [3, 3], [0, 3, 6], [0, 4, 8])
    with pytest.raises(RuntimeError, match='graph 1'):
        rr.host()
    row_beg, row_len, cols, vals = rr.host(check=False)
    assert row_len[:3].tolist() == [1, 2, 1] and cols[1:3].tolist() == [2, 0]       # graph 0 is untouched: row 1 = (3., b=2), (1., b=0)


# ---- argument checks of the C entry points (they return before any device work)
def _abi_case():
    ei = np.array([[0, 1, 2], [1, 2, 0]], dtype=np.int64)
    sc = np.ones(3, dtype=np.float32)
    nf = np.array([3], dtype=np.int32)
    out = [np.zeros(8, dtype=np.int32) for _ in range(5)]
    fb = _lib.FrontierBatch(1, 3, 3, ei.ctypes.data, sc.ctypes.data, None, None, nf.ctypes.data)
    need = ctypes.c_size_t()
    assert _lib.lib().gnnmp_frontier_workspace_bytes(ctypes.byref(fb), ctypes.byref(need)) == 0 and need.value > 0
    ws = np.zeros(need.value + 256, dtype=np.uint8)
    ws_ptr = (ws.ctypes.data + 255) & ~255
    return fb, [o.ctypes.data for o in out], ws_ptr, need.value, (ei, sc, nf, out, ws)


def test_frontier_abi_argument_checks():
    L = _lib.lib()
    NULL, ARG, WORKSPACE = -1, -6, -4
    fb, outs, ws, need, keep = _abi_case()
    assert L.gnnmp_frontier_workspace_bytes(None, ctypes.byref(ctypes.c_size_t())) == NULL
    assert L.gnnmp_frontier_workspace_bytes(ctypes.byref(fb), None) == NULL
    assert L.gnnmp_frontier_rank(None, *outs, ws, need, None) == NULL
    for i in range(5):                                               # each output pointer, then the workspace
        args = list(outs)
        args[i] = None
        assert L.gnnmp_frontier_rank(ctypes.byref(fb), *args, ws, need, None) == NULL
    assert L.gnnmp_frontier_rank(ctypes.byref(fb), *outs, None, need, None) == NULL
    for field in ('edge_index', 'scores', 'n_free'):
        fb2, *_ = _abi_case()
        setattr(fb2, field, None)
        assert L.gnnmp_frontier_rank(ctypes.byref(fb2), *outs, ws, need, None) == NULL, field
    fb2, *_ = _abi_case()                                            # prefix arrays may be left out for ONE graph only
    fb2.n_graphs = 2
    assert L.gnnmp_frontier_rank(ctypes.byref(fb2), *outs, ws, need, None) == NULL
    for field in ('n_graphs', 'total_nodes', 'total_edges'):
        fb2, *_ = _abi_case()
        setattr(fb2, field, -1 if field != 'n_graphs' else 0)
        assert L.gnnmp_frontier_workspace_bytes(ctypes.byref(fb2), ctypes.byref(ctypes.c_size_t())) == ARG, field
        assert L.gnnmp_frontier_rank(ctypes.byref(fb2), *outs, ws, need, None) == ARG, field
    assert L.gnnmp_frontier_rank(ctypes.byref(fb), *outs, ws, need - 1, None) == WORKSPACE
    assert L.gnnmp_frontier_rank(ctypes.byref(fb), *outs, ws + 4, need, None) == WORKSPACE      # misaligned
    w, t = ctypes.c_int32(), ctypes.c_int32()
    assert L.gnnmp_frontier_limits(None, ctypes.byref(t)) == NULL and L.gnnmp_frontier_limits(ctypes.byref(w), None) == NULL
    assert L.gnnmp_frontier_limits(ctypes.byref(w), ctypes.byref(t)) == 0 and 64 <= w.value < t.value


def test_frontier_batch_mirrors_the_header():
    """Field names and order of gnnmp_frontier_batch against the ctypes mirror (as test_abi_symbols does for the others)."""
    import re
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(repo, 'include', 'gnnmp.h')).read(), flags=re.S)
    body = re.search(r'typedef struct\s*\{([^}]*)\}\s*gnnmp_frontier_batch;', text).group(1)
    names = []
    for decl in body.split(';'):
        if decl.strip():
            parts = decl.strip().split(',')
            names.extend([parts[0].split()[-1].lstrip('*')] + [x.strip().lstrip('*') for x in parts[1:]])
    assert names == [f[0] for f in _lib.FrontierBatch._fields_]
    assert ctypes.sizeof(_lib.FrontierBatch) == 16 + 5 * 8
