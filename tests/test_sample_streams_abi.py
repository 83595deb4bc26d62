"""Argument checks of the three entries of the batched resample rounds (gnnmp_maze_sample_streams, gnnmp_maze_rounds_gather,
gnnmp_maze_rounds_carry): they come before any device work, so no GPU is needed and nothing is launched (the pointers handed
over are not device memory)."""
import ctypes

import numpy as np

import gnnmp  # noqa: F401
from gnnmp import _lib

ERR_NULL, ERR_DIMS, ERR_ARG = -1, -2, -6
FAKE = 4096


def _batch(n_problems=2, width=15, n_free=8, cap=24, n_attempts=64, attempts=FAKE, att_ptr=FAKE, att_ptr_host=None, maps=FAKE,
           init=FAKE, goal=FAKE, active=None):
    return _lib.MazeStreamsBatch(n_problems, width, n_free, cap, n_attempts, attempts, att_ptr, att_ptr_host, maps, init, goal,
                                 active)


def _sample(sb, dim=2, free_pool=FAKE, n_free=FAKE, coll_pool=FAKE, n_coll=FAKE, used=FAKE, checks=FAKE, status=FAKE):
    p = lambda x: None if x is None else ctypes.c_void_p(x)      # noqa: E731
    return _lib.lib().gnnmp_maze_sample_streams(ctypes.byref(sb) if sb is not None else None, dim, p(free_pool), p(n_free),
                                                p(coll_pool), p(n_coll), p(used), p(checks), p(status), None)


def _state(n_problems=2, cap=24, pair_cap=100, **null):
    names = [f[0] for f in _lib.MazeRoundsState._fields_[3:]]
    return _lib.MazeRoundsState(n_problems, cap, pair_cap, *[None if null.get(f) else FAKE for f in names])


def test_symbols_are_exported_and_structs_mirror_the_header():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gnnmp_maze_sample_streams', 'gnnmp_maze_rounds_gather', 'gnnmp_maze_rounds_carry'):
        assert hasattr(L, name), name
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gnnmp.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for cname, cls in (('gnnmp_maze_streams_batch', _lib.MazeStreamsBatch), ('gnnmp_maze_rounds_state', _lib.MazeRoundsState)):
        body = re.search(r'typedef struct\s*\{([^}]*)\}\s*%s;' % cname, text).group(1)
        fields = []
        for decl in body.split(';'):
            if decl.strip():
                fields.extend(x.split()[-1].lstrip('*') for x in decl.split(','))
        assert [f[0] for f in cls._fields_] == fields, cname


def test_sample_streams_dim():
    for dim in (0, 1, 4, -2):
        assert _sample(_batch(), dim=dim) == ERR_DIMS


def test_sample_streams_null_pointers():
    assert _sample(None) == ERR_NULL
    for name in ('free_pool', 'n_free', 'coll_pool', 'n_coll', 'used', 'checks', 'status'):
        assert _sample(_batch(), **{name: None}) == ERR_NULL, name
    for name in ('attempts', 'att_ptr', 'maps', 'init', 'goal'):
        assert _sample(_batch(**{name: None}), dim=3) == ERR_NULL, name


def test_sample_streams_counts():
    for kw in (dict(n_free=0), dict(n_free=-1), dict(n_free=9, cap=8), dict(width=0), dict(n_problems=0), dict(n_attempts=-1)):
        assert _sample(_batch(**kw)) == ERR_ARG, kw


def test_sample_streams_att_ptr_host():
    for ptr in ([0, 40, 39], [-1, 10, 20], [0, 10, 65], [5, 4, 64]):
        h = np.array(ptr, dtype=np.int64)
        assert _sample(_batch(att_ptr_host=h.ctypes.data)) == ERR_ARG, ptr


def _gather(st, dim=2, v_rows=10, v=FAKE, node_ptr=FAKE, n_free=FAKE, slot=FAKE, resume=None, n_active=2):
    p = lambda x: None if x is None else ctypes.c_void_p(x)      # noqa: E731
    return _lib.lib().gnnmp_maze_rounds_gather(ctypes.byref(st) if st is not None else None, dim, None, n_active, v_rows, p(v),
                                               p(node_ptr), p(n_free), p(slot), ctypes.byref(resume) if resume is not None else None, None)


def test_gather_checks():
    assert _gather(_state(), dim=4) == ERR_DIMS
    assert _gather(None) == ERR_NULL
    for name in ('v', 'node_ptr', 'n_free', 'slot'):
        assert _gather(_state(), **{name: None}) == ERR_NULL, name
    for name in ('free_pool', 'coll_pool', 'n_free', 'n_coll'):
        assert _gather(_state(**{name: True})) == ERR_NULL, name
    assert _gather(_state(), resume=_lib.MazeResume(FAKE, FAKE, None, FAKE, FAKE, FAKE)) == ERR_NULL
    assert _gather(_state(tree_prev=True), resume=_lib.MazeResume(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE)) == ERR_NULL
    assert _gather(_state(n_problems=0)) == ERR_ARG
    assert _gather(_state(cap=0)) == ERR_ARG
    assert _gather(_state(pair_cap=0)) == ERR_ARG
    assert _gather(_state(n_problems=1 << 20, pair_cap=1 << 20)) == ERR_ARG
    assert _gather(_state(), v_rows=-1) == ERR_ARG
    assert _gather(_state(), n_active=0) == ERR_ARG
    assert _gather(_state(), n_active=3) == ERR_ARG


def _carry(st, n_active=2, **null):
    names = ('slot_of', 'node_ptr', 'edge_ptr', 'success', 'n_explored', 'explored', 'prev', 'n_pairs', 'explored_edges', 'path_len',
             'path', 'checks', 'status')
    args = [None if null.get(f) else ctypes.c_void_p(FAKE) for f in names]
    return _lib.lib().gnnmp_maze_rounds_carry(ctypes.byref(st) if st is not None else None, n_active, *args, None)


def test_carry_checks():
    assert _carry(None) == ERR_NULL
    for name in ('node_ptr', 'edge_ptr', 'success', 'n_explored', 'explored', 'prev', 'n_pairs', 'explored_edges', 'path_len', 'path',
                 'checks', 'status'):
        assert _carry(_state(), **{name: True}) == ERR_NULL, name
    for name in [f[0] for f in _lib.MazeRoundsState._fields_[3:]]:
        assert _carry(_state(**{name: True})) == ERR_NULL, name
    assert _carry(_state(), n_active=0) == ERR_ARG
    assert _carry(_state(), n_active=3) == ERR_ARG
    assert _carry(_state(pair_cap=0)) == ERR_ARG
