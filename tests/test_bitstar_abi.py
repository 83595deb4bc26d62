"""Argument checks of the BIT* entry points (gnnmp_bitstar_sample / _workspace_bytes / _lds_nodes / _plan): they come before any
device work, so no GPU is needed and nothing is launched (the pointers handed over are not device memory)."""
import ctypes
import os
import re

import numpy as np

import gnnmp  # noqa: F401
from gnnmp import _lib

ERR_NULL, ERR_DIMS, ERR_WORKSPACE, ERR_ARG = -1, -2, -4, -6
FAKE = 4096
BATCH_PTRS = [f[0] for f in _lib.BITStarBatch._fields_[8:]]
RESULT_FIELDS = [f[0] for f in _lib.BITStarResult._fields_]
STREAM_PTRS = ('attempts', 'att_ptr', 'maps', 'init_states', 'goal_states')


def _batch(n_problems=2, dim=2, width=15, batch=5, n_batches=4, n_nodes=22, flags=0, edge_cap=44, **null):
    return _lib.BITStarBatch(n_problems, dim, width, batch, n_batches, n_nodes, flags, edge_cap,
                             *[None if null.get(f) else FAKE for f in BATCH_PTRS])


def _result(**null):
    return _lib.BITStarResult(*[None if null.get(f) else FAKE for f in RESULT_FIELDS])


def _plan(b, r, ws=FAKE, ws_bytes=1 << 30):
    return _lib.lib().gnnmp_bitstar_plan(ctypes.byref(b) if b is not None else None, ctypes.byref(r) if r is not None else None,
                                         None if ws is None else ctypes.c_void_p(ws), ws_bytes, None)


def _streams(n_problems=2, width=15, n_free=5, cap=22, n_attempts=100, att_ptr_host=None, **null):
    ptr = lambda f: None if null.get(f) else FAKE      # noqa: E731
    return _lib.MazeStreamsBatch(n_problems, width, n_free, cap, n_attempts, ptr('attempts'), ptr('att_ptr'),
                                 att_ptr_host.ctypes.data if att_ptr_host is not None else None, ptr('maps'), ptr('init_states'),
                                 ptr('goal_states'), None)


def _sample(sb, dim=2, n_batches=4, pool=FAKE, used=FAKE, checks=FAKE, status=FAKE):
    vp = lambda x: None if x is None else ctypes.c_void_p(x)      # noqa: E731
    return _lib.lib().gnnmp_bitstar_sample(ctypes.byref(sb) if sb is not None else None, dim, n_batches, vp(pool), vp(used), vp(checks),
                                           vp(status), None)


def _struct_fields(text, name):
    body = re.search(r'typedef struct\s*\{([^}]*)\}\s*%s;' % name, text).group(1)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            fields.extend(x.split()[-1].lstrip('*') for x in decl.split(','))
    return fields


def test_symbols_abi_version_and_structs_mirror_the_header():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gnnmp_bitstar_sample', 'gnnmp_bitstar_workspace_bytes', 'gnnmp_bitstar_lds_nodes', 'gnnmp_bitstar_plan'):
        assert hasattr(L, name), name
    assert _lib.lib().gnnmp_abi_version() == _lib.ABI_VERSION >= 7
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gnnmp.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert [f[0] for f in _lib.BITStarBatch._fields_] == _struct_fields(text, 'gnnmp_bitstar_batch')
    assert [f[0] for f in _lib.BITStarResult._fields_] == _struct_fields(text, 'gnnmp_bitstar_result')


def test_workspace_bytes_and_lds_nodes():
    L = _lib.lib()
    need = ctypes.c_size_t(7)
    assert L.gnnmp_bitstar_lds_nodes() >= 1002                   # batch 50 / t_max 1000 keeps its node state in LDS
    assert L.gnnmp_bitstar_workspace_bytes(2, 22, 44, None) == ERR_NULL
    for args in ((0, 22, 44), (-1, 22, 44), (2, 2, 1), (2, 0, 1), (2, 22, 0), (2, 22, -4), (2, 22, 22 * 21 + 1)):
        assert L.gnnmp_bitstar_workspace_bytes(*args, ctypes.byref(need)) == ERR_ARG, args
    assert L.gnnmp_bitstar_workspace_bytes(3, 1002, 2004, ctypes.byref(need)) == 0
    # per queue entry a float64 value and two int32 ids, per node a float64 value and a flag byte
    assert need.value >= 3 * (2004 * 16 + 1002 * 9) and need.value % 256 == 0
    small = need.value
    assert L.gnnmp_bitstar_workspace_bytes(3, 1002, 1002 * 1001, ctypes.byref(need)) == 0 and need.value > small
    assert L.gnnmp_bitstar_workspace_bytes(6, 1002, 2004, ctypes.byref(need)) == 0 and need.value > small


def test_plan_checks_come_before_any_launch():
    assert _plan(None, _result()) == ERR_NULL
    assert _plan(_batch(), None) == ERR_NULL
    for dim in (0, 1, 4, -2):
        assert _plan(_batch(dim=dim), _result()) == ERR_DIMS, dim
    for name in BATCH_PTRS:
        assert _plan(_batch(**{name: True}), _result()) == ERR_NULL, name
    for name in RESULT_FIELDS:
        assert _plan(_batch(dim=3), _result(**{name: True})) == ERR_NULL, name
    for kw in (dict(n_problems=0), dict(n_problems=-3), dict(width=0), dict(batch=0), dict(batch=-1), dict(n_batches=0),
               dict(n_nodes=21), dict(n_nodes=2, batch=1, n_batches=1), dict(edge_cap=0), dict(edge_cap=-1), dict(edge_cap=22 * 21 + 1),
               dict(flags=2), dict(flags=-1), dict(batch=2 ** 30, n_batches=2 ** 30)):
        assert _plan(_batch(**kw), _result()) == ERR_ARG, kw
    assert _plan(_batch(flags=1), _result(), ws=None) == ERR_NULL          # bit 0 is accepted; the edge queue always needs the workspace
    need = ctypes.c_size_t()
    assert _lib.lib().gnnmp_bitstar_workspace_bytes(2, 22, 44, ctypes.byref(need)) == 0 and need.value > 0
    assert _plan(_batch(), _result(), ws=FAKE, ws_bytes=need.value - 1) == ERR_WORKSPACE
    assert _plan(_batch(), _result(), ws=FAKE + 8, ws_bytes=need.value) == ERR_WORKSPACE


def test_sample_checks_come_before_any_launch():
    assert _sample(None) == ERR_NULL
    for dim in (0, 1, 4):
        assert _sample(_streams(), dim=dim) == ERR_DIMS, dim
    for name in STREAM_PTRS:
        assert _sample(_streams(**{name: True})) == ERR_NULL, name
    for name in ('pool', 'used', 'checks', 'status'):
        assert _sample(_streams(), **{name: None}) == ERR_NULL, name
    for kw in (dict(n_problems=0), dict(width=0), dict(n_free=0), dict(n_attempts=-1), dict(cap=21)):
        assert _sample(_streams(**kw)) == ERR_ARG, kw
    assert _sample(_streams(), n_batches=0) == ERR_ARG
    assert _sample(_streams(), n_batches=5) == ERR_ARG                     # 2 + 5 * 5 rows do not fit cap = 22
    for ptr in ([0, 60, 50], [-1, 50, 100], [0, 50, 101]):
        assert _sample(_streams(att_ptr_host=np.array(ptr, dtype=np.int64))) == ERR_ARG, ptr
