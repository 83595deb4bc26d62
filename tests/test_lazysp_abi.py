"""Argument checks of the LazySP entry points (gnnmp_lazysp_pair_cap / _sample / _gather / _workspace_bytes / _round): they come
before any device work, so no GPU is needed and nothing is launched (the pointers handed over are not device memory)."""
import ctypes
import os
import re

import numpy as np

import gnnmp  # noqa: F401
from gnnmp import _lib, lazysp

ERR_NULL, ERR_DIMS, ERR_WORKSPACE, ERR_ARG = -1, -2, -4, -6
FAKE = 4096
STATE_FIELDS = [f[0] for f in _lib.LazySPState._fields_[3:]]


def _p(x):
    return None if x is None else ctypes.c_void_p(x)


def _state(n_problems=2, cap=24, pair_cap=100, **null):
    return _lib.LazySPState(n_problems, cap, pair_cap, *[None if null.get(f) else FAKE for f in STATE_FIELDS])


def _batch(n_problems=2, width=15, n_free=8, cap=24, n_attempts=64, attempts=FAKE, att_ptr=FAKE, att_ptr_host=None, maps=FAKE,
           init=FAKE, goal=FAKE, active=None):
    return _lib.MazeStreamsBatch(n_problems, width, n_free, cap, n_attempts, attempts, att_ptr, att_ptr_host, maps, init, goal, active)


def test_symbols_are_exported_and_the_struct_mirrors_the_header():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gnnmp_lazysp_pair_cap', 'gnnmp_lazysp_sample', 'gnnmp_lazysp_gather', 'gnnmp_lazysp_workspace_bytes',
                 'gnnmp_lazysp_lds_nodes', 'gnnmp_lazysp_round'):
        assert hasattr(L, name), name
    assert _lib.lib().gnnmp_abi_version() == _lib.ABI_VERSION >= 5
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gnnmp.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    body = re.search(r'typedef struct\s*\{([^}]*)\}\s*gnnmp_lazysp_state;', text).group(1)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            fields.extend(x.split()[-1].lstrip('*') for x in decl.split(','))
    assert [f[0] for f in _lib.LazySPState._fields_] == fields


def _pair_cap(batch, k1s, out=True):
    arr = np.asarray(k1s, dtype=np.int32)
    cap = ctypes.c_int64(-1)
    rc = _lib.lib().gnnmp_lazysp_pair_cap(batch, len(k1s), arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if k1s is not None else None,
                                          ctypes.byref(cap) if out else None)
    return rc, cap.value


def test_pair_cap_helper():
    """The C helper and lazysp.rounds_pair_cap are the same derived bound: sum over the rounds of min(k1 N, N (N - 1) / 2)."""
    for batch, t_max, k in ((50, 1000, 10), (50, 300, 10), (20, 100, 10), (1, 6, 10), (7, 20, 2), (61, 61, 10), (3, 9, 40)):
        R = lazysp.n_rounds(batch, t_max)
        ns = [2 + r * batch for r in range(1, R + 1)]
        k1s = [lazysp.k1_of(k, n) for n in ns]
        want = sum(min(min(k1, n) * n, n * (n - 1) // 2) for k1, n in zip(k1s, ns))
        assert lazysp.rounds_pair_cap(batch, t_max, k) == want
        assert _pair_cap(batch, k1s) == (0, want)
    assert _pair_cap(1, [3]) == (0, 3)                          # N = 3: the three pairs of a triangle
    assert lazysp.k1_of(10, 100) == 10 and lazysp.k1_of(10, 52) == 9 and lazysp.k1_of(10, 1002) == 16
    assert _pair_cap(0, [3])[0] == ERR_ARG
    assert _pair_cap(5, [3, 0])[0] == ERR_ARG
    assert _pair_cap(5, [3], out=False)[0] == ERR_NULL
    assert _lib.lib().gnnmp_lazysp_pair_cap(5, 1, None, ctypes.byref(ctypes.c_int64())) == ERR_NULL
    assert _lib.lib().gnnmp_lazysp_pair_cap(5, 0, np.zeros(1, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                            ctypes.byref(ctypes.c_int64())) == ERR_ARG
    assert _pair_cap(30000, [30000] * 8)[0] == ERR_ARG           # beyond 2^30 entries


def _sample(sb, st, dim=2, used=FAKE, checks=FAKE, status=FAKE):
    return _lib.lib().gnnmp_lazysp_sample(ctypes.byref(sb) if sb is not None else None, dim, ctypes.byref(st) if st is not None else None,
                                          _p(used), _p(checks), _p(status), None)


def test_sample_checks():
    for dim in (0, 1, 4, -2):
        assert _sample(_batch(), _state(), dim=dim) == ERR_DIMS
    assert _sample(None, _state()) == ERR_NULL
    assert _sample(_batch(), None) == ERR_NULL
    for name in ('used', 'checks', 'status'):
        assert _sample(_batch(), _state(), **{name: None}) == ERR_NULL, name
    for name in ('attempts', 'att_ptr', 'maps', 'init', 'goal'):
        assert _sample(_batch(**{name: None}), _state(), dim=3) == ERR_NULL, name
    for name in ('pool', 'n_nodes', 'checks'):
        assert _sample(_batch(), _state(**{name: True})) == ERR_NULL, name
    for kw in (dict(n_free=0), dict(n_free=-1), dict(n_free=25), dict(width=0), dict(n_problems=0), dict(n_problems=3),
               dict(n_attempts=-1)):
        assert _sample(_batch(**kw), _state()) == ERR_ARG, kw
    assert _sample(_batch(), _state(cap=0)) == ERR_ARG
    assert _sample(_batch(), _state(pair_cap=0)) == ERR_ARG
    for ptr in ([0, 40, 39], [-1, 10, 20], [0, 10, 65], [5, 4, 64]):
        h = np.array(ptr, dtype=np.int64)
        assert _sample(_batch(att_ptr_host=h.ctypes.data), _state()) == ERR_ARG, ptr


def _gather(st, dim=2, n_active=2, slot_of=FAKE, k1_table=FAKE, v_rows=10, v=FAKE, node_ptr=FAKE, n_free=FAKE, k1=FAKE):
    return _lib.lib().gnnmp_lazysp_gather(ctypes.byref(st) if st is not None else None, dim, n_active, _p(slot_of), _p(k1_table), v_rows,
                                          _p(v), _p(node_ptr), _p(n_free), _p(k1), None)


def test_gather_checks():
    assert _gather(_state(), dim=4) == ERR_DIMS
    assert _gather(None) == ERR_NULL
    for name in ('slot_of', 'k1_table', 'v', 'node_ptr', 'n_free', 'k1'):
        assert _gather(_state(), **{name: None}) == ERR_NULL, name
    for name in ('pool', 'n_nodes'):
        assert _gather(_state(**{name: True})) == ERR_NULL, name
    for st in (_state(n_problems=0), _state(cap=0), _state(pair_cap=0), _state(n_problems=1 << 20, pair_cap=1 << 20)):
        assert _gather(st) == ERR_ARG
    assert _gather(_state(), v_rows=-1) == ERR_ARG
    assert _gather(_state(), n_active=0) == ERR_ARG
    assert _gather(_state(), n_active=3) == ERR_ARG


def test_workspace_bytes():
    L = _lib.lib()
    need = ctypes.c_size_t()
    assert L.gnnmp_lazysp_workspace_bytes(2, 24, 100, None) == ERR_NULL
    for args in ((0, 24, 100), (2, 0, 100), (2, 24, -1)):
        assert L.gnnmp_lazysp_workspace_bytes(*args, ctypes.byref(need)) == ERR_ARG, args
    assert L.gnnmp_lazysp_workspace_bytes(2, 24, 100, ctypes.byref(need)) == 0
    # per edge a float64 cost and a flag, per problem (cap + 3) x (dist 8 + prev 4 + block starts 4) bytes
    assert need.value >= 100 * 9 + 2 * 27 * 16 and need.value % 256 == 0
    small = need.value
    assert L.gnnmp_lazysp_workspace_bytes(2, 24, 100000, ctypes.byref(need)) == 0 and need.value > small
    assert L.gnnmp_lazysp_lds_nodes() >= 64


def _round(st, dim=2, n_active=2, slot_of=FAKE, ei=FAKE, total=100, edge_ptr=FAKE, maps=FAKE, width=15, ws=FAKE, ws_bytes=1 << 20):
    return _lib.lib().gnnmp_lazysp_round(ctypes.byref(st) if st is not None else None, dim, n_active, _p(slot_of), _p(ei), total,
                                         _p(edge_ptr), _p(maps), width, _p(ws), ws_bytes, None)


def test_round_checks():
    assert _round(_state(), dim=1) == ERR_DIMS
    assert _round(None) == ERR_NULL
    for name in ('ei', 'edge_ptr', 'maps', 'ws'):
        assert _round(_state(), **{name: None}) == ERR_NULL, name
    for name in STATE_FIELDS:
        assert _round(_state(**{name: True})) == ERR_NULL, name
    for kw in (dict(n_active=0), dict(n_active=3), dict(width=0), dict(total=-1)):
        assert _round(_state(), **kw) == ERR_ARG, kw
    assert _round(_state(pair_cap=0)) == ERR_ARG
    need = ctypes.c_size_t()
    assert _lib.lib().gnnmp_lazysp_workspace_bytes(2, 24, 100, ctypes.byref(need)) == 0
    assert _round(_state(), ws_bytes=need.value - 1) == ERR_WORKSPACE
    assert _round(_state(), ws=FAKE + 8) == ERR_WORKSPACE       # not 256-byte aligned
