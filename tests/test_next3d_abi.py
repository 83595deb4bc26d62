"""Argument checks of the 3-D NEXT network entry points (gnnmp_next3d_weights_floats / _workspace_bytes / _pb_forward /
_state_forward): they come before any device work, so no GPU is needed and nothing is launched (the pointers handed over are not
device memory; every call here is either refused or a no-op)."""
import ctypes
import os
import re

import gnnmp  # noqa: F401
from gnnmp import _lib

ERR_NULL, ERR_DIMS, ERR_ARG = -1, -2, -6
FAKE = 4096
PB_PTRS = ['maps', 'goals', 'weights', 'pb_rep', 'workspace']
ST_PTRS = [f[0] for f in _lib.Next3dStateForward._fields_[5:]]


def _ws_bytes(n):
    b = ctypes.c_size_t()
    assert _lib.lib().gnnmp_next3d_workspace_bytes(n, ctypes.byref(b)) == 0
    return b.value


def _pb(n_problems=2, dim=7, point_dim=3, width=15, iters=20, workspace_bytes=None, **null):
    if workspace_bytes is None:
        workspace_bytes = _ws_bytes(max(n_problems, 0))
    ptrs = [None if null.get(f) else FAKE for f in PB_PTRS]
    return _lib.Next3dPbForward(n_problems, dim, point_dim, width, iters, *ptrs, workspace_bytes)


def _st(n_states=3, n_problems=2, dim=7, point_dim=3, width=15, **null):
    return _lib.Next3dStateForward(n_states, n_problems, dim, point_dim, width, *[None if null.get(f) else FAKE for f in ST_PTRS])


def _call(fn, d):
    return getattr(_lib.lib(), fn)(ctypes.byref(d) if d is not None else None, None)


def _struct_fields(text, name):
    body = re.search(r'typedef struct\s*\{([^}]*)\}\s*%s;' % name, text).group(1)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            fields.extend(x.split()[-1].lstrip('*') for x in decl.split(','))
    return fields


def test_symbols_abi_version_and_structs_mirror_the_header():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gnnmp_next3d_weights_floats', 'gnnmp_next3d_workspace_bytes', 'gnnmp_next3d_pb_forward',
                 'gnnmp_next3d_state_forward'):
        assert hasattr(L, name), name
    assert _lib.lib().gnnmp_abi_version() == _lib.ABI_VERSION == 9          # additive: the version did not move
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gnnmp.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert [f[0] for f in _lib.Next3dPbForward._fields_] == _struct_fields(text, 'gnnmp_next3d_pb')
    assert [f[0] for f in _lib.Next3dStateForward._fields_] == _struct_fields(text, 'gnnmp_next3d_states')
    assert PB_PTRS == [f[0] for f in _lib.Next3dPbForward._fields_[5:10]]


def test_weights_floats_and_workspace_bytes():
    L = _lib.lib()
    n = ctypes.c_size_t(7)
    assert L.gnnmp_next3d_weights_floats(7, 3, None) == ERR_NULL
    for dim, pd in ((0, 3), (16, 3), (-1, 3), (7, 2), (7, 0), (7, 4), (14, 9)):
        assert L.gnnmp_next3d_weights_floats(dim, pd, ctypes.byref(n)) == ERR_DIMS, (dim, pd)
    counts = set()
    for dim, pd in ((1, 3), (6, 3), (7, 3), (13, 3), (14, 6), (15, 6)):
        assert L.gnnmp_next3d_weights_floats(dim, pd, ctypes.byref(n)) == 0
        counts.add(n.value)
    assert len(counts) == 1 and counts.pop() > 3 * 27 * 64 * 64
    assert L.gnnmp_next3d_workspace_bytes(1, None) == ERR_NULL
    assert L.gnnmp_next3d_workspace_bytes(-1, ctypes.byref(n)) == ERR_ARG
    sizes = [_ws_bytes(b) for b in (0, 1, 2, 3, 16, 64)]
    assert sizes[0] == 0 and all(a < b for a, b in zip(sizes, sizes[1:]))      # monotone in B
    assert sizes[1] >= 4 * 3375 * 64 * 4 and sizes[1] % 16 == 0                # h twice, c and the hidden layer at least


def test_pb_forward_checks_come_before_any_launch():
    fn = 'gnnmp_next3d_pb_forward'
    assert _call(fn, None) == ERR_NULL
    for dim in (0, 16, -2):
        assert _call(fn, _pb(dim=dim)) == ERR_DIMS, dim
    for pd in (0, 2, 4, 9):
        assert _call(fn, _pb(point_dim=pd)) == ERR_DIMS, pd
    for width in (0, 14, 16, -15):
        assert _call(fn, _pb(width=width)) == ERR_DIMS, width
    assert _call(fn, _pb(dim=0, n_problems=-1)) == ERR_DIMS          # the dimensions before the counts
    assert _call(fn, _pb(n_problems=-1)) == ERR_ARG
    assert _call(fn, _pb(iters=-1)) == ERR_ARG
    assert _call(fn, _pb(workspace_bytes=_ws_bytes(2) - 1)) == ERR_ARG
    assert _call(fn, _pb(n_problems=3, workspace_bytes=_ws_bytes(2))) == ERR_ARG
    d = _pb()
    d.workspace = FAKE + 4                                           # not 16-byte aligned
    assert _call(fn, d) == ERR_ARG
    assert _call(fn, _pb(iters=-1, maps=True)) == ERR_ARG            # the counts before the arrays
    for dim, pd in ((7, 3), (14, 6)):
        for name in PB_PTRS:
            assert _call(fn, _pb(dim=dim, point_dim=pd, **{name: True})) == ERR_NULL, name
    assert _call(fn, _pb(n_problems=0)) == 0                         # a successful no-op: the fake pointers are never touched
    assert _call(fn, _pb(n_problems=0, iters=0, dim=14, point_dim=6, workspace_bytes=0)) == 0


def test_state_forward_checks_come_before_any_launch():
    fn = 'gnnmp_next3d_state_forward'
    assert _call(fn, None) == ERR_NULL
    for dim in (0, 16, -2):
        assert _call(fn, _st(dim=dim)) == ERR_DIMS, dim
    for pd in (0, 2, 5):
        assert _call(fn, _st(point_dim=pd)) == ERR_DIMS, pd
    for width in (0, 14, 16):
        assert _call(fn, _st(width=width)) == ERR_DIMS, width
    assert _call(fn, _st(n_states=-1)) == ERR_ARG
    assert _call(fn, _st(n_problems=-1)) == ERR_ARG
    assert _call(fn, _st(n_states=-1, y=True)) == ERR_ARG            # the counts before the arrays
    for dim, pd in ((6, 3), (14, 6)):
        for name in ST_PTRS:
            assert _call(fn, _st(dim=dim, point_dim=pd, **{name: True})) == ERR_NULL, name
    assert _call(fn, _st(n_states=0)) == 0
    assert _call(fn, _st(n_states=0, n_problems=0, dim=13)) == 0
