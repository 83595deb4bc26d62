"""Argument checks of the 3-D NEXT training entry points (gnnmp_next3d_train_workspace_bytes / _weights_t_floats /
_train_forward / _state_backward / _pb_backward), no GPU.

As tests/test_next_train_abi.py: every call here ends at an argument error, at the no-work return or at the workspace check, and
every one of those comes before the first HIP call of its entry point: the pointers handed over are not device memory (address
4096), and no call passes all checks with non-zero work, so nothing is ever launched or written.  The no-work calls must return
0: on a machine without a GPU any HIP call fails with GNNMP_ERR_HIP, so a 0 there shows that none was made."""
import ctypes
import os
import re

import numpy as np
import pytest

import gnnmp  # noqa: F401
from gnnmp import _lib

ERR_NULL, ERR_DIMS, ERR_WORKSPACE, ERR_ARG = -1, -2, -4, -6
FAKE = 4096
FWD_PTRS = [f[0] for f in _lib.Next3dTrain._fields_[6:-1]]
BWD_PTRS = [f[0] for f in _lib.Next3dTrainBwd._fields_[6:-1]]
BIG = 1 << 44
DIMS = ((7, 3), (14, 6), (1, 3), (15, 6))


def _fwd(n_problems=2, n_states=3, dim=7, point_dim=3, width=15, iters=20, ws=FAKE, ws_bytes=BIG, **null):
    ptrs = [None if null.get(f) else FAKE for f in FWD_PTRS]
    ptrs[-1] = None if null.get('workspace') else ws
    return _lib.Next3dTrain(n_problems, n_states, dim, point_dim, width, iters, *ptrs, ws_bytes)


def _bwd(n_problems=2, n_states=3, dim=7, point_dim=3, width=15, iters=20, ws=FAKE, ws_bytes=BIG, **null):
    ptrs = [None if null.get(f) else FAKE for f in BWD_PTRS]
    ptrs[-1] = None if null.get('workspace') else ws
    return _lib.Next3dTrainBwd(n_problems, n_states, dim, point_dim, width, iters, *ptrs, ws_bytes)


def _call(fn, d):
    return getattr(_lib.lib(), fn)(ctypes.byref(d) if d is not None else None, None)


def _bytes(b, it, s):
    n = ctypes.c_size_t(7)
    assert _lib.lib().gnnmp_next3d_train_workspace_bytes(b, it, s, ctypes.byref(n)) == 0
    return int(n.value)


def _struct_fields(text, name):
    body = re.search(r'typedef struct\s*\{([^}]*)\}\s*%s;' % name, text).group(1)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            fields.extend(x.split()[-1].lstrip('*') for x in decl.split(','))
    return fields


def test_symbols_and_structs_mirror_the_header():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gnnmp_next3d_train_workspace_bytes', 'gnnmp_next3d_weights_t_floats', 'gnnmp_next3d_train_forward',
                 'gnnmp_next3d_state_backward', 'gnnmp_next3d_pb_backward'):
        assert hasattr(L, name), name
    assert _lib.lib().gnnmp_abi_version() == _lib.ABI_VERSION
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gnnmp.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert [f[0] for f in _lib.Next3dTrain._fields_] == _struct_fields(text, 'gnnmp_next3d_train')
    assert [f[0] for f in _lib.Next3dTrainBwd._fields_] == _struct_fields(text, 'gnnmp_next3d_train_bwd')
    assert _lib.Next3dTrain._fields_[-1][1] is ctypes.c_size_t and _lib.Next3dTrainBwd._fields_[-1][1] is ctypes.c_size_t


def test_workspace_bytes_is_zero_safe_increasing_aligned_and_does_not_wrap():
    L = _lib.lib()
    n = ctypes.c_size_t(7)
    assert L.gnnmp_next3d_train_workspace_bytes(1, 1, 1, None) == ERR_NULL
    for args in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        assert L.gnnmp_next3d_train_workspace_bytes(*args, ctypes.byref(n)) == ERR_ARG, args
    assert _bytes(0, 0, 0) % 256 == 0
    for b, it, s in ((0, 0, 0), (1, 0, 0), (0, 5, 0), (0, 0, 3), (2, 20, 13), (64, 20, 640), (1 << 20, 20, 1 << 22)):
        base = _bytes(b, it, s)
        assert base % 256 == 0, (b, it, s)
        assert _bytes(b + 1, it, s) > base and _bytes(b, it, s + 1) > base, (b, it, s)
        if b > 0:
            assert _bytes(b, it + 1, s) > base, (b, it, s)
        else:
            assert _bytes(b, it + 1, s) >= base
    # the saved rows: x9 and the hidden layer, h and c of rounds + 1 slots, the conv output of every round, each with a zero row
    slot = 3376 * 64
    saved = 4 * (3376 * 16 + slot * (1 + 2 * 21 + 20))
    assert _bytes(3, 20, 0) - _bytes(2, 20, 0) >= saved
    assert _bytes(1 << 20, 20, 0) > (1 << 20) * saved > 1 << 45                 # computed in size_t: no 32-bit wrap
    from gnnmp import next_train3d
    for dim, pd in DIMS:
        assert L.gnnmp_next3d_weights_t_floats(dim, pd, None) == ERR_NULL
        assert L.gnnmp_next3d_weights_t_floats(dim, pd, ctypes.byref(n)) == 0 and n.value == 3 * 108 * 1024 + 128 * 256 + 64
        shapes = next_train3d.param_shapes(dim, pd)
        zeros = {k: np.zeros(s, dtype=np.float32) for k, s in shapes.items()}
        assert next_train3d.pack_weights_t(zeros).shape[0] == n.value
    for dim, pd in ((0, 3), (16, 3), (7, 4), (7, 0)):
        assert L.gnnmp_next3d_weights_t_floats(dim, pd, ctypes.byref(n)) == ERR_DIMS


@pytest.mark.parametrize('fn,make,ptrs', [('gnnmp_next3d_train_forward', _fwd, FWD_PTRS), ('gnnmp_next3d_state_backward', _bwd, BWD_PTRS),
                                          ('gnnmp_next3d_pb_backward', _bwd, BWD_PTRS)])
def test_checks_come_in_order_and_before_any_hip_call(fn, make, ptrs):
    assert _call(fn, None) == ERR_NULL
    for dim, pd in ((0, 3), (16, 3), (-2, 6), (7, 2), (7, 9)):
        assert _call(fn, make(dim=dim, point_dim=pd, n_problems=-1, goals=True)) == ERR_DIMS, (dim, pd)   # dims before counts and arrays
    for width in (0, 14, 16, -15):
        assert _call(fn, make(width=width, n_states=-1)) == ERR_DIMS, width
    for dim, pd in DIMS:
        for bad in ({'n_problems': -1}, {'n_states': -1}, {'iters': -1}):
            assert _call(fn, make(dim=dim, point_dim=pd, goals=True, **bad)) == ERR_ARG, bad             # counts before arrays
        for name in ptrs:
            assert _call(fn, make(dim=dim, point_dim=pd, **{name: True})) == ERR_NULL, name
            assert _call(fn, make(dim=dim, point_dim=pd, n_problems=0, n_states=0, **{name: True})) == ERR_NULL, name   # arrays before no work
        # no work: 0, and before the workspace check (the workspace is too small and misaligned here)
        assert _call(fn, make(dim=dim, point_dim=pd, n_problems=0, ws=FAKE + 8, ws_bytes=0)) == 0
        assert _call(fn, make(dim=dim, point_dim=pd, n_problems=0, n_states=0, iters=0, ws=FAKE + 8, ws_bytes=0)) == 0
        need = _bytes(2, 20, 3)
        if fn == 'gnnmp_next3d_state_backward':
            assert _call(fn, make(dim=dim, point_dim=pd, n_states=0, ws=FAKE + 8, ws_bytes=0)) == 0
        else:                                   # the problem side has work without rows: it gets as far as the workspace check
            assert _call(fn, make(dim=dim, point_dim=pd, n_states=0, ws_bytes=_bytes(2, 20, 0) - 1)) == ERR_WORKSPACE
        # work, but a workspace that is too small or misaligned: refused before any HIP call
        assert _call(fn, make(dim=dim, point_dim=pd, ws_bytes=need - 1)) == ERR_WORKSPACE
        assert _call(fn, make(dim=dim, point_dim=pd, ws_bytes=0)) == ERR_WORKSPACE
        assert _call(fn, make(dim=dim, point_dim=pd, ws=FAKE + 128, ws_bytes=BIG)) == ERR_WORKSPACE
        assert _call(fn, make(dim=dim, point_dim=pd, ws=FAKE + 4, ws_bytes=need)) == ERR_WORKSPACE
