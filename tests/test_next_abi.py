"""Argument checks of the NEXT network entry points (gnnmp_next_weights_floats / _pb_forward / _state_forward): they come before
any device work, so no GPU is needed and nothing is launched (the pointers handed over are not device memory)."""
import ctypes
import os
import re

import numpy as np

import gnnmp  # noqa: F401
from gnnmp import _lib, next_model

ERR_NULL, ERR_DIMS, ERR_ARG = -1, -2, -6
FAKE = 4096
PB_PTRS = [f[0] for f in _lib.NextPbForward._fields_[4:]]
ST_PTRS = [f[0] for f in _lib.NextStateForward._fields_[4:]]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _pb(n_problems=2, dim=2, width=15, iters=20, **null):
    return _lib.NextPbForward(n_problems, dim, width, iters, *[None if null.get(f) else FAKE for f in PB_PTRS])


def _st(n_states=3, n_problems=2, dim=2, width=15, **null):
    return _lib.NextStateForward(n_states, n_problems, dim, width, *[None if null.get(f) else FAKE for f in ST_PTRS])


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
    for name in ('gnnmp_next_weights_floats', 'gnnmp_next_pb_forward', 'gnnmp_next_state_forward'):
        assert hasattr(L, name), name
    assert _lib.lib().gnnmp_abi_version() == _lib.ABI_VERSION >= 8
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gnnmp.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert [f[0] for f in _lib.NextPbForward._fields_] == _struct_fields(text, 'gnnmp_next_pb')
    assert [f[0] for f in _lib.NextStateForward._fields_] == _struct_fields(text, 'gnnmp_next_states')


def test_weights_floats_matches_the_packer():
    n = ctypes.c_size_t(7)
    L = _lib.lib()
    assert L.gnnmp_next_weights_floats(2, None) == ERR_NULL
    for dim in (0, 1, 4, -3):
        assert L.gnnmp_next_weights_floats(dim, ctypes.byref(n)) == ERR_DIMS, dim
    for dim in (2, 3):
        assert L.gnnmp_next_weights_floats(dim, ctypes.byref(n)) == 0
        with np.load(os.path.join(GOLDEN, 'next_%d_weights.npz' % dim)) as f:
            packed = next_model.pack_weights({k: f[k] for k in f.files}, dim)
        assert packed.shape == (n.value,) and packed.dtype == np.float32


def test_pb_forward_checks_come_before_any_launch():
    fn = 'gnnmp_next_pb_forward'
    assert _call(fn, None) == ERR_NULL
    for dim in (0, 1, 4, -2):
        assert _call(fn, _pb(dim=dim)) == ERR_DIMS, dim
    for width in (0, 14, 16, -15):
        assert _call(fn, _pb(width=width)) == ERR_DIMS, width
    assert _call(fn, _pb(n_problems=-1)) == ERR_ARG
    assert _call(fn, _pb(iters=-1)) == ERR_ARG
    for dim in (2, 3):
        for name in PB_PTRS:
            assert _call(fn, _pb(dim=dim, **{name: True})) == ERR_NULL, name
    assert _call(fn, _pb(n_problems=0)) == 0                      # a successful no-op: the fake pointers are never touched
    assert _call(fn, _pb(n_problems=0, iters=0, dim=3)) == 0


def test_state_forward_checks_come_before_any_launch():
    fn = 'gnnmp_next_state_forward'
    assert _call(fn, None) == ERR_NULL
    for dim in (0, 1, 4, -2):
        assert _call(fn, _st(dim=dim)) == ERR_DIMS, dim
    for width in (0, 14, 16):
        assert _call(fn, _st(width=width)) == ERR_DIMS, width
    assert _call(fn, _st(n_states=-1)) == ERR_ARG
    assert _call(fn, _st(n_problems=-1)) == ERR_ARG
    for dim in (2, 3):
        for name in ST_PTRS:
            assert _call(fn, _st(dim=dim, **{name: True})) == ERR_NULL, name
    assert _call(fn, _st(n_states=0)) == 0
    assert _call(fn, _st(n_states=0, n_problems=0, dim=3)) == 0
