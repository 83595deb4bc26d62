"""Argument checks of the replay entry points (gnnmp_next_replay_append_trees / _append_paths, gnnmp_next_path_loss), no GPU.

As in tests/test_next_train_abi.py, every call here ends at an argument error or at the no-work return, and every one of those
comes before the first HIP call of its entry point: the pointers handed over are not device memory (address 4096) and no call
passes all checks with work to do, so nothing is ever launched or written.  The no-work calls must return 0: on a machine without
a GPU any HIP call fails with GNNMP_ERR_HIP, so a 0 there shows that none was made; on a machine with a GPU the same calls, run
in the process of the GPU tests, leave the fake pointers untouched for the same reason."""
import ctypes
import os
import re

import pytest

import gnnmp  # noqa: F401
from gnnmp import _lib

ERR_NULL, ERR_DIMS, ERR_ARG = -1, -2, -6
FAKE = 4096
STORE_PTRS = [f[0] for f in _lib.NextReplay._fields_[3:]]
TREE_PTRS = [f[0] for f in _lib.NextReplayTrees._fields_[2:]]
PATH_PTRS = [f[0] for f in _lib.NextReplayPaths._fields_[2:]]
LOSS_IN = ['y', 'actions', 'values', 'ptr']
LOSS_OUT = ['terms', 'loss', 'dy']


def _store(dim=2, cap_paths=4, cap_states=40, **null):
    return _lib.NextReplay(dim, cap_paths, cap_states, *[None if null.get(f) else FAKE for f in STORE_PTRS])


def _trees(n_problems=2, t_max=60, **null):
    return _lib.NextReplayTrees(n_problems, t_max, *[None if null.get(f) else FAKE for f in TREE_PTRS])


def _paths(n_paths=2, n_states=9, **null):
    return _lib.NextReplayPaths(n_paths, n_states, *[None if null.get(f) else FAKE for f in PATH_PTRS])


def _loss(n_paths=2, n_states=9, dim=2, divisor=8, **null):
    return _lib.NextPathLoss(n_paths, n_states, dim, divisor, *[None if null.get(f) else FAKE for f in LOSS_IN + LOSS_OUT])


def _append(fn, store, src):
    ref = lambda d: ctypes.byref(d) if d is not None else None      # noqa: E731
    return getattr(_lib.lib(), fn)(ref(store), ref(src), None)


def _path_loss(d):
    return _lib.lib().gnnmp_next_path_loss(ctypes.byref(d) if d is not None else None, None)


def _struct_fields(text, name):
    body = re.search(r'typedef struct\s*\{([^}]*)\}\s*%s;' % name, text).group(1)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            fields.extend(x.split()[-1].lstrip('*') for x in decl.split(','))
    return fields


def test_symbols_exist_abi_stays_and_structs_mirror_the_header():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gnnmp_next_replay_append_trees', 'gnnmp_next_replay_append_paths', 'gnnmp_next_path_loss'):
        assert hasattr(L, name), name
    assert _lib.lib().gnnmp_abi_version() == _lib.ABI_VERSION == 9
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gnnmp.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for cls, name in ((_lib.NextReplay, 'gnnmp_next_replay'), (_lib.NextReplayTrees, 'gnnmp_next_replay_trees'),
                      (_lib.NextReplayPaths, 'gnnmp_next_replay_paths'), (_lib.NextPathLoss, 'gnnmp_next_path_loss_desc')):
        assert [f[0] for f in cls._fields_] == _struct_fields(text, name), name


@pytest.mark.parametrize('fn,make,ptrs,count', [('gnnmp_next_replay_append_trees', _trees, TREE_PTRS, 'n_problems'),
                                                ('gnnmp_next_replay_append_paths', _paths, PATH_PTRS, 'n_paths')])
def test_append_checks_come_in_order_and_before_any_hip_call(fn, make, ptrs, count):
    assert _append(fn, None, make()) == ERR_NULL
    assert _append(fn, _store(), None) == ERR_NULL
    for dim in (0, 1, 4, -2):
        assert _append(fn, _store(dim=dim, cap_paths=-1, states64=True), make(**{count: -1})) == ERR_DIMS, dim      # dims first
    for dim in (2, 3):
        for bad in ({'cap_paths': -1}, {'cap_states': -1}):
            assert _append(fn, _store(dim=dim, counts=True, **bad), make()) == ERR_ARG, bad                         # counts before arrays
        assert _append(fn, _store(dim=dim, counts=True), make(**{count: -1})) == ERR_ARG
        second = 't_max' if count == 'n_problems' else 'n_states'
        assert _append(fn, _store(dim=dim), make(**{second: -1, ptrs[0]: True})) == ERR_ARG
        for name in STORE_PTRS:
            assert _append(fn, _store(dim=dim, **{name: True}), make()) == ERR_NULL, name
            assert _append(fn, _store(dim=dim, **{name: True}), make(**{count: 0})) == ERR_NULL, name               # arrays before no work
        for name in ptrs:
            assert _append(fn, _store(dim=dim), make(**{name: True})) == ERR_NULL, name
            assert _append(fn, _store(dim=dim), make(**{count: 0, name: True})) == ERR_NULL, name
        # no work: 0, nothing launched, nothing written -- whatever the capacities are
        assert _append(fn, _store(dim=dim), make(**{count: 0})) == 0
        assert _append(fn, _store(dim=dim, cap_paths=0, cap_states=0), make(**{count: 0})) == 0
    assert _append('gnnmp_next_replay_append_trees', _store(), _trees(t_max=2 ** 31 - 1)) == ERR_ARG                # t_max + 1 wraps
    assert _append('gnnmp_next_replay_append_trees', _store(), _trees(n_problems=0, t_max=0)) == 0


def test_path_loss_checks_come_in_order_and_before_any_hip_call():
    assert _path_loss(None) == ERR_NULL
    for dim in (0, 1, 4, -2):
        assert _path_loss(_loss(dim=dim, n_paths=-1, y=True)) == ERR_DIMS, dim
    for dim in (2, 3):
        for bad in ({'n_paths': -1}, {'n_states': -1}, {'divisor': 0}, {'divisor': -8}):
            assert _path_loss(_loss(dim=dim, y=True, **bad)) == ERR_ARG, bad
        for name in LOSS_IN:
            assert _path_loss(_loss(dim=dim, **{name: True})) == ERR_NULL, name
            assert _path_loss(_loss(dim=dim, n_paths=0, **{name: True})) == ERR_NULL, name                           # arrays before no work
        assert _path_loss(_loss(dim=dim, terms=True)) == ERR_NULL                                                    # loss needs terms
        assert _path_loss(_loss(dim=dim, n_paths=0, terms=True)) == ERR_NULL
        # no work: G = 0, or no output asked for
        assert _path_loss(_loss(dim=dim, n_paths=0)) == 0
        assert _path_loss(_loss(dim=dim, n_paths=0, n_states=0)) == 0
        assert _path_loss(_loss(dim=dim, terms=True, loss=True, dy=True)) == 0
        assert _path_loss(_loss(dim=dim, n_paths=0, terms=True, loss=True, dy=True)) == 0
