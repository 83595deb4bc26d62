"""Argument checks of the smoother's replay entry points (gnnmp_smooth_replay_append / _gather, gnnmp_smooth_path_loss), no GPU.

As in tests/test_next_replay_abi.py, every call here ends at an argument error or at the no-work return, and every one of those
comes before the first HIP call of its entry point: the pointers handed over are not device memory (address 4096) and no call
passes all checks with work to do, so nothing is ever launched or written.  The no-work calls must return 0: on a machine without
a GPU any HIP call fails with GNNMP_ERR_HIP, so a 0 there shows that none was made."""
import ctypes
import os
import re

import gnnmp  # noqa: F401
from gnnmp import _lib

ERR_NULL, ERR_DIMS, ERR_ARG = -1, -2, -6
FAKE = 4096
STORE_INTS = [f[0] for f in _lib.SmoothReplay._fields_[:6]]
STORE_PTRS = [f[0] for f in _lib.SmoothReplay._fields_[6:]]
SRC_PTRS = [f[0] for f in _lib.SmoothReplaySrc._fields_[4:]]
BATCH_PTRS = [f[0] for f in _lib.SmoothBatch._fields_[8:]]
LOSS_PTRS = [f[0] for f in _lib.SmoothPathLoss._fields_[4:]]


def _store(config_size=2, cap_samples=4, cap_path_rows=40, cap_free_rows=50, cap_coll_rows=60, epoch=0, **null):
    return _lib.SmoothReplay(config_size, cap_samples, cap_path_rows, cap_free_rows, cap_coll_rows, epoch,
                             *[None if null.get(f) else FAKE for f in STORE_PTRS])


def _src(n_samples=2, total_path=9, total_nodes=30, take_upper=2, **null):
    return _lib.SmoothReplaySrc(n_samples, total_path, total_nodes, take_upper, *[None if null.get(f) else FAKE for f in SRC_PTRS])


def _out(n_problems=2, total_path=9, total_free=20, total_collided=10, total_edges=23, **null):
    return _lib.SmoothBatch(n_problems, total_path, total_free, total_collided, total_edges, 5, 20, 13,
                            *[None if null.get(f) else FAKE for f in BATCH_PTRS])


def _loss(n_paths=2, total_rows=9, config_size=2, divisor=2, **null):
    return _lib.SmoothPathLoss(n_paths, total_rows, config_size, divisor, *[None if null.get(f) else FAKE for f in LOSS_PTRS])


def _ref(d):
    return ctypes.byref(d) if d is not None else None


def _append(store, src):
    return _lib.lib().gnnmp_smooth_replay_append(_ref(store), _ref(src), None)


def _gather(store, out, n_group=2, n_samples=3, idx=FAKE, target=FAKE):
    return _lib.lib().gnnmp_smooth_replay_gather(_ref(store), n_group, n_samples, idx, _ref(out), target, None)


def _path_loss(d):
    return _lib.lib().gnnmp_smooth_path_loss(_ref(d), None)


def _struct_fields(text, name):
    body = re.search(r'typedef struct\s*\{([^}]*)\}\s*%s;' % name, text).group(1)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            fields.extend(x.split()[-1].lstrip('*') for x in decl.split(','))
    return fields


def test_symbols_exist_abi_stays_and_structs_mirror_the_header():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gnnmp_smooth_replay_append', 'gnnmp_smooth_replay_gather', 'gnnmp_smooth_path_loss'):
        assert hasattr(L, name), name
    assert _lib.lib().gnnmp_abi_version() == _lib.ABI_VERSION == 9
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gnnmp.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for cls, name in ((_lib.SmoothReplay, 'gnnmp_smooth_replay'), (_lib.SmoothReplaySrc, 'gnnmp_smooth_replay_src'),
                      (_lib.SmoothPathLoss, 'gnnmp_smooth_path_loss_desc')):
        assert [f[0] for f in cls._fields_] == _struct_fields(text, name), name


def test_append_checks_come_in_order_and_before_any_hip_call():
    assert _append(None, _src()) == ERR_NULL
    assert _append(_store(), None) == ERR_NULL
    for C in (0, 1, 15, -2):
        assert _append(_store(config_size=C, cap_samples=-1, path=True), _src(n_samples=-1)) == ERR_DIMS, C           # dims first
    for C in (2, 3, 14):
        for name in STORE_INTS[1:]:
            assert _append(_store(config_size=C, counts=True, **{name: -1}), _src()) == ERR_ARG, name               # counts before arrays
        for bad in ({'n_samples': -1}, {'total_path': -1}, {'total_nodes': -1}, {'take_upper': -1}, {'take_upper': 3}):
            assert _append(_store(config_size=C, counts=True), _src(path=True, **bad)) == ERR_ARG, bad
        for name in STORE_PTRS:
            assert _append(_store(config_size=C, **{name: True}), _src()) == ERR_NULL, name
            assert _append(_store(config_size=C, **{name: True}), _src(n_samples=0, take_upper=0)) == ERR_NULL, name   # arrays before no work
        for name in SRC_PTRS:
            assert _append(_store(config_size=C), _src(**{name: True})) == ERR_NULL, name
            assert _append(_store(config_size=C), _src(take_upper=0, **{name: True})) == ERR_NULL, name
        # no work: B = 0, or nothing taken -- 0, nothing launched, nothing written, whatever the capacities are
        assert _append(_store(config_size=C), _src(n_samples=0, take_upper=0)) == 0
        assert _append(_store(config_size=C), _src(take_upper=0)) == 0
        assert _append(_store(config_size=C, cap_samples=0, cap_path_rows=0, cap_free_rows=0, cap_coll_rows=0, epoch=7),
                       _src(take_upper=0)) == 0


def test_gather_checks_come_in_order_and_before_any_hip_call():
    assert _gather(None, _out()) == ERR_NULL
    assert _gather(_store(), None) == ERR_NULL
    for C in (0, 1, 15):
        assert _gather(_store(config_size=C, epoch=-1, path=True), _out(), n_group=-1) == ERR_DIMS, C
    for C in (2, 3, 14):
        assert _gather(_store(config_size=C, cap_free_rows=-1, counts=True), _out()) == ERR_ARG
        assert _gather(_store(config_size=C, counts=True), _out(n_problems=-1), n_group=-1) == ERR_ARG
        assert _gather(_store(config_size=C, counts=True), _out(), n_samples=-1) == ERR_ARG
        assert _gather(_store(config_size=C, counts=True), _out(n_problems=3)) == ERR_ARG                             # out is not the group's
        for bad in ('total_path', 'total_free', 'total_collided', 'total_edges'):
            assert _gather(_store(config_size=C, counts=True), _out(path=True, **{bad: -1})) == ERR_ARG, bad
        for name in STORE_PTRS:
            assert _gather(_store(config_size=C, **{name: True}), _out()) == ERR_NULL, name
            assert _gather(_store(config_size=C, **{name: True}), _out(n_problems=0), n_group=0) == ERR_NULL, name
        for name in BATCH_PTRS:
            assert _gather(_store(config_size=C), _out(**{name: True})) == ERR_NULL, name
            assert _gather(_store(config_size=C), _out(n_problems=0, **{name: True}), n_group=0) == ERR_NULL, name
        assert _gather(_store(config_size=C), _out(), idx=None) == ERR_NULL
        assert _gather(_store(config_size=C), _out(), target=None) == ERR_NULL
        # no work: G = 0
        assert _gather(_store(config_size=C), _out(n_problems=0), n_group=0) == 0
        assert _gather(_store(config_size=C), _out(n_problems=0, total_path=0, total_free=0, total_collided=0, total_edges=0),
                       n_group=0, n_samples=0) == 0


def test_path_loss_checks_come_in_order_and_before_any_hip_call():
    assert _path_loss(None) == ERR_NULL
    for C in (0, 1, 15, -3):
        assert _path_loss(_loss(config_size=C, n_paths=-1, pred=True)) == ERR_DIMS, C
    for C in (2, 3, 14):
        for bad in ({'n_paths': -1}, {'total_rows': -1}, {'divisor': 0}, {'divisor': -8}):
            assert _path_loss(_loss(config_size=C, pred=True, **bad)) == ERR_ARG, bad
        for name in LOSS_PTRS:
            assert _path_loss(_loss(config_size=C, **{name: True})) == ERR_NULL, name
            assert _path_loss(_loss(config_size=C, n_paths=0, **{name: True})) == ERR_NULL, name                       # arrays before no work
        assert _path_loss(_loss(config_size=C, n_paths=0)) == 0
        assert _path_loss(_loss(config_size=C, n_paths=0, total_rows=0)) == 0
