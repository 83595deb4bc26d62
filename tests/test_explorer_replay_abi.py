"""Argument checks of the explorer loop's entry points (gnnmp_episode_dataset_gather, gnnmp_episode_frontier_loss), no GPU.

As in tests/test_smoother_replay_abi.py, every call here ends at an argument error or at the no-work return, and every one of
those comes before the first HIP call of its entry point: the pointers handed over are not device memory (address 4096) and no
call passes all checks with work to do, so nothing is ever launched or written.  The no-work calls must return 0: on a machine
without a GPU any HIP call fails with GNNMP_ERR_HIP, so a 0 there shows that none was made."""
import ctypes
import os
import re

import gnnmp  # noqa: F401
from gnnmp import _lib

ERR_NULL, ERR_DIMS, ERR_ARG = -1, -2, -6
FAKE = 4096
STORE_INTS = [f[0] for f in _lib.EpisodeDataset._fields_[:6]]
STORE_PTRS = [f[0] for f in _lib.EpisodeDataset._fields_[6:]]
OUT_PTRS = [f[0] for f in _lib.EpisodeDatasetBatch._fields_[4:]]
LOSS_PTRS = [f[0] for f in _lib.EpisodeFrontierLoss._fields_[3:]]


def _store(n_problems=3, total_nodes=30, total_edges=200, total_obs=40, config_size=2, obs_size=2, **null):
    return _lib.EpisodeDataset(n_problems, total_nodes, total_edges, total_obs, config_size, obs_size,
                               *[None if null.get(f) else FAKE for f in STORE_PTRS])


def _out(n_problems=2, total_nodes=20, total_edges=130, total_obs=25, **null):
    return _lib.EpisodeDatasetBatch(n_problems, total_nodes, total_edges, total_obs, *[None if null.get(f) else FAKE for f in OUT_PTRS])


def _loss(n_problems=2, total_edges=130, divisor=1.0, **null):
    return _lib.EpisodeFrontierLoss(n_problems, total_edges, divisor, *[None if null.get(f) else FAKE for f in LOSS_PTRS])


def _ref(d):
    return ctypes.byref(d) if d is not None else None


def _gather(store, out, n_group=2, idx=FAKE):
    return _lib.lib().gnnmp_episode_dataset_gather(_ref(store), n_group, idx, _ref(out), None)


def _frontier_loss(d):
    return _lib.lib().gnnmp_episode_frontier_loss(_ref(d), None)


def _struct_fields(text, name):
    body = re.search(r'typedef struct\s*\{([^}]*)\}\s*%s;' % name, text).group(1)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            fields.extend(x.split()[-1].lstrip('*') for x in decl.split(','))
    return fields


def test_symbols_exist_abi_stays_and_structs_mirror_the_header():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gnnmp_episode_dataset_gather', 'gnnmp_episode_frontier_loss'):
        assert hasattr(L, name), name
    assert _lib.lib().gnnmp_abi_version() == _lib.ABI_VERSION == 9
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gnnmp.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for cls, name in ((_lib.EpisodeDataset, 'gnnmp_episode_dataset'), (_lib.EpisodeDatasetBatch, 'gnnmp_episode_dataset_batch'),
                      (_lib.EpisodeFrontierLoss, 'gnnmp_episode_frontier_loss_desc')):
        assert [f[0] for f in cls._fields_] == _struct_fields(text, name), name


def test_gather_checks_come_in_order_and_before_any_hip_call():
    assert _gather(None, _out()) == ERR_NULL
    assert _gather(_store(), None) == ERR_NULL
    for dims in ({'config_size': 0}, {'config_size': 1}, {'config_size': 15}, {'obs_size': 0}, {'obs_size': 17}, {'obs_size': -1}):
        assert _gather(_store(total_nodes=-1, v=True, **dims), _out(), n_group=-1) == ERR_DIMS, dims                    # dims first
    for C in (2, 3, 14):
        for name in STORE_INTS[:4]:
            assert _gather(_store(config_size=C, status=True, **{name: -1}), _out()) == ERR_ARG, name                 # counts before arrays
        assert _gather(_store(config_size=C, status=True), _out(n_problems=-1), n_group=-1) == ERR_ARG
        assert _gather(_store(config_size=C, status=True), _out(n_problems=3)) == ERR_ARG                             # out is not the group's
        for bad in ('total_nodes', 'total_edges', 'total_obs'):
            assert _gather(_store(config_size=C, status=True), _out(v=True, **{bad: -1})) == ERR_ARG, bad
        for name in STORE_PTRS:
            assert _gather(_store(config_size=C, **{name: True}), _out()) == ERR_NULL, name
            assert _gather(_store(config_size=C, **{name: True}), _out(n_problems=0), n_group=0) == ERR_NULL, name    # arrays before no work
        for name in OUT_PTRS:
            assert _gather(_store(config_size=C), _out(**{name: True})) == ERR_NULL, name
            assert _gather(_store(config_size=C), _out(n_problems=0, **{name: True}), n_group=0) == ERR_NULL, name
        assert _gather(_store(config_size=C), _out(), idx=None) == ERR_NULL
        assert _gather(_store(config_size=C), _out(n_problems=0), n_group=0, idx=None) == ERR_NULL
        # no work: G = 0 -- 0, nothing launched, nothing written, whatever the store holds
        assert _gather(_store(config_size=C), _out(n_problems=0), n_group=0) == 0
        assert _gather(_store(config_size=C, n_problems=0, total_nodes=0, total_edges=0, total_obs=0),
                       _out(n_problems=0, total_nodes=0, total_edges=0, total_obs=0), n_group=0) == 0


def test_frontier_loss_checks_come_in_order_and_before_any_hip_call():
    assert _frontier_loss(None) == ERR_NULL
    for bad in ({'n_problems': -1}, {'total_edges': -1}, {'divisor': 0.0}, {'divisor': -8.0}, {'divisor': float('inf')}):
        assert _frontier_loss(_loss(scores=True, **bad)) == ERR_ARG, bad                                               # counts before arrays
    for name in LOSS_PTRS:
        assert _frontier_loss(_loss(**{name: True})) == ERR_NULL, name
        assert _frontier_loss(_loss(n_problems=0, **{name: True})) == ERR_NULL, name                                  # arrays before no work
    assert _frontier_loss(_loss(n_problems=0)) == 0
    assert _frontier_loss(_loss(n_problems=0, total_edges=0, divisor=8.0)) == 0
