"""Argument checks of the RRT* entry points (gnnmp_rrtstar_workspace_bytes / _lds_nodes / _plan): they come before any device
work, so no GPU is needed and nothing is launched (the pointers handed over are not device memory)."""
import ctypes
import os
import re

import gnnmp  # noqa: F401
from gnnmp import _lib

ERR_NULL, ERR_DIMS, ERR_WORKSPACE, ERR_ARG = -1, -2, -4, -6
FAKE = 4096
BATCH_PTRS = [f[0] for f in _lib.RRTStarBatch._fields_[6:]]
TREE_FIELDS = [f[0] for f in _lib.RRTStarTree._fields_]


def _batch(n_problems=2, dim=2, width=15, t_max=100, stop=1, n_draws=400, **null):
    return _lib.RRTStarBatch(n_problems, dim, width, t_max, stop, n_draws, *[None if null.get(f) else FAKE for f in BATCH_PTRS])


def _tree(**null):
    return _lib.RRTStarTree(*[None if null.get(f) else FAKE for f in TREE_FIELDS])


def _plan(b, t, ws=None, ws_bytes=0):
    return _lib.lib().gnnmp_rrtstar_plan(ctypes.byref(b) if b is not None else None, ctypes.byref(t) if t is not None else None,
                                         None if ws is None else ctypes.c_void_p(ws), ws_bytes, None)


def _struct_fields(text, name):
    body = re.search(r'typedef struct\s*\{([^}]*)\}\s*%s;' % name, text).group(1)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            fields.extend(x.split()[-1].lstrip('*') for x in decl.split(','))
    return fields


def test_symbols_abi_version_and_structs_mirror_the_header():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gnnmp_rrtstar_workspace_bytes', 'gnnmp_rrtstar_lds_nodes', 'gnnmp_rrtstar_plan'):
        assert hasattr(L, name), name
    assert _lib.lib().gnnmp_abi_version() == _lib.ABI_VERSION >= 6
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gnnmp.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert [f[0] for f in _lib.RRTStarBatch._fields_] == _struct_fields(text, 'gnnmp_rrtstar_batch')
    assert [f[0] for f in _lib.RRTStarTree._fields_] == _struct_fields(text, 'gnnmp_rrtstar_tree')


def test_workspace_bytes_and_lds_nodes():
    L = _lib.lib()
    need = ctypes.c_size_t(7)
    lds = L.gnnmp_rrtstar_lds_nodes()
    assert lds >= 1001                                           # t_max = 1000 keeps its node state in LDS
    assert L.gnnmp_rrtstar_workspace_bytes(2, 100, None) == ERR_NULL
    for args in ((0, 100), (-1, 100), (2, 0), (2, -5)):
        assert L.gnnmp_rrtstar_workspace_bytes(*args, ctypes.byref(need)) == ERR_ARG, args
    assert L.gnnmp_rrtstar_workspace_bytes(3, lds - 1, ctypes.byref(need)) == 0 and need.value == 0
    assert L.gnnmp_rrtstar_workspace_bytes(3, lds, ctypes.byref(need)) == 0
    # per node three coordinates and the cost in float64 and one flag byte
    assert need.value >= 3 * (lds + 1) * 33 and need.value % 256 == 0
    small = need.value
    assert L.gnnmp_rrtstar_workspace_bytes(6, lds, ctypes.byref(need)) == 0 and need.value > small


def test_plan_checks_come_before_any_launch():
    assert _plan(None, _tree()) == ERR_NULL
    assert _plan(_batch(), None) == ERR_NULL
    for dim in (0, 1, 4, -2):
        assert _plan(_batch(dim=dim), _tree()) == ERR_DIMS, dim
    for name in BATCH_PTRS:
        assert _plan(_batch(**{name: True}), _tree()) == ERR_NULL, name
    for name in TREE_FIELDS:
        assert _plan(_batch(dim=3), _tree(**{name: True})) == ERR_NULL, name
    for kw in (dict(n_problems=0), dict(n_problems=-3), dict(width=0), dict(t_max=0), dict(t_max=-1), dict(t_max=2 ** 31 - 1)):
        assert _plan(_batch(**kw), _tree()) == ERR_ARG, kw
    # a draw block shorter than one iteration (2 + dim doubles), or one whose offsets would not fit the used counts
    assert _plan(_batch(dim=2, n_draws=3), _tree()) == ERR_ARG
    assert _plan(_batch(dim=3, n_draws=4), _tree()) == ERR_ARG
    assert _plan(_batch(n_draws=0), _tree()) == ERR_ARG
    assert _plan(_batch(n_draws=-8), _tree()) == ERR_ARG
    assert _plan(_batch(n_draws=2 ** 31), _tree()) == ERR_ARG
    # beyond the LDS node count the workspace is needed, large enough and 256-byte aligned
    lds = _lib.lib().gnnmp_rrtstar_lds_nodes()
    need = ctypes.c_size_t()
    assert _lib.lib().gnnmp_rrtstar_workspace_bytes(2, lds, ctypes.byref(need)) == 0 and need.value > 0
    big = _batch(t_max=lds, n_draws=4 * lds)
    assert _plan(big, _tree()) == ERR_NULL
    assert _plan(big, _tree(), ws=FAKE, ws_bytes=need.value - 1) == ERR_WORKSPACE
    assert _plan(big, _tree(), ws=FAKE + 8, ws_bytes=need.value) == ERR_WORKSPACE
