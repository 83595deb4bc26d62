"""Argument checks of gnnmp_stick_sample: they come before any device work (no GPU needed), and they are the ones
gnnmp_maze_sample makes, plus the new checks_out array."""
import ctypes

import gnnmp  # noqa: F401
from gnnmp import _lib

ERR_NULL, ERR_ARG = -1, -6
FAKE = 4096


def _batch(n_problems=1, width=15, n_free=8, n_attempts=64, attempts=FAKE, maps=FAKE, init=FAKE, goal=FAKE):
    return _lib.MazeSampleBatch(n_problems, width, n_free, n_attempts, attempts, maps, init, goal)


def _call(sb, cursor=FAKE, v=FAKE, node_ptr=FAKE, used=FAKE, checks=FAKE, ok=FAKE):
    p = lambda x: None if x is None else ctypes.c_void_p(x)      # noqa: E731
    return _lib.lib().gnnmp_stick_sample(ctypes.byref(sb) if sb is not None else None, p(cursor), p(v), p(node_ptr), p(used),
                                         p(checks), p(ok), None)


def test_symbol_is_exported():
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'gnnmp_stick_sample')


def test_null_pointers_are_refused():
    assert _call(None) == ERR_NULL
    for name in ('cursor', 'v', 'node_ptr', 'used', 'checks', 'ok'):
        assert _call(_batch(), **{name: None}) == ERR_NULL, name
    for name in ('attempts', 'maps', 'init', 'goal'):
        assert _call(_batch(**{name: None})) == ERR_NULL, name


def test_bad_counts_are_refused():
    assert _call(_batch(n_free=0)) == ERR_ARG
    assert _call(_batch(n_free=-3)) == ERR_ARG
    assert _call(_batch(width=0)) == ERR_ARG
    assert _call(_batch(width=-1)) == ERR_ARG
    assert _call(_batch(n_problems=0)) == ERR_ARG
    assert _call(_batch(n_attempts=-1)) == ERR_ARG
