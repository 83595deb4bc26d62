"""Argument checks of gnnmp_mt19937_seed / gnnmp_mt19937_uniform (include/gnnmp.h): every bad argument is refused with its
error code before anything is launched, so dummy pointers are enough and no GPU is needed."""
import ctypes
import math

import pytest

import gnnmp  # noqa: F401
from gnnmp import _lib

OK_PTR = 0x1000                        # never dereferenced: every call below returns before a launch
NULL, DIMS, ARG = -1, -2, -6


def _batch(n=4, dim=3, out_rows=16, counts=OK_PTR, out_ptr=OK_PTR, active=None, low=(-1.0, -1.0, -0.4), rng=(2.0, 2.0, 0.8)):
    b = _lib.MtUniformBatch(n, dim, out_rows, counts, out_ptr, active)
    for c in range(3):
        b.low[c], b.range[c] = low[c], rng[c]
    return b


def _uniform(b, state=OK_PTR, out=OK_PTR, commit=0, status=OK_PTR):
    return _lib.lib().gnnmp_mt19937_uniform(ctypes.byref(b) if b is not None else None, state, out, commit, status, None)


def test_struct_mirrors_the_header():
    assert [f[0] for f in _lib.MtUniformBatch._fields_] == ['n_streams', 'dim', 'out_rows', 'counts', 'out_ptr', 'active', 'low', 'range']
    assert ctypes.sizeof(_lib.MtUniformBatch) == 4 + 4 + 8 + 3 * 8 + 6 * 8
    assert _lib.MtUniformBatch.low.offset == 40 and _lib.MtUniformBatch.range.offset == 64


def test_seed_arguments():
    L = _lib.lib()
    assert L.gnnmp_mt19937_seed(4, None, OK_PTR, None) == NULL
    assert L.gnnmp_mt19937_seed(4, OK_PTR, None, None) == NULL
    assert L.gnnmp_mt19937_seed(0, OK_PTR, OK_PTR, None) == ARG
    assert L.gnnmp_mt19937_seed(-3, OK_PTR, OK_PTR, None) == ARG


def test_uniform_null_pointers():
    assert _uniform(None) == NULL
    assert _uniform(_batch(), state=None) == NULL
    assert _uniform(_batch(), status=None) == NULL
    assert _uniform(_batch(counts=None)) == NULL
    assert _uniform(_batch(out_ptr=None)) == NULL                 # out given without out_ptr


@pytest.mark.parametrize('dim', [0, 4, -1])
def test_uniform_dim_outside_1_to_3(dim):
    assert _uniform(_batch(dim=dim)) == DIMS


def test_uniform_scalar_arguments():
    assert _uniform(_batch(n=0)) == ARG
    assert _uniform(_batch(n=-2)) == ARG
    assert _uniform(_batch(out_rows=-1)) == ARG
    assert _uniform(_batch(), out=None, commit=0) == ARG          # neither rows nor a state to store: nothing to do


@pytest.mark.parametrize('bad', [math.inf, -math.inf, math.nan])
@pytest.mark.parametrize('col', [0, 1, 2])
def test_uniform_bounds_must_be_finite(bad, col):
    low, rng = [-1.0, -1.0, -0.4], [2.0, 2.0, 0.8]
    low[col] = bad
    assert _uniform(_batch(low=low)) == ARG
    low[col] = -1.0
    rng[col] = bad
    assert _uniform(_batch(rng=rng)) == ARG
    if col == 2:                                                  # a column behind dim is not looked at: dim itself is refused first
        assert _uniform(_batch(dim=4, rng=rng)) == DIMS
