"""Launch sizes of the explorer's batched training path (gnnmp_explorer_train_batch_plan, host only): per loop iteration the
graphs still running -- a prefix of the batch, which comes longest loop first -- and their padded node / edge rows, every
graph rounded up to 256 as the prep stage does for node_ptr_pad and the CSR ranges.  The forward and the backward size their
launches with this function, so it is held to a restatement of the rule."""
import pytest

import gnnmp  # noqa: F401
from gnnmp import _lib

ERR_NULL, ERR_ARG = -1, -6
PAD = 256


def restated(loops, nodes, edges):
    up = lambda x: (x + PAD - 1) // PAD * PAD        # noqa: E731
    active, nrows, erows = [], [], []
    for it in range(max(loops)):
        run = [g for g in range(len(loops)) if loops[g] > it]
        assert run == list(range(len(run)))          # a prefix
        active.append(len(run))
        nrows.append(sum(up(nodes[g]) for g in run))
        erows.append(sum(up(edges[g]) for g in run))
    return active, nrows, erows


CASES = {
    'ragged': ([5, 3, 3, 1, 1], [33, 256, 257, 64, 1], [150, 1024, 1025, 300, 0]),
    'single': ([4], [100], [520]),
    'equal': ([3, 3, 3], [40, 64, 130], [160, 256, 520]),
    'ones': ([1, 1], [255, 512], [256, 3000]),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_plan_equals_restated_rule(name):
    loops, nodes, edges = CASES[name]
    got = _lib.explorer_train_batch_plan(loops, nodes, edges)
    assert got == restated(loops, nodes, edges)
    a, nr, er = got
    assert len(a) == loops[0] and a[0] == len(loops)
    assert all(x % PAD == 0 for x in nr + er)
    assert all(x >= y for x, y in zip(nr, nr[1:])) and all(x >= y for x, y in zip(er, er[1:]))


def test_plan_of_the_issue_case_by_hand():
    a, nr, er = _lib.explorer_train_batch_plan([5, 3, 3, 1, 1], [33, 256, 257, 64, 1], [0, 0, 0, 0, 0])
    assert a == [5, 3, 3, 1, 1]
    assert nr == [256 + 256 + 512 + 256 + 256, 1024, 1024, 256, 256]
    assert er == [0, 0, 0, 0, 0]


def test_plan_argument_errors():
    raw = _lib.explorer_train_batch_plan_raw
    assert raw([3, 4], [10, 10], [5, 5])[0] == ERR_ARG               # an ascending pair
    assert raw([2, 0], [10, 10], [5, 5])[0] == ERR_ARG               # a loop of 0
    assert raw([0], [10], [5])[0] == ERR_ARG
    assert raw([2, 1], [10, -1], [5, 5])[0] == ERR_ARG               # a negative count
    assert raw([_lib.TRAIN_BATCH_MAX_LOOP + 1], [10], [5])[0] == ERR_ARG
    assert raw([_lib.TRAIN_BATCH_MAX_LOOP], [10], [5])[0] == 0
    L = _lib.lib()
    import ctypes
    n = ctypes.c_int32()
    one = _lib.i32_array([1])
    assert L.gnnmp_explorer_train_batch_plan(1, None, one, one, 0, None, None, None, ctypes.byref(n)) == ERR_NULL
    assert L.gnnmp_explorer_train_batch_plan(1, one, one, one, 0, None, None, None, None) == ERR_NULL
    assert L.gnnmp_explorer_train_batch_plan(1, one, one, one, 1, None, None, None, ctypes.byref(n)) == ERR_NULL
    assert L.gnnmp_explorer_train_batch_plan(0, one, one, one, 0, None, None, None, ctypes.byref(n)) == ERR_ARG
    three = _lib.i32_array([3])
    buf = (ctypes.c_int32 * 2)()
    assert L.gnnmp_explorer_train_batch_plan(1, three, one, one, 2, buf, buf, buf, ctypes.byref(n)) == ERR_ARG   # cap below the loop
