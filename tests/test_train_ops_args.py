"""The test hooks of the training operators (gnnmp_train_op and friends, include/gnnmp.h) validate everything before any
launch, so all of this runs without a GPU -- and the CPU half of the BatchNorm bar of tests/test_train_ops_gpu.py: the
reference pair (torch float32 batch norm against float64) itself stays inside 1e-5 * scale on the unit-scale inputs."""
import ctypes

import pytest

from gnnmp import _lib
import train_ops_host as H

OK, ERR_NULL, ERR_DIMS, ERR_ARG = 0, -1, -2, -6
FAKE = 4096                       # a non-NULL address no call may dereference: every call below has at least one bad argument

# op -> (dims that are fine, number of buffers, needs a geometry)
GOOD = {
    'LINEAR': ([5, 3, 2, 1], 4, False), 'LINEAR_DX': ([5, 3, 2, 0], 3, False), 'LINEAR_DW': ([5, 3, 2], 5, False),
    'RELU_BWD': ([7], 2, False), 'FILL': ([7], 1, False), 'NODE_IN': ([], 1, True), 'EDGE_IN': ([], 1, True), 'H0': ([32], 2, True),
    'H0_BWD': ([64], 2, True), 'CONCAT': ([5, 32, 4], 5, False), 'SPLIT': ([5, 32, 4, 3, 1], 2, False), 'MSG_IN': ([32], 4, True),
    'MSG_IN_BWD': ([32], 3, True), 'POL_IN': ([64], 3, True), 'POL_IN_BWD': ([64], 2, True), 'SEGMENT_MAX': ([32], 3, True),
    'SEGMENT_MAX_BWD': ([64, 32], 3, False), 'SCORES_OUT': ([], 2, True), 'SCORES_IN': ([], 2, True),
    'SM_NODES_IN': ([3, 2, 2, 7], 4, False), 'BN_FWD': ([9, 32, 1], 5, False), 'BN_BWD': ([9, 32], 7, False),
    'SM_MSG_IN': ([32, 9], 5, False), 'SM_MSG_IN_BWD': ([32, 9], 5, False), 'SM_SCATTER_ADD': ([32, 9], 4, False),
    'SM_SCATTER_ADD_BWD': ([32, 9], 4, False), 'ADD_ROWS': ([7], 3, False), 'SM_PATH_UPDATE': ([3, 2], 3, False),
    'SM_PATH_UPDATE_BWD': ([3, 2], 3, False), 'SM_COORDS_BWD': ([3, 2], 2, False), 'SCALE': ([7], 2, False),
}

# (op, index in dims) where 0 is legal: flags, `part` of SPLIT, and the sizes whose launcher returns early or reads no row.  With
# one of these at 0 the argument set would be VALID, so it is never sent with fake addresses.
ZERO_OK = {('LINEAR', 0), ('LINEAR', 3), ('LINEAR_DX', 0), ('LINEAR_DX', 3), ('LINEAR_DW', 0), ('FILL', 0), ('SCALE', 0),
           ('SM_NODES_IN', 1), ('SM_NODES_IN', 2), ('SPLIT', 3), ('SPLIT', 4), ('BN_FWD', 2)}


def fake_geom(**kw):
    g = _lib.TrainGeom(2, 2, 512, 512, *([FAKE] * 13))
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_table_covers_every_operator():
    assert sorted(GOOD) == sorted(_lib.TRAIN_OPS)
    assert _lib.train_op_raw(len(_lib.TRAIN_OPS), [], []) == ERR_ARG and _lib.train_op_raw(-1, [], []) == ERR_ARG


@pytest.mark.parametrize('op', _lib.TRAIN_OPS)
def test_bad_arguments_fail_before_any_launch(op):
    dims, nb, needs_geom = GOOD[op]
    geom = fake_geom() if needs_geom else None
    bufs = [FAKE] * nb
    for i in range(len(dims)):                                   # a negative size, a size beyond int32
        for bad in (-1, 1 << 31):
            d = list(dims)
            d[i] = bad
            assert _lib.train_op_raw(op, d, bufs, geom) == ERR_ARG, (i, bad)
    assert _lib.train_op_raw(op, dims + [1], bufs, geom) == ERR_ARG           # wrong number of dims / buffers
    assert _lib.train_op_raw(op, dims, bufs + [FAKE], geom) == ERR_ARG
    assert _lib.train_op_raw(op, dims, bufs[:-1], geom) == ERR_ARG
    optional = {'LINEAR': {2}, 'LINEAR_DW': {3}}.get(op, set())
    for i in range(nb):                                          # a required buffer that is NULL
        if i in optional:                                        # a complete, valid argument set must never be sent with fake addresses
            continue
        b = list(bufs)
        b[i] = None
        assert _lib.train_op_raw(op, dims, b, geom) == ERR_NULL, i
    for i in range(len(dims)):                                   # a size of 0 that the launcher does not guard
        if (op, i) in ZERO_OK:
            continue
        d = list(dims)
        d[i] = 0
        assert _lib.train_op_raw(op, d, bufs, geom) in (ERR_ARG, ERR_DIMS), i
    if needs_geom:
        assert _lib.train_op_raw(op, dims, bufs, None) == ERR_NULL
        assert _lib.train_op_raw(op, dims, bufs, fake_geom(csr=None)) == ERR_NULL
        assert _lib.train_op_raw(op, dims, bufs, fake_geom(out_slot=None)) == ERR_NULL
        assert _lib.train_op_raw(op, dims, bufs, fake_geom(n_pad=-32)) == ERR_ARG
        assert _lib.train_op_raw(op, dims, bufs, fake_geom(n_graphs=0)) == ERR_ARG
        assert _lib.train_op_raw(op, dims, bufs, fake_geom(e_pad=0)) == ERR_ARG
        assert _lib.train_op_raw(op, dims, bufs, fake_geom(e_pad=100)) == ERR_DIMS
        if dims:                                                 # D the geometry kernels do not serve
            for D in (16, 48, 128):
                assert _lib.train_op_raw(op, [D], bufs, geom) == ERR_DIMS, D


def test_flags_and_part_ranges():
    assert _lib.train_op_raw('LINEAR', [5, 3, 2, 2], [FAKE] * 4) == ERR_ARG
    assert _lib.train_op_raw('LINEAR_DX', [5, 3, 2, 2], [FAKE] * 3) == ERR_ARG
    assert _lib.train_op_raw('BN_FWD', [9, 32, 2], [FAKE] * 5) == ERR_ARG
    assert _lib.train_op_raw('SPLIT', [5, 32, 4, 4, 0], [FAKE] * 2) == ERR_ARG
    assert _lib.train_op_raw('SPLIT', [5, 32, 5, 0, 0], [FAKE] * 2) == ERR_ARG
    assert _lib.train_op_raw('SPLIT', [5, 32, 4, 0, 2], [FAKE] * 2) == ERR_ARG
    assert _lib.train_op_raw('CONCAT', [5, 32, 0], [FAKE] * 5) == ERR_ARG
    assert _lib.train_op_raw('CONCAT', [5, 32, 5], [FAKE] * 5) == ERR_ARG
    assert _lib.train_op_raw('CONCAT', [5, 32, 3], [FAKE, FAKE, None, None, FAKE]) == ERR_NULL      # a2 is read when parts = 3
    assert _lib.train_op_raw('SM_NODES_IN', [3, 2, 0, 7], [FAKE, None, None, FAKE]) == ERR_NULL     # F = 2 rows need free_pts


def test_geometry_hook_and_helpers_validate():
    L = _lib.lib()
    need = ctypes.c_size_t()
    geom = _lib.TrainGeom()
    b = _lib.Batch(2, 10, 4, 0, 0, FAKE, FAKE, None, FAKE, FAKE, FAKE, None)
    assert L.gnnmp_train_geom_workspace_bytes(None, 2, ctypes.byref(need)) == ERR_NULL
    assert L.gnnmp_train_geom_workspace_bytes(ctypes.byref(b), 0, ctypes.byref(need)) == ERR_ARG
    assert L.gnnmp_train_geom_workspace_bytes(ctypes.byref(b), 2, ctypes.byref(need)) == OK and need.value > 0
    neg = _lib.Batch(2, -10, 4, 0, 0, FAKE, FAKE, None, FAKE, FAKE, FAKE, None)
    assert L.gnnmp_train_geom_workspace_bytes(ctypes.byref(neg), 2, ctypes.byref(need)) == ERR_ARG
    assert L.gnnmp_train_geom_build(ctypes.byref(neg), 2, FAKE, 1 << 30, ctypes.byref(geom), None) == ERR_ARG
    assert L.gnnmp_train_geom_build(ctypes.byref(b), 2, None, 1 << 30, ctypes.byref(geom), None) == ERR_NULL
    assert L.gnnmp_train_geom_build(ctypes.byref(b), 2, FAKE, 1 << 30, None, None) == ERR_NULL
    no_ptr = _lib.Batch(2, 10, 4, 0, 0, FAKE, FAKE, None, FAKE, None, FAKE, None)
    assert L.gnnmp_train_geom_build(ctypes.byref(no_ptr), 2, FAKE, 1 << 30, ctypes.byref(geom), None) == ERR_NULL
    assert L.gnnmp_train_geom_build(ctypes.byref(b), 2, FAKE, 16, ctypes.byref(geom), None) == -4           # workspace too small
    assert L.gnnmp_train_geom_build(ctypes.byref(b), 2, FAKE + 4, 1 << 30, ctypes.byref(geom), None) == -4   # misaligned
    assert L.gnnmp_train_dw_scratch_floats(-1, 3, 2) == ERR_ARG
    assert _lib.train_dw_scratch_floats(129, 3, 2) == 2 * (3 * 2 + 2)
    d = (ctypes.c_int64 * 3)(5, 3, 2)
    assert L.gnnmp_train_op_path(_lib.TRAIN_OPS.index('FILL'), d, 3) == ERR_ARG
    assert L.gnnmp_train_op_path(0, d, 2) == ERR_ARG and L.gnnmp_train_op_path(0, None, 3) == ERR_ARG
    bad = (ctypes.c_int64 * 3)(5, -3, 2)
    assert L.gnnmp_train_op_path(0, bad, 3) == ERR_ARG


def test_dispatch_thresholds_are_the_documented_ones():
    """O >= 8 (linear), O >= 8 and K >= 8 (dx), O >= 8 and K >= 4 (dw): asked of the launchers' own predicate."""
    for op in ('LINEAR', 'LINEAR_DX', 'LINEAR_DW'):
        seen = set()
        for K, O in H.MODEL_PAIRS + H.BOUNDARY_PAIRS:
            path = _lib.train_op_path(op, 33, K, O)
            assert path == H.expected_path(op, K, O), (op, K, O)
            seen.add(path)
        assert seen == {'mfma', 'plain'}


@pytest.mark.parametrize('D', H.BN_D)
@pytest.mark.parametrize('N', H.BN_TIGHT_N)
def test_batchnorm_reference_pair_is_tight_on_unit_scale_inputs(N, D):
    """N = 1 and N = 2 are left to the general bar (train_ops_host.BN_TIGHT_N says why): torch's own float32 result is
    3e-5 .. 2e-4 off float64 there."""
    for relu in (0, 1):
        _, _, own, scale = H.bn_pair('unit', N, D, relu)
        for k in H.BN_TENSORS:
            assert own[k] <= 1e-5 * scale[k] + 1e-6, (k, own[k], scale[k])
