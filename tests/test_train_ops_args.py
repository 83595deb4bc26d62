"""The test hooks of the training operators (gnnmp_train_op and friends, include/gnnmp.h) validate everything before any
launch, so all of this runs without a GPU -- and the CPU half of the BatchNorm bar of tests/test_train_ops_gpu.py: the
reference pair (torch float32 batch norm against float64) itself stays inside 1e-5 * scale on the unit-scale inputs.  The host
references of the batched operators check themselves here too: with one problem, active, each is the one-problem reference."""
import ctypes

import numpy as np
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
    # the batched paths: [B, A, P, Nn, Ec, D or C, ...] and the four prefix arrays in front of the launcher's buffers
    'SM_NODES_IN_SEG': ([2, 1, 5, 9, 64, 7], 8, False), 'BN_SEG_FWD': ([2, 1, 5, 9, 64, 32, 1, 192], 10, False),
    'BN_SEG_BWD': ([2, 1, 5, 9, 64, 32], 10, False), 'BN_SEG_DGB': ([3, 2, 32], 3, False),
    'SM_MSG_IN_SEG': ([2, 1, 5, 9, 64, 32], 9, False), 'SM_MSG_IN_BWD_SEG': ([2, 1, 5, 9, 64, 32], 9, False),
    'SM_SCATTER_ADD_SEG': ([2, 1, 5, 9, 64, 32], 8, False), 'SM_SCATTER_ADD_BWD_SEG': ([2, 1, 5, 9, 64, 32], 8, False),
    'SM_ADD_PATH_SEG': ([2, 1, 5, 9, 64, 32], 7, False), 'SM_ADD_PATH_BWD_SEG': ([2, 1, 5, 9, 64, 32], 6, False),
    'SM_PATH_UPDATE_SEG': ([2, 1, 5, 9, 64, 7], 7, False), 'SM_PATH_UPDATE_BWD_SEG': ([2, 1, 5, 9, 64, 7], 7, False),
    'SM_COORDS_BWD_SEG': ([2, 1, 5, 9, 64, 7], 6, False), 'FINAL_CAT': ([32, 16384, 2, 512, 256], 3, False),
    'SEED_DH': ([512, 256, 32], 3, False), 'LINEAR_DW_ORDER': ([5, 3, 2, 9], 5, False),
}
SEG_OPS = [op for op in GOOD if op.endswith('_SEG') or op in ('BN_SEG_FWD', 'BN_SEG_BWD')]

# (op, index in dims) where 0 is legal: flags, `part` of SPLIT, and the sizes whose launcher returns early or reads no row.  With
# one of these at 0 the argument set would be VALID, so it is never sent with fake addresses.
ZERO_OK = {('LINEAR', 0), ('LINEAR', 3), ('LINEAR_DX', 0), ('LINEAR_DX', 3), ('LINEAR_DW', 0), ('FILL', 0), ('SCALE', 0),
           ('SM_NODES_IN', 1), ('SM_NODES_IN', 2), ('SPLIT', 3), ('SPLIT', 4), ('BN_FWD', 2),
           ('BN_SEG_FWD', 6), ('BN_SEG_FWD', 7), ('SEED_DH', 1), ('LINEAR_DW_ORDER', 0), ('LINEAR_DW_ORDER', 3)}
ZERO_OK |= {(op, i) for op in SEG_OPS for i in (1, 2, 3, 4)}          # A, P, Nn, Ec: every segmented launcher guards an empty range


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
    optional = {'LINEAR': {2}, 'LINEAR_DW': {3}, 'LINEAR_DW_ORDER': {3}, 'BN_SEG_FWD': {9}}.get(op, set())
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


# ======================================================================================================================
# the batched paths: B problems with the prefix [0, A) active; a loop count per graph
# ======================================================================================================================
@pytest.mark.parametrize('op', SEG_OPS)
def test_segmented_operators_reject_a_bad_active_count(op):
    dims, nb, _ = GOOD[op]
    bufs = [FAKE] * nb
    for B, A in ((2, 3), (1, 2), (0, 0), (-1, 0), (2, -1)):
        assert _lib.train_op_raw(op, [B, A] + dims[2:], bufs) == ERR_ARG, (B, A)
    for i in (2, 3, 4):                                          # negative totals
        d = list(dims)
        d[i] = -5
        assert _lib.train_op_raw(op, d, bufs) == ERR_ARG, i
    for i in range(4):                                           # all four prefix arrays are required
        b = list(bufs)
        b[i] = None
        assert _lib.train_op_raw(op, dims, b) == ERR_NULL, i


def test_loop_count_operators_reject_bad_row_tables():
    b3 = [FAKE] * 3
    cat = lambda D, stride, rows, n_it=None, bufs=b3: _lib.train_op_raw('FINAL_CAT', [D, stride, len(rows) if n_it is None else n_it] + rows, bufs)
    assert cat(32, 16384, [256, 512]) == ERR_ARG                 # ascending
    assert cat(32, 16384, [512, 512, 768]) == ERR_ARG
    assert cat(32, 16384, [300, 256]) == ERR_DIMS                # not multiples of 256
    assert cat(32, 16384, [512, 100]) == ERR_DIMS
    assert cat(32, 16384, [], n_it=0) == ERR_ARG                 # n_it outside 1 .. GNNMP_TRAIN_BATCH_MAX_LOOP
    assert cat(32, 16384, [256] * (_lib.TRAIN_BATCH_MAX_LOOP + 1)) == ERR_ARG
    assert cat(32, 16384, [512, 256], n_it=1) == ERR_ARG         # a table longer / shorter than n_it
    assert cat(32, 16384, [512, 256], n_it=3) == ERR_ARG
    assert _lib.train_op_raw('FINAL_CAT', [32, 16384], b3) == ERR_ARG
    assert cat(32, 16386, [512, 256]) == ERR_DIMS                # it_stride not a multiple of 4
    for D in (16, 48, 128):
        assert cat(D, 16384, [512, 256]) == ERR_DIMS
    assert cat(32, 16384, [512, 256], bufs=[FAKE, FAKE + 4, FAKE]) == ERR_DIMS      # rows are moved in 16-byte pieces
    assert cat(32, 16384, [512, 256], bufs=[FAKE, None, FAKE]) == ERR_NULL
    seed = lambda *d: _lib.train_op_raw('SEED_DH', list(d), b3)
    assert seed(256, 512, 32) == ERR_ARG                         # rows_next beyond rows_it
    assert seed(300, 256, 32) == ERR_DIMS and seed(512, 100, 32) == ERR_DIMS
    assert seed(512, 256, 128) == ERR_DIMS and seed(512, 256, 0) == ERR_ARG
    assert _lib.train_op_raw('SEED_DH', [512, 256, 64], [FAKE + 8, FAKE, FAKE]) == ERR_DIMS


def test_linear_dw_order_rejects_an_order_inside_the_rows():
    for R_order in (1, 4):
        assert _lib.train_op_raw('LINEAR_DW_ORDER', [5, 3, 2, R_order], [FAKE] * 5) == ERR_ARG
    assert _lib.train_op_raw('LINEAR_DW_ORDER', [5, 3, 2, -1], [FAKE] * 5) == ERR_ARG
    for K, O in H.DW_ORDER_PAIRS:                                # the same launcher: the same dispatch
        assert _lib.train_op_path('LINEAR_DW_ORDER', 256, K, O) == _lib.train_op_path('LINEAR_DW', 256, K, O) == H.expected_path('LINEAR_DW', K, O)
    assert {H.expected_path('LINEAR_DW', K, O) for K, O in H.DW_ORDER_PAIRS} == {'mfma', 'plain'}
    assert any(H.dw_slice_width(R) != H.dw_slice_width(Ro) for R, Ro in H.DW_ORDER_ROWS)       # an order that changes the slices


def test_ragged_batch_of_the_segmented_operators():
    s = H.seg_ragged_batch(1)
    assert s['B'] == 6 and s['P'] == 92 and s['Nn'] == 614 and s['sizes'].sum(1).tolist() == [2, 10, 293, 256, 11, 42]
    for b in range(s['B']):                                      # the edge-space start of the kNN stage, spelled out
        assert s['e0'][b] == ((int(s['edge_ptr'][b]) + 10 * int(s['path_ptr'][b]) + 31) // 32) * 32 + 32 * b and s['e0'][b] % 32 == 0
    u = s['used']
    assert (s['e_dst'][u] < s['sizes'][s['slot_b'][u], 0]).all() and (s['e_src'][u] < s['sizes'][s['slot_b'][u]].sum(1)).all()
    e = np.nonzero(u & (s['slot_b'] == 2))[0]
    assert len({(int(s['e_src'][i]), int(s['e_dst'][i])) for i in e}) < e.size                  # duplicate edges


@pytest.mark.parametrize('P,F,Co,n', [(5, 4, 3, 30), (2, 0, 0, -1), (33, 7, 0, 0), (3, 0, 6, 7)])
def test_segmented_references_are_the_one_problem_references_at_one_problem(P, F, Co, n):
    rng = np.random.default_rng(P * 100 + F)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)
    s = H.seg_edges(H.seg_layout([(P, F, Co)], [4]), [n], rng)
    Nn, Ec, C, D, ne = s['Nn'], s['Ec'], 3, 8, int(s['n_edges'][0])
    assert Nn == P + F + Co and s['e0'][0] == 0 and s['cap'][0] == Ec
    src, dst = s['e_src'], s['e_dst']
    sj, ti = src[:ne], dst[:ne]
    cur, fr, co, old = f(P, C), f(F, C), f(Co, C), f(Nn, C + 3)
    got, mask = H.nodes_in_seg_ref(s, 1, 2.5, cur, fr, co, old)
    assert np.array_equal(got, H.sm_nodes_in_ref(cur, fr, co, 2.5)) and mask.all()
    got, mask = H.nodes_in_seg_ref(s, 0, 2.5, cur, fr, co, old)
    assert np.array_equal(got, old) and not mask.any()
    X = f(Nn, D)
    assert np.array_equal(H.msg_in_seg_ref(s, 1, X), H.sm_msg_in_ref(src, dst, ne, X))
    assert not H.msg_in_seg_ref(s, 0, X).any()
    dZ = f(Ec, 3 * D)
    z = dZ[:ne]
    acc, mag, fan, mask = H.msg_in_bwd_seg_ref(s, 1, dZ)
    a1, m1 = H.segment_sum_ref(Nn, D, [(sj, z[:, :D]), (sj, z[:, D:2 * D]), (ti, z[:, 2 * D:]), (ti, -z[:, :D])])
    assert np.array_equal(acc, a1) and np.array_equal(mag, m1) and mask.all()
    assert fan == (int((np.bincount(sj, minlength=Nn) + np.bincount(ti, minlength=Nn)).max()) if ne else 1)
    M = f(Ec, D)
    acc, mag, fan = H.scatter_add_seg_ref(s, 1, M)
    a1, m1 = H.segment_sum_ref(Nn, D, [(ti, M[:ne])])
    assert np.array_equal(acc, a1[:P]) and np.array_equal(mag, m1[:P]) and not a1[P:].any()
    dS = f(P, D)
    ref = np.zeros((Ec, D), np.float32)
    ref[:ne] = dS[ti]
    assert np.array_equal(H.scatter_add_bwd_seg_ref(s, 1, dS), ref) and not H.scatter_add_bwd_seg_ref(s, 0, dS).any()
    Y, oldp = f(P, D), f(P, D)
    got, mask = H.add_path_seg_ref(s, 1, X, Y, oldp)
    assert np.array_equal(got, X[:P] + Y) and mask.all()
    assert np.array_equal(H.add_path_bwd_seg_ref(s, 1, Y), np.concatenate([Y, np.zeros((F + Co, D), np.float32)]))
    prev, prop = f(P, C), f(P, C)
    assert np.array_equal(H.path_update_seg_ref(s, 1, prev, prop), H.sm_path_update_ref(prev, prop))
    assert np.array_equal(H.path_update_seg_ref(s, 0, prev, prop), prev)
    dp, dq = H.path_update_bwd_seg_ref(s, 1, prev)
    assert np.array_equal(dp + dq, prev) and np.array_equal(dp, H.sm_path_update_ref(np.zeros_like(prev), prev))
    dp, dq = H.path_update_bwd_seg_ref(s, 0, prev)
    assert not dp.any() and np.array_equal(dq, prev)
    dXin, oldc = f(Nn, C + 3), f(P, C)
    got, mask = H.coords_bwd_seg_ref(s, 1, dXin, oldc)
    assert np.array_equal(got, oldc + dXin[:P, :C]) and mask.all()
    part, dg, db = f(1, 1, 2, D), f(D), f(D)
    g1, b1 = H.bn_seg_dgb_ref(part, dg, db)
    assert np.array_equal(g1, dg + part[0, 0, 0]) and np.array_equal(b1, db + part[0, 0, 1]) and g1.dtype == np.float32


def test_loop_count_references():
    rng = np.random.default_rng(3)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)
    NC, Hs = f(256, 4), f(1, 256, 4)
    assert np.array_equal(H.final_cat_ref([256], NC, Hs), np.concatenate([NC, Hs[0]], 1))       # one iteration: model.py:143 as it stands
    rows = [768, 512, 512, 256]
    NC, Hs = f(768, 4), f(4, 768, 4)
    got = H.final_cat_ref(rows, NC, Hs)
    assert np.array_equal(got[:256, 4:], Hs[3, :256]) and np.array_equal(got[256:512, 4:], Hs[2, 256:512])
    assert np.array_equal(got[512:, 4:], Hs[0, 512:]) and np.array_equal(got[:, :4], NC)
    d_dec, dXin = f(512, 4), f(512, 16)
    assert np.array_equal(H.seed_dh_ref(0, d_dec, dXin), d_dec) and np.array_equal(H.seed_dh_ref(512, d_dec, dXin), dXin[:, 12:])
    got = H.seed_dh_ref(256, d_dec, dXin)
    assert np.array_equal(got[:256], dXin[:256, 12:]) and np.array_equal(got[256:], d_dec[256:])
    for t in H.FINAL_CAT_TABLES:
        assert 1 <= len(t) <= 64 and all(r % 256 == 0 for r in t) and all(a >= b for a, b in zip(t, t[1:]))
    assert len(H.FINAL_CAT_TABLES[2]) == 64
