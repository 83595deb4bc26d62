"""CSR build of the prep stage's one-launch form: rows assembled in LDS and written out in slot order against the record-by-record
scatter (GNNMP_PREP_LDS_ROWS=0, read per call), in one process.

Both routes take the slots from the same LDS histogram, arrival ranks and block scan; only the way to memory differs.  The
arrival order inside a target's segment depends on timing, so the CSR is compared after the training path's segment sort
(gnnmp_train_geom_build: slots of a target ascending by caller column) -- that is a comparison of per-target SETS of (source,
column) -- and everything else the stage writes byte for byte: the whole explorer carve of the workspace (row_beg, deg,
node / edge tile -> graph maps, tile_meta, blk_span, goal node, padded prefix arrays, status words), started from the same junk.
The dumped geometry is also checked against the caller's edge list (train_ops_host.check_geometry), and the scores of a
forward over the same batch are compared bit for bit."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import gnnmp
from gnnmp import _lib
from conftest import load_weights
import train_ops_host as H

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SWITCH = 'GNNMP_PREP_LDS_ROWS'


@contextlib.contextmanager
def scatter_route(on):
    old = os.environ.get(SWITCH)
    if on:
        os.environ[SWITCH] = '0'
    else:
        os.environ.pop(SWITCH, None)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = old


def make_batch(graphs, seed):
    """graphs: [(n_nodes, edge_index [2, E] int64)] -> the host batch of train_ops_host.check_geometry (C = 2)"""
    rng = np.random.default_rng(seed)
    node_ptr = np.cumsum([0] + [n for n, _ in graphs]).astype(np.int32)
    edge_ptr = np.cumsum([0] + [e.shape[1] for _, e in graphs]).astype(np.int32)
    v = rng.uniform(-1, 1, size=(node_ptr[-1], 2)).astype(np.float32)
    goal = rng.uniform(-1, 1, size=(len(graphs), 2)).astype(np.float32)
    goal_local = []
    for g, (n, _) in enumerate(graphs):
        d = ((v[node_ptr[g]:node_ptr[g + 1]].astype(np.float64) - goal[g].astype(np.float64)) ** 2).sum(1)
        goal_local.append(int(np.argmin(d)))
    return dict(C=2, G=len(graphs), sizes=[n for n, _ in graphs], node_ptr=node_ptr, edge_ptr=edge_ptr, v=v, goal=goal,
                edge_index=np.concatenate([e for _, e in graphs], 1).astype(np.int64).reshape(2, -1), goal_local=goal_local)


def rand_edges(rng, n, e, targets=None):
    return np.stack([rng.integers(0, n, size=e), rng.integers(0, targets or n, size=e)])


def dump_geometry(b, scatter):
    """(explorer carve of the workspace as bytes, arrays of the geometry) after gnnmp_train_geom_build"""
    L = _lib.lib()
    E = b['edge_index'].shape[1]
    shape = _lib.Batch(b['G'], int(b['node_ptr'][-1]), E, 0, 0, None, None, None, None, None, None, None)
    need = ctypes.c_size_t()
    _lib.check(L.gnnmp_train_geom_workspace_bytes(ctypes.byref(shape), 2, ctypes.byref(need)), 'geom_workspace_bytes')
    ins = [b['v'].view(np.uint8).reshape(-1), b['goal'].view(np.uint8).reshape(-1), b['node_ptr'].view(np.uint8),
           b['edge_ptr'].view(np.uint8), np.ascontiguousarray(b['edge_index']).view(np.uint8).reshape(-1)]
    offs, o = [], (need.value + 255) & ~255
    for a in ins:
        offs.append(o)
        o += (a.size + 255) & ~255
    host = np.zeros(o + 256, np.uint8)
    host[:need.value] = 0xA5                                     # junk where the workspace is: nothing may rely on zeros
    for a, off in zip(ins, offs):
        host[off:off + a.size] = a
    mem = torch.from_numpy(host).to(DEV)
    base = mem.data_ptr()
    assert base % 256 == 0
    batch = _lib.Batch(b['G'], int(b['node_ptr'][-1]), E, 0, 0, base + offs[0], base + offs[1], None,
                       base + offs[4] if E else None, base + offs[2], base + offs[3], None)
    geom = _lib.TrainGeom()
    with scatter_route(scatter):
        _lib.check(L.gnnmp_train_geom_build(ctypes.byref(batch), 2, base, need.value, ctypes.byref(geom),
                                            torch.cuda.current_stream().cuda_stream), 'geom_build')
        torch.cuda.synchronize()
    dump = mem.cpu().numpy()

    def arr(ptr, n):
        off = ptr - base
        assert 0 <= off and off + 4 * n <= need.value
        return dump[off:off + 4 * n].view(np.int32).copy()
    Np, Ep = geom.n_pad, geom.e_pad
    gd = dict(n_pad=Np, e_pad=Ep, node_ptr_pad=arr(geom.node_ptr_pad, b['G'] + 1), ntile_graph=arr(geom.ntile_graph, Np // 32),
              goal_node=arr(geom.goal_node, b['G']), row_beg=arr(geom.row_beg, Np), deg=arr(geom.deg, Np), csr=arr(geom.csr, 4 * Ep),
              out_beg=arr(geom.out_beg, Np), out_cnt=arr(geom.out_cnt, Np), out_slot=arr(geom.out_slot, Ep))
    carve = dump[:geom.out_beg - base].copy()                    # the out lists of the training path start where the explorer carve ends
    return carve, gd


def scores(b, scatter, n_obs=5, loop=2):
    rng = torch.Generator().manual_seed(7)
    graphs = []
    for g in range(b['G']):
        n0, n1, e0, e1 = b['node_ptr'][g], b['node_ptr'][g + 1], b['edge_ptr'][g], b['edge_ptr'][g + 1]
        graphs.append({'v': torch.from_numpy(b['v'][n0:n1]), 'goal': torch.from_numpy(b['goal'][g]),
                       'obstacles': torch.rand(n_obs, 2, generator=rng) - 0.5, 'edge_index': torch.from_numpy(b['edge_index'][:, e0:e1])})
    m = gnnmp.EncoderProcessDecoder(2, 2, 32, 2).eval()
    m.load_state_dict(load_weights('weights_maze'))
    m.status_checks = False
    gb = gnnmp.GraphBatch.from_graphs(graphs, 2, DEV)
    with scatter_route(scatter):
        s = m.forward_batch(gb, loop)
        torch.cuda.synchronize()
    cb = m._cbatch(gb)
    first = ctypes.c_int32(-5)
    rc = _lib.lib().gnnmp_explorer_status(m._native(torch.device(DEV)), ctypes.byref(cb), m._ws.data_ptr(), m._ws.numel(), None,
                                          ctypes.byref(first))
    return s.cpu(), rc, first.value


def both_routes(b, check=True):
    carve_l, gd_l = dump_geometry(b, scatter=False)
    carve_s, gd_s = dump_geometry(b, scatter=True)
    for k in gd_l:
        assert np.array_equal(gd_l[k], gd_s[k]), k
    assert np.array_equal(carve_l, carve_s)
    if check:
        H.check_geometry(b, gd_l)
    s_l, rc_l, first_l = scores(b, scatter=False)
    s_s, rc_s, first_s = scores(b, scatter=True)
    assert s_l.numpy().tobytes() == s_s.numpy().tobytes()
    assert (rc_l, first_l) == (rc_s, first_s)
    return gd_l, rc_l, first_l


def test_one_graph_across_a_tile_boundary():
    rng = np.random.default_rng(1)
    gd, rc, _ = both_routes(make_batch([(33, rand_edges(rng, 33, 70))], 1))
    assert rc == 0 and gd['e_pad'] >= 96 and int(gd['deg'].sum()) == 70


def test_ragged_graphs():
    rng = np.random.default_rng(2)
    graphs = [(1, np.zeros((2, 0), np.int64)), (64, rand_edges(rng, 64, 31)), (257, rand_edges(rng, 257, 2048))]
    gd, rc, _ = both_routes(make_batch(graphs, 2))
    assert rc == 0 and int(gd['deg'].sum()) == 31 + 2048


def test_nodes_without_incoming_edges():
    rng = np.random.default_rng(3)
    n = 200
    b = make_batch([(n, rand_edges(rng, n, 900, targets=150)), (40, rand_edges(rng, 40, 100))], 3)      # nodes 150 .. 199: sources only
    gd, rc, _ = both_routes(b)
    assert rc == 0 and (gd['deg'][gd['node_ptr_pad'][0] + 150:gd['node_ptr_pad'][0] + 200] == 0).all()


@pytest.mark.parametrize('over', [0, 1], ids=['fits', 'one_too_many'])
def test_at_the_lds_capacity(over):
    """One graph of 13000 nodes is cut into eight slices of 1632 padded nodes; slices of that size keep the large counter layout,
    whose record area is smaller than the 16 k columns a workgroup may keep in registers.  Every edge points into the first
    slice: E = capacity takes the LDS route there, E = capacity + 1 the scatter (the other seven slices own nothing)."""
    n = 13000
    cap = int(_lib.lib().gnnmp_prep_lds_row_capacity(13312 // 8))           # the launch's bound on padded nodes: N + 255, rounded up
    assert 8192 < cap < 16384 - 1                                # parts = 1 and the columns stay in registers up to 16 k edges
    assert int(_lib.lib().gnnmp_prep_lds_row_capacity(128)) >= 16384      # small slices: room for whatever stays in registers
    rng = np.random.default_rng(4)
    e = cap + over
    gd, rc, _ = both_routes(make_batch([(n, rand_edges(rng, n, e, targets=1600))], 4))
    assert rc == 0 and gd['n_pad'] == 13312 and int(gd['deg'][:1632].sum()) == e


def test_node_id_out_of_range_keeps_its_status():
    rng = np.random.default_rng(5)
    graphs = [(50, rand_edges(rng, 50, 300)), (33, rand_edges(rng, 33, 70))]
    graphs[1][1][1, 5] = 33                                      # a target one behind the second graph
    graphs[0][1][0, 7] = -1
    b = make_batch(graphs, 5)
    _, rc, first = both_routes(b, check=False)
    assert rc == -8 and first == 0                               # GNNMP_ERR_INDEX, first offending graph
