"""gnnmp_episode_dataset_gather (gnnmp.explorer_replay.ExplorerDataset.batch): a group of labelled graphs out of the device
dataset in one launch, bit for bit against a torch gather of the same rows.

The store: a problem of ONE node (its one self-loop), one with an empty map (0 obstacle rows), one of 400 nodes (a workgroup of
256 threads strides its copy more than once), the rest between 100 and 150 nodes; appended in two chunks.  The index lists:
[3, 0, 3, 4] (a repeat, descending order), G = 1, and G = 70 (the scan crosses one wave's 64 entries)."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import episodes as ep
from gnnmp import explorer_replay as er

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = {2: [1, 120, 400, 131, 147, 103], 3: [101, 130, 1]}
LISTS = {'repeat': [3, 0, 3, 4], 'G1': [2], 'G70': np.random.RandomState(70).randint(0, 6, 70).tolist()}
_STORE = {}


def _store(dim):
    """The problems, the dataset and ONE TrainingGraphs over all of them (what the torch gather reads), built once."""
    if dim not in _STORE:
        rng = np.random.default_rng(20 + dim)
        sizes = SIZES[dim]
        lim = np.array([1.0, 1.0, 0.4])[:dim]
        pts = [rng.uniform(-lim, lim, (n, dim)) for n in sizes]
        maps = (rng.random((len(sizes), 15, 15)) < 0.2).astype(np.float64)
        maps[1] = 0.0                                             # no obstacle rows
        nptr = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        ds = er.ExplorerDataset(dim, DEV)
        cut = 2
        assert ds.add(torch.from_numpy(np.concatenate(pts[:cut])).to(DEV), nptr[:cut + 1], maps[:cut]) == cut
        assert ds.add(torch.from_numpy(np.concatenate(pts[cut:])).to(DEV), [x - nptr[cut] for x in nptr[cut:]], maps[cut:]) == len(sizes) - cut
        full = ep.maze_training_graphs(torch.from_numpy(np.concatenate(pts)).to(DEV), nptr, maps, dim)
        _STORE[dim] = (pts, maps, ds, full)
    return _STORE[dim]


def _rows(ptr, idx):
    return torch.from_numpy(np.concatenate([np.arange(ptr[i], ptr[i + 1]) for i in idx] + [np.zeros(0, np.int64)]).astype(np.int64)).to(DEV)


def _check_equal(g, full, idx):
    """Every array of the gathered batch against the torch gather of problems ``idx`` out of ``full``."""
    nodes, edges, obs = (_rows(p, idx) for p in (full.node_ptr_host, full.edge_ptr_host, full.obs_ptr_host))
    assert torch.equal(g.v, full.v[nodes]) and g.v.dtype == torch.float32
    assert torch.equal(g.points64, full.points64[nodes]) and g.points64.dtype == torch.float64
    assert torch.equal(g.edge_index, full.edge_index[:, edges]) and g.edge_index.dtype == torch.int64
    assert torch.equal(g.edge_free, full.edge_free[edges]) and g.edge_free.dtype == torch.uint8
    assert torch.equal(g.edge_cost, full.edge_cost[edges]) and g.edge_cost.dtype == torch.float64
    assert torch.equal(g.obstacles, full.obstacles[obs]) and g.obstacles.dtype == torch.float32
    for name in ('node_ptr', 'edge_ptr', 'obs_ptr'):
        host = getattr(full, name + '_host')
        want = np.concatenate([[0], np.cumsum([host[i + 1] - host[i] for i in idx])]).astype(np.int64)
        got = getattr(g, name)
        assert got.dtype == torch.int32 and got.cpu().tolist() == want.tolist(), name
        assert getattr(g, name + '_host') == want.tolist(), name
    assert g.n_problems == len(idx) and g.total_nodes == int(nodes.numel()) and g.total_edges == int(edges.numel())


def test_store_holds_what_it_was_given():
    pts, maps, ds, full = _store(2)
    assert len(ds) == 6 and ds.sizes() == SIZES[2]
    assert full.sizes()[0] == 1 and full.edge_ptr_host[1] == 1                  # the single node's one self-loop
    assert full.obs_ptr_host[2] == full.obs_ptr_host[1]                         # the empty map
    for name in ('v', 'points64', 'edge_index', 'edge_free', 'edge_cost', 'obstacles'):
        assert torch.equal(getattr(ds, name), getattr(full, name)), name
    for name in ('node_ptr', 'edge_ptr', 'obs_ptr'):
        assert getattr(ds, name).cpu().tolist() == getattr(full, name + '_host') == getattr(ds, 'host_' + name).tolist(), name


@pytest.mark.parametrize('which', list(LISTS))
def test_gather_equals_torch_gather(which):
    pts, maps, ds, full = _store(2)
    idx = LISTS[which]
    g = ds.batch(idx)
    _check_equal(g, full, idx)
    ds.check_status()


def test_gather_maze3():
    pts, maps, ds, full = _store(3)
    idx = [1, 0, 2, 1]
    _check_equal(ds.batch(idx), full, idx)
    ds.check_status()


def test_gathered_graphs_give_the_same_shortest_paths():
    pts, maps, ds, full = _store(2)
    idx = LISTS['repeat']
    g = ds.batch(idx)
    nptr = np.concatenate([[0], np.cumsum([SIZES[2][i] for i in idx])]).tolist()
    direct = ep.maze_training_graphs(torch.from_numpy(np.concatenate([pts[i] for i in idx])).to(DEV), nptr, maps[idx], 2)
    goal = [7, 0, 55, 146]
    a, b = ep.shortest_paths(g, goal), ep.shortest_paths(direct, goal)
    for key in ('dist', 'prev', 'n_valid'):
        assert torch.equal(a[key], b[key]), key
    assert int(a['n_valid'][1]) == 1                                            # the single node reaches itself only


@pytest.mark.parametrize('bad', [6, -1, 2 ** 31 + 5])
def test_index_outside_the_store_sets_status_and_leaves_the_other_slots(bad):
    pts, maps, ds, full = _store(2)
    g = ds.batch([3, bad, 1])
    # the bad slot is an empty problem; the other two are where a gather of [3, 1] puts them
    assert g.node_ptr_host[1] == g.node_ptr_host[2] and g.n_problems == 3
    nodes, edges, obs = (_rows(p, [3, 1]) for p in (full.node_ptr_host, full.edge_ptr_host, full.obs_ptr_host))
    assert torch.equal(g.v, full.v[nodes]) and torch.equal(g.points64, full.points64[nodes])
    assert torch.equal(g.edge_index, full.edge_index[:, edges]) and torch.equal(g.edge_cost, full.edge_cost[edges])
    assert torch.equal(g.edge_free, full.edge_free[edges]) and torch.equal(g.obstacles, full.obstacles[obs])
    for name in ('node_ptr', 'edge_ptr', 'obs_ptr'):
        assert getattr(g, name).cpu().tolist() == getattr(g, name + '_host'), name
    with pytest.raises(RuntimeError, match='status 1'):
        ds.check_status()
    ds.check_status()                                                           # cleared by the raise
