"""gnnmp_frontier_rank (csrc/frontier_kernels.hip) against its numpy restatement ``rank_rows_host``: exact -- row_beg, row_len,
the cols prefix and the vals prefix bitwise -- on a ragged batch, at every row length where the kernels change path
(``gnnmp_frontier_limits``), with duplicate columns, with and without prefix arrays, twice in a row, and with a node id outside
its graph; then ``planner.explore(frontier='ranked')`` against ``sparse=True`` on real maze problems with the shipped weights."""
import numpy as np
import pytest
import torch

from conftest import golden_files, load_weights
import gnnmp
from gnnmp import planner
from gnnmp.frontier import limits, rank_rows, rank_rows_host
from gnnmp.maze2d import Maze2D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
VALUES = np.array([-2.1, -1.3, 0.0, -0.0, 0.5, 0.5, 0.5, 1.7], dtype=np.float32)       # ties, +-0, negatives


def _random_graph(rng, n, e, values=VALUES):
    """Random columns (self loops and repeated cells included, unsorted) and a collided suffix."""
    ei = rng.randint(0, n, size=(2, e)).astype(np.int64) if e else np.zeros((2, 0), dtype=np.int64)
    return ei, rng.choice(values, size=e).astype(np.float32), n - int(rng.randint(0, n // 4 + 1))


def _join(graphs, sizes):
    nptr = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    eptr = np.concatenate(([0], np.cumsum([g[0].shape[1] for g in graphs]))).astype(np.int32)
    return (np.ascontiguousarray(np.concatenate([g[0] for g in graphs], axis=1)), np.concatenate([g[1] for g in graphs]),
            np.array([g[2] for g in graphs], dtype=np.int32), nptr, eptr)


def _device(sc, ei, nf, nptr=None, eptr=None, n_nodes=None, out=None):
    t = lambda x: None if x is None else torch.from_numpy(np.asarray(x)).to(DEV)          # noqa: E731
    return rank_rows(t(sc), t(ei), t(np.atleast_1d(np.asarray(nf, dtype=np.int32))), t(nptr), t(eptr), n_nodes=n_nodes, out=out)


def _prefix_index(row_beg, row_len):
    """Positions of every row's live prefix in cols / vals."""
    rep = np.repeat(np.arange(row_len.shape[0]), row_len)
    return row_beg[rep].astype(np.int64) + np.arange(rep.shape[0]) - np.repeat(np.cumsum(row_len) - row_len, row_len)


def _assert_equal(got, ref):
    (gb, gl, gc, gv), (rb, rl, rc, rv) = got, ref
    assert np.array_equal(gb, rb)
    assert np.array_equal(gl, rl)
    at = _prefix_index(rb, rl)
    assert np.array_equal(gc[at], rc[at])
    assert np.array_equal(gv[at].view(np.int32), rv[at].view(np.int32))
    return at


@pytest.fixture(scope='module')
def ragged():
    rng = np.random.RandomState(7)
    sizes = [1, 2, 37, 300, 1100]
    graphs = [_random_graph(rng, 1, 0),                                     # no column at all
              (np.array([[0, 1, 1], [1, 0, 1]], dtype=np.int64), np.zeros(3, dtype=np.float32), 2),      # every score 0
              _random_graph(rng, 37, 400), _random_graph(rng, 300, 6000), _random_graph(rng, 1100, 22000)]
    ei, sc, nf, nptr, eptr = _join(graphs, sizes)
    return {'graphs': graphs, 'sizes': sizes, 'ei': ei, 'sc': sc, 'nf': nf, 'nptr': nptr, 'eptr': eptr,
            'ref': rank_rows_host(sc, ei, nf, nptr, eptr).host()}


def test_ragged_batch(ragged):
    r = ragged
    got = _device(r['sc'], r['ei'], r['nf'], r['nptr'], r['eptr'], n_nodes=int(r['nptr'][-1])).host()
    at = _assert_equal(got, r['ref'])
    assert at.size > 10000 and r['ref'][1][:3].tolist() == [0, 0, 0]        # the empty and the all-zero graph: no live cell


def test_row_length_boundaries():
    """One hub row per graph, of every length at which another path is taken; few distinct scores, so the order inside a row
    rests on the source-id rule."""
    wave, tile = limits()
    lengths = [0, 1, 2, wave - 1, wave, wave + 1, tile - 1, tile, tile + 1, 3000]
    assert sorted(set(lengths)) == lengths
    rng = np.random.RandomState(11)
    graphs, sizes = [], []
    for L in lengths:
        n = L + 3
        hub = int(rng.randint(0, n))
        src = np.array([x for x in range(n) if x != hub][:L], dtype=np.int64)          # L distinct sources: in-degree L exactly
        extra = rng.randint(0, n, size=(2, 4)).astype(np.int64)
        extra[1][extra[1] == hub] = (hub + 1) % n
        ei = np.concatenate((np.stack((src, np.full(L, hub, dtype=np.int64))), extra), axis=1)
        sc = rng.choice(np.array([0.5, 0.5, 0.5, 1.0, -1.0, 0.0], dtype=np.float32), size=ei.shape[1])
        perm = rng.permutation(ei.shape[1])
        graphs.append((ei[:, perm], sc[perm], n - (L % 3 == 0)))
        sizes.append(n)
    ei, sc, nf, nptr, eptr = _join(graphs, sizes)
    ref = rank_rows_host(sc, ei, nf, nptr, eptr).host()
    got = _device(sc, ei, nf, nptr, eptr, n_nodes=int(nptr[-1])).host()
    _assert_equal(got, ref)
    assert int(ref[1].max()) > 2000                                          # the hub of 3000 keeps most of its cells


def test_graph_beyond_the_lds_histogram():
    """A graph with more nodes than any LDS table of counters could hold (160 KB = 40 k ints): its target histogram and row
    cursors go through global memory.  A small graph rides along on the LDS path."""
    rng = np.random.RandomState(12)
    sizes = [50000, 30]
    graphs = [_random_graph(rng, 50000, 120000), _random_graph(rng, 30, 200)]
    hub = graphs[0][0]
    hub[1, :700] = 4321                                                      # and one row of the big graph beyond the wave path
    ei, sc, nf, nptr, eptr = _join(graphs, sizes)
    ref = rank_rows_host(sc, ei, nf, nptr, eptr).host()
    got = _device(sc, ei, nf, nptr, eptr, n_nodes=int(nptr[-1])).host()
    _assert_equal(got, ref)
    assert int(ref[1][4321]) > limits()[0]


def test_duplicate_columns_last_one_wins():
    """A short row, a row of one tile and a row of more than two tiles whose sources repeat: whatever order the cells arrive
    in, pairs of one source sit in different tiles of the long row."""
    wave, tile = limits()
    rng = np.random.RandomState(13)
    graphs, sizes = [], []
    for L, distinct in ((40, 15), (wave + 300, wave), (2 * tile + 100, tile)):
        n = distinct + 2
        src = rng.randint(1, n, size=L).astype(np.int64)
        ei = np.stack((src, np.zeros(L, dtype=np.int64)))
        sc = rng.choice(np.array([0.25, 0.5, 0.5, 1.75, 3.0, 0.0, 0.0], dtype=np.float32), size=L)
        graphs.append((ei, sc, n))
        sizes.append(n)
    # and by hand: cell (0, 1) three times, last value 0 -> dead; cell (0, 2) twice, last value wins over a larger earlier one
    graphs.append((np.array([[1, 2, 1, 2, 1], [0, 0, 0, 0, 0]], dtype=np.int64), np.array([5., 9., 6., 1., 0.], dtype=np.float32), 3))
    sizes.append(3)
    ei, sc, nf, nptr, eptr = _join(graphs, sizes)
    ref = rank_rows_host(sc, ei, nf, nptr, eptr).host()
    got = _device(sc, ei, nf, nptr, eptr, n_nodes=int(nptr[-1])).host()
    _assert_equal(got, ref)
    lo = int(got[0][nptr[3]])
    assert int(got[1][nptr[3]]) == 1 and int(got[2][lo]) == 2 and float(got[3][lo]) == 1.0
    assert int(ref[1][nptr[2]]) < tile                                       # fewer live cells than sources: duplicates were merged


def test_one_graph_without_prefix_arrays(ragged):
    r = ragged
    ei, sc, nf = r['graphs'][3]
    got = _device(sc, ei, nf, n_nodes=r['sizes'][3]).host()
    n0, n1, e0 = int(r['nptr'][3]), int(r['nptr'][4]), int(r['eptr'][3])
    rb, rl, rc, rv = r['ref']
    sub = (rb[n0:n1] - e0, rl[n0:n1], rc[e0:e0 + ei.shape[1]], rv[e0:e0 + ei.shape[1]])
    _assert_equal(got, sub)


def test_two_runs_are_byte_identical(ragged):
    r = ragged
    holder = None
    blocks = []
    for _ in range(2):
        holder = _device(r['sc'], r['ei'], r['nf'], r['nptr'], r['eptr'], n_nodes=int(r['nptr'][-1]), out=holder)
        rb, rl, co, va = holder.host()
        at = _prefix_index(rb, rl)
        blocks.append(b''.join(x.tobytes() for x in (rb, rl, co[at], va[at])))
    assert blocks[0] == blocks[1]


def test_bad_node_id_names_its_graph():
    rng = np.random.RandomState(17)
    sizes = [50, 20, 64, 33]
    clean = [_random_graph(rng, n, 12 * n) for n in sizes]
    ei2 = clean[2][0].copy()
    ei2[0, 5], ei2[1, 17], ei2[0, 100], ei2[1, 200] = 64, -1, 1 << 40, -(1 << 40)         # just outside, negative, far outside
    graphs = clean[:2] + [(ei2, clean[2][1], clean[2][2])] + clean[3:]
    ei, sc, nf, nptr, eptr = _join(graphs, sizes)
    rr = _device(sc, ei, nf, nptr, eptr, n_nodes=int(nptr[-1]))
    with pytest.raises(RuntimeError, match=r'graph 2\b'):
        rr.host()
    assert rr.status.cpu().tolist() == [0, 0, -8, 0]
    got = rr.host(check=False)
    _assert_equal(got, rank_rows_host(sc, ei, nf, nptr, eptr).host(check=False))           # (it drops the same columns)
    # the other three graphs: as if graph 2 had been in order
    ei_c, sc_c, _, _, _ = _join(clean, sizes)
    rb, rl, rc, rv = rank_rows_host(sc_c, ei_c, nf, nptr, eptr).host()
    for g in (0, 1, 3):
        n0, n1 = int(nptr[g]), int(nptr[g + 1])
        assert np.array_equal(got[0][n0:n1], rb[n0:n1]) and np.array_equal(got[1][n0:n1], rl[n0:n1])
        at = _prefix_index(rb[n0:n1], rl[n0:n1])
        assert np.array_equal(got[2][at], rc[at]) and np.array_equal(got[3][at].view(np.int32), rv[at].view(np.int32))


def _models():
    m = gnnmp.EncoderProcessDecoder(2, 2, 32, 2).eval()
    m.load_state_dict(load_weights('weights_maze'))
    ms = gnnmp.ModelSmoother(workspace_size=2, config_size=2, embed_size=128, obs_size=6).eval()
    ms.load_state_dict(load_weights('smooth_2d_attv3'))
    return m, ms


@pytest.mark.parametrize('n_problems,batch,t_max,k', [(4, 500, 500, 30), (6, 100, 300, 12)], ids=['default', 'resample_rounds'])
def test_explore_ranked_equals_the_sparse_frontier(n_problems, batch, t_max, k):
    """Real maze problems, shipped weights, seed 1234: the ranked frontier takes the decisions of the heap, problem by problem.
    The second setting needs resample rounds, so trees and the explored-edge history (the legacy-index quirk) carry over."""
    with np.load(golden_files('evalset_mazehard_first12')[0]) as f:
        r = {key: f[key] for key in f.files}
    m, ms = _models()
    runs = {}
    for mode, kw in (('ranked', dict(frontier='ranked')), ('heap', dict(sparse=True))):
        env = Maze2D(r['maps'], r['init_states'], r['goal_states'])
        np.random.seed(1234)
        torch.manual_seed(1234)
        out = []
        for idx in range(n_problems):
            env.init_new_problem(idx)
            out.append(planner.explore(env, m, ms, True, batch=batch, t_max=t_max, k=k, device=DEV, gpu_graph=True, **kw))
        runs[mode] = out
    rounds = 0
    for a, b in zip(runs['ranked'], runs['heap']):
        assert a['success'] == b['success']
        assert a['explored'] == b['explored']
        assert a['explored_edges'] == b['explored_edges']
        assert a['c_explore'] == b['c_explore'] and a['c_smooth'] == b['c_smooth']
        assert np.array_equal(np.array(a['path']), np.array(b['path']))
        assert np.array_equal(np.array(a['smooth_path']), np.array(b['smooth_path']))
        rounds = max(rounds, a['forward_split']['calls'])
    assert any(x['success'] for x in runs['ranked'])
    if batch < t_max:
        assert rounds > 1                                                    # the setting did take resample rounds
