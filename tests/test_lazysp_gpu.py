"""LazySP on the device (gnnmp.lazysp.plan_maze_batch and the gnnmp_lazysp_* entry points) against the recorded runs of the
reference (tests/golden/lazysp_*.npz) and, at shapes the fixtures do not reach, against gnnmp.lazysp.plan_host: every field
exactly.  Reads only tests/golden/ and the package."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import _lib, lazysp
from gnnmp.graph_build import build_edges_gpu

from test_lazysp_host import CASES, EXACT_FIELDS, assert_same_plan, load_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SCAN = 64                # nodes per pass of the minimum scan (one per lane) = path edges per pass of the parallel edge check


def problem_of(rec):
    return dict(map=rec['map'], init_state=rec['init_state'], goal_state=rec['goal_state'])


def settings_of(rec):
    return int(rec['dim']), int(rec['batch']), int(rec['t_max']), int(rec['k'])


GROUPS = {}
for _name in CASES:
    GROUPS.setdefault(settings_of(load_case(_name)), []).append(_name)
_HOST = {}


def host_plan(problem, seed, batch, t_max, k):
    """plan_host once per (problem, settings): the oracle is shared among the tests and left unchanged."""
    key = (problem['map'].tobytes(), problem['init_state'].tobytes(), problem['goal_state'].tobytes(), seed, batch, t_max, k)
    if key not in _HOST:
        _HOST[key] = lazysp.plan_host(problem, seed, batch=batch, t_max=t_max, k=k)
    return _HOST[key]


def assert_same_result(a, b, what):
    assert np.array_equal(a['samples'], b['samples']), what
    for key in EXACT_FIELDS + ('path',):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])) and np.asarray(a[key]).shape == np.asarray(b[key]).shape, \
            '%s: %s' % (what, key)


@pytest.mark.parametrize('group', sorted(GROUPS), ids=lambda g: 'maze%d_b%d_t%d_k%d' % g)
@pytest.mark.parametrize('draws', ['host', 'device'])
def test_plan_maze_batch_equals_reference(group, draws):
    """Every fixture of one setting as one batch, both ways of drawing: each field exactly the reference's."""
    dim, batch, t_max, k = group
    recs = [load_case(n) for n in GROUPS[group]]
    res = lazysp.plan_maze_batch([problem_of(r) for r in recs], DEV, [int(r['seed']) for r in recs], batch=batch, t_max=t_max, k=k,
                                 draws=draws)
    for name, rec, got in zip(GROUPS[group], recs, res):
        assert got['status'] == 0 and got['success'] == (len(rec['path_ids']) > 0), name
        assert_same_plan(got, rec, '%s (%s draws)' % (name, draws))


def run_abi(rec, pair_cap=None, spare_slot=False, attempts=None):
    """The rounds of one recorded problem through the C entry points with an explicit host loop (slot 0 of the store; with
    ``spare_slot`` a second slot that no call touches, its arrays filled with a sentinel).  ``attempts``: [n, dim] raw doubles
    that take the place of the seed's stream, one row a draw (``low + row * ranges``).  Returns (result dict, store)."""
    dim, batch, t_max, k = settings_of(rec)
    B = 2 if spare_slot else 1
    R = lazysp.n_rounds(batch, t_max)
    store = lazysp.LazySPStore(B, R * batch, lazysp.rounds_pair_cap(batch, t_max, k) if pair_cap is None else pair_cap, dim, DEV)
    if spare_slot:
        store.pairs[1].fill_(-7)
        store.pair_state[1].fill_(9)
        store.path[1].fill_(-7)
        store.pool[1].fill_(-7.0)
    f64 = lambda x, shape: torch.from_numpy(np.broadcast_to(np.asarray(x, dtype=np.float64), shape).copy()).to(DEV)      # noqa: E731
    w = rec['map'].shape[0]
    maps, init64, goal64 = f64(rec['map'], (B, w, w)), f64(rec['init_state'], (B, dim)), f64(rec['goal_state'], (B, dim))
    limits = np.asarray(lazysp._maze_class(dim).SAMPLE_LIMITS)
    k1_np = np.ones(store.cap + 3, dtype=np.int32)
    k1_np[2:] = [lazysp.k1_of(k, q) for q in range(2, store.cap + 3)]
    k1_table = torch.from_numpy(k1_np).to(DEV)
    active = torch.tensor([1] + [0] * (B - 1), dtype=torch.uint8, device=DEV)
    slot_of = torch.zeros(1, dtype=torch.int32, device=DEV)
    rs, buf = np.random.RandomState(int(rec['seed'])), np.zeros((0, dim))
    if attempts is not None:
        rs, buf = None, -limits + np.asarray(attempts, dtype=np.float64) * (limits - (-limits))
    rounds, rows = 0, []
    for r in range(1, R + 1):
        want = 64
        while True:
            if rs is not None and buf.shape[0] < want:
                buf = np.concatenate((buf, rs.uniform(-limits, limits, (want - buf.shape[0], dim))))
            att_ptr = np.array([0] + [buf.shape[0]] * B, dtype=np.int64)
            used, _, status = lazysp.lazysp_sample(store, torch.from_numpy(buf).to(DEV), att_ptr, maps, init64, goal64, batch, active=active)
            if int(status[0]) == 0:
                buf = buf[int(used[0]):]
                break
            assert int(status[0]) == 1 and int(used[0]) == 0 and rs is not None
            want *= 2
        g = lazysp.lazysp_gather(store, slot_of, k1_table, 2 + r * batch)
        assert g['node_ptr'].tolist() == [0, 2 + r * batch] and g['n_free'].tolist() == [2 + r * batch]
        assert g['k1'].tolist() == [lazysp.k1_of(k, 2 + r * batch)]
        assert torch.equal(g['v'], store.pool[0, :2 + r * batch].to(torch.float32))
        ei, edge_ptr = build_edges_gpu(g['v'], g['node_ptr'], g['n_free'], g['k1'])
        lazysp.lazysp_round(store, None, ei, edge_ptr, maps)
        torch.cuda.synchronize()
        rounds = r
        state = store.pair_state[0, :int(store.n_pairs[0])]
        rows.append((int(store.n_nodes[0]), int(store.checks[0]), int((state == 1).sum()), int((state == 2).sum())))
        if int(store.solved[0]) or int(store.status[0]):
            break
    n, npairs, plen = int(store.n_nodes[0]), int(store.n_pairs[0]), int(store.path_len[0])
    pairs, st = store.pairs[0, :npairs].cpu().numpy(), store.pair_state[0, :npairs].cpu().numpy()
    pts = store.pool[0, :n].cpu().numpy()
    ids = store.path[0, :plen].cpu().numpy().astype(np.int64)
    return {'samples': pts, 'checks': int(store.checks[0]), 'path_ids': ids, 'path': pts[ids], 'T': rounds * batch,
            'valid_edges': lazysp._unordered(pairs[st == 1]), 'invalid_edges': lazysp._unordered(pairs[st == 2]),
            'dijkstra_runs': int(store.dijkstra_runs[0]), 'invalid_order': pairs[st == 2].astype(np.int64).reshape(-1, 2),
            'status': int(store.status[0]), 'n_pairs': npairs, 'pairs': pairs, 'pair_state': st,
            'rounds': np.array(rows, dtype=np.int64).reshape(-1, 4)}, store


@pytest.mark.parametrize('name', ['maze2_b20_t100_i3', 'maze3_round1_i6', 'maze2_firstinf_i0', 'maze2_b1_t6_i1'])
def test_c_abi_equals_reference(name):
    rec = load_case(name)
    got, _ = run_abi(rec)
    assert got['status'] == 0
    got['rounds'] = rec['rounds']                                  # (per-round figures: test_plan_maze_batch_equals_reference)
    assert_same_plan(got, rec, name)


def test_permuted_and_chunked_batches_and_two_runs():
    """Per-problem results do not depend on the order of the batch or on how it is cut, and a run repeats bit for bit.  The batch
    holds a problem finished in round 1 next to problems that go on for several rounds: their later rounds are undisturbed."""
    names = GROUPS[(2, 20, 100, 10)]
    recs = [load_case(n) for n in names]
    assert any(len(r['rounds']) == 1 and len(r['path_ids']) for r in recs) and any(len(r['rounds']) > 1 for r in recs)
    run = lambda order: lazysp.plan_maze_batch([problem_of(recs[i]) for i in order], DEV, [int(recs[i]['seed']) for i in order],      # noqa: E731
                                               batch=20, t_max=100, k=10)
    full = run(range(len(recs)))
    again = run(range(len(recs)))
    perm = [2, 0, 3, 1]
    permuted = run(perm)
    chunks = run(perm[:3]) + run(perm[3:])
    late_only = run([i for i in range(len(recs)) if len(recs[i]['rounds']) > 1])
    for j, i in enumerate(perm):
        assert_same_result(permuted[j], full[i], 'permuted %s' % names[i])
        assert_same_result(chunks[j], full[i], 'chunked %s' % names[i])
    for a, b, n in zip(full, again, names):
        assert_same_result(a, b, 'second run %s' % n)
        assert np.array_equal(a['samples'].view(np.uint64), b['samples'].view(np.uint64))
    late = [i for i in range(len(recs)) if len(recs[i]['rounds']) > 1]
    for j, i in enumerate(late):
        assert_same_result(late_only[j], full[i], 'without the early finisher %s' % names[i])


def check_against_host(problems, seeds, batch, t_max, k):
    res = lazysp.plan_maze_batch(problems, DEV, seeds, batch=batch, t_max=t_max, k=k)
    hosts = [host_plan(p, s, batch, t_max, k) for p, s in zip(problems, seeds)]
    for i, (got, want) in enumerate(zip(res, hosts)):
        assert got['status'] == 0
        assert_same_plan(got, want, 'problem %d (batch %d, t_max %d, k %d)' % (i, batch, t_max, k))
    return res, hosts


@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('n_nodes', [SCAN - 1, SCAN, SCAN + 1, 2 * SCAN - 1, 2 * SCAN + 1])
def test_scan_width_boundaries(dim, n_nodes):
    """One fewer, exactly and one more node than the lanes of a scan pass (and than two passes), in one round."""
    recs = [load_case(n) for n in (('maze2_b50_t300_i1', 'maze2_b50_t300_i3') if dim == 2 else ('maze3_b50_t200_i0', 'maze3_round1_i6'))]
    check_against_host([problem_of(r) for r in recs], [5, 6], n_nodes - 2, n_nodes - 2, 10)


def test_lds_workspace_switch():
    """A node count on each side of the LDS / workspace switch of the per-node state, and the last LDS count itself."""
    lds = _lib.lib().gnnmp_lazysp_lds_nodes()
    recs = [load_case(n) for n in ('maze2_b50_t300_i2', 'maze2_b50_t300_i3')]
    for n_nodes in (lds, lds + 1):
        _, hosts = check_against_host([problem_of(r) for r in recs], [5, 5], n_nodes - 2, n_nodes - 2, 10)
        assert all(h['dijkstra_runs'] > 5 for h in hosts)           # the node state is rebuilt and reused, not written once


def serpentine(w=15):
    m = np.zeros((w, w))
    for i, row in enumerate(range(1, w, 2)):
        m[row, :] = 1
        if i % 2 == 0:
            m[row, w - 1:] = 0
        else:
            m[row, :1] = 0
    return m


def test_long_paths_over_several_edge_check_passes():
    """A serpentine corridor with few neighbours per node: paths of more than SCAN edges, so the parallel edge check needs
    several passes; among the runs the first blocked edge sits in the last lane of a pass (position SCAN - 1) and in the first
    lane of the next (position SCAN)."""
    c = lambda i: (i + 0.5) * 2 / 15 - 1      # noqa: E731
    pr = dict(map=serpentine(), init_state=np.array([c(0), c(0)]), goal_state=np.array([c(14), c(14)]))
    seeds = [3, 4, 5]
    res, hosts = check_against_host([pr] * 3, seeds, 500, 500, 6)
    blocked = np.concatenate([h['blocked_at'] for h in hosts])
    assert max(int(h['walk_edges'].max()) for h in hosts) > SCAN
    assert (blocked == SCAN - 1).any() and (blocked == SCAN).any() and (blocked > SCAN).any()
    assert any(len(h['path_ids']) > SCAN for h in hosts)


def test_carried_pair_that_left_the_graph():
    """Over several rounds a carried pair stops being an edge of the new, denser graph: it marks nothing and stays in the sets."""
    rec = load_case('maze2_b50_t300_i2')
    n = rec['samples'].shape[0]
    last = {(int(s), int(t)) for s, t in lazysp.graph_edges(rec['samples'], lazysp.k1_of(int(rec['k']), n))}
    carried = [tuple(p) for p in np.concatenate((rec['valid_edges'], rec['invalid_edges'])).tolist()]
    assert any(p not in last for p in carried)
    got = lazysp.plan_maze_batch([problem_of(rec)], DEV, [int(rec['seed'])], batch=50, t_max=300, k=10)[0]
    assert_same_plan(got, rec, 'maze2_b50_t300_i2')


@pytest.mark.parametrize('name', ['maze2_b20_t100_i1', 'maze3_round1_i6'])
def test_pair_list_full(name):
    """A pair list of exactly the entries the problem needs works; one entry fewer sets status bit 1, keeps every entry
    written inside the slot -- a prefix of the full list -- and leaves the neighbouring slot untouched."""
    rec = load_case(name)
    need = len(rec['valid_edges']) + len(rec['invalid_edges'])
    exact, store = run_abi(rec, pair_cap=need, spare_slot=True)
    print('pair_cap = need = %d: status %d, pairs %d, checks %d (reference %d), dijkstra runs %d (reference %d), samples equal %s'
          % (need, exact['status'], exact['n_pairs'], exact['checks'], int(rec['checks']), exact['dijkstra_runs'],
             int(rec['dijkstra_runs']), np.array_equal(exact['samples'], rec['samples'])))
    assert exact['status'] == 0 and exact['n_pairs'] == need
    exact['rounds'] = rec['rounds']
    assert_same_plan(exact, rec, name)
    short, store = run_abi(rec, pair_cap=need - 1, spare_slot=True)
    assert short['status'] & lazysp.STATUS_PAIR_OVERFLOW and len(short['path_ids']) == 0
    assert short['n_pairs'] <= need - 1 and np.array_equal(short['pairs'], exact['pairs'][:short['n_pairs']])
    assert bool((store.pairs[0, short['n_pairs']:] == 0).all()) and bool((store.pair_state[0, short['n_pairs']:] == 0).all())
    assert bool((store.pairs[1] == -7).all()) and bool((store.pair_state[1] == 9).all()) and bool((store.path[1] == -7).all())
    assert bool((store.pool[1] == -7.0).all())
