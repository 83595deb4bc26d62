"""The tie rules of LazySP's Dijkstra -- least key, LOWEST id among equal keys, strict ``alt < dist[v]`` -- on inputs that tie:
graphs and whole runs on a dyadic lattice (tests/golden/lazysp_lattice_*.npz, written by tools/gen_golden_lazysp.py), where
path lengths that are equal are equal bit for bit.  ``lazysp_lattice_dijkstra.npz`` holds what the reference's own
``dijkstra()`` returned on lattice graphs, with no kNN involved: it pins the claim that ``min_dist``'s walk over a ``set``
is the lowest-id order.  The other fixtures are whole runs of the reference on stored draws.  Every tie counter must be above
zero on every input, and each rule, swapped for its neighbour, must move a compared field.  No GPU."""
import glob
import os

import numpy as np
import pytest

from gnnmp import lazysp

from test_lazysp_host import EXACT_FIELDS, GOLDEN, assert_same_plan

LATTICE = sorted(os.path.basename(p)[len('lazysp_'):-len('.npz')] for p in glob.glob(os.path.join(GOLDEN, 'lazysp_lattice_*.npz'))
                 if not p.endswith('lattice_dijkstra.npz'))
INF = float('inf')
_RECS, _HOST = {}, {}


def load_lattice(name):
    if name not in _RECS:
        with np.load(os.path.join(GOLDEN, 'lazysp_%s.npz' % name)) as f:
            _RECS[name] = {k: f[k] for k in f.files}
    return _RECS[name]


def problem_of(rec):
    return dict(map=rec['map'], init_state=rec['init_state'], goal_state=rec['goal_state'])


def lattice_host(name):
    """plan_host on the stored attempts, once per fixture: shared with the GPU tests and left unchanged."""
    if name not in _HOST:
        rec = load_lattice(name)
        _HOST[name] = lazysp.plan_host(problem_of(rec), 0, batch=int(rec['batch']), t_max=int(rec['t_max']), k=int(rec['k']),
                                       attempts=rec['attempts'])
    return _HOST[name]


def dijkstra_graphs():
    """[(dense cost matrix, dist, prev, extract_ties, relax_ties)] of the fixture of the reference's own dijkstra()."""
    f = load_lattice('lattice_dijkstra')
    out = []
    for g in range(int(f['graphs'])):
        n = f['%d_points' % g].shape[0]
        e = f['%d_edges' % g].astype(np.int64)
        cost = np.full((n, n), INF)
        cost[e[:, 1], e[:, 0]] = f['%d_costs' % g]                   # cost[t, s]: what relaxing t offers s
        assert np.array_equal(f['%d_costs' % g], np.linalg.norm(f['%d_points' % g][e[:, 1]] - f['%d_points' % g][e[:, 0]], axis=1))
        out.append((cost, f['%d_dist' % g], f['%d_prev' % g].astype(np.int64), int(f['%d_extract_ties' % g]), int(f['%d_relax_ties' % g])))
    return out


def test_fixture_list():
    """Dijkstra runs on 63, 64, 65 and 129 nodes and on both sides of the device's LDS node count (1024), runs of several
    rounds that carry pairs over, solved and unsolved ones; the draws are distinct lattice points."""
    recs = {n: load_lattice(n) for n in LATTICE}
    sizes = {int(row[0]) for r in recs.values() for row in r['rounds']}
    assert {63, 64, 65, 129, 1024, 1025} <= sizes, sizes
    assert sum(len(r['rounds']) > 1 and int(r['rounds'][0, 2]) + int(r['rounds'][0, 3]) > 0 for r in recs.values()) >= 3
    assert any(len(r['path_ids']) > 0 for r in recs.values()) and any(len(r['path_ids']) == 0 for r in recs.values())
    assert {int(r['dim']) for r in recs.values()} == {2, 3}              # point robot and stick robot
    for name, r in recs.items():
        side = int(r['side'])
        assert np.array_equal(r['attempts'] * side, np.round(r['attempts'] * side)), name
        assert len({tuple(p) for p in r['samples'].tolist()}) == len(r['samples']), name
        assert bool(r['knn_equal']) == ('hostoracle' not in name), name
    assert {c.shape[0] for c, *_ in dijkstra_graphs()} == {63, 64, 65, 129}


@pytest.mark.parametrize('g', range(5))
def test_dijkstra_equals_the_references_on_lattice_graphs(g):
    """dist and prev of the reference's dijkstra() itself, full run; the early exit agrees on node 1 and on its chain."""
    cost, dist, prev, extract_ties, relax_ties = dijkstra_graphs()[g]
    st = dict(extract_ties=0, relax_ties=0)
    d, p = lazysp._dijkstra(cost, False, st)
    assert np.array_equal(d.view(np.uint64), dist.view(np.uint64)) and np.array_equal(p, prev)
    assert st == dict(extract_ties=extract_ties, relax_ties=relax_ties) and extract_ties > 0 and relax_ties > 0
    d1, p1 = lazysp._dijkstra(cost, True)
    cur = 1
    assert d1[1] == dist[1] and dist[1] < INF
    while cur != 0:
        assert p1[cur] == prev[cur]
        cur = int(prev[cur])


@pytest.mark.parametrize('name', LATTICE)
def test_plan_host_equals_reference_on_the_lattice(name):
    rec, got = load_lattice(name), lattice_host(name)
    assert_same_plan(got, rec, name)
    assert got['draws'] == rec['attempts'].shape[0]
    for key in ('extract_ties', 'relax_ties'):
        assert got[key] == int(rec[key]) and got[key] > 0, (name, key)


def highest_id(key):
    return len(key) - 1 - int(np.argmin(np.asarray(key)[::-1]))


MUTATIONS = {'extraction: highest id among equal keys': ('extract_index', highest_id),
             'relaxation: <= instead of <': ('relax_improves', lambda alt, dist: alt <= dist)}


def run_moved(name, monkeypatch, attr, rule):
    rec = load_lattice(name)
    with monkeypatch.context() as mp:
        mp.setattr(lazysp, attr, rule)
        try:
            got = lazysp.plan_host(problem_of(rec), 0, batch=int(rec['batch']), t_max=int(rec['t_max']), k=int(rec['k']),
                                   attempts=rec['attempts'])
        except (RuntimeError, ValueError):       # a cycle in prev, or a run that goes on drawing past the recorded attempts
            return ['path_ids']
    return [k for k in EXACT_FIELDS if not np.array_equal(np.asarray(got[k]), np.asarray(rec[k]))]


def moved_by(mutation, monkeypatch, _cache={}):
    """{input: fields that differ from the recording} under one mutated rule: the graphs of the Dijkstra fixture (full
    runs of ``_dijkstra``) and the recorded runs."""
    if mutation not in _cache:
        attr, rule = MUTATIONS[mutation]
        moved = {n: run_moved(n, monkeypatch, attr, rule) for n in LATTICE}
        with monkeypatch.context() as mp:
            mp.setattr(lazysp, attr, rule)
            for g, (cost, dist, prev, _, _) in enumerate(dijkstra_graphs()):
                d, p = lazysp._dijkstra(cost, False)
                moved['graph %d' % g] = [k for k, a, b in (('dist', d, dist), ('prev', p, prev)) if not np.array_equal(a, b)]
        _cache[mutation] = moved
    return _cache[mutation]


@pytest.mark.parametrize('mutation', sorted(MUTATIONS))
def test_every_mutated_rule_moves_every_input(mutation, monkeypatch):
    """Sensitivity: each rule swapped for its neighbour changes ``prev`` on every graph of the Dijkstra fixture and a
    compared field of every recorded run (the recording tool keeps only inputs of which this holds): no input is dead
    weight for either rule."""
    moved = moved_by(mutation, monkeypatch)
    print(mutation, moved)
    assert all(moved.values()), (mutation, [n for n, m in moved.items() if not m])


def test_seeded_runs_are_untouched_by_the_attempts_argument():
    """``attempts=`` with the rows a seed gives is the seeded run."""
    pr = problem_of(load_lattice(LATTICE[0]))
    a = lazysp.plan_host(pr, 11, batch=20, t_max=40, k=10)
    b = lazysp.plan_host(pr, 0, batch=20, t_max=40, k=10, attempts=np.random.RandomState(11).random_sample((4000, 2)))
    assert_same_plan(a, b, 'seed against its rows')
    assert a['draws'] == b['draws']
    with pytest.raises(ValueError):
        lazysp.plan_host(pr, 0, batch=20, t_max=40, k=10, attempts=np.zeros((3, 2)))
