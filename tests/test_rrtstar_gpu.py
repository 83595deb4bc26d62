"""RRT* on the device (gnnmp.rrtstar.plan_maze_batch, eval_rrt_device and the gnnmp_rrtstar_* entry points) against the recorded
runs of the reference (tests/golden/rrtstar_*.npz) and, at shapes the fixtures do not reach, against gnnmp.rrtstar.plan_host:
every field of the search tree exactly.  Reads only tests/golden/ and the package."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import maze2d, rrtstar

from test_rrtstar_host import CASES, assert_same_tree, host_plan, load_case, problem_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WAVE = 64                # nodes per pass of the nearest-neighbour scan and of the two rewiring passes (one per lane)


def settings_of(rec):
    return int(rec['dim']), int(rec['t_max']), bool(rec['stop_when_success'])


GROUPS = {}
for _name in CASES:
    GROUPS.setdefault(settings_of(load_case(_name)), []).append(_name)


@pytest.mark.parametrize('group', sorted(GROUPS), ids=lambda g: 'maze%d_t%d_stop%d' % g)
@pytest.mark.parametrize('draws', ['host', 'device'])
def test_plan_maze_batch_equals_reference(group, draws):
    """Every fixture of one setting as one batch, both ways of drawing: each field exactly the reference's; with the draws on
    the device the streams end where numpy's generator ends after the recorded number of doubles."""
    dim, t_max, stop = group
    recs = [load_case(n) for n in GROUPS[group]]
    streams = []
    res = rrtstar.plan_maze_batch([problem_of(r) for r in recs], DEV, [int(r['seed']) for r in recs], t_max=t_max,
                                  stop_when_success=stop, draws=draws, streams_out=streams)
    for name, rec, got in zip(GROUPS[group], recs, res):
        assert got['status'] == 0
        assert_same_tree(got, rec, '%s (%s draws)' % (name, draws))
    if draws == 'device':
        for i, rec in enumerate(recs):
            rs = np.random.RandomState(int(rec['seed']))
            rs.random_sample(int(rec['draws']))
            want, got = rs.get_state(), streams[0].state(i)
            assert np.array_equal(got[1], want[1]) and got[2] == want[2], GROUPS[group][i]
            nxt = np.random.RandomState()
            nxt.set_state(got)
            assert nxt.random_sample() == rs.random_sample()


def run_abi(recs, t_max, stop, draws_per_problem=None):
    """The problems ``recs`` (one robot) through gnnmp_rrtstar_plan with host-drawn blocks -> (the per-problem words as numpy
    [6, B]: n_nodes, success, last_iter, used, path_len, status; the tree tensors on the host)."""
    dim = int(recs[0]['dim'])
    n = rrtstar.draws_per_problem(t_max, dim) if draws_per_problem is None else draws_per_problem
    f64 = lambda key: torch.from_numpy(np.stack([np.asarray(r[key], dtype=np.float64) for r in recs])).to(DEV)      # noqa: E731
    raw = torch.from_numpy(np.stack([np.random.RandomState(int(r['seed'])).random_sample(n) for r in recs])).to(DEV)
    out = rrtstar.rrtstar_plan(f64('map'), f64('init_state'), f64('goal_state'), raw, t_max, stop)
    torch.cuda.synchronize()
    return out['small'].cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items() if k not in ('small', 'workspace')}


def tree_of(small, host, b):
    n, plen = int(small[0, b]), int(small[4, b])
    pts = host['states'][b, :n]
    ids = host['path'][b, :plen].astype(np.int64)
    return {'states': pts, 'parents': host['parents'][b, :n], 'rewired_parents': host['rewired_parents'][b, :n],
            'freesp': (host['flags'][b, :n] & 1).astype(bool), 'in_goal_region': (host['flags'][b, :n] & 2).astype(bool),
            'costs': host['costs'][b, :n], 'path_lengths': host['path_lengths'][b, :n],
            'cumulated_collision_checks': host['cumulated_checks'][b, :n], 'success': bool(small[1, b]), 'i': int(small[2, b]),
            'path_ids': ids, 'path': pts[ids], 'draws': int(small[3, b])}


@pytest.mark.parametrize('group', [g for g in sorted(GROUPS) if g[1] in (2, 300)], ids=lambda g: 'maze%d_t%d_stop%d' % g)
def test_c_abi_equals_reference(group):
    dim, t_max, stop = group
    recs = [load_case(n) for n in GROUPS[group]]
    small, host = run_abi(recs, t_max, stop)
    for b, (name, rec) in enumerate(zip(GROUPS[group], recs)):
        assert small[5, b] == 0
        assert_same_tree(tree_of(small, host, b), rec, name)


def test_draw_block_that_ends_early():
    """A block of exactly the doubles a problem draws works; with one double fewer the problem stops before the iteration that
    would read past its block (status bit 1) and holds the reference's tree up to there; its neighbour in the batch -- whose
    block follows in memory -- is untouched by it."""
    recs = [load_case('maze2_t100_i1'), load_case('maze2_t100_i0')]
    need = [int(r['draws']) for r in recs]
    assert need[0] > need[1]
    small, host = run_abi(recs, 100, True, draws_per_problem=need[0])
    assert small[5].tolist() == [0, 0] and small[3].tolist() == need
    for b, rec in enumerate(recs):
        assert_same_tree(tree_of(small, host, b), rec, 'exact block, problem %d' % b)
    small, host = run_abi(recs, 100, True, draws_per_problem=need[0] - 1)
    assert small[5].tolist() == [rrtstar.STATUS_DRAWS_SHORT, 0]
    assert_same_tree(tree_of(small, host, 1), recs[1], 'neighbour of the short block')
    n = int(small[0, 0])
    assert n == 100 and small[2, 0] == 98 and small[3, 0] <= need[0] - 1
    got = tree_of(small, host, 0)
    assert np.array_equal(got['states'], recs[0]['states'][:n])
    assert np.array_equal(got['cumulated_collision_checks'], recs[0]['cumulated_collision_checks'][:n])
    assert np.array_equal(got['parents'], recs[0]['parents'][:n])


def test_permuted_chunked_repeated_batches_and_two_runs():
    """Per-problem results do not depend on the order of the batch, on how it is cut or on what else is in it (the same problem
    twice included), and a run repeats bit for bit."""
    names = ['maze2_t300_i13', 'maze2_t300_i12', 'maze2_t100_i0', 'maze2_t100_i1', 'maze2_t100_firstgoal_s1004']
    recs = [load_case(n) for n in names]
    run = lambda order: rrtstar.plan_maze_batch([problem_of(recs[i]) for i in order], DEV, [int(recs[i]['seed']) for i in order],      # noqa: E731
                                                t_max=300)
    full = run(range(len(recs)))
    again = run(range(len(recs)))
    perm = [3, 0, 4, 2, 1]
    permuted = run(perm)
    chunks = run(perm[:2]) + run(perm[2:])
    repeated = run([1, 1, 4, 1])
    for j, i in enumerate(perm):
        assert_same_tree(permuted[j], full[i], 'permuted %s' % names[i])
        assert_same_tree(chunks[j], full[i], 'chunked %s' % names[i])
    for j, i in enumerate([1, 1, 4, 1]):
        assert_same_tree(repeated[j], full[i], 'repeated %s' % names[i])
    for a, b, n in zip(full, again, names):
        assert_same_tree(a, b, 'second run %s' % n)
    for i in (0, 1):                                                     # (t_max = 300: the recorded runs themselves)
        assert_same_tree(full[i], recs[i], names[i])


def check_against_host(problems, seeds, t_max, stop=True, draws='host'):
    res = rrtstar.plan_maze_batch(problems, DEV, seeds, t_max=t_max, stop_when_success=stop, draws=draws)
    hosts = [host_plan(p, s, t_max, stop) for p, s in zip(problems, seeds)]
    for i, (got, want) in enumerate(zip(res, hosts)):
        assert got['status'] == 0
        assert_same_tree(got, want, 'problem %d (t_max %d)' % (i, t_max))
    return res, hosts


UNSOLVED = {2: (('maze2_t100_i0', 1000), ('maze2_t100_i0', 5)), 3: (('maze3_t100_i0', 1000), ('maze3_t100_i1', 5))}


@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('t_max', [WAVE - 2, WAVE - 1, WAVE, 2 * WAVE - 1, 2 * WAVE])
def test_node_counts_around_the_wave_width(dim, t_max):
    """Unsolved problems reach exactly t_max + 1 nodes: the last iterations scan one fewer, exactly and one more node than the
    lanes of a pass (and than two passes)."""
    problems = [problem_of(load_case(name)) for name, _ in UNSOLVED[dim]]
    _, hosts = check_against_host(problems, [s for _, s in UNSOLVED[dim]], t_max)
    assert all(not h['success'] and h['states'].shape[0] == t_max + 1 for h in hosts)


@pytest.mark.parametrize('dim', [2, 3])
def test_lds_workspace_switch(dim):
    """A tree of one node fewer than the LDS node count (node state in LDS) and one of one node more (node state in the
    workspace); stop_when_success=False, so both reach exactly t_max + 1 nodes."""
    lds = rrtstar.lds_nodes()
    pr = problem_of(load_case('maze%d_t100_i1' % dim))
    for t_max in (lds - 2, lds):
        _, hosts = check_against_host([pr], [5], t_max, stop=False, draws='device' if t_max == lds else 'host')
        assert hosts[0]['states'].shape[0] == t_max + 1 and hosts[0]['stats']['max_near'] > WAVE


def test_more_than_one_wave_of_near_nodes():
    """A map that is blocked except for a pocket of 3 x 3 cells holding start and goal: the tree cannot leave, collided nodes
    pile up within the rewiring radius, and some iteration has more than 64 near nodes, collided ones among them -- the
    rewiring passes take several groups of 64 and the second pass checks collided nodes."""
    c = lambda i: (i + 0.5) * 2 / 15 - 1      # noqa: E731
    m = np.ones((15, 15))
    m[6:9, 6:9] = 0
    pr = dict(map=m, init_state=np.array([c(6), c(6)]), goal_state=np.array([c(8), c(8)]))
    _, hosts = check_against_host([pr, pr], [3, 4], 400, stop=False)
    assert hosts[0]['stats']['max_near'] > WAVE and hosts[0]['stats']['max_near_collided'] > 0
    assert hosts[0]['stats']['collided_second_pass'] > 0 and hosts[0]['stats']['goal_rechecks'] > 0 and hosts[0]['success']
    # the stick robot: a recorded problem whose tree is boxed in early
    pr3 = problem_of(load_case('maze3_t100_i1'))
    _, hosts = check_against_host([pr3], [7], 128)
    assert hosts[0]['stats']['max_near'] > WAVE and hosts[0]['stats']['max_near_collided'] > 0


def test_stick_edges_inside_rewiring_checks():
    """The interpolated sticks of a rewiring check on a map of the test's own (all free, as test_stick_steer_gpu.py has one).
    A rewiring check joins nodes less than 3 RRT_EPS = 0.15 apart, so it has at most K = int(0.15 / 0.015) = 10 sticks, and a
    first step of at most RRT_EPS has K <= 3: more than 64 interpolated sticks -- a second pass of the lanes -- cannot occur
    inside RRT*, whatever the map.  What can occur is covered: the largest K there is (9) and free edges all through."""
    pr = dict(map=np.zeros((15, 15)), init_state=np.array([0., 0., 0.]), goal_state=np.array([0.8, 0.8, 0.2]))
    _, hosts = check_against_host([pr, pr], [3, 4], 200, stop=False)
    assert all(h['stats']['max_rewire_k'] == 9 for h in hosts)
    assert all(h['freesp'].all() for h in hosts) and any((h['parents'] != h['rewired_parents']).any() for h in hosts)


def test_eval_rrt_device_equals_the_host_aggregate():
    """eval_rrt_device on 8 problems of the fixtures' family, cut into chunks: eval_rrt's tuple from plan_host's trees, the
    subtraction of the first iteration's checks included."""
    names = ['maze2_t100_i0', 'maze2_t100_i1', 'maze2_t300_i12', 'maze2_t300_i13']
    recs = [load_case(n) for n in names]
    env = maze2d.Maze2D(np.stack([r['map'] for r in recs]), np.stack([r['init_state'] for r in recs]),
                        np.stack([r['goal_state'] for r in recs]))
    indexes = [0, 1, 2, 3, 3, 2, 1, 0]
    seeds = [1000, 1001, 1012, 1013, 21, 22, 23, 24]
    rows = []
    n_success, collision, cost, paths = rrtstar.eval_rrt_device(env, indexes, seeds=seeds, t_max=300, device=DEV, chunk=3, rows_out=rows)
    hosts = [host_plan(problem_of(recs[i]), s, 300, True) for i, s in zip(indexes, seeds)]
    want_checks = [int(h['cumulated_collision_checks'][-1]) - int(h['cumulated_collision_checks'][1]) for h in hosts]
    assert n_success == sum(h['success'] for h in hosts) and 2 <= n_success
    assert collision == float(np.mean(want_checks)) and [r[1] for r in rows] == want_checks
    assert all(int(h['cumulated_collision_checks'][1]) > 0 for h in hosts)          # the quirk subtracts something
    assert cost == float(np.mean([h['path_lengths'][-1] for h in hosts if h['success']]))
    assert (n_success, collision, cost) == rrtstar.eval_aggregate(hosts)
    assert len(paths) == 8 and all(np.array_equal(p, h['path']) for p, h in zip(paths, hosts))
    # default seeds: one stream per problem index, whatever the chunking
    a = rrtstar.eval_rrt_device(env, [0, 1, 2, 3], seed=7, t_max=100, device=DEV, chunk=4)
    b = rrtstar.eval_rrt_device(env, [0, 1, 2, 3], seed=7, t_max=100, device=DEV, chunk=1, draws='device')
    assert a[:3] == b[:3] or (np.isnan(a[2]) and np.isnan(b[2]) and a[:2] == b[:2])
