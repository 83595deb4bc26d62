"""BIT* on the device (gnnmp.bitstar.plan_maze_batch, eval_bit_device and the gnnmp_bitstar_* entry points) against the recorded
runs of the reference (tests/golden/bitstar_*.npz) and, at shapes the fixtures do not reach, against gnnmp.bitstar.plan_host:
every field and counter exactly.  Reads only tests/golden/ and the package."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import bitstar, maze2d

from test_bitstar_host import CASES, assert_same_plan, host_plan, load_case, problem_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEARCH_FIELDS = ('vertices', 'parents', 'g', 'samples_left', 'checks', 'g_goal', 'T', 'path_ids')      # what gnnmp_bitstar_plan decides
OUTPUTS = ('g', 'parents', 'vertices', 'path', 'counters')


def settings_of(rec):
    return int(rec['dim']), int(rec['batch']), int(rec['t_max'])


GROUPS, ALL_GROUPS = {}, {}
for _name in CASES:
    _rec = load_case(_name)
    ALL_GROUPS.setdefault(settings_of(_rec), []).append(_name)
    if not bool(_rec['crafted']):
        GROUPS.setdefault(settings_of(_rec), []).append(_name)
GROUP_IDS = lambda g: 'maze%d_b%d_t%d' % g      # noqa: E731


def assert_stream_ends_where_numpy_ends(streams, i, seed, draws, what):
    rs = np.random.RandomState(int(seed))
    rs.random_sample(int(draws))
    want, got = rs.get_state(), streams.state(i)
    assert np.array_equal(got[1], want[1]) and got[2] == want[2], what
    nxt = np.random.RandomState()
    nxt.set_state(got)
    assert nxt.random_sample() == rs.random_sample(), what


@pytest.mark.parametrize('group', sorted(GROUPS), ids=GROUP_IDS)
@pytest.mark.parametrize('draws', ['host', 'device'])
def test_plan_maze_batch_equals_reference(group, draws):
    """Every fixture of one setting as one batch, both ways of drawing: each field and counter exactly the reference's; with
    the draws on the device the streams end where numpy's generator ends after the recorded number of doubles -- the batches
    that were reached, not the batches that were classified up front."""
    dim, batch, t_max = group
    recs = [load_case(n) for n in GROUPS[group]]
    streams = []
    res = bitstar.plan_maze_batch([problem_of(r) for r in recs], DEV, [int(r['seed']) for r in recs], batch=batch, t_max=t_max,
                                  draws=draws, streams_out=streams)
    for name, rec, got in zip(GROUPS[group], recs, res):
        assert got['status'] == 0 and got['success'] == (float(rec['g_goal']) < np.inf)
        assert_same_plan(got, rec, '%s (%s draws)' % (name, draws))
    if draws == 'device':
        for i, rec in enumerate(recs):
            assert_stream_ends_where_numpy_ends(streams[0], i, rec['seed'], rec['draws'], GROUPS[group][i])


@pytest.mark.parametrize('draws', ['host', 'device'])
def test_plan_maze_batch_hands_out_longer_attempt_blocks(draws, monkeypatch):
    """A first attempt block far too short for the 1000 free draws: every problem reports status 1 from the sampler and gets a
    block twice as long until it fits; the answers and the streams' end do not change."""
    monkeypatch.setattr(bitstar, '_DRAWS_PER_FREE', [0.01, 0.01])
    group = (2, 50, 1000)
    recs = [load_case(n) for n in GROUPS[group]]
    streams = []
    res = bitstar.plan_maze_batch([problem_of(r) for r in recs], DEV, [int(r['seed']) for r in recs], batch=50, t_max=1000, draws=draws,
                                  streams_out=streams)
    for i, (name, rec, got) in enumerate(zip(GROUPS[group], recs, res)):
        assert_same_plan(got, rec, name)
        if draws == 'device':
            assert_stream_ends_where_numpy_ends(streams[0], i, rec['seed'], rec['draws'], name)


def run_abi(plans, batch, t_max, edge_cap=None, flags=0):
    """The problems of ``plans`` (fixtures or plan_host results of one robot and setting, each with ``map``) through
    gnnmp_bitstar_plan on their recorded points and per-batch tables -> the outputs on the host.  Rows and table entries
    behind the batches a run reached are never read: zeros, radius 1."""
    nb = bitstar.n_batches(batch, t_max)
    rows, dim = 2 + nb * batch, plans[0]['points'].shape[1]
    pool, r_tab, c_tab = np.zeros((len(plans), rows, dim)), np.ones((len(plans), nb)), np.zeros((len(plans), nb), dtype=np.int64)
    for b, p in enumerate(plans):
        k = len(p['r_by_batch'])
        pool[b, :p['points'].shape[0]] = p['points']
        r_tab[b, :k], c_tab[b, :k] = p['r_by_batch'], p['checks_by_batch']
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    out = bitstar.bitstar_plan(dev(np.stack([np.asarray(p['map'], dtype=np.float64) for p in plans])), dev(pool), dev(r_tab), dev(c_tab),
                               batch, nb, edge_cap=edge_cap, flags=flags)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if k != 'workspace'}


def plan_of(out, b, plan, batch):
    """Problem b of run_abi's outputs in plan_host's layout; what the sampling decides is taken from ``plan``."""
    dim = plan['points'].shape[1]
    used = np.asarray(plan['used_by_batch'], dtype=np.int64)
    got = bitstar._problem_result(b, batch, dim, np.asarray(plan['points'])[None].repeat(b + 1, axis=0), used[None].repeat(b + 1, axis=0),
                                  np.asarray(plan['checks_by_batch'])[None].repeat(b + 1, axis=0),
                                  np.asarray(plan['r_by_batch'])[None].repeat(b + 1, axis=0), out, out['small'], out['counters'])
    return got


@pytest.mark.parametrize('group', sorted(ALL_GROUPS), ids=GROUP_IDS)
def test_c_abi_with_the_workspace_flag_equals_reference(group):
    """The same groups, the crafted tie case among them, through gnnmp_bitstar_plan with bit 0 of flags set."""
    dim, batch, t_max = group
    recs = [load_case(n) for n in ALL_GROUPS[group]]
    out = run_abi(recs, batch, t_max, flags=1)
    plain = run_abi(recs, batch, t_max, flags=0)
    for b, (name, rec) in enumerate(zip(ALL_GROUPS[group], recs)):
        assert out['small'][4, b] == 0, name
        assert_same_plan(plan_of(out, b, rec, batch), rec, name, fields=SEARCH_FIELDS)
    for key in OUTPUTS + ('small',):
        assert np.array_equal(out[key].view(np.uint8), plain[key].view(np.uint8)), key


def test_order_and_chunking_do_not_matter():
    group = (2, 50, 1000)
    recs = [load_case(n) for n in GROUPS[group]]
    problems, seeds = [problem_of(r) for r in recs], [int(r['seed']) for r in recs]
    whole = bitstar.plan_maze_batch(problems, DEV, seeds, batch=50, t_max=1000)
    back = bitstar.plan_maze_batch(problems[::-1], DEV, seeds[::-1], batch=50, t_max=1000)[::-1]
    cut = (bitstar.plan_maze_batch(problems[:2], DEV, seeds[:2], batch=50, t_max=1000)
           + bitstar.plan_maze_batch(problems[2:], DEV, seeds[2:], batch=50, t_max=1000))
    for name, want, a, c in zip(GROUPS[group], whole, back, cut):
        assert_same_plan(a, want, name + ' reversed')
        assert_same_plan(c, want, name + ' in two chunks')


def test_edge_cap_of_8_flags_the_problems_that_need_more_and_leaves_the_neighbour_alone():
    group = (2, 7, 35)
    recs = [load_case(n) for n in GROUPS[group]]
    need = [int(r['max_edge_queue']) for r in recs]
    assert min(need) <= 8 < max(need)
    ample, tight = run_abi(recs, 7, 35), run_abi(recs, 7, 35, edge_cap=8)
    for b, (name, rec) in enumerate(zip(GROUPS[group], recs)):
        if need[b] > 8:
            assert tight['small'][4, b] & bitstar.STATUS_EDGE_QUEUE_FULL, name
            continue
        assert tight['small'][4, b] == 0, name
        for key in OUTPUTS:
            assert np.array_equal(tight[key][b].view(np.uint8), ample[key][b].view(np.uint8)), (name, key)
        assert np.array_equal(tight['small'][:, b], ample['small'][:, b]), name
        assert_same_plan(plan_of(tight, b, rec, 7), rec, name, fields=SEARCH_FIELDS)


@pytest.mark.parametrize('draws', ['host', 'device'])
def test_plan_maze_batch_runs_a_full_queue_again(draws):
    """edge_cap = 8: the problems that fill it are run again alone with the provable bound; nothing raises, the answers and the
    streams' end are the fixtures'."""
    group = (2, 7, 35)
    recs = [load_case(n) for n in GROUPS[group]]
    streams = []
    res = bitstar.plan_maze_batch([problem_of(r) for r in recs], DEV, [int(r['seed']) for r in recs], batch=7, t_max=35, draws=draws,
                                  edge_cap=8, streams_out=streams)
    for i, (name, rec, got) in enumerate(zip(GROUPS[group], recs, res)):
        assert got['status'] == 0
        assert_same_plan(got, rec, name)
        if draws == 'device':
            assert_stream_ends_where_numpy_ends(streams[0], i, rec['seed'], rec['draws'], name)


@pytest.mark.parametrize('name', ['maze2_b7_t35_i19', 'maze3_b50_t300_i4'])
def test_sampler_with_a_block_one_draw_short(name):
    """A fixture that reached every batch: its attempts minus the last one -- status 1, pool and tables untouched; the whole
    block then gives the recorded points and per-batch counts."""
    rec = load_case(name)
    assert name in CASES and len(rec['r_by_batch']) == bitstar.n_batches(int(rec['batch']), int(rec['t_max']))
    dim, batch, nb = int(rec['dim']), int(rec['batch']), len(rec['r_by_batch'])
    limits = np.asarray(bitstar._maze_class(dim).SAMPLE_LIMITS, dtype=np.float64)
    n_att = int(rec['used_by_batch'][-1])
    att = torch.from_numpy(np.random.RandomState(int(rec['seed'])).uniform(-limits, limits, (n_att, dim))).to(DEV)
    dev = lambda key: torch.from_numpy(np.asarray(rec[key], dtype=np.float64)[None].copy()).to(DEV)      # noqa: E731
    maps, init64, goal64 = dev('map'), dev('init_state'), dev('goal_state')
    pool = torch.full((1, 2 + nb * batch, dim), 7.0, dtype=torch.float64, device=DEV)
    used = torch.full((1, nb), -3, dtype=torch.int64, device=DEV)
    checks = torch.full((1, nb), -5, dtype=torch.int64, device=DEV)
    status = torch.full((1,), 9, dtype=torch.int32, device=DEV)
    bitstar.bitstar_sample(att[:n_att - 1], [0, n_att - 1], maps, init64, goal64, batch, nb, pool, used, checks, status)
    assert status.item() == 1
    assert (pool == 7.0).all().item() and (used == -3).all().item() and (checks == -5).all().item()
    bitstar.bitstar_sample(att, [0, n_att], maps, init64, goal64, batch, nb, pool, used, checks, status)
    assert status.item() == 0
    assert np.array_equal(pool[0].cpu().numpy().view(np.uint64), rec['points'].view(np.uint64))
    assert np.array_equal(used[0].cpu().numpy(), rec['used_by_batch']) and np.array_equal(checks[0].cpu().numpy(), rec['checks_by_batch'])


def test_walled_in_start_against_plan_host():
    """A start inside a closed cell of a crafted map: every edge that leaves the cell is blocked, every batch ends through the
    empty-queues path.  Batch 50 and enough batches to pass the LDS node count, next to a fixture problem in the same launch."""
    t_max = 50 * (bitstar.lds_nodes() // 50 + 1)
    assert 2 + t_max > bitstar.lds_nodes() >= 2 + 1000
    grid = np.zeros((15, 15))
    grid[0, :] = grid[-1, :] = grid[:, 0] = grid[:, -1] = 1
    grid[6:9, 6:9] = 1
    grid[7, 7] = 0
    walled = dict(map=grid, init_state=np.array([0.0, 0.0]), goal_state=np.array([0.8, 0.8]))
    rec = load_case('maze2_b50_t1000_i1')
    problems, seeds = [walled, problem_of(rec)], [4242, int(rec['seed'])]
    want = [host_plan(pr, s, 50, t_max) for pr, s in zip(problems, seeds)]
    assert len(want[0]['vertices']) <= 8 and want[0]['g_goal'] == np.inf and want[0]['T'] == t_max
    assert want[0]['stats']['edge_checks'] > 0
    streams = []
    res = bitstar.plan_maze_batch(problems, DEV, seeds, batch=50, t_max=t_max, draws='device', streams_out=streams)
    for i, (got, w) in enumerate(zip(res, want)):
        assert got['status'] == 0
        assert_same_plan(got, w, 'problem %d' % i)
        assert_stream_ends_where_numpy_ends(streams[0], i, seeds[i], w['draws'], 'problem %d' % i)


def test_eval_bit_device_aggregates():
    names = GROUPS[(2, 50, 1000)][:3] + GROUPS[(2, 7, 35)]
    recs = [load_case(n) for n in names]
    env = maze2d.Maze2D(np.stack([r['map'] for r in recs]), np.stack([r['init_state'] for r in recs]),
                        np.stack([r['goal_state'] for r in recs]))
    for batch, t_max, idx in ((50, 1000, [0, 1, 2]), (7, 35, [3, 4, 5])):
        rows = []
        n, collision, cost, paths = bitstar.eval_bit_device(env, idx, seeds=[int(recs[i]['seed']) for i in idx], batch=batch, t_max=t_max,
                                                            device=DEV, chunk=2, rows_out=rows)
        assert (n, collision, cost) == bitstar.eval_aggregate([recs[i] for i in idx])
        assert n == sum(float(recs[i]['g_goal']) < np.inf for i in idx) and len(rows) == 3
        for i, p in zip(idx, paths):
            assert np.array_equal(p, recs[i]['points'][recs[i]['path_ids']])
