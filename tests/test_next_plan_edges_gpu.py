"""The edges of NEXT's device tree loop (gnnmp_next_plan) that tests/test_next_plan_device_gpu.py leaves alone: node counts at the
256-thread stride (256, 257 nodes) and at the cap of the LDS arrays (1023, 1024 nodes), the default t_max = 1000, k = 1 / 2 / 16,
c = 0 / 2.5, g_explore_eps = 0 / 1, exact ties in every arg-max, status bit 8, a two-node tree and a batch larger than the CU
count.  The reference everywhere is ``next_plan.plan_host`` on the device ``Model2D`` through ``NoiseModel``, with the same draws
and the same noise: one block ``torch.randn(1023, 16, dim)`` per (problem, seed), of which every run takes the leading
``[:t_max, :k]`` slice on both sides.  Every tree field but ``w`` is compared bit for bit, as in that file.

Seeds and margins.  ``min_margin > MIN_MARGIN`` is a condition on the inputs (a near-tie could be flipped by a last-bit difference
of ``w``), asserted first.  All runs use the recorded seeds of the problems (maze2 i0 2000, i1 2001; maze3 i0 2000, i1 2001,
i2 2002): none fell short at a long t_max, so no other stream was needed (``SEEDS`` is where one would go).  The margins they
reached on an MI355X (profiles/next_plan_parity.txt):
  maze2 i0, seed 2000: t_max 255 and 256 2.855e-05, t_max 1022 and 1023 1.203e-06
  maze3 i0, seed 2000: t_max 255 and 256 1.956e-05, t_max 1022 and 1023 1.780e-06
  t_max 1000 with stop_when_success, the default noise block of eval: maze2 i0 1.464e-05, i1 1.557e-03; maze3 i0 1.248e-04,
  i1 3.498e-03, i2 5.608e-05
  t_max 60 with k = 1 / 2 / 16, c = 2.5, g_explore_eps = 0: all five problems, the smallest 7.909e-06 (maze2 i1, k = 16)
The status-bit test adds stream 1647 (dim 2) / 346 (dim 3) on the first problem, whose first iterations are uniform, uniform,
goal, so that a tree of four nodes stands before the first guided iteration; the two-node test uses stream 9, whose first double
(0.0104) samples the goal.  Neither run reaches an arg-max.

The bar of ``w[j]`` is derived, not measured: ``(n + 1) * 2 ** -52`` relative, n the node count.  w[j] is a sum of at most n
positive terms max(exp(a), 1e-3) in [1e-3, 1].  The arguments a are bit-equal on both sides (no contraction: every operation
before the exp is rounded on its own, on the same inputs).  Each side's exp is taken to be within 1 ulp, so each term is within
2 ** -52 relative of the true one, and so is the exact sum of a side's terms: 2 * 2 ** -52 between the two sides.  Any summation
order of n positive terms is within (n - 1) half ulps (2 ** -53) relative of their exact sum: (n - 1) * 2 ** -52 between the
sides.  Together (n + 1) * 2 ** -52.  The 1e-3 floor is exact and only removes error.

``w_sum`` has no such bound (its history of add and subtract cancels), so it is measured: the worst relative error against
``plan_host`` over the runs of this file on an MI355X was 4.668e-16 (W_SUM_MEASURED, rounded up), and the bar is 10 x that, the
convention of test_next_plan_device_gpu.py for a different reduction order (profiles/next_plan_parity.txt).  It is far below
3 * t_max times the derived bar of ``w`` at 1024 nodes (7e-10), beyond which it would be a finding to explain and not a bar.

Mutations of the kernel these tests were checked against (each built once, then reverted; the older suite passes on all of them):
``>`` to ``>=`` in select's in-thread loop -- the tie tests at t_max 300 and 1023 fail (at 70 no thread scans two nodes);
``oi < id`` to ``oi > id`` in block_argmax, in the wave butterfly or in the cross-wave step -- every tie test fails; block_w's scan
bound ``min(n, 768)`` -- the node-count tests at 1022 and 1023 and the tie tests at 1023 fail; dropping the ``p.k > 1`` guard
changes no output (candidate 0 is taken either way, only time is spent), so no test of results can see it."""
import contextlib

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_plan, rrtstar
from test_next_plan_device_gpu import (DEV, MIN_MARGIN, _RECS, _load, _model, _names, _problem, assert_same_tree, device_run, host_run,
                                       same_bits)

pytestmark = pytest.mark.gpu
T_CAP = 1023                           # the last node fills slot 1023 of the LDS arrays
K_MAX = next_plan.K_MAX
T_EDGES = (255, 256, 1022, 1023)
W_SUM_MEASURED = 4.7e-16
W_SUM_RTOL = 10 * W_SUM_MEASURED
SEEDS = {}                             # name -> another RandomState stream than the recorded one (none was needed)
FIRST_GUIDED_LATE = {2: 1647, 3: 346}  # streams whose first iterations are uniform, uniform, goal: the first guided one is the fourth
GOAL_FIRST = 9                         # RandomState(9)'s first double is 0.0104 < 0.05: iteration 0 samples the goal
_BLOCKS, _PAIRS = {}, {}


def w_bar(n):
    return (n + 1) * 2.0 ** -52


def _seed(name):
    return SEEDS.get(name, int(_load(name)['seed']))


def _noise(name, seed, t_max, k):
    """The leading [t_max, k] slice of the (problem, seed)'s one block."""
    if (name, seed) not in _BLOCKS:
        _BLOCKS[(name, seed)] = next_plan.default_eps([seed], T_CAP, K_MAX, int(_load(name)['dim']))[0]
    return _BLOCKS[(name, seed)][:t_max, :k].contiguous()


@contextlib.contextmanager
def pb_rep_edited(net, edit):
    """``plan_maze_batch`` computes pb_rep itself: inside, ``net.pb_forward`` returns ``edit`` of it."""
    real = net.pb_forward
    net.pb_forward = lambda *a, **kw: edit(real(*a, **kw))
    try:
        yield
    finally:
        del net.pb_forward


def run_pairs(names, t_max, stop, seeds=None, pb_edit=None, **kw):
    """[(device tree, plan_host tree, noise)] of ``names`` run as ONE batch on the device; ``kw``: g_explore_eps, c, k."""
    seeds = [_seed(n) for n in names] if seeds is None else list(seeds)
    key = (tuple(names), t_max, stop, tuple(seeds), pb_edit, tuple(sorted(kw.items())))
    if key not in _PAIRS:
        k = kw.get('k', 10)
        noise = [_noise(n, s, t_max, k) for n, s in zip(names, seeds)]
        with pb_rep_edited(_model(int(_load(names[0])['dim'])).net, pb_edit) if pb_edit else contextlib.nullcontext():
            got = device_run(names, t_max, stop, cache=False, seeds=seeds, eps=torch.stack(noise), **kw)
        want = [host_run(n, t_max, stop, eps=e, seed=s, pb_edit=pb_edit, **kw) for n, s, e in zip(names, seeds, noise)]
        _PAIRS[key] = list(zip(got, want, noise))
    return _PAIRS[key]


def check_tree(got, want, what):
    """Every field bit for bit, ``w`` within the derived bar, ``w_sum`` within the measured one."""
    assert got['status'] == 0, what
    assert_same_tree(got, want, what, False)
    n = want['w'].shape[0]
    w_err = float(np.max(np.abs(got['w'] - want['w']) / want['w']))
    s_err = abs(got['w_sum'] - want['w_sum']) / want['w_sum']
    st = want['stats']
    print('%s: %d nodes, guided %d (collided %d), wraps %d, min_margin %.3e, w rel err %.3e (bar %.3e), w_sum rel err %.3e (bar %.3e)'
          % (what, n, st['guided'], st['guided_collided'], st['wraps'], st['min_margin'], w_err, w_bar(n), s_err, W_SUM_RTOL))
    assert w_err <= w_bar(n), (what, w_err, w_bar(n))
    assert s_err <= W_SUM_RTOL, (what, s_err, W_SUM_RTOL)


def candidate_0(name, tree, noise, pb_edit=None):
    """Per guided node of ``tree`` the state ``candidate_step(parent, action_0)`` with action_0 = fl32(mean + fl32(scale * eps[g, 0]))."""
    rec = _load(name)
    dim = int(rec['dim'])
    ids = np.flatnonzero(tree['expanded_by_rrt'] == 0)
    model = _model(dim)
    model.set_problem(_problem(rec))
    if pb_edit is not None:
        model.pb_rep = pb_edit(model.pb_rep)
    parents = tree['states'][tree['parents'][ids]]
    mean = np.asarray(model.net_forward(parents)[0], dtype=np.float32).reshape(-1, dim)
    model.check_status()
    scale = next_plan.policy_scale(None, dim)
    out = []
    for g, par in enumerate(parents):
        action = (mean[g] + (scale * noise[g, 0].numpy()).astype(np.float32)).astype(np.float32)
        out.append(next_plan.candidate_step(np.array(par), action, dim))
    return ids, np.array(out).reshape(-1, dim)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. node counts at the 256-thread stride and at the cap
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('t_max', T_EDGES)
def test_node_counts_at_the_stride_and_at_the_cap(t_max, dim):
    name = _names(dim)[0]
    got, want, _ = run_pairs([name], t_max, False)[0]
    assert want['stats']['min_margin'] > MIN_MARGIN, (name, want['stats']['min_margin'])      # a condition on the inputs
    assert got['states'].shape[0] == t_max + 1
    check_tree(got, want, '%s seed %d t_max %d' % (name, _seed(name), t_max))


@pytest.mark.parametrize('dim', [2, 3])
def test_the_run_to_the_cap_reaches_the_named_situations(dim):
    name = _names(dim)[0]
    _, want, noise = run_pairs([name], T_CAP, False)[0]
    st = want['stats']
    guided = np.flatnonzero(want['expanded_by_rrt'] == 0)
    print('%s t_max %d: guided %d, collided %d, wraps %d, largest guided parent %d'
          % (name, T_CAP, st['guided'], st['guided_collided'], st['wraps'], want['parents'][guided].max()))
    assert st['guided'] > 768 and st['guided_collided'] > 0
    assert want['parents'][guided].max() >= 768, 'select never took a node of the fourth 256-stride'
    if dim == 3:                       # the run to 768 is a prefix of the run to the cap: what it lacks happened beyond node 768
        upto = host_run(name, 768, False, eps=noise[:768], seed=_seed(name))
        assert same_bits(upto['states'], want['states'][:769])
        assert st['wraps'] > upto['stats']['wraps'], 'no angle wrap beyond node 768'


@pytest.mark.parametrize('dim', [2, 3])
def test_eval_next_device_at_the_default_t_max(dim):
    import types
    names = _names(dim)
    recs = [_load(n) for n in names]
    host = [host_run(n, 1000, True) for n in names]                  # the default noise block of t_max = 1000, as eval draws it
    for n, h in zip(names, host):
        assert h['stats']['min_margin'] > MIN_MARGIN, (n, h['stats']['min_margin'])          # a condition on the inputs
        print('%s t_max 1000 stop: %d nodes, success %d, guided %d, min_margin %.3e'
              % (n, h['states'].shape[0], h['success'], h['stats']['guided'], h['stats']['min_margin']))
    env = types.SimpleNamespace(maps=[r['map'] for r in recs], init_states=[r['init_state'] for r in recs],
                                goal_states=[r['goal_state'] for r in recs])
    rows = []
    got = next_plan.eval_next_device(env, range(len(recs)), _model(dim).net, seeds=[int(r['seed']) for r in recs], device=DEV, chunk=2,
                                     rows_out=rows)
    want = rrtstar.eval_aggregate(host)
    assert got[0] == want[0] and got[1] == want[1]
    assert got[2] == want[2] or (np.isnan(got[2]) and np.isnan(want[2]))
    assert len(got[3]) == len(host) and all(same_bits(a, b['path']) for a, b in zip(got[3], host))
    assert [r[3] for r in rows] == [h['states'].shape[0] for h in host]
    assert [r[5] for r in rows] == [h['stats']['guided'] for h in host]


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. k, c and g_explore_eps
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('k', [1, 2, K_MAX])
def test_k_at_both_ends(k, dim):
    names = _names(dim)
    for name, (got, want, noise) in zip(names, run_pairs(names, 60, False, k=k)):
        assert want['stats']['min_margin'] > MIN_MARGIN, (name, want['stats']['min_margin'])
        assert want['stats']['guided'] > 0
        check_tree(got, want, '%s k %d' % (name, k))
        if k == 1:                     # no candidate is scored: the step goes to the only one
            ids, cand = candidate_0(name, got, noise)
            assert same_bits(got['states'][ids], cand), name


@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('c', [0.0, 2.5])
def test_c_off_and_large(c, dim):
    names = _names(dim)
    for name, (got, want, _) in zip(names, run_pairs(names, 60, False, c=c)):
        if c != 0.0:                   # at c = 0 no decision depends on w
            assert want['stats']['min_margin'] > MIN_MARGIN, (name, want['stats']['min_margin'])
        check_tree(got, want, '%s c %g' % (name, c))


def _goal_samples(seed, t_max, dim, g_explore_eps):
    """(iterations whose first double is below 0.05, doubles consumed) when every other iteration is guided (2 doubles)."""
    assert g_explore_eps == 0.0
    raw = np.random.RandomState(seed).random_sample(rrtstar.draws_per_problem(t_max, dim))
    pos = goals = 0
    for _ in range(t_max):
        goal = raw[pos] < rrtstar.MODEL_EPS
        goals, pos = goals + goal, pos + (1 if goal else 2)
    return goals, pos


@pytest.mark.parametrize('dim', [2, 3])
def test_every_iteration_without_a_goal_sample_is_guided_at_explore_rate_0(dim):
    names = _names(dim)
    for name, (got, want, _) in zip(names, run_pairs(names, 60, False, g_explore_eps=0.0)):
        assert want['stats']['min_margin'] > MIN_MARGIN, (name, want['stats']['min_margin'])
        goals, used = _goal_samples(_seed(name), 60, dim, 0.0)
        assert got['guided'] == 60 - goals == int((got['expanded_by_rrt'] == 0).sum()) and got['draws'] == used, name
        check_tree(got, want, '%s g_explore_eps 0' % name)


@pytest.mark.parametrize('dim', [2, 3])
def test_no_iteration_is_guided_at_explore_rate_1_and_the_tree_is_rrt_stars(dim):
    names = _names(dim)
    pairs = run_pairs(names, 60, False, g_explore_eps=1.0)
    star = rrtstar.plan_maze_batch([_problem(_load(n)) for n in names], DEV, [_seed(n) for n in names], t_max=60, stop_when_success=False)
    for name, (got, want, _), rrt in zip(names, pairs, star):
        assert got['guided'] == 0 and np.all(got['expanded_by_rrt'][1:] == 1), name
        check_tree(got, want, '%s g_explore_eps 1' % name)
        for key in ('states', 'parents', 'rewired_parents', 'freesp', 'in_goal_region', 'costs', 'path_lengths',
                    'cumulated_collision_checks', 'path', 'path_ids'):
            assert same_bits(got[key], rrt[key]), (name, key)
        assert got['draws'] == rrt['draws'] and got['success'] == rrt['success'] and got['i'] == rrt['i'], name


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. exact ties: the lower id wins
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('t_max', [70, 300, T_CAP])
def test_exact_ties_go_to_the_lower_id(t_max, dim):
    """pb_rep = 0 makes the value and the action mean the same constants for every state; with c = 0 every select score and every
    expand score is an exact tie: within one wave (70), across the waves (300) and across the four strides (1023)."""
    name = _names(dim)[0]
    got, want, noise = run_pairs([name], t_max, False, pb_edit=torch.zeros_like, c=0.0, g_explore_eps=0.0)[0]
    assert want['stats']['min_margin'] == 0.0, 'the ties were not real'
    assert len(set(want['state_values'].tolist())) == 1
    assert got['states'].shape[0] == t_max + 1
    check_tree(got, want, '%s ties t_max %d' % (name, t_max))
    ids, cand = candidate_0(name, got, noise, torch.zeros_like)
    assert ids.size == got['guided'] > t_max // 2
    assert np.all(got['parents'][ids] == 0), 'a guided parent other than node 0: %s' % got['parents'][ids][got['parents'][ids] != 0][:5]
    assert same_bits(got['states'][ids], cand), 'a guided child other than candidate 0'
    free = np.flatnonzero(got['freesp'] & ~got['in_goal_region'])
    assert free.size > min(t_max, 256) // 2, 'few nodes took part in the ties'
    if t_max == T_CAP:
        assert free.max() >= 768 and np.all(np.bincount(free // 256, minlength=4) > 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. STATUS_SCORE_NOT_FINITE
# ---------------------------------------------------------------------------------------------------------------------------------
def _inf_channel_0(pb):
    pb = pb.clone()
    pb[:, 0] = float('inf')
    return pb


@pytest.mark.parametrize('dim', [2, 3])
def test_a_score_that_is_not_finite_sets_bit_8_and_leaves_the_prefix(dim):
    t_max = 60
    names = _names(dim) + [_names(dim)[0]]
    seeds = [_seed(n) for n in names[:-1]] + [FIRST_GUIDED_LATE[dim]]
    recs = [_load(n) for n in names]
    model = _model(dim)
    noise = [_noise(n, s, t_max, 10) for n, s in zip(names, seeds)]
    f64 = lambda key: torch.from_numpy(np.stack([np.asarray(r[key], dtype=np.float64) for r in recs])).to(DEV)      # noqa: E731
    maps, init64, goal64 = f64('map'), f64('init_state'), f64('goal_state')
    raw = torch.from_numpy(np.stack([np.random.RandomState(s).random_sample(rrtstar.draws_per_problem(t_max, dim)) for s in seeds])).to(DEV)
    pb = _inf_channel_0(model.net.pb_forward(maps.to(torch.float32), goal64.to(torch.float32)))
    out = next_plan.next_plan_device(maps, init64, goal64, raw, pb, model.net._weights(torch.device(DEV)), torch.stack(noise).to(DEV),
                                     t_max, False)
    n_nodes, success, last_i, used, plen, status, guided = out['small'].cpu().numpy()
    seen = set()
    for i, (name, seed) in enumerate(zip(names, seeds)):
        full = host_run(name, t_max, False, eps=noise[i], seed=seed)
        n = int(n_nodes[i])
        seen.add(n)
        assert status[i] == next_plan.STATUS_SCORE_NOT_FINITE == 8 and guided[i] == 0, (name, status[i])
        assert n == int(np.flatnonzero(full['expanded_by_rrt'] == 0)[0]), 'n_nodes - 1 is the first guided iteration of the normal run'
        assert last_i[i] == n - 2
        assert np.all(np.isnan(out['state_values'][i, :n].cpu().numpy())), name
        if n == 1:
            assert same_bits(out['states'][i, :1].cpu().numpy(), np.asarray(recs[i]['init_state'], dtype=np.float64).reshape(1, dim))
            assert used[i] == 0 and not success[i]
            continue
        want = host_run(name, n - 1, False, eps=noise[i], seed=seed)
        assert want['stats']['guided'] == 0 and used[i] == want['draws'] and bool(success[i]) == want['success']
        assert same_bits(out['states'][i, :n].cpu().numpy(), want['states'])
        assert np.array_equal(out['parents'][i, :n].cpu().numpy(), want['parents'])
        assert same_bits(out['costs'][i, :n].cpu().numpy(), want['costs'])
        assert np.array_equal(out['cumulated_checks'][i, :n].cpu().numpy(), want['cumulated_collision_checks'])
    assert max(seen) >= 4, 'no run here has uniform and goal iterations before its first guided one'
    with pb_rep_edited(model.net, _inf_channel_0):
        with pytest.raises(RuntimeError, match='a score was not finite'):
            device_run(names, t_max, False, cache=False, seeds=seeds, eps=torch.stack(noise))
        res = device_run(names, t_max, False, cache=False, seeds=seeds, eps=torch.stack(noise), check=False)
    assert [r['status'] for r in res] == [8] * len(names) and [r['states'].shape[0] for r in res] == n_nodes.tolist()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. a two-node tree: the start lies inside the goal region
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', [2, 3])
def test_a_start_inside_the_goal_region_gives_a_two_node_tree(dim):
    name = 'free_map_start_in_goal_%d' % dim
    goal = np.array([0.5, -0.25, 0.1][:dim])
    init = goal.copy()
    init[0] += 0.03
    _RECS.setdefault(name, dict(dim=np.int64(dim), map=np.zeros((15, 15)), init_state=init, goal_state=goal, seed=np.int64(GOAL_FIRST)))
    got, want, _ = run_pairs([name], 60, True)[0]
    assert want['success'] and want['states'].shape[0] == 2 and want['i'] == 0, 'the first iteration samples the goal and reaches it'
    assert got['path_ids'].tolist() == [0, got['states'].shape[0] - 1] == [0, 1] and got['success']
    check_tree(got, want, name)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. more problems than CUs: workgroups that start after others have finished
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', [2, 3])
def test_a_batch_larger_than_the_cu_count(dim):
    B, t_max = 260, 8
    assert B > torch.cuda.get_device_properties(DEV).multi_processor_count
    names = _names(dim)
    many = (names * B)[:B]
    single = {n: run_pairs([n], t_max, False)[0] for n in names}
    for n, (got, want, _) in single.items():
        check_tree(got, want, '%s t_max 8' % n)
    res = device_run(many, t_max, False, cache=False, eps=torch.stack([_noise(n, _seed(n), t_max, 10) for n in many]),
                     seeds=[_seed(n) for n in many])
    assert len(res) == B
    for slot, (n, got) in enumerate(zip(many, res)):
        assert got['status'] == 0
        assert_same_tree(got, single[n][0], '%s in slot %d of %d' % (n, slot, B), True)


def test_the_measured_w_sum_error_is_no_finding():
    """Beyond 3 * t_max times the derived bar of w at 1024 nodes the error of w_sum would be something to explain, not a bar."""
    assert W_SUM_MEASURED <= 3 * T_CAP * w_bar(1024)
