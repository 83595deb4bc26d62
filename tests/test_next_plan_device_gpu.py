"""NEXT's guided tree loop on the device (gnnmp_next_plan) against ``gnnmp.next_plan.plan_host`` on the device ``Model2D`` with the
same noise (``NoiseModel``): the five recorded problems, their seeds and the recorded checkpoints.  Every tree field except
``w`` must be equal bit for bit -- the network evaluations inside the loop are the body of ``gnnmp_next_state_forward`` and
every float64 decision is one rounded operation at a time; ``w`` / ``w_sum`` go through the device's exp / log, which are not
numpy's, and are held to a relative bar.  That holds only when no arg-max of the run is a near-tie, so the host run's
``min_margin`` is asserted first: a condition on the inputs.

W_RTOL: the worst relative error of ``w`` and ``w_sum`` measured over the ten runs below (five problems, two settings) on an
MI355X was 7.267e-16 (W_MEASURED, rounded up); the bar is 10 x that, the margin for a different summation order over up to 301
terms (profiles/next_plan_parity.txt)."""
import glob
import os
import types

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_model, next_plan, rrtstar
from test_next_plan_host import EXACT

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'next_plan_maze*_t60_*.npz')))
DEV = 'cuda:0'
K = 10
SETTINGS = {'t60_stop': (60, True), 't300_full': (300, False)}
MIN_MARGIN = 1e-9
W_MEASURED = 7.3e-16
W_RTOL = 10 * W_MEASURED
BITWISE = tuple(k for k in EXACT if k != 'w')
_MODELS, _RECS, _HOST, _DEVICE = {}, {}, {}, {}


def _load(name):
    if name not in _RECS:
        with np.load(os.path.join(GOLDEN, name + '.npz')) as f:
            _RECS[name] = {k: f[k] for k in f.files}
    return _RECS[name]


def _names(dim):
    return [n for n in CASES if int(_load(n)['dim']) == dim]


def _problem(rec):
    return dict(map=rec['map'], init_state=rec['init_state'], goal_state=rec['goal_state'])


def _model(dim):
    if dim not in _MODELS:
        _MODELS[dim] = next_model.Model2D(None, dim=dim, device=DEV).load_state_dict(_load('next_%d_weights' % dim))
    return _MODELS[dim]


def _eps(names, t_max, k=K, seeds=None):
    dim = int(_load(names[0])['dim'])
    return next_plan.default_eps([int(_load(n)['seed']) for n in names] if seeds is None else seeds, t_max, k, dim)


def host_run(name, t_max, stop, eps=None, g_explore_eps=next_plan.G_EXPLORE_EPS, c=1.0, k=K, seed=None, pb_edit=None):
    """``plan_host`` on the device model with the noise block the device loop gets (cached for the default block).  ``seed``:
    another ``RandomState`` stream than the recorded one; ``pb_edit``: a function applied to the model's ``pb_rep`` after
    ``set_problem`` (never cached)."""
    key = (name, t_max, stop, g_explore_eps, c, k, seed)
    cached = eps is None and pb_edit is None
    if cached and key in _HOST:
        return _HOST[key]
    rec = _load(name)
    seed = int(rec['seed']) if seed is None else int(seed)
    model = _model(int(rec['dim']))
    model.set_problem(_problem(rec))
    if pb_edit is not None:
        model.pb_rep = pb_edit(model.pb_rep)
    noise = _eps([name], t_max, k, [seed])[0] if eps is None else eps
    out = next_plan.plan_host(_problem(rec), seed, next_plan.NoiseModel(model, noise), t_max=t_max, g_explore_eps=g_explore_eps,
                              stop_when_success=stop, c=c, k=k)
    model.check_status()
    if cached:
        _HOST[key] = out
    return out


def device_run(names, t_max, stop, draws='host', cache=True, g_explore_eps=next_plan.G_EXPLORE_EPS, c=1.0, k=K, seeds=None, **kw):
    key = (tuple(names), t_max, stop, draws, g_explore_eps, c, k, None if seeds is None else tuple(seeds))
    if cache and not kw and key in _DEVICE:
        return _DEVICE[key]
    recs = [_load(n) for n in names]
    seeds = [int(r['seed']) for r in recs] if seeds is None else [int(s) for s in seeds]
    eps = kw.pop('eps') if 'eps' in kw else _eps(names, t_max, k, seeds)
    res = next_plan.plan_maze_batch([_problem(r) for r in recs], DEV, seeds, _model(int(recs[0]['dim'])).net, t_max=t_max,
                                    stop_when_success=stop, draws=draws, eps=eps, g_explore_eps=g_explore_eps, c=c, k=k, **kw)
    if cache and not kw:
        _DEVICE[key] = res
    return res


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_tree(got, want, what, w_bitwise):
    """``got`` (device) against ``want`` (plan_host, or another device run with ``w_bitwise``)."""
    for key in BITWISE:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape, (what, key, g.shape, w.shape)
        assert same_bits(g, w.astype(g.dtype)), (what, key)
    assert got['success'] == want['success'] and got['i'] == want['i'] and got['draws'] == want['draws'], what
    assert got['guided'] == (want['guided'] if 'guided' in want else want['stats']['guided']), what
    assert same_bits(got['path'], want['path']), what
    if w_bitwise:
        assert same_bits(got['w'], want['w']) and got['w_sum'] == want['w_sum'], what
        return 0.0
    err = float(np.max(np.abs(got['w'] - want['w']) / want['w']))
    err = max(err, abs(got['w_sum'] - want['w_sum']) / want['w_sum'])
    return err


@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('setting', sorted(SETTINGS))
def test_device_loop_equals_plan_host(setting, dim):
    t_max, stop = SETTINGS[setting]
    names = _names(dim)
    res = device_run(names, t_max, stop)
    worst = 0.0
    for name, got in zip(names, res):
        want = host_run(name, t_max, stop)
        assert want['stats']['min_margin'] > MIN_MARGIN, (name, want['stats']['min_margin'])      # a condition on the inputs
        assert got['status'] == 0
        n = got['states'].shape[0]
        if not stop:
            assert n == t_max + 1
        err = assert_same_tree(got, want, '%s %s' % (name, setting), False)
        st = want['stats']
        print('%s %s: %d nodes, guided %d (collided %d), goal-region nodes %d, wraps %d, min_margin %.3e, w rel err %.3e'
              % (name, setting, n, st['guided'], st['guided_collided'], int(want['in_goal_region'].sum()), st['wraps'], st['min_margin'], err))
        worst = max(worst, err)
        # the values inside the loop are gnnmp_next_state_forward's, bit for bit
        model = _model(dim)
        model.set_problem(_problem(_load(name)))
        y = model.net.state_forward(torch.from_numpy(got['states'].astype(np.float32)).to(DEV),
                                    torch.zeros(n, dtype=torch.int32, device=DEV), model.pb_rep).cpu().numpy()
        model.check_status()
        assert same_bits(got['state_values'], y[:, -1].copy()), name
    print('%s dim %d: worst relative error of w / w_sum %.3e (bar %.3e)' % (setting, dim, worst, W_RTOL))
    assert worst <= W_RTOL, (worst, W_RTOL)


def test_the_settings_reach_the_named_situations():
    full = [host_run(n, *SETTINGS['t300_full']) for n in CASES]
    early = [host_run(n, *SETTINGS['t60_stop']) for n in CASES]
    assert len(CASES) == 5 and {int(_load(n)['dim']) for n in CASES} == {2, 3}
    assert all(r['states'].shape[0] == 301 for r in full), 'across the 64-lane groups and the 256-thread stride'
    assert all(r['states'].shape[0] < 64 for r in early)
    assert any(r['success'] and r['states'].shape[0] < 61 for r in early), 'an early success'
    assert any(r['in_goal_region'].sum() > 0 for r in full), 'terminal nodes leave non_terminal'
    assert any(r['stats']['guided_collided'] > 0 for r in full), 'collided guided steps'
    assert any(r['stats']['wraps'] > 0 for r in full), 'angle wraps'


@pytest.mark.parametrize('dim', [2, 3])
def test_problems_are_independent_and_runs_repeat(dim):
    t_max, stop = SETTINGS['t300_full']
    names = _names(dim)
    base = device_run(names, t_max, stop)
    again = device_run(names, t_max, stop, cache=False)
    rev = device_run(names[::-1], t_max, stop, cache=False)[::-1]
    single = [device_run([n], t_max, stop, cache=False)[0] for n in names]
    for name, a, b, c, d in zip(names, base, again, rev, single):
        for other, what in ((b, 'second run'), (c, 'reversed batch'), (d, 'alone')):
            assert_same_tree(other, a, '%s %s' % (name, what), True)


@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('setting', sorted(SETTINGS))
def test_device_draws_equal_host_draws(setting, dim):
    t_max, stop = SETTINGS[setting]
    names = _names(dim)
    streams = []
    res = device_run(names, t_max, stop, draws='device', cache=False, streams_out=streams)
    for i, (name, got, want) in enumerate(zip(names, res, device_run(names, t_max, stop))):
        assert got['status'] == 0
        assert_same_tree(got, want, '%s device draws' % name, True)
        rs = np.random.RandomState(int(_load(name)['seed']))
        rs.random_sample(got['draws'])
        ref, have = rs.get_state(), streams[0].state(i)
        assert np.array_equal(have[1], ref[1]) and have[2] == ref[2], name
        nxt = np.random.RandomState()
        nxt.set_state(have)
        assert nxt.random_sample() == rs.random_sample()


@pytest.mark.parametrize('dim', [2, 3])
def test_a_short_eps_block_sets_bit_4_and_leaves_the_prefix(dim):
    t_max, stop = SETTINGS['t60_stop']
    names = _names(dim)
    eps = _eps(names, t_max)
    res = device_run(names, t_max, stop, cache=False, eps=eps[:, :3].contiguous(), check=False)
    hit = 0
    for i, (name, got) in enumerate(zip(names, res)):
        full = host_run(name, t_max, stop)
        if full['stats']['guided'] <= 3:
            assert got['status'] == 0
            continue
        hit += 1
        assert got['status'] == next_plan.STATUS_EPS_SHORT and got['guided'] == 3, name
        n = got['states'].shape[0]
        assert (full['expanded_by_rrt'][:n] == 0).sum() == 3 and full['expanded_by_rrt'][n] == 0      # guided step 4 came next
        want = host_run(name, n - 1, stop, eps=eps[i])
        assert not (want['success'] and stop)
        assert_same_tree(got, want, '%s short eps' % name, False) <= W_RTOL
    assert hit > 0, 'no run here has more than three guided iterations'
    with pytest.raises(RuntimeError, match='eps block too short'):
        device_run(names, t_max, stop, cache=False, eps=eps[:, :3].contiguous())


@pytest.mark.parametrize('dim', [2, 3])
def test_a_short_draw_block_sets_bit_1_and_leaves_the_prefix(dim):
    t_max, stop = SETTINGS['t60_stop']
    names = _names(dim)
    recs = [_load(n) for n in names]
    model = _model(dim)
    eps = _eps(names, t_max)
    full = [host_run(n, t_max, stop) for n in names]
    short = min(r['draws'] for r in full) - 1                        # every problem runs out of doubles before its run ends
    assert short >= 2 + dim
    f64 = lambda key: torch.from_numpy(np.stack([np.asarray(r[key], dtype=np.float64) for r in recs])).to(DEV)      # noqa: E731
    maps, init64, goal64 = f64('map'), f64('init_state'), f64('goal_state')
    raw = torch.from_numpy(np.stack([np.random.RandomState(int(r['seed'])).random_sample(short) for r in recs])).to(DEV)
    pb = model.net.pb_forward(maps.to(torch.float32), goal64.to(torch.float32))
    out = next_plan.next_plan_device(maps, init64, goal64, raw, pb, model.net._weights(torch.device(DEV)), eps.to(DEV), t_max, stop)
    n_nodes, success, last_i, used, plen, status, guided = out['small'].cpu().numpy()
    for i, name in enumerate(names):
        assert status[i] == rrtstar.STATUS_DRAWS_SHORT and used[i] <= short and not success[i], name
        n = int(n_nodes[i])
        assert 1 <= n < full[i]['states'].shape[0]
        want = host_run(name, n - 1, stop, eps=eps[i]) if n > 1 else None
        if want is not None:
            assert used[i] == want['draws'] and guided[i] == want['stats']['guided'] and last_i[i] == want['i']
            assert same_bits(out['states'][i, :n].cpu().numpy(), want['states'])
            assert same_bits(out['costs'][i, :n].cpu().numpy(), want['costs'])
            assert same_bits(out['state_values'][i, :n].cpu().numpy(), want['state_values'])
            assert np.array_equal(out['cumulated_checks'][i, :n].cpu().numpy(), want['cumulated_collision_checks'])
            assert np.array_equal(out['visits'][i, :n].cpu().numpy(), want['visits'])


@pytest.mark.parametrize('dim', [2, 3])
def test_eval_next_device_equals_the_aggregate_of_plan_host(dim):
    names = _names(dim)
    recs = [_load(n) for n in names]
    env = types.SimpleNamespace(maps=[r['map'] for r in recs], init_states=[r['init_state'] for r in recs],
                                goal_states=[r['goal_state'] for r in recs])
    seeds = [int(r['seed']) for r in recs]
    rows = []
    got = next_plan.eval_next_device(env, range(len(recs)), _model(dim).net, seeds=seeds, t_max=60, device=DEV, chunk=2, rows_out=rows)
    host = [host_run(n, 60, True) for n in names]
    want = rrtstar.eval_aggregate(host)
    assert got[0] == want[0] and got[1] == want[1]
    assert got[2] == want[2] or (np.isnan(got[2]) and np.isnan(want[2]))
    assert len(got[3]) == len(host) and all(same_bits(a, b['path']) for a, b in zip(got[3], host))
    assert [r[3] for r in rows] == [h['states'].shape[0] for h in host]
