"""gnnmp.next_replay.collect_replay and train_env_maze on 16 maze problems per robot, at explore rate 1.0, where NEXT_plan never
takes the guided branch: its tree is RRT*'s and does not depend on the weights.

maze2: the first 16 problems of tests/golden/evalset_mazehard_first1000.npz, seeds i, t_max 200, fallback batch 50 / t_max 200.
The expected store comes from the two HOST planners (rrtstar.plan_host, then bitstar.plan_host on seed i ^ 0x9E3779B9 for the
failures, about 2 s): NEXT solves problem 14 with a path of 19 states, the fallback solves 14 problems, problem 2 stays unsolved
-- asserted as constants, so the test cannot quietly degenerate.  Then train_env_maze over the same problems with chunk 8, L 1
(rates 1.0, then 0.7) runs to the end: finite losses, a changed checkpoint, a history that adds up, a second run bit-equal.

maze3: the first 16 problems of tests/golden/evalset_maze3_first40_b200_k12_s9.npz, t_max 300, fallback t_max 600.  The host
planners take about 30 s for this set, so the expected store comes from next_plan.plan_maze_batch and bitstar.plan_maze_batch on
the device; the census (NEXT none, the fallback 14, problems 1 and 12 unsolved) is asserted as constants."""
import os

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import bitstar, next_model, next_plan, next_replay, next_train, rrtstar

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda:0'
XOR = 0x9E3779B9
N = 16


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}


def _problems(name):
    f = _load(name)
    return [dict(map=f['maps'][i], init_state=f['init_states'][i], goal_state=f['goal_states'][i]) for i in range(N)]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_store(store, dim, next_paths, fb_paths):
    """The store against {problem: path}: the NEXT successes ascending, then the fallback's ascending."""
    order = sorted(next_paths) + sorted(fb_paths)
    paths = [next_paths[i] if i in next_paths else fb_paths[i] for i in order]
    rows, ptr = np.concatenate(paths), np.concatenate([[0], np.cumsum([len(p) for p in paths])])
    n = len(rows)
    assert len(store) == len(order) and store.n_states == n
    assert store.host_problem.tolist() == order and store.problem[:len(order)].cpu().numpy().tolist() == order
    assert np.array_equal(store.path_ptr[:len(order) + 1].cpu().numpy(), ptr)
    actions, values = next_train.path_labels(rows, ptr, dim)
    assert same_bits(store.states64[:n].cpu().numpy(), rows)
    assert same_bits(store.states32[:n].cpu().numpy(), rows.astype(np.float32))
    assert same_bits(store.actions[:n].cpu().numpy(), actions) and same_bits(store.values[:n].cpu().numpy(), values)


def test_maze2_collect_equals_the_host_planners_and_train_env_runs():
    dim, t_max, fb_t = 2, 200, 200
    problems = _problems('evalset_mazehard_first1000.npz')
    w = _load('next_2_weights.npz')
    next_paths, fb_paths, unsolved = {}, {}, []
    for i, pr in enumerate(problems):
        r = rrtstar.plan_host(pr, i, t_max=t_max, stop_when_success=True)
        if r['success'] and len(r['path']):
            next_paths[i] = r['path']
            continue
        b = bitstar.plan_host(pr, i ^ XOR, batch=50, t_max=fb_t)
        if len(b['path']):
            fb_paths[i] = b['path']
        else:
            unsolved.append(i)
    assert sorted(next_paths) == [14] and len(next_paths[14]) == 19
    assert len(fb_paths) == 14 and unsolved == [2]

    net = next_model.NextNet(dim).load_state_dict(w)
    store = next_replay.ReplayStore(dim, N, N * (t_max + 1), DEV)
    stats, timings = {}, {}
    got = next_replay.collect_replay(net, problems, list(range(N)), list(range(N)), store, DEV, 1.0, t_max=t_max, fallback_batch=50,
                                     fallback_t_max=fb_t, stats=stats, timings=timings)
    assert got == {'next': 1, 'fallback': 14, 'unsolved': 1} and stats == got
    assert set(timings) == {'pb_forward', 'plan', 'append', 'fallback'}
    _check_store(store, dim, next_paths, fb_paths)

    def run():
        tn = next_train.NextNetTrain(dim, device=DEV).load_state_dict(w)
        hist = next_replay.train_env_maze(tn, problems, DEV, chunk=8, eps0=1.0, decay=0.7, L=1, t_max=t_max, fallback_batch=50,
                                          fallback_t_max=fb_t)
        return tn.state_dict(), hist

    sd, hist = run()
    assert [h['explore_eps'] for h in hist] == [1.0, 0.7]
    assert len(hist) == 2 and all(h['next'] + h['fallback'] + h['unsolved'] == 8 for h in hist)
    # the first chunk is planned at rate 1.0: its census is the host planners' for problems 0 .. 7
    assert (hist[0]['next'], hist[0]['fallback'], hist[0]['unsolved']) == (0, 7, 1)
    assert hist[0]['replay'] == 7 and hist[1]['replay'] == 7 + hist[1]['next'] + hist[1]['fallback']
    # L = 1: a replay of n samples gives n // 8 steps (the trailing n % 8 are dropped after the only pass)
    assert [len(h['losses']) for h in hist] == [hist[0]['replay'] // 8, hist[1]['replay'] // 8]
    assert len(hist[1]['losses']) >= 1
    assert all(np.isfinite(h['losses']).all() for h in hist)
    assert any(not np.array_equal(sd[k].cpu().numpy(), w[k]) for k in w)
    next_model.NextNet(dim).load_state_dict(sd)                  # the checkpoint loads
    print('maze2 train_env_maze: %s' % hist)
    sd2, hist2 = run()
    assert hist2 == hist and all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_maze3_collect_equals_the_device_planners():
    dim, t_max, fb_t = 3, 300, 600
    problems = _problems('evalset_maze3_first40_b200_k12_s9.npz')
    net = next_model.NextNet(dim).load_state_dict(_load('next_3_weights.npz'))
    seeds = list(range(N))
    res = next_plan.plan_maze_batch(problems, DEV, seeds, net, t_max=t_max, stop_when_success=True, g_explore_eps=1.0)
    next_paths = {i: r['path'] for i, r in enumerate(res) if r['success']}
    failed = [i for i in range(N) if i not in next_paths]
    fb = bitstar.plan_maze_batch([problems[i] for i in failed], DEV, [i ^ XOR for i in failed], batch=50, t_max=fb_t)
    fb_paths = {i: r['path'] for i, r in zip(failed, fb) if r['success']}
    unsolved = [i for i in failed if i not in fb_paths]
    assert sorted(next_paths) == [] and len(fb_paths) == 14 and unsolved == [1, 12]
    store = next_replay.ReplayStore(dim, N, N * 602, DEV)
    got = next_replay.collect_replay(net, problems, seeds, seeds, store, DEV, 1.0, t_max=t_max, fallback_batch=50, fallback_t_max=fb_t)
    assert got == {'next': 0, 'fallback': 14, 'unsolved': 2}
    _check_store(store, dim, next_paths, fb_paths)
