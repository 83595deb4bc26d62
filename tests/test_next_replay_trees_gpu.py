"""ReplayStore.append_trees (gnnmp_next_replay_append_trees) on the trees of gnnmp_next_plan: the five recorded problems
tests/golden/next_plan_maze*_t60_*.npz with their seeds and checkpoints (the setup of tests/test_next_plan_device_gpu.py),
through next_plan.next_plan_device, whose device tensors go straight into the store.

After append_trees the store holds exactly the successful problems' r['path'] of next_plan.plan_maze_batch (the same launch,
read back), in ascending batch position with their problem ids, and get_label's labels of those paths
(next_train.path_labels), bit for bit; a batch of only failures changes nothing."""
import glob
import os

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_model, next_plan, next_replay, next_train
from gnnmp.rrtstar import draws_per_problem
from gnnmp.streams_batch import RawDoubles, problem_tensors

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'next_plan_maze*_t60_*.npz')))
DEV = 'cuda:0'
K = 10


def _load(name):
    with np.load(os.path.join(GOLDEN, name + '.npz')) as f:
        return {k: f[k] for k in f.files}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _setup(dim):
    recs = [r for r in (_load(n) for n in CASES) if int(r['dim']) == dim]
    problems = [dict(map=r['map'], init_state=r['init_state'], goal_state=r['goal_state']) for r in recs]
    seeds = [int(r['seed']) for r in recs]
    net = next_model.NextNet(dim).load_state_dict(_load('next_%d_weights' % dim))
    return problems, seeds, net


def _device_trees(problems, seeds, net, t_max):
    """What plan_maze_batch launches, without its read-back."""
    dev = torch.device(DEV)
    dim, maps, init64, goal64 = problem_tensors(problems, dev, 'test')
    eps = next_plan.default_eps(seeds, t_max, K, dim).to(dev)
    pb_rep = net.pb_forward(maps.to(torch.float32), goal64.to(torch.float32))
    block = RawDoubles(seeds, draws_per_problem(t_max, dim), dev, 'host')
    return next_plan.next_plan_device(maps, init64, goal64, block.raw, pb_rep, net._weights(dev), eps, t_max, True,
                                      next_plan.G_EXPLORE_EPS, 1.0, K, next_plan.policy_scale(None, dim))


@pytest.mark.parametrize('dim', [2, 3])
def test_store_holds_the_successful_paths_in_order(dim):
    problems, seeds, net = _setup(dim)
    assert len(problems) == (2 if dim == 2 else 3)
    store = next_replay.ReplayStore(dim, 16, 4096, DEV)
    want_rows, want_len, want_ids = [], [], []
    for t_max, base in ((60, 100), (300, 200)):                  # two batches, the second lands behind the first
        res = next_plan.plan_maze_batch(problems, DEV, seeds, net, t_max=t_max, stop_when_success=True, k=K)
        out = _device_trees(problems, seeds, net, t_max)
        ids = base + np.arange(len(problems))
        added = store.append_trees(out, torch.from_numpy(ids).to(DEV))
        good = [b for b, r in enumerate(res) if r['success']]
        assert added == len(good)
        for b in good:
            assert len(res[b]['path']) >= 2
            want_rows.append(res[b]['path'])
            want_len.append(len(res[b]['path']))
            want_ids.append(int(ids[b]))
        print('dim %d t_max %d: success %s, path lengths %s' % (dim, t_max, [r['success'] for r in res], [len(r['path']) for r in res]))
    net.check_status()
    assert want_rows, 'none of the recorded problems is solved at 60 or 300 samples: the test shows nothing'
    rows, ptr = np.concatenate(want_rows), np.concatenate([[0], np.cumsum(want_len)])
    n = store.n_states
    assert len(store) == len(want_len) and n == len(rows)
    assert store.counts.cpu().numpy().tolist() == [len(want_len), n]
    assert np.array_equal(store.path_ptr[:len(store) + 1].cpu().numpy(), ptr) and np.array_equal(store.host_ptr, ptr)
    assert store.problem[:len(store)].cpu().numpy().tolist() == want_ids and store.host_problem.tolist() == want_ids
    actions, values = next_train.path_labels(rows, ptr, dim)
    assert same_bits(store.states64[:n].cpu().numpy(), rows)
    assert same_bits(store.states32[:n].cpu().numpy(), rows.astype(np.float32))
    assert same_bits(store.actions[:n].cpu().numpy(), actions)
    assert same_bits(store.values[:n].cpu().numpy(), values)
    # batch(): the rows of a group, gathered on the device
    idx = list(range(len(store)))[::-1] + [0]
    b = store.batch(idx)
    take = np.concatenate([np.arange(ptr[i], ptr[i + 1]) for i in idx])
    assert same_bits(b['states32'].cpu().numpy(), rows.astype(np.float32)[take])
    assert same_bits(b['actions'].cpu().numpy(), actions[take]) and same_bits(b['values'].cpu().numpy(), values[take])
    assert b['ptr'].cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([want_len[i] for i in idx])]).tolist()
    assert b['problem_of_state'].cpu().numpy().tolist() == np.repeat(np.arange(len(idx)), [want_len[i] for i in idx]).tolist()
    assert b['problems'].tolist() == [want_ids[i] for i in idx]


@pytest.mark.parametrize('dim', [2, 3])
def test_a_batch_of_only_failures_changes_nothing(dim):
    problems, seeds, net = _setup(dim)
    store = next_replay.ReplayStore(dim, 4, 64, DEV)
    rng = np.random.RandomState(3)
    first = rng.uniform(-0.3, 0.3, (5, dim))
    store.append_paths(first, [0, 5], [42])
    before = [t.clone() for t in (store.states64, store.states32, store.actions, store.values, store.path_ptr, store.problem, store.counts)]
    res = next_plan.plan_maze_batch(problems, DEV, seeds, net, t_max=2, stop_when_success=True, k=K)
    assert not any(r['success'] for r in res)                    # a condition on the inputs: nobody is solved in two samples
    out = _device_trees(problems, seeds, net, 2)
    assert store.append_trees(out, np.arange(len(problems))) == 0
    torch.cuda.synchronize()
    after = (store.states64, store.states32, store.actions, store.values, store.path_ptr, store.problem, store.counts)
    assert all(torch.equal(a, b) for a, b in zip(after, before))
    assert len(store) == 1 and store.n_states == 5 and int(store.status.item()) == 0
