"""ReplayStore.append_paths (gnnmp_next_replay_append_paths): the stored rows against the input and the labels against
gnnmp.next_train.path_labels (train_next.get_label restated on the host in float64), bit for bit, for both robots.

Cases: path lengths 1, 2, 63, 64, 65 and 130 (one wave walks a path in chunks of 64 rows); an edge of length exactly RRT_EPS
(not cut) and one just above (cut); a repeated state; for the stick robot orientation gaps that wrap in both directions and one of
exactly LIMITS[2]; 200 random paths in one call; the recorded paths of tests/golden/next_train_maze{2,3}.npz against the
reference's recorded actions and values; and the capacity rules: an exact fit is accepted, one path or one state too many
leaves the store untouched and raises, a second append lands behind the first."""
import os

import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_replay, next_train

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda:0'
EPS = next_train.RRT_EPS
LIM = np.array([1., 1., 0.4])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def random_path(rng, n, dim):
    """A walk inside the bounds whose steps lie on both sides of RRT_EPS; the stick's orientation crosses the period."""
    pts = [rng.uniform(-1, 1, dim) * LIM[:dim]]
    for _ in range(n - 1):
        step = rng.uniform(-1, 1, dim) * rng.choice([0.01, 0.04, 0.2])
        nxt = pts[-1] + step
        nxt[:2] = np.clip(nxt[:2], -1, 1)
        if dim == 3:
            nxt[2] = (nxt[2] + 0.4) % 0.8 - 0.4
        pts.append(nxt)
    return np.array(pts)


def edge_paths(dim):
    z = [0.] * (dim - 2)
    above = np.nextafter(EPS, 1.)
    paths = [np.array([[0., 0.] + z, [EPS, 0.] + z]),                              # exactly RRT_EPS: not cut
             np.array([[0., 0.] + z, [above, 0.] + z, [above, above] + z]),        # just above: cut
             np.array([[0.3, -0.2] + z, [0.3, -0.2] + z, [0.5, 0.1] + z, [0.5, 0.1] + z])]      # a repeated state
    if dim == 3:
        paths += [np.array([[0., 0., 0.37], [0.1, 0., -0.36], [0.1, 0.2, 0.39]]),  # the gap wraps down, then up
                  np.array([[0., 0., -0.39], [0.01, 0., 0.38], [0.02, 0.01, -0.4]]),   # short edges across the period: not cut
                  np.array([[0., 0., -0.2], [0.3, 0., 0.2], [0., 0., -0.2]]),      # |diff[2]| exactly LIMITS[2]: not wrapped
                  np.array([[0.5, 0.5, 0.4], [0.4, 0.5, -0.4], [0.9, 0.5, 0.4]])]  # the ends of the period
        assert paths[-2][1, 2] - paths[-2][0, 2] == 0.4
    return paths


def pack(paths):
    return np.concatenate(paths), np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)


def store_arrays(store):
    n = store.n_states
    counts = store.counts.cpu().numpy()
    assert counts.tolist() == [len(store), n]
    return {'states64': store.states64[:n].cpu().numpy(), 'states32': store.states32[:n].cpu().numpy(),
            'actions': store.actions[:n].cpu().numpy(), 'values': store.values[:n].cpu().numpy(),
            'path_ptr': store.path_ptr[:len(store) + 1].cpu().numpy(), 'problem': store.problem[:len(store)].cpu().numpy()}


def check_store(store, rows, ptr, ids, dim):
    got = store_arrays(store)
    actions, values = next_train.path_labels(rows, ptr, dim)
    assert same_bits(got['states64'], rows)
    assert same_bits(got['states32'], rows.astype(np.float32))
    assert same_bits(got['actions'], actions)
    assert same_bits(got['values'], values)
    assert np.array_equal(got['path_ptr'], ptr) and np.array_equal(store.host_ptr, ptr)
    assert np.array_equal(got['problem'], ids) and np.array_equal(store.host_problem, ids)
    return got


@pytest.mark.parametrize('dim', [2, 3])
def test_lengths_and_edge_cases(dim):
    rng = np.random.RandomState(70 + dim)
    paths = [random_path(rng, n, dim) for n in (1, 2, 63, 64, 65, 130)] + edge_paths(dim)
    rows, ptr = pack(paths)
    ids = np.arange(100, 100 + len(paths))
    store = next_replay.ReplayStore(dim, len(paths) + 3, len(rows) + 50, DEV)
    assert store.append_paths(rows, ptr, ids) == len(paths)
    got = check_store(store, rows, ptr, ids, dim)
    a = got['actions']
    e = int(ptr[6])                                              # the first edge path: (0, 0) -> (RRT_EPS, 0)
    assert a[e, 0] == np.float32(EPS) and a[e, 1] == 0           # not cut: next - prev itself
    assert np.all(a[ptr[1:] - 1] == 0)                           # the last state's action
    assert np.all(got['values'][ptr[1:] - 1] == 0) and np.all(got['values'] <= 0)
    rep = int(ptr[8])                                            # the repeated state: a zero edge, the same value twice
    assert np.all(a[rep] == 0) and got['values'][rep] == got['values'][rep + 1]
    if dim == 2:        # every action is at most RRT_EPS long (the stick's can differ by a period: interpolate wraps its result)
        assert np.sqrt((a.astype(np.float64) ** 2).sum(axis=1)).max() <= EPS * (1 + 1e-6)


@pytest.mark.parametrize('dim', [2, 3])
def test_200_random_paths_in_one_call_and_a_second_call_behind_it(dim):
    rng = np.random.RandomState(80 + dim)
    paths = [random_path(rng, int(rng.randint(1, 41)), dim) for _ in range(200)]
    rows, ptr = pack(paths)
    ids = rng.randint(0, 2000, 200)
    store = next_replay.ReplayStore(dim, 260, len(rows) + 400, DEV)
    store.append_paths(rows, ptr, ids)
    check_store(store, rows, ptr, ids, dim)
    more = [random_path(rng, n, dim) for n in (5, 1, 70)]
    rows2, ptr2 = pack(more)
    assert store.append_paths(torch.from_numpy(rows2).to(DEV), ptr2, [7, 8, 9]) == 3
    assert len(store) == 203
    check_store(store, np.concatenate([rows, rows2]), np.concatenate([ptr, ptr[-1] + ptr2[1:]]), np.concatenate([ids, [7, 8, 9]]), dim)
    # and the same store again from scratch: the same bits
    again = next_replay.ReplayStore(dim, 260, len(rows) + 400, DEV)
    again.append_paths(rows, ptr, ids)
    again.append_paths(rows2, ptr2, [7, 8, 9])
    for k, v in store_arrays(store).items():
        assert same_bits(v, store_arrays(again)[k]), k


@pytest.mark.parametrize('dim', [2, 3])
def test_recorded_paths_give_the_recorded_labels(dim):
    with np.load(os.path.join(GOLDEN, 'next_train_maze%d.npz' % dim)) as f:
        fx = {k: f[k] for k in f.files}
    store = next_replay.ReplayStore(dim, 2, 17, DEV)             # an exact fit
    store.append_paths(fx['paths'], fx['path_ptr'], [3, 11])
    got = check_store(store, fx['paths'], fx['path_ptr'], np.array([3, 11]), dim)
    assert np.array_equal(got['actions'], fx['actions'].astype(np.float32))         # get_label's own outputs (-0. == 0.)
    assert np.array_equal(got['values'], fx['values'].astype(np.float32))


@pytest.mark.parametrize('dim', [2, 3])
def test_capacity_is_all_or_nothing(dim):
    rng = np.random.RandomState(90 + dim)
    first = [random_path(rng, n, dim) for n in (4, 9)]
    rows, ptr = pack(first)
    store = next_replay.ReplayStore(dim, 4, 13 + 10, DEV)
    store.append_paths(rows, ptr, [0, 1])
    before = {k: v.clone() for k, v in (('s64', store.states64), ('s32', store.states32), ('a', store.actions), ('v', store.values),
                                         ('ptr', store.path_ptr), ('pb', store.problem), ('counts', store.counts))}

    def untouched():
        torch.cuda.synchronize()
        assert len(store) == 2 and store.n_states == 13
        assert torch.equal(store.counts, before['counts']) and int(store.status.item()) == 0
        for key, t in (('s64', store.states64), ('s32', store.states32), ('a', store.actions), ('v', store.values)):
            assert torch.equal(t[:13], before[key][:13]), key
        assert torch.equal(store.path_ptr[:3], before['ptr'][:3]) and torch.equal(store.problem[:2], before['pb'][:2])

    three = pack([random_path(rng, n, dim) for n in (2, 2, 2)])                      # one path too many (6 states would fit)
    with pytest.raises(RuntimeError, match='do not fit'):
        store.append_paths(*three, [5, 6, 7])
    untouched()
    eleven = pack([random_path(rng, n, dim) for n in (5, 6)])                       # one state too many
    with pytest.raises(RuntimeError, match='do not fit'):
        store.append_paths(*eleven, [5, 6])
    untouched()
    bad = pack([random_path(rng, n, dim) for n in (3, 3)])
    with pytest.raises(RuntimeError, match='malformed'):
        store.append_paths(bad[0], np.array([0, 4, 4]), [5, 6])                     # a path without a state
    untouched()
    ten = pack([random_path(rng, n, dim) for n in (5, 5)])                          # the exact fit
    assert store.append_paths(*ten, [5, 6]) == 2
    check_store(store, np.concatenate([rows, ten[0]]), np.concatenate([ptr, 13 + ten[1][1:]]), np.array([0, 1, 5, 6]), dim)
    with pytest.raises(RuntimeError, match='do not fit'):
        store.append_paths(random_path(rng, 1, dim), [0, 1], [9])
    assert len(store) == 4 and store.n_states == 23
