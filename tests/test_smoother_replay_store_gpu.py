"""The smoother's replay store on the device (gnnmp.smoother_replay.SmoothReplayStore over gnnmp_smooth_replay_append /
gnnmp_smooth_replay_gather) against the host construction, bit for bit: ``SmoothBatch(...)`` from lists,
``planner._chain_edge_indices`` and the 500-row filler rule of ``planner._smooth_maze_batch`` / ``obs_data(for_smoother=True)``.

Sample layouts: no collided rows (filler), ``n_free = 2`` only, 501 free + 700 collided rows (truncation), no free rows
(filler), a candidate with two path rows that is not taken; path lengths 3, 4 and 65 (the first beyond one wave of rows);
mixed ``take`` flags and none taken; two appends in a row; a group with a repeated index in a loop order that is not the stored
order; more than 64 candidates and more than 64 group entries (the second chunk of both scans)."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import planner
from gnnmp.smoother import SmoothBatch
from gnnmp.smoother_replay import SmoothReplayStore

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# (path rows, free rows, collided rows) of the candidates
LAYOUT = [(3, 40, 0), (4, 2, 0), (65, 501, 700), (5, 0, 7), (2, 9, 9), (4, 30, 20)]


def _source(C, layout, seed):
    gen = torch.Generator().manual_seed(seed)
    rows = lambda n: torch.rand(n, C, generator=gen) * 2 - 1      # noqa: E731
    return [dict(path=rows(P), target=rows(P), free=rows(F), coll=rows(Co)) for P, F, Co in layout]


def _append(store, cands, take, ids, take_upper=None):
    ptr = lambda counts: torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=DEV)      # noqa: E731
    return store.append(torch.cat([c['path'] for c in cands]).to(DEV), torch.cat([c['target'] for c in cands]).to(DEV),
                        ptr([c['path'].shape[0] for c in cands]),
                        torch.cat([torch.cat((c['free'], c['coll'])) for c in cands]).to(DEV),
                        ptr([c['free'].shape[0] + c['coll'].shape[0] for c in cands]),
                        torch.tensor([c['free'].shape[0] for c in cands], dtype=torch.int32, device=DEV),
                        torch.tensor(take, dtype=torch.int32, device=DEV), torch.tensor(ids, dtype=torch.int32, device=DEV),
                        take_upper=take_upper)


def _stored(c):
    """What the store keeps of a candidate: planner._smooth_maze_batch's rule."""
    C = c['path'].shape[1]
    side = lambda t: t[:500] if t.shape[0] else torch.zeros(1, C)      # noqa: E731
    return dict(path=c['path'], target=c['target'], free=side(c['free']), coll=side(c['coll']))


def _check_store(store, want, ids):
    """The device arrays and the mirror against the list ``want`` of stored samples."""
    n = len(want)
    assert len(store) == n
    for name, key in (('path', 'path'), ('target', 'target'), ('free', 'free'), ('collided', 'coll')):
        rows = torch.cat([w[key] for w in want]) if n else torch.zeros(0, store.C)
        assert torch.equal(getattr(store, name)[:rows.shape[0]].cpu(), rows), name
    for dev_ptr, host_ptr, key in ((store.path_ptr, store.host_path_ptr, 'path'), (store.free_ptr, store.host_free_ptr, 'free'),
                                   (store.coll_ptr, store.host_coll_ptr, 'coll')):
        ptr = np.concatenate([[0], np.cumsum([w[key].shape[0] for w in want])]).astype(np.int64)
        assert np.array_equal(host_ptr, ptr), key
        assert np.array_equal(dev_ptr[:n + 1].cpu().numpy(), ptr), key
    assert store.host_problem.tolist() == list(ids) and store.problem[:n].cpu().tolist() == list(ids)
    bank = store.counts.cpu().numpy().reshape(2, 4)[store.epoch & 1]
    assert bank.tolist() == list(store.rows_in_use())
    assert int(store.status.cpu()) == 0


def _check_batch(store, want, idx, loops):
    sb, targets, order = store.batch(idx, loops)
    assert sorted(order) == list(range(len(idx)))
    assert [loops[b] for b in order] == sorted(loops, reverse=True)
    pick = [want[idx[b]] for b in order]
    lengths = [w['path'].shape[0] for w in pick]
    edges = torch.from_numpy(planner._chain_edge_indices(lengths))
    off = np.concatenate([[0], np.cumsum([3 * p - 2 for p in lengths])])
    ref = SmoothBatch([w['path'] for w in pick], [w['free'] for w in pick], [w['coll'] for w in pick],
                      [edges[:, a:b] for a, b in zip(off[:-1], off[1:])], DEV)
    if len(pick) == 1:                                            # the one-problem constructor keeps no concatenation
        assert torch.equal(sb.edge_index.cpu(), planner.chain_edge_index(lengths[0]))
    for name in ('path', 'free', 'collided', 'edge_index', 'path_ptr', 'free_ptr', 'coll_ptr', 'edge_ptr'):
        got, exp = getattr(sb, name), getattr(ref, name)
        assert got.dtype == exp.dtype and torch.equal(got.cpu(), exp.cpu()), name
    assert torch.equal(targets.cpu(), torch.cat([w['target'] for w in pick]))
    for name in ('n', 'max_path', 'max_samples', 'max_edges', 'path_counts', 'free_counts', 'coll_counts', 'edge_counts'):
        assert getattr(sb, name) == getattr(ref, name), name
    return sb


@pytest.mark.parametrize('C', [2, 3, 14])
def test_append_then_gather_bit_for_bit(C):
    cands = _source(C, LAYOUT, 10 + C)
    store = SmoothReplayStore(C, 16, 400, 2000, 2000, DEV)
    # nothing taken: a launch that adds nothing
    assert _append(store, cands, [0] * 6, list(range(6))) == 0
    _check_store(store, [], [])
    # mixed flags; the two-row candidate is not taken
    take = [1, 0, 1, 1, 0, 1]
    assert _append(store, cands, take, [100 + i for i in range(6)]) == 4
    want = [_stored(c) for c, t in zip(cands, take) if t]
    ids = [100, 102, 103, 105]
    _check_store(store, want, ids)
    assert want[1]['free'].shape[0] == 500 and want[1]['coll'].shape[0] == 500                 # truncation
    assert not want[0]['coll'].any() and want[0]['coll'].shape[0] == 1                           # filler, collided side
    assert not want[2]['free'].any() and want[2]['free'].shape[0] == 1                           # filler, free side
    # a second call behind the first: the other counts bank; take_upper as the caller's bound
    assert _append(store, cands[:2], [1, 1], [7, 8], take_upper=2) == 2
    want += [_stored(cands[0]), _stored(cands[1])]
    ids += [7, 8]
    _check_store(store, want, ids)
    assert want[5]['free'].shape[0] == 2                                                         # n_free = 2 only
    # a group with a repeated index, in a loop order that is not the stored order; one sample alone; all of them
    _check_batch(store, want, [2, 0, 1, 2, 5], [3, 9, 5, 1, 9])
    _check_batch(store, want, [1], [4])
    _check_batch(store, want, [5, 4, 3, 2, 1, 0], [1, 2, 3, 4, 5, 6])
    with pytest.raises(IndexError):
        store.batch([6], [1])
    store.check_status()


def test_more_than_one_chunk_of_candidates_and_of_group_entries():
    C = 2
    layout = [(3 + i % 4, 1 + i % 5, i % 3) for i in range(70)]
    cands = _source(C, layout, 5)
    take = [int(i % 7 != 3) for i in range(70)]
    store = SmoothReplayStore(C, 64, 400, 400, 400, DEV)
    assert _append(store, cands, take, list(range(70))) == sum(take)
    want = [_stored(c) for c, t in zip(cands, take) if t]
    _check_store(store, want, [i for i in range(70) if take[i]])
    rng = np.random.RandomState(3)
    idx = rng.randint(0, len(want), 70).tolist()
    _check_batch(store, want, idx, rng.randint(1, 10, 70).tolist())


def _snapshot(store):
    arrays = [getattr(store, n).clone() for n in ('path', 'target', 'free', 'collided', 'path_ptr', 'free_ptr', 'coll_ptr', 'problem')]
    mirror = [a.copy() for a in (store.host_path_ptr, store.host_free_ptr, store.host_coll_ptr, store.host_problem)]
    return arrays, mirror, store.rows_in_use()


def _unchanged(store, snap):
    arrays, mirror, use = snap
    names = ('path', 'target', 'free', 'collided', 'path_ptr', 'free_ptr', 'coll_ptr', 'problem')
    assert all(torch.equal(getattr(store, n), a) for n, a in zip(names, arrays))
    assert all(np.array_equal(a, b) for a, b in zip((store.host_path_ptr, store.host_free_ptr, store.host_coll_ptr,
                                                     store.host_problem), mirror))
    assert store.rows_in_use() == use
    assert store.counts.cpu().numpy().reshape(2, 4)[store.epoch & 1].tolist() == list(use)
    assert int(store.status.cpu()) == 0                           # the raise cleared it


@pytest.mark.parametrize('which', ['samples', 'path rows', 'free rows', 'collided rows'])
def test_overflow_of_each_capacity_is_all_or_nothing(which):
    C = 3
    cands = _source(C, [(4, 10, 5), (3, 6, 0), (5, 0, 4)], 21)
    first, rest = cands[:1], cands[1:]
    need = {'samples': 3, 'path rows': 12, 'free rows': 17, 'collided rows': 10}      # all three: 4+3+5, 10+6+1, 5+1+4
    caps = dict(need)
    caps[which] -= 1
    store = SmoothReplayStore(C, caps['samples'], caps['path rows'], caps['free rows'], caps['collided rows'], DEV)
    assert _append(store, first, [1], [0]) == 1
    snap = _snapshot(store)
    with pytest.raises(RuntimeError, match='do not fit'):
        _append(store, rest, [1, 1], [1, 2])
    _unchanged(store, snap)
    # what fits afterwards is appended behind the first sample
    fits = {'samples': [1, 0], 'path rows': [1, 0], 'free rows': [0, 1], 'collided rows': [1, 0]}[which]
    assert _append(store, rest, fits, [1, 2]) == 1
    _check_store(store, [_stored(first[0]), _stored(rest[fits.index(1)])], [0, 1 + fits.index(1)])


def test_a_taken_source_of_two_path_rows_is_malformed():
    C = 2
    cands = _source(C, [(4, 10, 5), (2, 6, 3), (3, 5, 5)], 33)
    store = SmoothReplayStore(C, 8, 100, 100, 100, DEV)
    assert _append(store, cands[:1], [1], [0]) == 1
    snap = _snapshot(store)
    with pytest.raises(RuntimeError, match='malformed source'):
        _append(store, cands, [1, 1, 1], [1, 2, 3])
    _unchanged(store, snap)
    with pytest.raises(RuntimeError, match='malformed source'):     # more flags set than the caller's bound
        _append(store, cands, [1, 0, 1], [1, 2, 3], take_upper=1)
    _unchanged(store, snap)
    assert _append(store, cands, [1, 0, 1], [1, 2, 3]) == 2        # the same candidates without the short one
    _check_store(store, [_stored(cands[0]), _stored(cands[0]), _stored(cands[2])], [0, 1, 3])
