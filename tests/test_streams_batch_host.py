"""streams_batch.AttemptBlocks with host draws on the CPU: the attempt-block loop of the batched planners without their kernels.
The stand-in sampler classifies a block with ``Maze2D`` / ``Maze3D.classify_draws``: status 1 when the block holds fewer than n
free draws, otherwise ``used`` = index of the n-th free draw + 1.  Problems 0-11 of the maze2 set at n = 30 and of the maze3 set
at n = 10 from an estimate of 0 (a first block of 64 rows) mix problems that finish, retry and retry twice in one call."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import gnnmp  # noqa: F401
from gnnmp import streams_batch
from gnnmp.maze2d import Maze2D, Maze3D

SETS = {2: ('evalset_mazehard_first1000.npz', 30), 3: ('evalset_maze3_first40_b200_k12_s9.npz', 10)}
ROWS = 1024                            # rows of every reference stream: more than any run below draws
_CACHE = {}


def _case(dim):
    """Environments, seeds, reference streams and their free flags, computed once and left unchanged."""
    if dim not in _CACHE:
        name, n = SETS[dim]
        cls = Maze2D if dim == 2 else Maze3D
        lim = streams_batch.sample_limits(dim)
        seeds = streams_batch.stream_seeds(1234, range(12))
        envs, ref, free = [], [], []
        with np.load(os.path.join(GOLDEN, name)) as f:
            for i, s in enumerate(seeds):
                envs.append(streams_batch.problem_env(dict(map=f['maps'][i], init_state=f['init_states'][i], goal_state=f['goal_states'][i])))
                assert type(envs[-1]) is cls
                ref.append(np.random.RandomState(s).uniform(-lim, lim, (ROWS, dim)))
                free.append(envs[-1].classify_draws(ref[-1])[0])
        _CACHE[dim] = dict(n=n, seeds=seeds, envs=envs, ref=ref, free=free)
    return _CACHE[dim]


def _sampler(c, n, log, with_used=True):
    """The stand-in ``sample`` callback; ``log[b]`` receives (block, used) of every attempt of problem b (used 0 = ran out)."""
    def sample(att, att_ptr, mask_d):
        att, B = att.numpy(), len(c['envs'])
        status, used = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        for b in range(B):
            block = att[att_ptr[b]:att_ptr[b + 1]]
            if not mask_d[b]:
                assert block.shape[0] == 0
                continue
            hits = np.flatnonzero(c['envs'][b].classify_draws(block)[0])
            if hits.size < n:
                status[b] = 1
            else:
                used[b] = hits[n - 1] + 1
            log[b].append((block.copy(), int(used[b])))
        return (torch.from_numpy(status), torch.from_numpy(used)) if with_used else (torch.from_numpy(status),)
    return sample


def _predict(free, n, want, pos, have):
    """Blocks one problem sees in a round that starts with ``pos`` rows consumed and ``have`` rows drawn -> (sizes, new pos, new
    have): the buffer is topped up to ``want`` rows, doubled until it holds n free draws, then cut behind the n-th."""
    sizes = []
    while True:
        have = max(have, pos + want)
        sizes.append(have - pos)
        hits = np.flatnonzero(free[pos:have])
        if hits.size >= n:
            return sizes, pos + int(hits[n - 1]) + 1, have
        want *= 2


def _first_round_sizes(c):
    return [[64] if f[:64].sum() >= c['n'] else [64, 128] if f[:128].sum() >= c['n'] else [64, 128, 256] for f in c['free']]


@pytest.mark.parametrize('dim', [2, 3])
def test_inputs_mix_finishing_and_retrying_problems(dim):
    """The precondition of the tests below, from numpy's own draws."""
    c = _case(dim)
    c64, c128, c256 = (np.array([int(f[:m].sum()) for f in c['free']]) for m in (64, 128, 256))
    if dim == 2:
        assert sorted(c64[c64 >= 30]) == [30, 30, 30, 31, 35, 39] and sorted(c64[c64 < 30]) == [26, 29, 29, 29, 29, 29]
        assert (c128 >= 56).all()
    else:
        assert (c64 >= 10).sum() == 8 and ((c64 < 10) & (c128 >= 10)).sum() == 3
        assert (c64[1], c128[1], c256[1]) == (3, 9, 17) and np.flatnonzero(c128 < 10).tolist() == [1]


@pytest.mark.parametrize('dim', [2, 3])
def test_two_committed_rounds_consume_the_stream_prefix(dim):
    c = _case(dim)
    n, B = c['n'], 12
    estimate = [0.0, 0.0]
    blocks = streams_batch.AttemptBlocks(c['seeds'], dim, 'cpu', 'host', estimate)
    pos, have, taken = [0] * B, [0] * B, [[] for _ in range(B)]
    for rnd in range(2):
        old = estimate[dim - 2]
        want = int(n * old * 1.25) + 64
        assert want == 64 or rnd == 1
        log = [[] for _ in range(B)]
        words = blocks.run(np.arange(B), n, _sampler(c, n, log), no_room='stand-in: %s')
        consumed = 0
        for b in range(B):
            sizes, new_pos, have[b] = _predict(c['free'][b], n, want, pos[b], have[b])
            assert [blk.shape[0] for blk, _ in log[b]] == sizes, (rnd, b)
            if rnd == 0:
                assert sizes == _first_round_sizes(c)[b], b
            for blk, used in log[b]:                                   # every block starts where the last round stopped
                assert np.array_equal(blk, c['ref'][b][pos[b]:pos[b] + blk.shape[0]]), (rnd, b)
            assert [u for _, u in log[b][:-1]] == [0] * (len(sizes) - 1)
            used = log[b][-1][1]
            assert used == new_pos - pos[b] and int(words[1][b]) == used and int(words[0][b]) == 0
            taken[b].append(log[b][-1][0][:used])
            consumed += used
            pos[b] = new_pos
        assert estimate[dim - 2] == max(1.5, 0.5 * old + 0.5 * consumed / (n * B))
        assert estimate[3 - dim] == 0.0
    for b in range(B):                                                 # nothing lost, repeated or reordered across the carry
        end = int(np.flatnonzero(c['free'][b])[2 * n - 1]) + 1
        assert np.array_equal(np.concatenate(taken[b]), c['ref'][b][:end]), b
        assert np.array_equal(blocks.bufs[b], c['ref'][b][pos[b]:have[b]]), b


@pytest.mark.parametrize('dim', [2, 3])
def test_a_round_of_some_problems_leaves_the_others_alone(dim):
    c = _case(dim)
    n = c['n']
    blocks = streams_batch.AttemptBlocks(c['seeds'], dim, 'cpu', 'host', [0.0, 0.0])
    log = [[] for _ in range(12)]
    blocks.run(np.array([1, 4, 7]), n, _sampler(c, n, log), no_room='stand-in: %s')
    for b in range(12):
        assert bool(log[b]) == (b in (1, 4, 7))
        assert blocks.bufs[b].shape[0] == 0 or b in (1, 4, 7)
    assert [blk.shape[0] for blk, _ in log[1]] == _first_round_sizes(c)[1]


@pytest.mark.parametrize('dim', [2, 3])
def test_a_run_without_commit_gets_the_same_blocks_and_trims_nothing(dim):
    """The way BIT* samples: the sampler returns its status only and starts over on every longer block."""
    c = _case(dim)
    n = c['n']
    estimate = [0.0, 0.0]
    blocks = streams_batch.AttemptBlocks(c['seeds'], dim, 'cpu', 'host', estimate)
    for rnd in range(2):                                               # the second run draws nothing new
        log = [[] for _ in range(12)]
        blocks.run(np.arange(12), n, _sampler(c, n, log, with_used=False), commit=False, no_room='stand-in: %s')
        for b in range(12):
            sizes = _first_round_sizes(c)[b]
            assert [blk.shape[0] for blk, _ in log[b]] == (sizes if rnd == 0 else sizes[-1:]), (rnd, b)
            for blk, _ in log[b]:
                assert np.array_equal(blk, c['ref'][b][:blk.shape[0]]), (rnd, b)
            assert np.array_equal(blocks.bufs[b], c['ref'][b][:sizes[-1]]), (rnd, b)
        assert estimate == [0.0, 0.0]


def test_a_status_above_one_raises_the_callers_text():
    c = _case(2)
    blocks = streams_batch.AttemptBlocks(c['seeds'], 2, 'cpu', 'host', [0.0, 0.0])

    def sample(att, att_ptr, mask_d):
        status = torch.zeros(12, dtype=torch.int32)
        status[5] = 2
        return status, torch.zeros(12, dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r'no room for problem\(s\) \[5\]'):
        blocks.run(np.arange(12), 30, sample, no_room='no room for problem(s) %s')
