"""gnnmp.rng.MTStreams (gnnmp_mt19937_seed / gnnmp_mt19937_uniform) against numpy's own ``RandomState``: rows and states
compared with ``np.array_equal`` -- no tolerance anywhere.  Row counts sit on both sides of every edge of the kernel: the
twist's segments (words 227 and 454), the end of a 624-word block, several blocks; the bounds include columns whose limits
are not powers of two (the stick robot's z = +-0.4, and 0.3 .. 1.7), where a fused multiply-add would change the draws."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import planner
from gnnmp.maze2d import LIMITS3
from gnnmp.rng import MTStreams

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEEDS = [0, 1, 0xffffffff] + planner.stream_seeds(1234, range(5))
# rows per stream, by row width: a row takes 2 * dim words, so word 227 / 454 / 624 fall at these counts
COUNTS = {1: [0, 1, 113, 114, 227, 228, 311, 312, 313, 1000],
          2: [0, 1, 56, 57, 113, 114, 155, 156, 157, 1000],
          3: [0, 1, 37, 38, 75, 76, 103, 104, 105, 1000]}
ON_BLOCK = {1: 312, 2: 156, 3: 104}    # exactly one block: pos stays 624 and the key is not twisted a second time
BOUNDS = {1: [((-1.0,), (1.0,)), ((0.3,), (1.7,))],
          2: [((-1.0, -1.0), (1.0, 1.0)), ((0.3, -1.0), (1.7, 1.0))],
          3: [(tuple(-LIMITS3), tuple(LIMITS3)), ((0.3, -1.0, -0.4), (1.7, 1.0, 0.4))]}
CASES = [(dim, lo, hi) for dim in (1, 2, 3) for lo, hi in BOUNDS[dim]]


def _seeds(n):
    return [SEEDS[i % len(SEEDS)] for i in range(n)]


def _gen(seed):
    return np.random.RandomState(int(seed) & 0xffffffff)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(np.asarray(a[1], dtype=np.uint32), np.asarray(b[1], dtype=np.uint32)) and int(a[2]) == int(b[2])


def _split(rows, counts):
    ptr = np.concatenate(([0], np.cumsum(counts)))
    rows = rows.cpu().numpy()
    return [rows[ptr[i]:ptr[i + 1]] for i in range(len(counts))]


def test_seeding_equals_numpy():
    s = MTStreams(SEEDS, DEV)
    for i, seed in enumerate(SEEDS):
        ref = _gen(seed).get_state()
        assert ref[2] == 624
        assert _same_state(s.state(i), ref), seed
    g = np.random.RandomState()
    g.set_state(s.state(3))                                       # the tuple is one set_state accepts
    assert np.array_equal(g.uniform(-1, 1, (5, 2)), _gen(SEEDS[3]).uniform(-1, 1, (5, 2)))


@pytest.mark.parametrize('dim,lo,hi', CASES)
def test_ragged_fill_commit_then_continue(dim, lo, hi):
    """One ragged launch (every count of the list, one stream each) with commit: rows and states are numpy's; a second
    committed fill continues where the first ended (a rows then b rows = numpy's a + b rows)."""
    counts = COUNTS[dim]
    seeds = _seeds(len(counts))
    s = MTStreams(seeds, DEV)
    gens = [_gen(x) for x in seeds]
    lo, hi = np.array(lo), np.array(hi)
    rows, status = s.uniform(counts, lo, hi, commit=True)
    assert rows.shape == (sum(counts), dim) and rows.dtype == torch.float64
    assert not status.any().item()
    for i, (got, c) in enumerate(zip(_split(rows, counts), counts)):
        assert np.array_equal(got, gens[i].uniform(lo, hi, (c, dim))), (i, c)
        assert _same_state(s.state(i), gens[i].get_state()), (i, c)
    j = counts.index(ON_BLOCK[dim])
    ref = gens[j].get_state()                                     # consumed exactly to the end of a block: numpy has not twisted again
    assert ref[2] == 624 and s.state(j)[2] == 624 and np.array_equal(s.state(j)[1], ref[1])
    more = counts[::-1]
    rows, status = s.uniform(more, lo, hi, commit=True)
    assert not status.any().item()
    for i, (got, c) in enumerate(zip(_split(rows, more), more)):
        assert np.array_equal(got, gens[i].uniform(lo, hi, (c, dim))), (i, counts[i], c)
        assert _same_state(s.state(i), gens[i].get_state()), (i, counts[i], c)


@pytest.mark.parametrize('dim', [2, 3])
def test_fill_without_commit_repeats(dim):
    counts = COUNTS[dim]
    seeds = _seeds(len(counts))
    s = MTStreams(seeds, DEV)
    lo, hi = (np.array(x) for x in BOUNDS[dim][1])
    a, _ = s.uniform(counts, lo, hi)
    b, _ = s.uniform(counts, lo, hi)
    assert torch.equal(a, b)
    for i, seed in enumerate(seeds):
        assert _same_state(s.state(i), _gen(seed).get_state()), i
    longer = [c + 7 for c in counts]                              # the same state, filled from again with a longer count
    c, _ = s.uniform(longer, lo, hi)
    for i, (short, long_) in enumerate(zip(_split(a, counts), _split(c, longer))):
        assert np.array_equal(long_[:counts[i]], short), i
        assert np.array_equal(long_, _gen(seeds[i]).uniform(lo, hi, (longer[i], dim))), i


@pytest.mark.parametrize('dim', [2, 3])
def test_advance_then_fill(dim):
    """advance(u) then a fill = numpy's rows [u:], u over the edge counts (as an int32 device tensor, the sampler's form)."""
    skip = COUNTS[dim]
    seeds = _seeds(len(skip))
    s = MTStreams(seeds, DEV)
    lo, hi = (np.array(x) for x in BOUNDS[dim][0])
    status = s.advance(torch.tensor(skip, dtype=torch.int32, device=DEV), dim)
    assert not status.any().item()
    take = [40] * len(skip)
    rows, _ = s.uniform(take, lo, hi, commit=True)
    for i, got in enumerate(_split(rows, take)):
        g = _gen(seeds[i])
        assert np.array_equal(got, g.uniform(lo, hi, (skip[i] + 40, dim))[skip[i]:]), (i, skip[i])
        assert _same_state(s.state(i), g.get_state()), (i, skip[i])


@pytest.mark.parametrize('dim', [1, 2, 3])
def test_continues_a_numpy_state_with_odd_pos(dim):
    """States uploaded from generators that drew ONE 32-bit word first: every double then straddles odd word positions,
    and one of them takes word 623 of a block and word 0 of the next."""
    counts = COUNTS[dim]
    gens = [_gen(x) for x in _seeds(len(counts))]
    for k, g in enumerate(gens):
        if k % 2:
            g.uniform(size=100)                                   # some start in the middle of a later block
        g.bytes(4)
        assert g.get_state()[2] % 2 == 1
    s = MTStreams.from_states([g.get_state() for g in gens], DEV)
    lo, hi = (np.array(x) for x in BOUNDS[dim][1])
    rows, status = s.uniform(counts, lo, hi, commit=True)
    assert not status.any().item()
    for i, (got, c) in enumerate(zip(_split(rows, counts), counts)):
        assert np.array_equal(got, gens[i].uniform(lo, hi, (c, dim))), (i, c)
        assert _same_state(s.state(i), gens[i].get_state()), (i, c)


def test_active_mask_leaves_streams_alone():
    counts = [50, 120, 0, 300, 7, 104, 105, 33]
    s = MTStreams(SEEDS, DEV)
    mask = np.array([1, 0, 1, 0, 1, 1, 0, 1], dtype=np.uint8)
    ptr = np.concatenate(([0], np.cumsum(counts)))
    out = torch.full((int(ptr[-1]), 3), -7.25, dtype=torch.float64, device=DEV)
    rows, status = s.uniform(counts, -LIMITS3, LIMITS3, out_ptr=ptr, commit=True, active=torch.from_numpy(mask).to(DEV), out=out)
    assert rows.data_ptr() == out.data_ptr()
    status = status.cpu().numpy()
    for i, got in enumerate(_split(rows, counts)):
        g = _gen(SEEDS[i])
        if mask[i]:
            assert np.array_equal(got, g.uniform(-LIMITS3, LIMITS3, (counts[i], 3))), i
        else:
            assert (got == -7.25).all(), i
        assert _same_state(s.state(i), g.get_state()), i
        assert status[i] == 0
    st = s.advance(counts, 3, active=torch.from_numpy(1 - mask).to(DEV))      # now only the others move
    assert not st.any().item()
    for i in range(len(counts)):
        g = _gen(SEEDS[i])
        g.uniform(-LIMITS3, LIMITS3, (counts[i], 3))
        assert _same_state(s.state(i), g.get_state()), i


def test_block_outside_out_is_status_2():
    """A block that ends behind out_rows, one that starts before row 0 and a negative count: status 2, nothing written,
    state untouched, and the other streams complete."""
    n = len(SEEDS)
    counts = [10, 20, 30, 40, 50, 60, -1, 25]
    ptr = np.array([0, 10, 30, 60, -5, 150, 210, 210, 235], dtype=np.int64)
    ptr[5] = 180                                                  # stream 5: rows [180, 240) of a 200-row buffer
    out = torch.full((200, 2), 9.5, dtype=torch.float64, device=DEV)
    s = MTStreams(SEEDS, DEV)
    c = torch.tensor(counts, dtype=torch.int32, device=DEV)
    _, status = s.uniform(c, (-1.0, -1.0), (1.0, 1.0), out_ptr=torch.from_numpy(ptr).to(DEV), commit=True, out=out)
    assert status.cpu().tolist() == [0, 0, 0, 0, 2, 2, 2, 2]     # stream 4 starts at -5; 7's block [210, 235) lies behind the buffer
    got = out.cpu().numpy()
    written = np.zeros(200, dtype=bool)
    for i in range(n):
        g = _gen(SEEDS[i])
        if i < 4:
            lo_row = int(ptr[i])
            assert np.array_equal(got[lo_row:lo_row + counts[i]], g.uniform(-1, 1, (counts[i], 2))), i
            written[lo_row:lo_row + counts[i]] = True
        assert _same_state(s.state(i), g.get_state()), i
    assert (got[~written] == 9.5).all()


def test_two_runs_are_bit_identical():
    counts = COUNTS[3]
    runs = []
    for _ in range(2):
        s = MTStreams(_seeds(len(counts)), DEV)
        rows, _ = s.uniform(counts, -LIMITS3, LIMITS3, commit=True)
        runs.append((rows.cpu().numpy(), s._state.cpu().numpy()))
    assert np.array_equal(runs[0][0].view(np.uint64), runs[1][0].view(np.uint64))
    assert np.array_equal(runs[0][1], runs[1][1])
