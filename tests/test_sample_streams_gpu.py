"""Per-problem-stream rejection sampling that appends (gnnmp_maze_sample_streams) and the assembly of a round's node rows
(gnnmp_maze_rounds_gather), csrc/maze_kernels.hip, against ``Maze2D`` / ``Maze3D.classify_draws`` plus the append rule of
``explore`` restated in numpy (eval_gnn.py:180 for the first sampling, :243-245 for the later ones).  Everything is compared
bit for bit: rows, counts, draws consumed, collision checks."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import planner
from gnnmp.maze2d import Maze2D, Maze3D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7.0


def _env(dim, w, rng):
    """One random problem: sparse enough maps that a 0.2-long stick still finds room."""
    density = {(2, 15): 0.4, (2, 70): 0.4, (3, 15): 0.10, (3, 70): 0.02}[(dim, w)]
    grid = (rng.random((w, w)) < density).astype(np.float64)
    lim = np.array([1.0, 1.0, 0.4])[:dim]
    cls = Maze3D if dim == 3 else Maze2D
    e = cls(grid[None], rng.uniform(-lim, lim, (1, dim)), rng.uniform(-lim, lim, (1, dim)))
    e.init_new_problem(0)
    return e


def _crafted(env, pattern, rng):
    """Draws of ``env`` whose free flags are ``pattern`` (bool [m]), picked from classified uniform draws."""
    dim = env.config_dim
    lim = np.asarray(env.SAMPLE_LIMITS, dtype=np.float64)
    pattern = np.asarray(pattern, dtype=bool)
    need = {True: int(pattern.sum()), False: int((~pattern).sum())}
    have = {True: np.zeros((0, dim)), False: np.zeros((0, dim))}
    while any(have[f].shape[0] < need[f] for f in (True, False)):
        d = rng.uniform(-lim, lim, (4096, dim))
        free, _ = env.classify_draws(d)
        have[True], have[False] = np.concatenate((have[True], d[free])), np.concatenate((have[False], d[~free]))
    out = np.empty((pattern.size, dim))
    out[pattern], out[~pattern] = have[True][:need[True]], have[False][:need[False]]
    assert np.array_equal(env.classify_draws(out)[0], pattern)
    return out


def _pattern(n, p, tail, rng):
    """Free flags with the n-th free draw at index p, the other n - 1 spread before it, and ``tail`` mixed draws behind."""
    pat = np.zeros(p + 1 + tail, dtype=bool)
    pat[p] = True
    if n > 1:
        pat[rng.choice(p, n - 1, replace=False)] = True
    pat[p + 1:] = rng.random(tail) < 0.5
    return pat


def _oracle(env, draws, n, free_rows, coll_rows):
    """The append rule on the host: (free rows, collided rows, used, checks) or None when the block ends too early."""
    free, checks = env.classify_draws(draws)
    idx = np.flatnonzero(free)
    if idx.size < n:
        return None
    used = int(idx[n - 1]) + 1
    d, f = draws[:used].astype(np.float32), free[:used]
    if free_rows.shape[0] == 0:                                   # eval_gnn.py:180-184
        rej = d[~f][:n]
        ends = np.stack((env.init_state, env.goal_state)).astype(np.float32)
        return np.concatenate((ends, d[f])), rej, used, int(checks[:used].sum())
    fr = np.concatenate((free_rows, d[f]))                        # eval_gnn.py:241-245
    return fr, np.concatenate((coll_rows, d[~f]))[:fr.shape[0]], used, int(checks[:used].sum())


class _Batch:
    def __init__(self, envs, cap):
        self.envs, self.dim, self.B = envs, envs[0].config_dim, len(envs)
        self.store = planner.MazeRoundsStore(self.B, cap, 4, self.dim, DEV)
        self.store.free_pool.fill_(SENTINEL)
        self.store.coll_pool.fill_(SENTINEL)
        as64 = lambda rows: torch.from_numpy(np.ascontiguousarray(np.asarray(rows, dtype=np.float64))).to(DEV)      # noqa: E731
        self.maps = as64([e.map for e in envs])
        self.init64 = as64([np.asarray(e.init_state).reshape(self.dim) for e in envs])
        self.goal64 = as64([np.asarray(e.goal_state).reshape(self.dim) for e in envs])
        self.free = [np.zeros((0, self.dim), dtype=np.float32) for _ in envs]      # the host's copy of the pools
        self.coll = [np.zeros((0, self.dim), dtype=np.float32) for _ in envs]

    def launch(self, blocks, n, active=None):
        ptr = np.concatenate(([0], np.cumsum([b.shape[0] for b in blocks]))).astype(np.int64)
        att = torch.from_numpy(np.concatenate(blocks)).to(DEV)
        act = None if active is None else torch.from_numpy(np.asarray(active, dtype=np.uint8)).to(DEV)
        used, checks, status = planner.maze_sample_streams(self.store, att, ptr, self.maps, self.init64, self.goal64, n, active=act)
        torch.cuda.synchronize()
        return used.cpu().numpy(), checks.cpu().numpy(), status.cpu().numpy()

    def pools(self):
        s = self.store
        return s.free_pool.cpu().numpy(), s.coll_pool.cpu().numpy(), s.n_free.cpu().numpy(), s.n_coll.cpu().numpy()

    def check_round(self, blocks, n, active=None):
        """One launch against the oracle; keeps the host's copy of the pools up to date."""
        before = self.pools()
        used, checks, status = self.launch(blocks, n, active)
        fp, cp, nf, nc = self.pools()
        for b, env in enumerate(self.envs):
            exp = None if (active is not None and not active[b]) else _oracle(env, blocks[b], n, self.free[b], self.coll[b])
            if exp is None:                                        # masked out, or its block ended early: untouched
                if active is None or active[b]:
                    assert status[b] == 1 and used[b] == 0 and checks[b] == 0, b
                assert nf[b] == before[2][b] and nc[b] == before[3][b], b
                assert np.array_equal(fp[b], before[0][b]) and np.array_equal(cp[b], before[1][b]), b
                continue
            fr, co, u, c = exp
            assert status[b] == 0 and used[b] == u and checks[b] == c, (b, status[b], used[b], u, checks[b], c)
            assert nf[b] == fr.shape[0] and nc[b] == co.shape[0], (b, nf[b], fr.shape[0], nc[b], co.shape[0])
            assert np.array_equal(fp[b, :nf[b]], fr) and np.array_equal(cp[b, :nc[b]], co), b
            assert (fp[b, nf[b]:] == SENTINEL).all() and (cp[b, nc[b]:] == SENTINEL).all(), b      # nothing behind the counts
            self.free[b], self.coll[b] = fr, co
        return used, checks, status


POSITIONS = (63, 64, 1023, 1024, 2047, 2048, 11, 300)             # index of the n-th free draw (step position = index % 1024)


@pytest.mark.parametrize('dim,w', [(2, 15), (2, 70), (3, 15), (3, 70)])
def test_crafted_streams(dim, w):
    """40 problems (more workgroups than XCDs), the n-th free draw at every edge of a 1024-draw step and of a wave; problem 3's
    block ends one draw early, problem 5 is masked out."""
    rng = np.random.default_rng(100 * dim + w)
    n, B = 8, 40
    envs = [_env(dim, w, rng) for _ in range(B)]
    blocks = []
    for b, env in enumerate(envs):
        p = POSITIONS[b % len(POSITIONS)]
        blk = _crafted(env, _pattern(n, p, tail=int(rng.integers(0, 40)), rng=rng), rng)
        blocks.append(blk[:p] if b == 3 else blk)                 # problem 3: one draw short of its n-th free one
    active = np.ones(B, dtype=np.uint8)
    active[5] = 0
    bt = _Batch(envs, cap=16)
    used, checks, status = bt.check_round(blocks, n, active)
    assert status[3] == 1 and (np.delete(status, [3, 5]) == 0).all()
    assert sorted(set(used[used > 0] - 1)) == sorted(set(POSITIONS))
    if dim == 2:
        assert np.array_equal(checks, used)
    # the same launch on a fresh store: identical, bit for bit
    again = _Batch(envs, cap=16)
    assert all(np.array_equal(x, y) for x, y in zip(again.launch(blocks, n, active), (used, checks, status)))
    assert all(np.array_equal(x, y) for x, y in zip(again.pools(), bt.pools()))
    # problem 3 alone with its whole block, the others masked out: now it completes, and nobody else moves
    blocks[3] = _crafted(envs[3], _pattern(n, POSITIONS[3], 5, rng), rng)
    only = np.zeros(B, dtype=np.uint8)
    only[3] = 1
    bt.check_round(blocks, n, only)
    assert bt.pools()[2][3] == n + 2


@pytest.mark.parametrize('dim', [2, 3])
def test_single_problem_and_first_draw(dim):
    """B = 1; n = 1 with the free draw at step position 0 (used = 1), then a second round of one draw at index 1024."""
    rng = np.random.default_rng(7 + dim)
    env = _env(dim, 15, rng)
    bt = _Batch([env], cap=2)
    used, _, _ = bt.check_round([_crafted(env, [True, False, True], rng)], 1)
    assert used[0] == 1
    used, _, _ = bt.check_round([_crafted(env, [False] * 1024 + [True], rng)], 1)
    assert used[0] == 1025 and bt.pools()[3][0] == 4               # collided: 0 kept in round 0, then up to len(free) = 4
    # a third round does not fit cap = 2: status 2, untouched
    before = bt.pools()
    _, _, status = bt.launch([_crafted(env, [True], rng)], 1)
    assert status[0] == 2 and all(np.array_equal(x, y) for x, y in zip(before, bt.pools()))


@pytest.mark.parametrize('dim', [2, 3])
def test_draws_beyond_the_cached_ballots(dim):
    """The kernel keeps the free flags of its first 32 x 1024 draws in LDS between its two passes and classifies the later
    ones a second time.  n = 33 000 with the n-th free draw at index 35 333 (step 34, mid-step): free and rejected draws of
    steps 32 .. 34 are both stored (round 0 keeps up to n rejected draws, here all 2 334), beside a problem that ends
    inside the cached steps and one whose block ends in step 33, a draw early."""
    rng = np.random.default_rng(500 + dim)
    n, p = 33000, 34 * 1024 + 517
    envs = [_env(dim, 15, rng) for _ in range(3)]
    long_ = _crafted(envs[0], _pattern(n, p, 20, rng), rng)
    short = _crafted(envs[1], _pattern(n, n + 50, 3, rng), rng)
    early = _crafted(envs[2], _pattern(n, 33 * 1024 + 5, 0, rng), rng)[:-1]
    bt = _Batch(envs, cap=n)
    used, checks, status = bt.check_round([long_, short, early], n)
    assert used.tolist() == [p + 1, n + 51, 0] and status.tolist() == [0, 0, 1]
    assert bt.pools()[3].tolist() == [p + 1 - n, 51, 0]
    # the long problem again, now as a later round (collided rows appended behind the first round's, cut at len(free))
    bt2 = _Batch(envs[:1], cap=2 * n)
    bt2.check_round([_crafted(envs[0], _pattern(n, n + 9, 0, rng), rng)], n)
    bt2.check_round([long_], n)
    assert bt2.pools()[3][0] == 10 + p + 1 - n


def _rounds_blocks(env, n, rejected, rng):
    """A block whose first n free draws have ``rejected`` rejected draws in front of the n-th one."""
    pat = np.zeros(n + rejected, dtype=bool)
    pat[-1] = True
    pat[rng.choice(n + rejected - 1, n - 1, replace=False)] = True
    return _crafted(env, np.concatenate((pat, rng.random(9) < 0.5)), rng)


@pytest.mark.parametrize('dim', [2, 3])
def test_three_rounds_and_gather(dim):
    """n = 8, three launches on the same pools; the cap on the collided rows binds differently in each: round 1 has more than n
    rejected draws (cut to n), round 2 fewer than it takes to reach 2n + 2, round 3 crosses 3n + 2 in the middle of a step.
    Then the gather of a mix of active and inactive problems."""
    rng = np.random.default_rng(31 + dim)
    n = 8
    rejected = [(12, 3, 30), (9, 0, 16), (40, 9, 1500), (3, 20, 2), (0, 0, 0)]      # per problem: rounds 1 / 2 / 3
    envs = [_env(dim, 15, rng) for _ in rejected]
    bt = _Batch(envs, cap=24)
    for r in range(3):
        bt.check_round([_rounds_blocks(env, n, rej[r], rng) for env, rej in zip(envs, rejected)], n)
    fp, cp, nf, nc = bt.pools()
    assert nf.tolist() == [26] * 5
    assert nc.tolist() == [26, 24, 26, 20, 0]                       # problem 0: 8 -> 11 -> 26 (cut); problem 3: 3 -> 18 (cut) -> 20
    for active in (None, [1, 0, 1, 1, 0], [0, 0, 0, 0, 1], [0, 1, 0, 0, 0]):
        sel = [b for b in range(len(envs)) if active is None or active[b]]
        rows = sum(int(nf[b] + nc[b]) for b in sel)
        act = None if active is None else torch.from_numpy(np.asarray(active, dtype=np.uint8)).to(DEV)
        g = planner.maze_rounds_gather(bt.store, len(sel), rows, active=act, trees=False)
        torch.cuda.synchronize()
        want = np.concatenate([np.concatenate((bt.free[b], bt.coll[b])) for b in sel])
        assert np.array_equal(g['v'].cpu().numpy(), want)
        assert g['node_ptr'].cpu().tolist() == np.concatenate(([0], np.cumsum([nf[b] + nc[b] for b in sel]))).tolist()
        assert g['n_free'].cpu().tolist() == [int(nf[b]) for b in sel]
        assert g['slot_of'].cpu().tolist() == sel
