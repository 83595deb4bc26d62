"""Search trees carried from round to round on the device (gnnmp_maze_rounds_gather + gnnmp_maze_explore_ex +
gnnmp_maze_rounds_carry) against the existing route, ``planner.maze_explore_device(resume=[dicts])``, which rebuilds the trees on
the host between rounds.  Small graphs, seeded random scores (frontiers die often), three rounds; after every round both
routes must agree for every problem on the explored list, the parents, the full pair list, success, path and checks."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import planner
from gnnmp.graph_build import build_edges_gpu, k1_of
from gnnmp.maze2d import Maze2D, Maze3D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, K, ROUNDS, W = 10, 4, 3, 15
GUARD = 64


def _free_state(grid, dim, rng):
    lim = np.array([1.0, 1.0, 0.4])[:dim]
    cls = Maze3D if dim == 3 else Maze2D
    while True:
        s = rng.uniform(-lim, lim, dim)
        e = cls(grid[None], s[None], s[None])
        e.init_new_problem(0)
        if e._state_fp(s):
            return s


def _problems(dim, rng):
    """0: start inside an obstacle (its tree stays node 0); 1: goal 0.02 from the start (solved in round 1 by a boosted score),
    between 0 and 2, which continue (2's goal lies inside an obstacle block); 3: random."""
    cls = Maze3D if dim == 3 else Maze2D
    envs = []
    for b in range(4):
        grid = (rng.random((W, W)) < (0.08 if dim == 3 else 0.3)).astype(np.float64)
        init, goal = _free_state(grid, dim, rng), _free_state(grid, dim, rng)
        if b == 0:
            grid[:] = 0.0
            grid[7, 7] = 1.0
            init = np.array([0.0, 0.0, 0.1][:dim])                # cell (7, 7)
        if b == 1:
            grid[:] = 0.0
            goal = init.copy()
            goal[0] += 0.02 if init[0] < 0.5 else -0.02
        if b == 2:                                                # goal in the middle of a 3 x 3 block: never reached
            grid[3:6, 3:6] = 1.0
            init = _free_state(grid, dim, rng)
            goal = np.array([-0.4, -0.4, 0.0][:dim])              # centre of cell (4, 4), 0.2 from the nearest free point
        e = cls(grid[None], init[None], goal[None])
        e.init_new_problem(0)
        envs.append(e)
    return envs


def _run_rounds(dim, pair_cap=None, seed=0, guard=None):
    rng = np.random.default_rng(seed)
    envs = _problems(dim, rng)
    B, cap = len(envs), N * ROUNDS
    store = planner.MazeRoundsStore(B, cap, pair_cap or planner.rounds_pair_cap(N, cap, K), dim, DEV)
    if guard is not None:                                         # the pair lists inside a caller's buffer with guard words around
        inner = guard[GUARD:-GUARD].view(B, store.pair_cap, 2)
        inner.copy_(store.tree_pairs)
        store.tree_pairs = inner
        store.rebind()
    as64 = lambda rows: torch.from_numpy(np.ascontiguousarray(np.asarray(rows, dtype=np.float64))).to(DEV)      # noqa: E731
    maps = as64([e.map for e in envs])
    init64, goal64 = as64([e.init_state for e in envs]), as64([e.goal_state for e in envs])
    lim = np.asarray(envs[0].SAMPLE_LIMITS)
    host = [{'explored': [0], 'prev': {0: 0}, 'pairs': [[0, 0]], 'checks': 0, 'success': False, 'path': []} for _ in envs]
    act = list(range(B))
    gen = torch.Generator().manual_seed(seed)
    for r in range(ROUNDS):
        blocks = [rng.uniform(-lim, lim, (600 if b in act else 0, dim)) for b in range(B)]
        ptr = np.concatenate(([0], np.cumsum([x.shape[0] for x in blocks]))).astype(np.int64)
        mask = np.zeros(B, dtype=np.uint8)
        mask[act] = 1
        mask_d = torch.from_numpy(mask).to(DEV)
        _, _, status = planner.maze_sample_streams(store, torch.from_numpy(np.concatenate(blocks)).to(DEV), ptr, maps, init64,
                                                   goal64, N, active=mask_d)
        assert not status.cpu().numpy()[act].any()
        nf = 2 + (r + 1) * N
        ncoll = store.n_coll.cpu().numpy()
        g = planner.maze_rounds_gather(store, len(act), sum(nf + int(ncoll[b]) for b in act), active=mask_d)
        assert g['slot_of'].cpu().tolist() == act
        ei, edge_ptr = build_edges_gpu(g['v'], g['node_ptr'], g['n_free'], [k1_of(K, nf)] * len(act))
        scores = torch.rand(ei.shape[1], generator=gen)
        if 1 in act:                                              # problem 1: the cell (0, 1) = edge 1 -> 0 wins at once
            e0, e1 = edge_ptr.cpu().tolist()[act.index(1):act.index(1) + 2]
            sub = ei[:, e0:e1].cpu()
            hit = ((sub[0] == 1) & (sub[1] == 0)).nonzero().reshape(-1)
            assert hit.numel() == 1
            scores[e0 + int(hit)] = 10.0
        scores = scores.to(DEV)
        act_d = torch.tensor(act, device=DEV)
        maps_r, goal_r = maps[act_d].contiguous(), goal64[act_d].contiguous()
        # route 1: the trees through Python
        success, n_expl, n_pairs, plen, checks, expl, ee, ee_off, path, prev = planner.maze_explore_device(
            g['v'], g['node_ptr'], edge_ptr, [nf] * len(act), ei, scores, maps_r, goal_r,
            resume=[{'explored': host[b]['explored'], 'prev': host[b]['prev'], 'pairs': host[b]['pairs']} for b in act], want_prev=True)
        nptr = g['node_ptr'].cpu().tolist()
        for j, b in enumerate(act):
            h = host[b]
            h['explored'] = expl[nptr[j]:nptr[j] + n_expl[j]].tolist()
            h['pairs'] = h['pairs'] + ee[ee_off[j]:ee_off[j + 1]].reshape(-1, 2).tolist()
            h['prev'] = {a: int(prev[nptr[j] + a]) for a in h['explored']}
            h['checks'] += int(checks[j])
            h['success'] = bool(success[j])
            h['path'] = path[nptr[j]:nptr[j] + plen[j]].tolist()
        # route 2: the device carry
        cstat = planner.maze_rounds_explore(store, g, ei, edge_ptr, scores, maps_r, goal_r).cpu().tolist()
        yield r, act, host, store, cstat
        act = [b for b in act if not host[b]['success']]
        if not act:
            break


def _assert_same(host, store, problems):
    s = store
    ne, npairs, ok, plen = (t.cpu().tolist() for t in (s.tree_n_explored, s.tree_n_pairs, s.tree_success, s.tree_path_len))
    expl, prev, path, pairs, chk = (t.cpu().numpy() for t in (s.tree_explored, s.tree_prev, s.tree_path, s.tree_pairs, s.tree_checks))
    for b in problems:
        h = host[b]
        assert expl[b, :ne[b]].tolist() == h['explored'], b
        assert {a: int(prev[b, a]) for a in h['explored']} == h['prev'], b
        assert pairs[b, :npairs[b]].tolist() == h['pairs'], b
        assert bool(ok[b]) == h['success'] and int(chk[b]) == h['checks'], b
        assert path[b, :plen[b]].tolist() == h['path'], b


@pytest.mark.parametrize('dim', [2, 3])
def test_device_carry_equals_host_resume(dim):
    rounds_of = {}
    for r, act, host, store, cstat in _run_rounds(dim, seed=11 + dim):
        assert not any(cstat)
        _assert_same(host, store, range(len(host)))               # the finished ones keep what they had
        for b in act:
            rounds_of[b] = r + 1
        if r == 0:
            assert host[1]['success'] and host[1]['path'] == [0, 1]        # solved between two that continue
            assert not host[0]['success'] and not host[2]['success']
    assert rounds_of[1] == 1 and rounds_of[0] == ROUNDS and rounds_of[2] > 1
    assert host[0]['explored'] == [0]                             # the start sits in an obstacle: the tree is node 0
    assert len(host[0]['pairs']) > 1                              # ... though it kept trying edges
    assert max(len(h['explored']) for h in host) > 3


def test_pair_list_overflow_is_reported_and_contained():
    """A pair list too small on purpose: the problems whose new pairs do not fit get status bit 0, nothing of theirs is appended,
    and no slot sees a write outside its own room (the slots either side are the guard words)."""
    cap_pairs = 4
    guard = torch.full((2 * GUARD + 4 * cap_pairs * 2,), -99, dtype=torch.int32, device=DEV)
    gen = _run_rounds(2, pair_cap=cap_pairs, seed=13, guard=guard)
    r, act, host, store2, cstat = next(gen)
    gen.close()
    torch.cuda.synchronize()
    assert (guard[:GUARD] == -99).all() and (guard[-GUARD:] == -99).all()
    npairs = store2.tree_n_pairs.cpu().tolist()
    pairs = store2.tree_pairs.cpu().numpy()
    over = [len(h['pairs']) > cap_pairs for h in host]
    assert any(over) and not all(over)                            # problem 1 records [0, 0], [0, 1], [1, 0]: it fits
    for b in range(len(host)):
        assert cstat[b] == (1 if over[b] else 0), b
        if over[b]:
            assert npairs[b] == 1 and pairs[b, 0].tolist() == [0, 0] and not pairs[b, 1:].any(), b
        else:
            assert pairs[b, :npairs[b]].tolist() == host[b]['pairs'] and not pairs[b, npairs[b]:].any(), b
