"""Device-side training supervision (gnnmp.episodes, csrc/train_episode_kernels.hip) against the reference's own results
(the episodes_* fixtures) and against the plain-Python restatement (tests/episodes_host.py) on random batches, plus the
loss and its gradients against the reference's loss expression on a dense policy."""
import os

import numpy as np
import pytest
import torch

import gnnmp
from gnnmp import episodes as ep
from conftest import golden_files, load_weights
import episodes_host as H

DEV = 'cuda:0'
FILES = golden_files('episodes_')
pytestmark = pytest.mark.gpu


def load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def graphs_of(cases):
    """TrainingGraphs over the given fixture dicts (their own edges), labelled by the device."""
    ei = torch.cat([torch.from_numpy(c['edge_index'].astype(np.int64)) for c in cases], dim=1).to(DEV)
    nptr = np.concatenate([[0], np.cumsum([c['points'].shape[0] for c in cases])]).tolist()
    eptr = np.concatenate([[0], np.cumsum([c['edge_index'].shape[1] for c in cases])]).tolist()
    E = eptr[-1]
    obs = [ep.maze_obstacles(c['map']) for c in cases]
    pts = torch.cat([torch.from_numpy(c['points']) for c in cases]).to(DEV)
    g = ep.TrainingGraphs(pts.float(), ei, nptr, eptr, torch.empty(E, dtype=torch.uint8, device=DEV),
                          torch.empty(E, dtype=torch.float64, device=DEV), torch.from_numpy(np.concatenate(obs)).to(DEV),
                          np.concatenate([[0], np.cumsum([len(o) for o in obs])]).tolist())
    ep.label_maze(g, pts, torch.from_numpy(np.stack([c['map'] for c in cases])), int(cases[0]['points'].shape[1]))
    return g


def run_pipeline(g, scores, goal, start, max_steps, replay_step=None):
    paths = ep.shortest_paths(g, goal)
    step, status = ep.explore_steps(g, scores, start, paths['goal'], paths['n_valid'], max_steps)
    s = step if replay_step is None else torch.minimum(torch.as_tensor(replay_step, dtype=torch.int32, device=DEV), step)
    s = torch.where(status == 0, s, step)
    fr = ep.policy_frontier(g, scores, paths, start, paths['goal'], s, status)
    torch.cuda.synchronize()
    return paths, step, status, fr


@pytest.mark.parametrize('dim', [2, 3])
def test_fixtures_exact(dim):
    cases = [load(f) for f in FILES]
    cases = [c for c in cases if int(c['dim']) == dim]
    assert cases
    for max_steps in sorted({int(c['max_steps']) for c in cases}):
        cs = [c for c in cases if int(c['max_steps']) == max_steps]
        g = graphs_of(cs)
        scores = torch.from_numpy(np.concatenate([c['scores'] for c in cs])).to(DEV)
        goal = [int(c['goal']) for c in cs]
        start = [int(c['start']) for c in cs]
        paths, step, status, fr = run_pipeline(g, scores, goal, start, max_steps, [max(int(c['replay_step']), 0) for c in cs])
        free, cost = g.edge_free.cpu().numpy(), g.edge_cost.cpu().numpy()
        dist, prev = paths['dist'].cpu().numpy(), paths['prev'].cpu().numpy()
        for b, c in enumerate(cs):
            e0, e1 = g.edge_ptr_host[b], g.edge_ptr_host[b + 1]
            n0, n1 = g.node_ptr_host[b], g.node_ptr_host[b + 1]
            assert np.array_equal(free[e0:e1], c['edge_free']), b
            assert np.array_equal(cost[e0:e1], c['edge_cost']), b
            assert np.array_equal(dist[n0:n1], c['dist']) and np.array_equal(prev[n0:n1], c['prev']), b
            assert int(paths['n_valid'][b]) == int(c['n_valid'])
            assert int(status[b]) == int(c['status']) and int(step[b]) == int(c['step']), (b, int(status[b]), int(step[b]))
            ids, label = ep.frontier_slices(fr, b)
            assert np.array_equal(ids - e0, c['frontier'].astype(np.int64)), b
            assert label == int(c['label'])


def random_maps(n, rng, w=15):
    maps = (rng.random((n, w, w)) < 0.25).astype(np.float64)
    fixture_maps = [load(f)['map'] for f in FILES if load(f)['map'].shape[0] == w]
    for i in range(0, n, 4):                         # a quarter of them real mazes
        maps[i] = fixture_maps[i % len(fixture_maps)]
    return maps


def random_batch(dim, sizes, seed, zero_frac=0.05):
    rng = np.random.default_rng(seed)
    lim = np.array([1.0, 1.0, 0.4])[:dim]
    pts = [rng.uniform(-lim, lim, (n, dim)) for n in sizes]
    maps = random_maps(len(sizes), rng)
    nptr = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    g = ep.maze_training_graphs(torch.from_numpy(np.concatenate(pts)).to(DEV), nptr, maps, dim)
    E = g.total_edges
    sc = rng.standard_normal(E).astype(np.float32)
    sc[rng.random(E) < zero_frac] = 0.0
    return g, pts, maps, torch.from_numpy(sc).to(DEV), rng


def check_against_host(g, pts, maps, scores, goal, start, replay, max_steps=1000):
    paths, step, status, fr = run_pipeline(g, scores, goal, start, max_steps, replay)
    ei = g.edge_index.cpu().numpy()
    free, cost = g.edge_free.cpu().numpy(), g.edge_cost.cpu().numpy()
    sc = scores.cpu().numpy()
    dist, prev = paths['dist'].cpu().numpy(), paths['prev'].cpu().numpy()
    for b in range(g.n_problems):
        e0, e1 = g.edge_ptr_host[b], g.edge_ptr_host[b + 1]
        n0, n1 = g.node_ptr_host[b], g.node_ptr_host[b + 1]
        eb = ei[:, e0:e1]
        hf, hc = H.label_edges(pts[b], eb, maps[b])
        assert np.array_equal(free[e0:e1], hf) and np.array_equal(cost[e0:e1], hc), b
        out = H.episode(n1 - n0, eb, hf, hc, sc[e0:e1], goal[b], start[b], lambda s: min(replay[b], s), max_steps)
        assert np.array_equal(dist[n0:n1], out['dist']) and np.array_equal(prev[n0:n1], out['prev']), b
        assert int(paths['n_valid'][b]) == out['n_valid']
        assert int(status[b]) == out['status'] and int(step[b]) == out['step'], b
        if out['status'] == 0:
            ids, label = ep.frontier_slices(fr, b)
            _, lab_h = out['frontier'], out['label']
            assert np.array_equal(ids - e0, out['frontier']) and label == lab_h, b
    return status


def draws(g, rng, unreachable_every=8, tries=24):
    """Per problem: a goal with a large valid set (best of a few uniform draws), a start drawn from that set (as :165 does),
    every ``unreachable_every``-th problem a uniform start instead (which may be unreachable), and a replay step."""
    ei = g.edge_index.cpu().numpy()
    cost = g.edge_cost.cpu().numpy()
    goal, start = [], []
    for b, n in enumerate(g.sizes()):
        e0, e1 = g.edge_ptr_host[b], g.edge_ptr_host[b + 1]
        best = None
        for _ in range(tries):
            gg = int(rng.integers(n))
            dist, _, nv = H.shortest_paths(n, ei[:, e0:e1], cost[e0:e1], gg)
            if best is None or nv > best[1]:
                best = (gg, nv, dist)
        gg, nv, dist = best
        goal.append(gg)
        valid = np.flatnonzero(np.isfinite(dist))
        start.append(int(rng.integers(n)) if b % unreachable_every == unreachable_every - 1 else int(rng.choice(valid)))
    replay = [int(rng.integers(0, 400)) for _ in goal]
    return goal, start, replay


def test_random_maze2_batch_matches_restatement():
    rng0 = np.random.default_rng(3)
    sizes = rng0.integers(100, 401, 64).tolist()
    g, pts, maps, scores, rng = random_batch(2, sizes, 11)
    goal, start, replay = draws(g, rng)
    status = check_against_host(g, pts, maps, scores, goal, start, replay)
    assert int((status == 0).sum()) >= 40 and (status != 0).any()   # skipped problems mid-batch


def test_large_problems_beyond_lds():
    g, pts, maps, scores, rng = random_batch(2, [3000, 2100, 3000, 1500], 12)
    goal, start, replay = draws(g, rng, unreachable_every=1000, tries=6)
    status = check_against_host(g, pts, maps, scores, goal, start, replay)
    assert int((status[[0, 1, 2]] == 0).sum()) >= 2                  # frontiers and labels of > 1024-node problems compared


def test_random_maze3_batch_matches_restatement():
    rng0 = np.random.default_rng(4)
    g, pts, maps, scores, rng = random_batch(3, rng0.integers(100, 201, 16).tolist(), 13)
    goal, start, replay = draws(g, rng, unreachable_every=1000)
    status = check_against_host(g, pts, maps, scores, goal, start, replay)
    assert int((status == 0).sum()) >= 4


def _midpoints(l, r, w, level=0, half=None):
    """(level, half of the whole segment: 'L' / 'R' / None for its own midpoint, point) of every midpoint the bisection
    of l -> r visits on a map without obstacles."""
    dc = abs(H._cell(l[0], w) - H._cell(r[0], w)) + abs(H._cell(l[1], w) - H._cell(r[1], w))
    if not (dc > 1 and abs(l[0] - r[0]) + abs(l[1] - r[1]) > H.RRT_EPS):
        return []
    mid = ((l[0] + r[0]) / 2.0, (l[1] + r[1]) / 2.0)
    return ([(level, half, mid)] + _midpoints(l, mid, w, level + 1, half or 'L') + _midpoints(mid, r, w, level + 1, half or 'R'))


def test_long_maze2_edges_bisect_beyond_five_levels():
    """Edges of L1 length 3 on a 64 x 64 map split six times.  One is free; the other is blocked by a single obstacle cell
    that only midpoints of level >= 5 in its right half land in, so the walk has to get through the whole left half and
    down the right one to find it."""
    w = 64
    cell_of = lambda q: (H._cell(q[0], w), H._cell(q[1], w))
    a, b, c, d = (-0.95, -0.52), (0.93, 0.61), (-0.9, 0.7), (0.95, -0.45)
    mids = _midpoints(a, b, w)
    assert max(lv for lv, _, _ in mids) >= 5
    others = {cell_of(q) for q in (a, b, c, d)} | {cell_of(q) for _, _, q in _midpoints(c, d, w)}
    shallow = {cell_of(q) for lv, half, q in mids if lv < 5 or half != 'R'}
    cell = next(cell_of(q) for lv, half, q in mids if lv >= 5 and half == 'R' and cell_of(q) not in others | shallow)
    m = np.zeros((w, w))
    m[cell] = 1.0
    pts = np.array([a, b, c, d])
    ei = np.array([[0, 1, 2, 3], [1, 0, 3, 2]])
    hf, hc = H.label_edges(pts, ei, m)
    assert np.all(np.abs(pts[ei[0]] - pts[ei[1]]).sum(axis=1) > 2.9)
    assert hf[0] == 0 and hf[2] == 1                                 # a blocked and a free long edge
    g = graphs_of([{'points': pts, 'edge_index': ei, 'map': m}])
    assert np.array_equal(g.edge_free.cpu().numpy(), hf) and np.array_equal(g.edge_cost.cpu().numpy(), hc)


def _knn_edges(pts, k=5):
    """A symmetric k-nearest-neighbour edge set, columns sorted by (source, target) like construct_graph's."""
    dist = np.linalg.norm(pts[:, None, :] - pts[None, :, :], axis=-1)
    np.fill_diagonal(dist, np.inf)
    pairs = {(s, int(t)) for s in range(len(pts)) for t in np.argsort(dist[s])[:k]}
    return np.array(sorted(pairs | {(t, s) for s, t in pairs}), dtype=np.int64).T


@pytest.mark.parametrize('dim', [2, 3])
def test_labels_on_maps_beyond_the_lds_copy(dim):
    """Width 65 is 4225 cells, more than the 4096 bytes of the LDS copy: every query reads the map in global memory."""
    rng = np.random.default_rng(20 + dim)
    lim = np.array([1.0, 1.0, 0.4])[:dim]
    cases = []
    for _ in range(2):
        pts = rng.uniform(-lim, lim, (20, dim))
        cases.append({'points': pts, 'edge_index': _knn_edges(pts), 'map': (rng.random((65, 65)) < 0.02).astype(np.float64)})
    host = [H.label_edges(c['points'], c['edge_index'], c['map']) for c in cases]
    hf, hc = np.concatenate([h[0] for h in host]), np.concatenate([h[1] for h in host])
    assert 0 < int(hf.sum()) < len(hf)                               # free and blocked edges
    g = graphs_of(cases)
    assert np.array_equal(g.edge_free.cpu().numpy(), hf) and np.array_equal(g.edge_cost.cpu().numpy(), hc)


def test_loss_stays_finite_with_large_logits():
    """Masked slots of the ragged gather hold scores[0]; a logit far above the frontier's maximum must not reach exp()."""
    rng0 = np.random.default_rng(8)
    g, pts, maps, scores, rng = random_batch(2, rng0.integers(100, 201, 6).tolist(), 16)
    goal, start, replay = draws(g, rng, unreachable_every=1000)
    paths, step, status, fr = run_pipeline(g, scores, goal, start, 1000, replay)
    sc = scores.clone()
    sc[0] = 1000.0
    sc.requires_grad_(True)
    losses, ok = ep.frontier_loss(sc, fr)
    losses.sum().backward()
    assert bool(ok.any()) and bool(torch.isfinite(losses).all()) and bool(torch.isfinite(sc.grad).all())


def explorer_model():
    m = gnnmp.EncoderProcessDecoder(2, 2, 32, 2)
    m.load_state_dict(load_weights('weights_maze'))
    return m.to(DEV).train()


def test_loss_and_gradients_match_reference_expression():
    rng0 = np.random.default_rng(5)
    g, pts, maps, _, rng = random_batch(2, rng0.integers(100, 301, 12).tolist(), 14)
    m = explorer_model()
    goal = torch.tensor([int(rng.integers(n)) for n in g.sizes()], dtype=torch.int32, device=DEV)
    paths = ep.shortest_paths(g, goal)
    start = ep.draw_start(g, paths, torch.Generator(device=DEV).manual_seed(1))
    scores = m.train_scores(g.batch(paths['goal']), 3)
    step, status = ep.explore_steps(g, scores, start, paths['goal'], paths['n_valid'])
    s = ep.draw_step(step, torch.Generator(device=DEV).manual_seed(2))
    fr = ep.policy_frontier(g, scores, paths, start, paths['goal'], s, status)
    losses, ok = ep.frontier_loss(scores, fr)
    params = [p for p in m.parameters()]
    grads = torch.autograd.grad(losses.sum(), params, allow_unused=True, retain_graph=True)
    # the reference's expression on the dense policy of each problem, with the frontier of the host restatement
    ei = g.edge_index
    ref = []
    for b in range(g.n_problems):
        if not bool(ok[b]):
            ref.append(torch.zeros((), device=DEV))
            continue
        e0, e1 = g.edge_ptr_host[b], g.edge_ptr_host[b + 1]
        N = g.sizes()[b]
        P = scores.new_zeros(N, N).index_put((ei[1, e0:e1], ei[0, e0:e1]), scores[e0:e1])
        hf, hc = g.edge_free[e0:e1].cpu().numpy(), g.edge_cost[e0:e1].cpu().numpy()
        eb = ei[:, e0:e1].cpu().numpy()
        out = H.episode(N, eb, hf, hc, scores[e0:e1].detach().cpu().numpy(), int(paths['goal'][b]), int(start[b]),
                        lambda st: int(s[b]))
        rows, cols = torch.from_numpy(eb[1][out['frontier']]).to(DEV), torch.from_numpy(eb[0][out['frontier']]).to(DEV)
        ref.append(-P[rows, cols].log_softmax(dim=0)[out['label']])
    ref = torch.stack(ref)
    assert int(ok.sum()) > 0
    # 1e-6 relative, with 1 as the floor of the scale: a loss near 0 is log(sum) - (s - max) with sum = 1 + tiny, where
    # float32 resolves 6e-8 whatever the order of the sum
    assert bool(((losses - ref).abs() <= 1e-6 * ref.abs().clamp(min=1.0)).all()), (losses - ref).abs().max()
    rgrads = torch.autograd.grad(ref.sum(), params, allow_unused=True)
    gmax = max(float(x.abs().max()) for x in grads if x is not None)
    for (name, _), a, r in zip(m.named_parameters(), grads, rgrads):
        if name.startswith(('node_attentions', 'edge_attentions', 'obs_node_code', 'obs_edge_code')):
            assert a is None or float(a.abs().max()) == 0.0, name
            continue
        if a is None and r is None:
            continue
        a = torch.zeros_like(r) if a is None else a
        r = torch.zeros_like(a) if r is None else r
        assert float((a - r).abs().max()) <= 1e-5 * gmax + 1e-7, name


def test_training_step_deterministic():
    rng0 = np.random.default_rng(6)
    g, _, _, _, _ = random_batch(2, rng0.integers(100, 401, 16).tolist(), 15)
    m = explorer_model()
    outs = []
    for _ in range(2):
        loss, info = ep.training_step(m, g, loop=10, generator=torch.Generator(device=DEV).manual_seed(9),
                                      cpu_generator=torch.Generator().manual_seed(9))
        gr = torch.autograd.grad(loss, [p for p in m.parameters() if p.requires_grad], allow_unused=True)
        torch.cuda.synchronize()
        frs = [ep.frontier_slices(info['frontier'], i) for i in range(g.n_problems)]
        outs.append((float(loss), frs, info['status'].clone(), info['step'].clone(), [x.clone() for x in gr if x is not None]))
    a, b = outs
    assert a[0] == b[0] and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    for (fa, la), (fb, lb) in zip(a[1], b[1]):
        assert np.array_equal(fa, fb) and la == lb
    for x, y in zip(a[4], b[4]):
        assert torch.equal(x, y)
    assert np.isfinite(a[0])
