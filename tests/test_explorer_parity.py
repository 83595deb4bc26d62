"""GPU parity of the HIP explorer forward (through the C ABI) against
 (a) the golden vectors recorded from the unmodified reference, fp32 and fp64, and
 (b) the CPU oracle on seeded inputs, including the edge cases the domain has.

Tolerance (north_star: "within 1e-5 fp32"; SURVEY.md finding 0.7): the per-fixture bar of tests/parity_bar.py --
    atol = max(1e-5, 1.25 * own),  own = max|ref_fp32 - ref_fp64| of the reference itself on that fixture,
    |gpu - ref_fp64| <= atol   and   |gpu - ref_fp32| <= atol + own   elementwise, no relative term.
profiles/r02_parity.txt lists every fixture's three maxima and which ones meet the bare 1e-5."""
import os

import numpy as np
import pytest
import torch

from conftest import env_of, golden_files, load_weights
import gnnmp
import knn_host as K
from gnnmp.synth import ENVS, synth_graph
from oracle import ref_cpu
from parity_bar import assert_fp32_parity, explorer_oracle_pair

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def make_model(env, use_obstacles=True):
    e = ENVS[env]
    m = gnnmp.EncoderProcessDecoder(e['workspace'], e['C'], e['d'], e['S'], use_obstacles=use_obstacles).eval()
    m.load_state_dict(load_weights(e['ckpt']), strict=True)
    return m


def to_dev(g):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in g.items()}


def _load(path):
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize('path', golden_files('explorer_'), ids=os.path.basename)
def test_golden_scores(path):
    r = _load(path)
    env = env_of(path)
    m = make_model(env, bool(r['use_obstacles']))
    s = m.edge_scores(goal=torch.from_numpy(r['goal']).to(DEV), loop=int(r['loop']),
                      v=torch.from_numpy(r['v']).to(DEV), obstacles=torch.from_numpy(r['obstacles']).to(DEV),
                      edge_index=torch.from_numpy(r['edge_index']).to(DEV)).cpu()
    ref32 = torch.from_numpy(r['scores_fp32'])
    ref64 = torch.from_numpy(r['scores_fp64'])
    err32 = (s - ref32).abs().max().item()
    err64 = (s.double() - ref64).abs().max().item()
    own = (ref32.double() - ref64).abs().max().item()
    print('\n%s: max|gpu-ref32|=%.2e  max|gpu-ref64|=%.2e  (reference fp32-vs-fp64: %.2e)' %
          (os.path.basename(path), err32, err64, own))
    assert_fp32_parity(s, ref32, ref64, os.path.basename(path))
    # the planner consumes orderings: per-target argmax over incoming edges must agree wherever the
    # reference's top-2 margin is above the noise floor
    ei = torch.from_numpy(r['edge_index'])
    for t in ei[1].unique().tolist()[:64]:
        sel = (ei[1] == t).nonzero().squeeze(1)
        if sel.numel() < 2:
            continue
        top = ref64[sel].topk(2).values
        if (top[0] - top[1]) > 1e-3:
            assert int(s[sel].argmax()) == int(ref64[sel].argmax())


@pytest.mark.parametrize('path', [p for p in golden_files('explorer_') if 'N64_k4_L5.' in p or 'N200' in p],
                         ids=os.path.basename)
def test_golden_taps(path):
    r = _load(path)
    if 'tap_h' not in r:
        pytest.skip('fixture without taps')
    env = env_of(path)
    m = make_model(env, bool(r['use_obstacles']))
    g = dict(goal=torch.from_numpy(r['goal']).to(DEV), v=torch.from_numpy(r['v']).to(DEV),
             obstacles=torch.from_numpy(r['obstacles']).to(DEV), edge_index=torch.from_numpy(r['edge_index']).to(DEV))
    b = m._single(g['goal'], g['v'], g['obstacles'], g['edge_index'])
    L = int(r['loop'])
    m.forward_batch(b, L)
    h = m.debug_tap(b, 1).cpu()
    dec = m.debug_tap(b, 2).cpu()
    gi = int(m.debug_tap(b, 3).cpu()[0])
    w = load_weights(ENVS[env]['ckpt'])
    taps, taps64 = {}, {}
    args = (torch.from_numpy(r['v']), torch.from_numpy(r['goal']), torch.from_numpy(r['obstacles']))
    ref_cpu.explorer_forward(w, *args, torch.from_numpy(r['edge_index']), L, taps=taps)
    w64 = {k: (t.double() if t.is_floating_point() else t) for k, t in w.items()}
    ref_cpu.explorer_forward(w64, *[a.double() for a in args], torch.from_numpy(r['edge_index']), L, taps=taps64)
    assert gi == int(taps['goal_index'][0])
    # intermediates on the scores' bar (absolute, no relative term): the recorded reference hook (fp32) and the oracle's fp64
    # run of it.  Hidden rows reach |h| ~ 50 where the scores stay within [-32, 12], so the margin over the reference's own
    # fp32 error is 1.5 instead of 1.25 (measured worst case: 1.30 on snake7 h_3)
    TAPF = 1.5
    assert_fp32_parity(h.reshape(-1), torch.from_numpy(r['tap_h'][L - 1]).reshape(-1), taps64['h'][L - 1].reshape(-1), 'h_L', TAPF)
    assert_fp32_parity(dec.reshape(-1), torch.from_numpy(r['tap_decode']).reshape(-1), taps64['decode'].reshape(-1), 'decode', TAPF)
    # every intermediate h_i via shorter loops
    for li in range(1, L):
        m.forward_batch(b, li)
        hi = m.debug_tap(b, 1).cpu()
        assert_fp32_parity(hi.reshape(-1), torch.from_numpy(r['tap_h'][li - 1]).reshape(-1), taps64['h'][li - 1].reshape(-1), 'h_%d' % li, TAPF)


@pytest.mark.parametrize('path', golden_files('explorer_'), ids=os.path.basename)
def test_golden_bare_1e5(path):
    """north_star's bare figure: |gpu - ref_fp32| <= 1e-5 on every golden on which the reference's own fp32 run is within 1e-5
    of its fp64 run (elsewhere it is not a meaningful target: tests/parity_bar.py), and |gpu - ref_fp64| <= 1e-5 everywhere."""
    r = _load(path)
    env = env_of(path)
    m = make_model(env, bool(r['use_obstacles']))
    s = m.edge_scores(torch.from_numpy(r['goal']).to(DEV), int(r['loop']), torch.from_numpy(r['v']).to(DEV),
                      torch.from_numpy(r['obstacles']).to(DEV), torch.from_numpy(r['edge_index']).to(DEV)).cpu().double()
    ref32, ref64 = torch.from_numpy(r['scores_fp32']).double(), torch.from_numpy(r['scores_fp64'])
    own = float((ref32 - ref64).abs().max())
    assert float((s - ref64).abs().max()) <= 1e-5, (own, float((s - ref64).abs().max()))
    if own <= 1e-5:
        assert float((s - ref32).abs().max()) <= 1e-5, (own, float((s - ref32).abs().max()))


def test_pybullet_obstacle_layout():
    """The PyBullet environments hand obstacles over as [O, 2, 3] (half extents, centre: environment/kuka_env.py:98) and the
    reference views them as [-1, S] (model.py:126); the module call and the sparse entry point must accept that tensor as is."""
    r = _load([p for p in golden_files('explorer_') if 'kuka7_N64_k4_L5.' in p][0])
    m = make_model('kuka7')
    obs6 = torch.from_numpy(r['obstacles']).reshape(-1, 6)
    obs3 = obs6.reshape(-1, 2, 3).to(DEV)
    kw = dict(goal=torch.from_numpy(r['goal']).to(DEV), loop=int(r['loop']), v=torch.from_numpy(r['v']).to(DEV),
              edge_index=torch.from_numpy(r['edge_index']).to(DEV))
    s3 = m.edge_scores(obstacles=obs3, **kw)
    s6 = m.edge_scores(obstacles=obs6.to(DEV), **kw)
    assert torch.equal(s3, s6)
    assert_fp32_parity(s3.cpu(), torch.from_numpy(r['scores_fp32']), torch.from_numpy(r['scores_fp64']), '[O,2,3] obstacles')
    P = m(obstacles=obs3, free=kw['v'][:30], collided=kw['v'][30:], **kw)
    ei = kw['edge_index']
    assert torch.equal(P[ei[1], ei[0]], s3)


def test_dense_is_reference_layout():
    g = synth_graph('maze2', 100, 5, seed=5)
    m = make_model('maze2')
    d = to_dev(g)
    P = m(goal=d['goal'], loop=3, v=d['v'], obstacles=d['obstacles'], free=d['v'][:50], collided=d['v'][50:],
          edge_index=d['edge_index'], labels=torch.zeros(100, 3), k=10)
    s = m.edge_scores(d['goal'], 3, d['v'], d['obstacles'], d['edge_index'])
    assert P.shape == (100, 100) and P.device.type == 'cuda'
    ei = d['edge_index']
    assert torch.equal(P[ei[1], ei[0]], s)                      # P[target, source]
    mask = torch.ones_like(P, dtype=torch.bool)
    mask[ei[1], ei[0]] = False
    assert float(P[mask].abs().max()) == 0.0                    # zero-filled elsewhere (model.py:148)
    ref32, ref64 = explorer_oracle_pair(load_weights('weights_maze'), g, 3, dense=True)
    assert_fp32_parity(P.cpu().reshape(-1), ref32.reshape(-1), ref64.reshape(-1), 'dense')


@pytest.mark.parametrize('env,n,k', [('maze2', 300, 6), ('kuka7', 150, 5), ('ur5', 97, 4), ('kuka14', 130, 9)])
def test_oracle_seeded(env, n, k):
    g = synth_graph(env, n, k, seed=321)
    m = make_model(env)
    d = to_dev(g)
    s = m.edge_scores(d['goal'], 5, d['v'], d['obstacles'], d['edge_index']).cpu()
    ref32, ref64 = explorer_oracle_pair(load_weights(ENVS[env]['ckpt']), g, 5)
    assert_fp32_parity(s, ref32, ref64, env)


def test_batch_equals_per_graph_bitwise():
    m = make_model('maze2')
    graphs = [synth_graph('maze2', n, k, seed=100 + i, n_obs=o)
              for i, (n, k, o) in enumerate([(64, 4, 116), (200, 6, 57), (33, 3, 128), (257, 5, 1), (120, 7, 90)])]
    b = gnnmp.GraphBatch.from_graphs(graphs, 2, DEV)
    sb = m.forward_batch(b, 4)
    parts = b.split_edges(sb)
    for g, p in zip(graphs, parts):
        d = to_dev(g)
        s1 = m.edge_scores(d['goal'], 4, d['v'], d['obstacles'], d['edge_index'])
        assert torch.equal(s1, p)          # problems are independent: batching must not change a bit
        ref32, ref64 = explorer_oracle_pair(load_weights('weights_maze'), g, 4)
        assert_fp32_parity(p.cpu(), ref32, ref64, 'batched graph')


def test_edge_order_and_duplicates():
    """Per-edge scores do not depend on the column order; duplicated columns score identically."""
    g = synth_graph('maze2', 120, 5, seed=8)
    m = make_model('maze2')
    d = to_dev(g)
    s = m.edge_scores(d['goal'], 5, d['v'], d['obstacles'], d['edge_index'])
    gen = torch.Generator().manual_seed(0)
    perm = torch.randperm(g['edge_index'].shape[1], generator=gen).to(DEV)
    sp = m.edge_scores(d['goal'], 5, d['v'], d['obstacles'], d['edge_index'][:, perm])
    assert torch.equal(sp, s[perm])


@pytest.mark.parametrize('case', ['isolated', 'single_edge', 'no_self_loops', 'asymmetric'])
def test_degenerate_graphs(case):
    gen = torch.Generator().manual_seed(3)
    v = (torch.rand(40, 2, generator=gen) * 2 - 1)
    obstacles = torch.rand(7, 2, generator=gen) - 0.5
    full = ref_cpu.build_edges(v, 20, 4)
    if case == 'isolated':          # nodes 5 and 17 receive nothing: max-aggregation must give 0 there
        ei = full[:, (full[1] != 5) & (full[1] != 17)]
    elif case == 'single_edge':
        ei = torch.tensor([[3], [9]])
    elif case == 'no_self_loops':
        ei = full[:, full[0] != full[1]]
    else:
        ei = full[:, full[0] < full[1]]
    w = load_weights('weights_maze')
    m = make_model('maze2')
    s = m.edge_scores(v[1].to(DEV), 5, v.to(DEV), obstacles.to(DEV), ei.to(DEV)).cpu()
    ref32, ref64 = explorer_oracle_pair(w, dict(v=v, goal=v[1].clone(), obstacles=obstacles, edge_index=ei), 5)
    assert_fp32_parity(s, ref32, ref64, 'structure case')


@pytest.mark.parametrize('n_obs', [0, 1, 31, 32, 33, 128, 129, 300])
def test_obstacle_counts(n_obs):
    """Ragged obstacle sets: empty, tile edges (32/33), the maze maximum and beyond the LDS-resident
    chunk (online-softmax over several K/V chunks)."""
    gen = torch.Generator().manual_seed(n_obs)
    v = torch.rand(70, 2, generator=gen) * 2 - 1
    obstacles = torch.rand(n_obs, 2, generator=gen) - 0.5
    ei = ref_cpu.build_edges(v, 35, 4)
    w = load_weights('weights_maze')
    m = make_model('maze2')
    s = m.edge_scores(v[1].to(DEV), 5, v.to(DEV), obstacles.to(DEV), ei.to(DEV)).cpu()
    ref32, ref64 = explorer_oracle_pair(w, dict(v=v, goal=v[1].clone(), obstacles=obstacles, edge_index=ei), 5)
    assert_fp32_parity(s, ref32, ref64, 'structure case')


def test_use_obstacles_toggle_and_loop_validation():
    g = synth_graph('maze2', 80, 4, seed=2)
    d = to_dev(g)
    m = make_model('maze2')
    s_on = m.edge_scores(d['goal'], 2, d['v'], d['obstacles'], d['edge_index']).cpu()
    m.use_obstacles = False                      # eval_gnn.py:88 flips the attribute on a live model
    s_off = m.edge_scores(d['goal'], 2, d['v'], d['obstacles'], d['edge_index']).cpu()
    w = load_weights('weights_maze')
    for s, flag in ((s_on, True), (s_off, False)):
        ref32, ref64 = explorer_oracle_pair(w, g, 2, use_obstacles=flag)
        assert_fp32_parity(s, ref32, ref64, 'use_obstacles=%s' % flag)
    with pytest.raises(ValueError):
        m.edge_scores(d['goal'], 0, d['v'], d['obstacles'], d['edge_index'])
    with pytest.raises(RuntimeError):
        m.edge_scores(g['goal'], 1, g['v'], g['obstacles'], g['edge_index'])     # CPU tensors: no fallback


def test_weights_follow_in_place_updates():
    g = synth_graph('maze2', 50, 4, seed=4)
    d = to_dev(g)
    m = make_model('maze2')
    s0 = m.edge_scores(d['goal'], 1, d['v'], d['obstacles'], d['edge_index']).clone()
    with torch.no_grad():
        m.policy[4].weight.mul_(2.0)
    s1 = m.edge_scores(d['goal'], 1, d['v'], d['obstacles'], d['edge_index'])
    assert torch.allclose(s1, 2 * s0, rtol=1e-6, atol=1e-6)


def test_deepcopy_after_forward():
    """copy.deepcopy of a model that already owns a native handle: the copy builds its own handle (no shared pointer,
    no double free) and scores identically."""
    import copy
    g = to_dev(synth_graph('maze2', 80, 5, seed=3))
    m = make_model('maze2')
    a = m.edge_scores(g['goal'], 3, g['v'], g['obstacles'], g['edge_index'])
    m2 = copy.deepcopy(m)
    assert m2._handle is None
    b = m2.edge_scores(g['goal'], 3, g['v'], g['obstacles'], g['edge_index'])
    assert torch.equal(a, b)
    del m
    assert torch.equal(b, m2.edge_scores(g['goal'], 3, g['v'], g['obstacles'], g['edge_index']))


@pytest.mark.parametrize('n,k', [(64, 4), (1000, 8), (3000, 12)])
def test_single_graph_without_prefix_arrays(n, k):
    """gnnmp.h: one graph may be handed over by its totals alone (node_ptr = edge_ptr = obs_ptr = NULL, what the drop-in
    forward() does); same bits as the explicit one-graph batch (small graphs take the one-launch prep stage, the
    3000-node one the multi-pass one), and the library refuses NULL prefix arrays for more than one graph."""
    import ctypes
    from gnnmp import _lib
    m = make_model('maze2')
    d = to_dev(synth_graph('maze2', n, k, seed=n))
    explicit = m._single(d['goal'], d['v'], d['obstacles'], d['edge_index'])
    implicit = m._single(d['goal'], d['v'], d['obstacles'], d['edge_index'], prefix_arrays=False)
    assert implicit.node_ptr is None and implicit.n_graphs == 1 and implicit.dense_floats == n * n
    s_e, dn_e = m.forward_batch(explicit, 3, dense=True)
    s_i, dn_i = m.forward_batch(implicit, 3, dense=True)
    assert torch.equal(s_e, s_i) and torch.equal(dn_e, dn_i)
    assert torch.equal(m(goal=d['goal'], loop=3, v=d['v'], obstacles=d['obstacles'], edge_index=d['edge_index']),
                       dn_e.view(n, n))
    assert torch.equal(m.debug_tap(implicit, 1), m.debug_tap(explicit, 1))
    cb = m._cbatch(implicit)
    cb.n_graphs = 2
    rc = _lib.lib().gnnmp_explorer_forward(m._native(DEV), ctypes.byref(cb), 3, 1, s_i.data_ptr(), None, m._ws.data_ptr(),
                                           m._ws.numel(), None)
    assert rc == -1                                   # GNNMP_ERR_NULL


def test_optional_edge_index_range_check(monkeypatch):
    """GNNMP_CHECK_EDGE_INDEX=1 (read at import; here the module flag is flipped): ids outside [0, N_g) raise IndexError
    like the reference's tensor indexing would, instead of reading device memory out of bounds."""
    from gnnmp import explorer as E
    monkeypatch.setattr(E, '_CHECK_IDS', True)
    m = make_model('maze2')
    graphs = [synth_graph('maze2', 64, 4, seed=1), synth_graph('maze2', 40, 3, seed=2)]
    b = gnnmp.GraphBatch.from_graphs(graphs, 2, DEV)
    m.forward_batch(b, 2)                                          # valid ids pass
    bad = gnnmp.GraphBatch.from_graphs(graphs, 2, DEV)
    bad.edge_index[0, -1] = 40                                     # second graph has nodes 0..39
    with pytest.raises(IndexError):
        m.forward_batch(bad, 2)
    d = to_dev(graphs[0])
    ei = d['edge_index'].clone()
    ei[1, 0] = -1
    with pytest.raises(IndexError):
        m(goal=d['goal'], loop=2, v=d['v'], obstacles=d['obstacles'], edge_index=ei)


def test_large_graph_prep_paths():
    """A graph with more than 8192 nodes (counters of the CSR build in global memory instead of LDS) and ~100 k edges (its
    columns split over several workgroups, prep_hist / prep_scatter).  The full graph is too slow for the fp64 oracle, so
    the check is invariance, bitwise: the scores do not depend on how the build was split -- alone (12 parts) or batched
    with a small graph (6 parts) -- nor on the caller's column order (a different arrival rank for every edge).  Values
    against the oracle at a multi-part size: the full-size tests (30 k- and 80 k-edge graphs, tests/test_full_size_bf16_gpu.py)."""
    m = make_model('maze2')
    big = synth_graph('maze2', 9000, 8, seed=77)
    small = synth_graph('maze2', 64, 4, seed=78)
    d = to_dev(big)
    E = d['edge_index'].shape[1]
    assert d['v'].shape[0] > 8192 and E > 8 * 8192
    alone = m.edge_scores(d['goal'], 2, d['v'], d['obstacles'], d['edge_index'])
    assert bool(torch.isfinite(alone).all())
    b = gnnmp.GraphBatch.from_graphs([big, small], 2, DEV)
    both = b.split_edges(m.forward_batch(b, 2))
    assert torch.equal(both[0], alone)
    ds = to_dev(small)
    assert torch.equal(both[1], m.edge_scores(ds['goal'], 2, ds['v'], ds['obstacles'], ds['edge_index']))
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(5)).to(DEV)
    shuffled = m.edge_scores(d['goal'], 2, d['v'], d['obstacles'], d['edge_index'][:, perm])
    assert torch.equal(shuffled, alone[perm])


# ---------------------------------------------------------------------------------------------------------------------
# Goal node (model.py:132, knn(v, goal, 1)): the arg-min of the float32 squared distance, LOWEST index on equal distance
# (goal_body; goal_partial combined by prep_scatter_kernel for graphs from 4096 nodes in the column-split build).  The goal
# lies off every node and the nearest rows of v are exact copies of each other, so their distances are equal bit for bit;
# the node is read with debug_tap(batch, 3) and compared with tests/knn_host.argmin_stable32.
# ---------------------------------------------------------------------------------------------------------------------

def _tied_goal_graph(n, copies, seed, k1=5, n_obs=20, edges=None):
    """Random maze2 graph whose rows `copies` are one point, 1/256 from the goal and nearer to it than every other row."""
    gen = torch.Generator().manual_seed(seed)
    v = torch.rand(n, 2, generator=gen) * 2 - 1
    goal = torch.tensor([0.28125, -0.4375])
    far = (v - goal).norm(dim=1) < 0.02                        # nobody else near the goal
    v[far] = v[far] + 0.25
    v[list(copies)] = goal + torch.tensor([1.0 / 256, 0.0])
    d = (v.double() - goal.double()).pow(2).sum(1)
    assert int((d == d.min()).sum()) == len(copies) and K.argmin_stable32(v, goal) == min(copies)
    if edges is None:
        ei = K.build_edges_stable(v, n // 2, k1)
    else:
        ei = torch.randint(0, n, (2, edges), generator=gen)
    return {'v': v, 'goal': goal, 'obstacles': torch.rand(n_obs, 2, generator=gen) - 0.5, 'edge_index': ei}


def _goal_nodes(m, graphs, loop=2):
    """Scores per graph and the goal node per graph of one batched forward."""
    b = gnnmp.GraphBatch.from_graphs(graphs, 2, DEV)
    parts = b.split_edges(m.forward_batch(b, loop))
    return parts, [int(x) for x in m.debug_tap(b, 3).cpu().tolist()]


def _pin_knn(monkeypatch, highest=False):
    """The oracle's goal node pinned to the lowest (or, as the counter-check, the highest) index at the minimum float32 distance."""
    def knn(x, y, k, input_dtype=False):
        assert k == 1 and y.shape[0] == 1
        xf = x.float()
        i = x.shape[0] - 1 - K.argmin_stable32(xf.flip(0), y.float()) if highest else K.argmin_stable32(xf, y.float())
        return torch.tensor([[0], [i]])
    monkeypatch.setattr(ref_cpu, 'knn', knn)


def _check_scores_need_the_right_node(s, g, loop, monkeypatch, what):
    """Scores on the fp32 bar against the oracle with the lowest tied index; host-side condition: the oracle with the highest
    tied index is at least 100 x the case's own fp32-vs-fp64 error away, so the wrong node cannot pass."""
    w = load_weights('weights_maze')
    with monkeypatch.context() as mp:
        _pin_knn(mp)
        ref32, ref64 = explorer_oracle_pair(w, g, loop)
    with monkeypatch.context() as mp:
        _pin_knn(mp, highest=True)
        wrong32, _ = explorer_oracle_pair(w, g, loop)
    own = (ref32.double() - ref64).abs().max().item()
    moved = (wrong32 - ref32).abs().max().item()
    print('\n%s: the highest tied index moves the scores by %.2e, own fp32-vs-fp64 error %.2e' % (what, moved, own))
    assert moved >= 100 * own, (moved, own)
    assert_fp32_parity(s, ref32, ref64, what)


@pytest.mark.parametrize('n,copies', [(100, (3, 40)),                  # two lanes of one wave
                                      (300, (10, 200)),                # two waves of the workgroup
                                      (300, (7, 70, 263)),             # three copies: lanes and waves
                                      (1100, (17, 1041)),              # one thread's first and second stride trip (i, i + 1024)
                                      (2200, (1100, 2124, 76)),        # ... second and third trip, and the lowest in another thread
                                      (130, (5, 127)), (400, (390, 12)), (700, (9, 350, 697))],      # slices of the sliced CSR build
                         ids=lambda x: str(x).replace(' ', ''))
def test_goal_node_among_identical_rows_single_graph(n, copies, monkeypatch):
    g = _tied_goal_graph(n, copies, seed=n + len(copies))
    m = make_model('maze2')
    parts, nodes = _goal_nodes(m, [g])
    assert nodes == [K.argmin_stable32(g['v'], g['goal'])] == [min(copies)]
    d = to_dev(g)
    assert torch.equal(parts[0], m.edge_scores(d['goal'], 2, d['v'], d['obstacles'], d['edge_index']))
    _check_scores_need_the_right_node(parts[0].cpu(), g, 2, monkeypatch, 'copies at %s of %d' % (copies, n))


def test_goal_node_among_identical_rows_column_split_build(monkeypatch):
    """The shape of test_column_split_csr_build_ragged_batch (tests/test_explorer_fuzz_gpu.py; edge columns of a graph split
    over several workgroups, the goal arg-min on the graph's last part) with tied goals in the large graphs, and a graph of
    4200 nodes whose arg-min is split over the parts (goal_partial, from 4096 nodes) with the copies in different parts."""
    from test_explorer_fuzz_gpu import random_graph
    gen = torch.Generator().manual_seed(909)
    m = make_model('maze2')
    graphs = [_tied_goal_graph(2500, (2400, 31, 1055), 1, n_obs=30, edges=40000), random_graph(gen, 40, 0, 5),
              random_graph(gen, 1, 3, 0), _tied_goal_graph(3000, (2999, 1500), 2, n_obs=90, edges=52000),
              random_graph(gen, 150, 600, 116, hub=90), _tied_goal_graph(1800, (1700, 64), 3, n_obs=1, edges=25000)]
    b = gnnmp.GraphBatch.from_graphs(graphs, 2, DEV)
    assert b.total_edges // b.n_graphs > 2 * 8192
    parts, nodes = _goal_nodes(m, graphs)
    assert nodes == [K.argmin_stable32(g['v'], g['goal']) for g in graphs]
    assert nodes[0] == 31 and nodes[3] == 1500 and nodes[5] == 64
    _check_scores_need_the_right_node(parts[5].cpu(), graphs[5], 2, monkeypatch, 'column-split build')
    big = _tied_goal_graph(4200, (4100, 3000, 600, 1624), 4, n_obs=5, edges=70000)       # 8 parts of 525 nodes
    _, nodes = _goal_nodes(m, [big])
    assert nodes == [600]
    big['v'][600] += 0.5                                                                 # the lowest copy now in the fourth part
    _, nodes = _goal_nodes(m, [big])
    assert nodes == [K.argmin_stable32(big['v'], big['goal'])] == [1624]


def test_goal_node_among_equidistant_lattice_nodes():
    """Distinct nodes at the same distance: every point of a 14 x 14 lattice in a shuffled order, the goal on a cell centre
    (four corners at 2 (1/16)^2, exact in float32)."""
    v = K.lattice(196, 2, 0.125, 7, 0)
    goal = torch.tensor([0.0625, -0.1875])
    d = K.sqdist64(goal.view(1, 2), v)[0]
    tied = np.flatnonzero(d == d.min())
    assert tied.size == 4 and K.argmin_stable32(v, goal) == tied[0]
    g = {'v': v, 'goal': goal, 'obstacles': torch.rand(9, 2, generator=torch.Generator().manual_seed(7)) - 0.5,
         'edge_index': K.build_edges_stable(v, 98, 4)}
    m = make_model('maze2')
    for graphs in ([g], [g, synth_graph('maze2', 64, 4, seed=1), g]):
        _, nodes = _goal_nodes(m, graphs)
        assert nodes[0] == nodes[-1] == int(tied[0])
