"""The explorer's training path with a loop count per graph (gnnmp_explorer_train_batch_*, EncoderProcessDecoder.train_scores_batch,
episodes.forward_scores_batched): one forward and one backward for a batch whose graphs stop after their own number of
iterations (train_explorer.py:148 draws one per sample).

  1  uniform loops are the existing call, bit for bit (scores and parameter gradients); the existing call past the batched
     call's loop bound
  2  ragged loops against the fp64 oracle: scores per graph at the bar of parity_bar.py, gradients against the SUM over
     graphs of the oracle's float64 gradients at the bound of test_explorer_autograd_gpu.py,
         |g - g64| <= max(1e-4 max|g64|, 4 own) + 1e-6 per tensor, own = max|g32 - g64| of the same oracle in float32;
     maze2 (d = 32) and kuka7 (d = 64, with and without obstacles)
  3  a graph stops contributing when it stops
  4  order and determinism
  5  the launch sizes are the prep stage's padded prefixes
  6  errors
  7  the episodes wiring
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_weights
import gnnmp
from gnnmp import _lib, episodes as ep
from gnnmp.explorer import TRAINABLE
from gnnmp.synth import ENVS, synth_graph
from oracle import ref_cpu
from parity_bar import ATOL_FLOOR, assert_fp32_parity

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ERR_NULL, ERR_DIMS, ERR_WORKSPACE, ERR_ARG = -1, -2, -4, -6

RAGGED_SIZES, RAGGED_LOOPS = (33, 64, 257, 100, 40), (2, 5, 1, 5, 3)       # caller order: not sorted, a tie at the maximum


def make(env, use_obstacles=True):
    e = ENVS[env]
    m = gnnmp.EncoderProcessDecoder(e['workspace'], e['C'], e['d'], e['S'], use_obstacles=use_obstacles)
    m.load_state_dict(load_weights(e['ckpt']), strict=True)
    return m.train()


def graphs_of(env, sizes, k, seed0):
    return [synth_graph(env, n, k, seed=seed0 + i) for i, n in enumerate(sizes)]


def batch_of(env, graphs):
    return gnnmp.GraphBatch.from_graphs(graphs, ENVS[env]['S'], DEV)


def edge_ptr(graphs):
    return np.concatenate([[0], np.cumsum([g['edge_index'].shape[1] for g in graphs])]).tolist()


def coef_of(graphs, seed=7):
    E = edge_ptr(graphs)[-1]
    return torch.randn(E, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def trainable(m):
    man = dict(m._manifest)
    return [(n, p) for n, p in m.named_parameters() if n.split('.')[0] in TRAINABLE and n in man]


def grads_of(m, loss):
    m.zero_grad()
    loss.backward()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def assert_frozen_untouched(m, grads):
    names = {n for n, _ in trainable(m)}
    for n, g in grads.items():
        assert n in names or float(g.abs().max()) == 0.0, n          # behind the reference's detach (model.py:141,142,146)
    assert names <= set(grads), sorted(names - set(grads))


_oracle = {}


def oracle(env, sizes, k, seed0, loops, use_obstacles=True):
    """Per graph: the oracle's scores and its gradients of sum(coef * scores) in float32 and float64 -- computed once per case."""
    key = (env, tuple(sizes), k, seed0, tuple(loops), use_obstacles)
    if key in _oracle:
        return _oracle[key]
    graphs = graphs_of(env, sizes, k, seed0)
    w = load_weights(ENVS[env]['ckpt'])
    coef, ept = coef_of(graphs), edge_ptr(graphs)
    out = []
    for i, (g, lp) in enumerate(zip(graphs, loops)):
        rec = {}
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            wd = {n: (t.to(dt).clone().requires_grad_(True) if t.is_floating_point() else t) for n, t in w.items()}
            s = ref_cpu.explorer_forward(wd, g['v'].to(dt), g['goal'].to(dt), g['obstacles'].to(dt), g['edge_index'], lp,
                                         use_obstacles=use_obstacles, detach=True)
            (s * coef[ept[i]:ept[i + 1]].to(dt)).sum().backward()
            rec['s' + tag] = s.detach()
            rec['g' + tag] = {n: t.grad.double() for n, t in wd.items() if torch.is_tensor(t) and t.is_floating_point()
                              and t.grad is not None}
        out.append(rec)
    _oracle[key] = (graphs, coef, ept, out)
    return _oracle[key]


def oracle_sum(recs, which, keep):
    tot = {}
    for i, r in enumerate(recs):
        if i in keep:
            for n, g in r[which].items():
                tot[n] = tot[n] + g if n in tot else g.clone()
    return tot


def assert_grads_within_bound(m, grads, g64, g32, what):
    worst = 0.0
    for n, _ in trainable(m):
        ref = g64.get(n)
        if ref is None:
            continue
        scale = float(ref.abs().max())
        own = float((g32[n] - ref).abs().max())
        err = float((grads[n].cpu().double() - ref).abs().max())
        worst = max(worst, err / (scale + 1e-30))
        print('%s %-28s err %.3e  scale %.3e  own %.3e' % (what, n, err, scale, own))
        assert err <= max(1e-4 * scale, 4.0 * own) + 1e-6, (what, n, err, scale, own)
    return worst


# ---------------------------------------------------------------------------------------------------------------- 1
def test_uniform_loops_are_the_existing_call():
    graphs = graphs_of('maze2', (40, 64, 130), 4, 100)
    m = make('maze2')
    b = batch_of('maze2', graphs)
    E, L = b.total_edges, 3
    coef = coef_of(graphs).float().to(DEV)
    ei = b.edge_index
    rows = (ei[1] < 8) & (torch.arange(E, device=DEV) < edge_ptr(graphs)[1])       # "frontier": edges into graph 0's first eight nodes
    pick = 3

    def loss_lin(s):
        return (s * coef).sum()

    def loss_ce(s):                                                                 # train_explorer.py:174
        return -s[rows].log_softmax(dim=0)[pick]

    for name, loss_fn in (('linear', loss_lin), ('cross-entropy', loss_ce)):
        s0 = m.train_scores(b, L)
        g0 = grads_of(m, loss_fn(s0))
        s1 = m.train_scores_batch(b, [L] * 3)
        g1 = grads_of(m, loss_fn(s1))
        assert torch.equal(s0.detach(), s1.detach()), name
        assert set(g0) == set(g1)
        for n in g0:
            assert torch.equal(g0[n], g1[n]), (name, n)
        # and with the host sizes handed in instead of read back
        s2 = m.train_scores_batch(b, [L] * 3, [40, 64, 130], [g['edge_index'].shape[1] for g in graphs])
        assert torch.equal(s0.detach(), s2.detach())


def test_uniform_call_past_the_batched_loop_bound():
    """train_scores takes any loop count (its plan is one row count, not a table of TRAIN_BATCH_MAX_LOOP entries);
    train_scores_batch keeps its bound."""
    L = _lib.TRAIN_BATCH_MAX_LOOP + 1
    graphs = graphs_of('maze2', (33,), 4, 100)
    m = make('maze2')
    b = batch_of('maze2', graphs)
    coef = coef_of(graphs).float().to(DEV)
    runs = []
    for _ in range(2):
        s = m.train_scores(b, L)
        runs.append((s.detach().clone(), grads_of(m, (s * coef).sum())))
    s0, g0 = runs[0]
    assert s0.shape == (b.total_edges,) and bool(torch.isfinite(s0).all())
    assert_frozen_untouched(m, g0)
    assert all(bool(torch.isfinite(g).all()) for g in g0.values())
    assert torch.equal(s0, runs[1][0]) and set(g0) == set(runs[1][1])
    for n in g0:
        assert torch.equal(g0[n], runs[1][1][n]), n
    with pytest.raises(ValueError):
        m.train_scores_batch(b, [L])
    g, w = graphs[0], load_weights(ENVS['maze2']['ckpt'])
    ref = {}
    for dt in (torch.float32, torch.float64):
        wd = {n: (t.to(dt) if t.is_floating_point() else t) for n, t in w.items()}
        with torch.no_grad():
            ref[dt] = ref_cpu.explorer_forward(wd, g['v'].to(dt), g['goal'].to(dt), g['obstacles'].to(dt), g['edge_index'], L,
                                               use_obstacles=True, detach=True)
    c = assert_fp32_parity(s0.cpu(), ref[torch.float32], ref[torch.float64], 'maze2 N 33 loop %d' % L)
    print('loop %d: max|gpu - oracle64| %.3e  own %.3e  bar %.3e' % (L, c['err64'], c['own'], c['atol']))


# ---------------------------------------------------------------------------------------------------------------- 2
def _ragged_case(env, sizes, k, seed0, loops, use_obstacles=True):
    graphs, coef, ept, recs = oracle(env, sizes, k, seed0, loops, use_obstacles)
    m = make(env, use_obstacles)
    b = batch_of(env, graphs)
    s = m.train_scores_batch(b, loops)
    assert s.shape == (ept[-1],) and s.requires_grad
    for i, r in enumerate(recs):
        c = assert_fp32_parity(s.detach()[ept[i]:ept[i + 1]].cpu(), r['s32'], r['s64'], '%s graph %d loop %d' % (env, i, loops[i]))
        print('%s graph %d (N %d, loop %d): max|gpu - oracle64| %.3e  own %.3e  bar %.3e' % (env, i, sizes[i], loops[i], c['err64'], c['own'], c['atol']))
    grads = grads_of(m, (s * coef.float().to(DEV)).sum())
    assert_frozen_untouched(m, grads)
    keep = set(range(len(graphs)))
    worst = assert_grads_within_bound(m, grads, oracle_sum(recs, 'g64', keep), oracle_sum(recs, 'g32', keep), env)
    print('%s ragged loops %s: worst relative gradient error %.2e' % (env, list(loops), worst))
    return m, b, s, grads


def test_ragged_loops_match_oracle_maze2():
    _ragged_case('maze2', RAGGED_SIZES, 4, 200, RAGGED_LOOPS)


@pytest.mark.parametrize('use_obstacles', [True, False], ids=['obstacles', 'no-obstacles'])
def test_ragged_loops_match_oracle_kuka7(use_obstacles):
    _ragged_case('kuka7', (64, 200), 4, 300, (1, 4), use_obstacles)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_a_stopped_graph_contributes_nothing():
    graphs, coef, ept, recs = oracle('maze2', RAGGED_SIZES, 4, 200, RAGGED_LOOPS)
    stop = RAGGED_LOOPS.index(1)
    keep = set(range(len(graphs))) - {stop}
    g64, g32 = oracle_sum(recs, 'g64', keep), oracle_sum(recs, 'g32', keep)
    m = make('maze2')
    cot = coef.float().clone()
    cot[ept[stop]:ept[stop + 1]] = 0.0
    s = m.train_scores_batch(batch_of('maze2', graphs), RAGGED_LOOPS)
    full = grads_of(m, (s * cot.to(DEV)).sum())
    assert_grads_within_bound(m, full, g64, g32, 'zeroed cotangent')        # the oracle's sum WITHOUT that graph
    rest = [g for i, g in enumerate(graphs) if i != stop]
    rest_cot = torch.cat([cot[ept[i]:ept[i + 1]] for i in sorted(keep)])
    s2 = m.train_scores_batch(batch_of('maze2', rest), [lp for i, lp in enumerate(RAGGED_LOOPS) if i != stop])
    removed = grads_of(m, (s2 * rest_cot.to(DEV)).sum())
    assert set(full) == set(removed)
    for n, _ in trainable(m):
        ref = g64.get(n)
        if ref is None:
            continue
        scale, own = float(ref.abs().max()), float((g32[n] - ref).abs().max())
        err = float((full[n] - removed[n]).abs().max())
        assert err <= max(1e-4 * scale, 4.0 * own) + 1e-6, (n, err, scale, own)


# ---------------------------------------------------------------------------------------------------------------- 4
def test_order_and_determinism():
    graphs = graphs_of('maze2', RAGGED_SIZES, 4, 200)
    coef, ept = coef_of(graphs).float(), edge_ptr(graphs)
    m = make('maze2')
    b = batch_of('maze2', graphs)
    runs = []
    for _ in range(2):
        s = m.train_scores_batch(b, RAGGED_LOOPS)
        runs.append((s.detach().clone(), grads_of(m, (s * coef.to(DEV)).sum())))
    assert torch.equal(runs[0][0], runs[1][0])
    assert set(runs[0][1]) == set(runs[1][1]) and len(runs[0][1]) >= 20
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n
    # another caller order, every graph keeping its loop: the same bits per graph
    perm = [3, 0, 4, 2, 1]
    pg = [graphs[i] for i in perm]
    sp = m.train_scores_batch(batch_of('maze2', pg), [RAGGED_LOOPS[i] for i in perm]).detach()
    pept = edge_ptr(pg)
    for j, i in enumerate(perm):
        assert torch.equal(sp[pept[j]:pept[j + 1]], runs[0][0][ept[i]:ept[i + 1]]), (j, i)
    # one graph is train_scores on that graph
    g = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in graphs[3].items()}
    b1 = m._single(g['goal'], g['v'], g['obstacles'], g['edge_index'])
    c1 = coef[ept[3]:ept[4]].to(DEV)
    s0 = m.train_scores(b1, 3)
    g0 = grads_of(m, (s0 * c1).sum())
    s1 = m.train_scores_batch(b1, [3])
    g1 = grads_of(m, (s1 * c1).sum())
    assert torch.equal(s0.detach(), s1.detach()) and set(g0) == set(g1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# ---------------------------------------------------------------------------------------------------------------- 5
def test_launch_sizes_are_the_padded_prefixes():
    graphs = graphs_of('maze2', RAGGED_SIZES, 4, 200)
    m = make('maze2')
    b = batch_of('maze2', graphs)
    G = len(graphs)
    ncnt, ecnt = list(RAGGED_SIZES), [g['edge_index'].shape[1] for g in graphs]
    order = sorted(range(G), key=lambda g: -RAGGED_LOOPS[g])
    assert order == [1, 3, 4, 0, 2]                                              # stable: the tie keeps the caller's order
    sb, _ = m._sorted_batch(b, order, ncnt, ecnt)
    loops = [RAGGED_LOOPS[g] for g in order]
    active, nrows, erows = _lib.explorer_train_batch_plan(loops, [ncnt[g] for g in order], [ecnt[g] for g in order])
    assert active == [5, 4, 3, 2, 2]
    # the prep stage's own node_ptr_pad / CSR row starts for that batch, through the geometry hook
    L = _lib.lib()
    cb = m._cbatch(sb)
    need = ctypes.c_size_t()
    _lib.check(L.gnnmp_train_geom_workspace_bytes(ctypes.byref(cb), 2, ctypes.byref(need)), 'geom_workspace_bytes')
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    geom = _lib.TrainGeom()
    _lib.check(L.gnnmp_train_geom_build(ctypes.byref(cb), 2, ws.data_ptr(), ws.numel(), ctypes.byref(geom),
                                        torch.cuda.current_stream().cuda_stream), 'geom_build')
    dump = ws.cpu().numpy()

    def arr(ptr, n):
        off = ptr - ws.data_ptr()
        assert 0 <= off and off + 4 * n <= need.value
        return dump[off:off + 4 * n].view(np.int32)
    npp = arr(geom.node_ptr_pad, G + 1)
    row_beg = arr(geom.row_beg, geom.n_pad)
    for it, a in enumerate(active):
        assert nrows[it] == int(npp[a]), (it, a)
        # the CSR range of the first graph NOT running starts where the active edge rows end
        if a < G:
            assert erows[it] == int(row_beg[npp[a]]), (it, a)
    assert nrows[0] <= geom.n_pad and erows[0] <= geom.e_pad
    assert all(int(x) % 256 == 0 for x in npp)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_errors():
    graphs = graphs_of('maze2', (40, 64, 130), 4, 100)
    m = make('maze2')
    b = batch_of('maze2', graphs)
    with pytest.raises(ValueError):
        m.train_scores_batch(b, [1, 2])
    with pytest.raises(ValueError):
        m.train_scores_batch(b, [2, 0, 1])
    with pytest.raises(ValueError):
        m.train_scores_batch(b, [2, 1, 1], [40, 64], [1, 2, 3])
    cpu = gnnmp.GraphBatch.from_graphs(graphs, 2, 'cpu')
    with pytest.raises(RuntimeError, match='GPU only'):
        m.train_scores_batch(cpu, [1, 1, 1])
    m.mlp_dtype = 'bf16'
    with pytest.raises(RuntimeError, match='fp32'):
        m.train_scores_batch(b, [1, 1, 1])
    m.mlp_dtype = 'fp32'
    # the C ABI
    L = _lib.lib()
    h = m._native(DEV)
    cb = m._cbatch(b)
    ncnt, ecnt = _lib.i32_array([40, 64, 130]), _lib.i32_array([g['edge_index'].shape[1] for g in graphs])
    arr = _lib.i32_array
    need = ctypes.c_size_t()
    ref = ctypes.c_size_t()
    wsb = L.gnnmp_explorer_train_batch_workspace_bytes
    assert wsb(h, ctypes.byref(cb), arr([3, 2, 1]), ncnt, ecnt, ctypes.byref(need)) == 0
    assert L.gnnmp_explorer_train_workspace_bytes(h, ctypes.byref(cb), 3, ctypes.byref(ref)) == 0
    assert 0 < need.value <= ref.value                       # never more than the uniform call at the largest loop
    assert wsb(h, ctypes.byref(cb), arr([1, 2, 1]), ncnt, ecnt, ctypes.byref(need)) == ERR_ARG          # ascending
    assert wsb(h, ctypes.byref(cb), arr([2, 1, 0]), ncnt, ecnt, ctypes.byref(need)) == ERR_ARG
    assert wsb(h, ctypes.byref(cb), arr([2, 1, 1]), arr([40, 64, 131]), ecnt, ctypes.byref(need)) == ERR_ARG   # not the batch's total
    assert wsb(h, ctypes.byref(cb), None, ncnt, ecnt, ctypes.byref(need)) == ERR_NULL
    assert wsb(h, ctypes.byref(cb), arr([2, 1, 1]), None, ecnt, ctypes.byref(need)) == ERR_NULL
    buf = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    out = torch.empty(b.total_edges, dtype=torch.float32, device=DEV)
    grad = torch.empty(int(L.gnnmp_explorer_grad_floats(h)), dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    fwd, bwd = L.gnnmp_explorer_train_batch_forward, L.gnnmp_explorer_train_batch_backward
    assert fwd(h, ctypes.byref(cb), arr([1, 2, 1]), ncnt, ecnt, 1, out.data_ptr(), buf.data_ptr(), buf.numel(), st) == ERR_ARG
    assert bwd(h, ctypes.byref(cb), arr([1, 2, 1]), ncnt, ecnt, out.data_ptr(), grad.data_ptr(), buf.data_ptr(), buf.numel(), st) == ERR_ARG
    assert fwd(h, ctypes.byref(cb), arr([3, 2, 1]), ncnt, ecnt, 1, out.data_ptr(), buf.data_ptr(), 256, st) == ERR_WORKSPACE
    assert bwd(h, ctypes.byref(cb), arr([3, 2, 1]), ncnt, ecnt, out.data_ptr(), grad.data_ptr(), buf.data_ptr(), 256, st) == ERR_WORKSPACE
    assert fwd(h, ctypes.byref(cb), arr([3, 2, 1]), ncnt, ecnt, 1, None, buf.data_ptr(), buf.numel(), st) == ERR_NULL
    assert fwd(h, ctypes.byref(cb), arr([3, 2, 1]), ncnt, None, 1, out.data_ptr(), buf.data_ptr(), buf.numel(), st) == ERR_NULL
    mb = make('maze2')
    mb.mlp_dtype = 'bf16'
    hb = mb._native(DEV)
    assert wsb(hb, ctypes.byref(cb), arr([3, 2, 1]), ncnt, ecnt, ctypes.byref(need)) == ERR_DIMS
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_episodes_wiring():
    rng = np.random.default_rng(21)
    sizes = rng.integers(100, 201, 6).tolist()
    pts = [rng.uniform(-1.0, 1.0, (n, 2)) for n in sizes]
    maps = (rng.random((6, 15, 15)) < 0.25).astype(np.float64)
    nptr = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    g = ep.maze_training_graphs(torch.from_numpy(np.concatenate(pts)).to(DEV), nptr, maps, 2)
    m = make('maze2').to(DEV).train()
    loss, info = ep.training_step(m, g, loop=10, generator=torch.Generator(device=DEV).manual_seed(4),
                                  cpu_generator=torch.Generator().manual_seed(4), batched=True)
    assert len(set(info['loops'])) > 1                       # the draws are ragged: the batched call has something to do
    assert bool(torch.isfinite(loss)) and bool(info['counted'].any())
    grads = grads_of(m, loss)
    assert set(grads) == {n for n, _ in trainable(m)}
    assert all(bool(torch.isfinite(x).all()) for x in grads.values())
    # both forwards are fp32 evaluations of the same function
    goal, loops = info['paths']['goal'], info['loops']
    with torch.no_grad():
        a = ep.forward_scores_batched(m, g, goal, loops)
        b = ep.forward_scores(m, g, goal, loops)
    err = float((a - b).abs().max())
    print('forward_scores_batched vs forward_scores over %d edges, loops %s: max difference %.3e' % (a.numel(), loops, err))
    assert a.shape == b.shape == (g.total_edges,)
    assert err <= 2 * ATOL_FLOOR
