"""Batched training call of the smoother: ``ModelSmoother.forward_train_batch`` / ``training_loss`` and
gnnmp_smoother_train_batch_* (B problems, a loop count each, one forward and one backward).

Yardsticks: the fp64 oracle (oracle.ref_cpu, training mode, run problem by problem) and the per-problem path
``forward_train``.  Bars as in tests/test_smoother_autograd_scale_gpu.py:

    forward:   allclose(rtol 1e-5, atol max(1e-5, 4 * own_out)) against the oracle in fp64 and fp32
    gradients: |g - g_oracle64| <= max(1e-4 * max|g_oracle64|, 4 * own) + 1e-6 per parameter tensor
    own:       fp32 oracle and two fp64 runs with the weights one fp32 ulp off, as there
    against the per-problem path: twice those bars (both sides are within the bar of the oracle)
    BatchNorm running statistics: rtol 1e-5, atol 1e-6 (that file's _check), against the oracle and against the chained
               per-problem calls; num_batches_tracked exactly

Every input satisfies that file's kNN margin (seeds picked on the CPU, the assertion stays in the test)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import load_weights
from gnnmp import _lib
from gnnmp.smoother import SMOOTHER_TRAINABLE, SmoothBatch
from test_smoother_autograd_scale_gpu import (KNN_MARGIN, _knn_margin, _linear_all, _mse_inner, _oracle, _perturbed, _problem,
                                              case_h)
from test_smoother_parity import CONF, chain_edges, make

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RAGGED_SEED = 2
MAZE_SEED = 1
ERR_NULL, ERR_DIMS, ERR_WORKSPACE, ERR_ARG = -1, -2, -4, -6          # include/gnnmp.h
_REF = {}


def ragged():
    """Case 1: no interior row | fewer samples than k, ends first | crosses a 32-row tile, one collided row, ends last | plain."""
    gen = torch.Generator().manual_seed(RAGGED_SEED)
    return [_problem(gen, 2, P, F, Co, 1.0, loop) for P, F, Co, loop in ((2, 50, 30, 3), (3, 4, 3, 1), (33, 60, 1, 4), (12, 40, 25, 2))]


def _mse_counted(outs, probs):
    """train_smoother.py:55-58 with the paths of line 97 (no interior waypoint) left out of sum and divisor."""
    terms = [torch.nn.functional.mse_loss(q['target'].to(o.dtype).to(o.device)[1:-1], o[1:-1])
             for o, q in zip(outs, probs) if q['path'].shape[0] > 2]
    return sum(terms) / len(terms)


def reference(key, name, probs, loss_fn):
    """fp64 / fp32 oracle of ``probs`` run problem by problem, and the bars' ``own`` terms; computed once per case."""
    if key not in _REF:
        C, scale = CONF[name]
        w = load_weights(name)
        for q in probs:
            assert _knn_margin(w, scale, q) > KNN_MARGIN, key
        o64, g64, run64 = _oracle(w, scale, probs, loss_fn, torch.float64)
        o32, g32, _ = _oracle(w, scale, probs, loss_fn, torch.float32)
        own_out = max((a.double() - b).abs().max().item() for a, b in zip(o32, o64))
        own = {k: (g32[k].double() - g64[k]).abs().max().item() for k in SMOOTHER_TRAINABLE}
        for seed in (1, 2):
            op, gp, _ = _oracle(_perturbed(w, seed), scale, probs, loss_fn, torch.float64)
            own_out = max(own_out, max((a - b).abs().max().item() for a, b in zip(op, o64)))
            own = {k: max(own[k], (gp[k] - g64[k]).abs().max().item()) for k in SMOOTHER_TRAINABLE}
        bars = {k: max(1e-4 * g64[k].abs().max().item(), 4 * own[k]) + 1e-6 for k in SMOOTHER_TRAINABLE}
        _REF[key] = dict(o64=o64, o32=o32, g64=g64, run64=run64, atol=max(1e-5, 4 * own_out), bars=bars,
                         nbt=int(w['node_code.1.num_batches_tracked']))
    return _REF[key]


def batch_of(probs):
    return SmoothBatch([q['path'] for q in probs], [q['free'] for q in probs], [q['collided'] for q in probs],
                       [q['edge_index'] for q in probs], DEV)


def split(out, probs):
    res, r = [], 0
    for q in probs:
        res.append(out[r:r + q['path'].shape[0]])
        r += q['path'].shape[0]
    return res


def run_batch(name, probs, loss_fn):
    m = make(name)
    m.train()
    out = m.forward_train_batch(batch_of(probs), [q['loop'] for q in probs])
    assert out.requires_grad and out.shape[0] == sum(q['path'].shape[0] for q in probs)
    outs = split(out, probs)
    loss_fn(outs, probs).backward()
    return m, [o.detach().cpu() for o in outs]


def run_per_problem(name, probs, loss_fn):
    m = make(name)
    m.train()
    outs = [m.forward_train(path=q['path'].to(DEV), free=q['free'].to(DEV), collided=q['collided'].to(DEV),
                            edge_index=q['edge_index'].to(DEV), loop=q['loop']) for q in probs]
    loss_fn(outs, probs).backward()
    return m, [o.detach().cpu() for o in outs]


def grads(m):
    sd = m.state_dict(keep_vars=True)
    for k in SMOOTHER_TRAINABLE:
        assert sd[k].grad is not None and bool(torch.isfinite(sd[k].grad).all()), k
    return {k: sd[k].grad.detach().cpu().double() for k in SMOOTHER_TRAINABLE}


def check_against_oracle(what, m, outs, ref, probs):
    for o, r64, r32 in zip(outs, ref['o64'], ref['o32']):
        err = (o.double() - r64).abs().max().item()
        print('%s forward err %.3e (atol %.1e)' % (what, err, ref['atol']))
        assert torch.allclose(o.double(), r64, rtol=1e-5, atol=ref['atol']), (what, err)
        assert torch.allclose(o, r32, rtol=1e-5, atol=ref['atol']), what
    g = grads(m)
    for k in SMOOTHER_TRAINABLE:
        err = (g[k] - ref['g64'][k]).abs().max().item()
        print('%s %s gradient err %.3e bar %.3e' % (what, k, err, ref['bars'][k]))
        assert err <= ref['bars'][k], (what, k, err, ref['bars'][k])
    bn = m.node_code[1]
    assert int(bn.num_batches_tracked) == ref['nbt'] + sum(q['loop'] for q in probs)
    assert torch.allclose(bn.running_mean.cpu().double(), ref['run64'][0], rtol=1e-5, atol=1e-6)
    assert torch.allclose(bn.running_var.cpu().double(), ref['run64'][1], rtol=1e-5, atol=1e-6)


def check_against_module(what, m, outs, m2, outs2, ref):
    """Batched against per-problem: twice the bars; running statistics as in _check."""
    for a, b in zip(outs, outs2):
        err = (a - b).abs().max().item()
        print('%s forward, batch vs per problem: %.3e' % (what, err))
        assert torch.allclose(a, b, rtol=2e-5, atol=2 * ref['atol']), (what, err)
    g, g2 = grads(m), grads(m2)
    for k in SMOOTHER_TRAINABLE:
        err = (g[k] - g2[k]).abs().max().item()
        assert err <= 2 * ref['bars'][k], (what, k, err, ref['bars'][k])
    bn, bn2 = m.node_code[1], m2.node_code[1]
    assert int(bn.num_batches_tracked) == int(bn2.num_batches_tracked)
    assert torch.allclose(bn.running_mean, bn2.running_mean, rtol=1e-5, atol=1e-6)
    assert torch.allclose(bn.running_var, bn2.running_var, rtol=1e-5, atol=1e-6)


def test_ragged_mixed_loops_edge_shapes():
    """Case 1: P = 2 / 3 / 33 / 12, loops 3 / 1 / 4 / 2, a loss over every output row."""
    probs = ragged()
    assert [(q['path'].shape[0], q['loop']) for q in probs] == [(2, 3), (3, 1), (33, 4), (12, 2)]
    ref = reference('ragged', 'smooth_2d_attv3', probs, _linear_all)
    m, outs = run_batch('smooth_2d_attv3', probs, _linear_all)
    check_against_oracle('ragged', m, outs, ref, probs)


def test_reference_optimizer_step():
    """Case 2: eight ur5 problems, loops 1 .. 9, the mean MSE over [1:-1]; one batched forward + one backward against the
    oracle and against eight forward_train calls + one backward on a second module with the same weights."""
    name = 'smooth_ur5_attv3'
    probs = case_h(name, 814)
    assert len(probs) == 8 and max(q['path'].shape[0] for q in probs) > 32 and len({q['loop'] for q in probs}) > 2
    ref = reference('step', name, probs, _mse_inner)
    m, outs = run_batch(name, probs, _mse_inner)
    check_against_oracle('step', m, outs, ref, probs)
    m2, outs2 = run_per_problem(name, probs, _mse_inner)
    check_against_module('step', m, outs, m2, outs2, ref)


def _c_forward(m, sb, loops):
    """gnnmp_smoother_train_batch_forward as is (problems in the given order, loops non-increasing): rows and stats."""
    from gnnmp.smoother import _cbatch
    L = _lib.lib()
    h = m._native(DEV, for_training=True)
    cb = _cbatch(sb)
    arr = (ctypes.c_int32 * len(loops))(*loops)
    need = ctypes.c_size_t()
    assert L.gnnmp_smoother_train_batch_workspace_bytes(h, ctypes.byref(cb), arr, ctypes.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(sb.path)
    stats = torch.full((len(loops), max(loops), 2, m.embed_size), float('nan'), device=DEV)
    assert L.gnnmp_smoother_train_batch_forward(h, ctypes.byref(cb), arr, out.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                                torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return out.cpu(), stats.cpu()


@pytest.mark.parametrize('order', [(0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2), (2, 0, 3, 1)])
def test_no_leakage_between_problems(order):
    """Case 3: every problem of case 1 alone (B = 1 through the new entry point) gives the bits -- output rows and BatchNorm
    statistics -- it gives inside the batch, whatever the order of the four; gradients of the reordered batch to the bar."""
    probs = ragged()
    ref = reference('ragged', 'smooth_2d_attv3', probs, _linear_all)
    m = make('smooth_2d_attv3')
    m.train()
    alone = [_c_forward(m, batch_of([q]), [q['loop']]) for q in probs]
    # the entry point itself: the given order, longest loop first inside it (a stable sort, as the wrapper does)
    run = sorted(order, key=lambda b: -probs[b]['loop'])
    out, stats = _c_forward(m, batch_of([probs[b] for b in run]), [probs[b]['loop'] for b in run])
    for i, (o, b) in enumerate(zip(split(out, [probs[b] for b in run]), run)):
        loop = probs[b]['loop']
        assert torch.equal(o, alone[b][0]), (order, b)
        assert torch.equal(stats[i, :loop], alone[b][1][0, :loop]), (order, b)
        assert bool((stats[i, loop:] == 0).all()), (order, b)
    # the wrapper: caller order in, caller order out
    shuffled = [probs[b] for b in order]
    mb, outs = run_batch('smooth_2d_attv3', shuffled, _linear_all)
    for o, b in zip(outs, order):
        assert torch.equal(o, alone[b][0]), (order, b)
    g = grads(mb)
    for k in SMOOTHER_TRAINABLE:
        assert (g[k] - ref['g64'][k]).abs().max().item() <= ref['bars'][k], (order, k)


def test_two_backward_passes_same_bits():
    """Case 4."""
    name = 'smooth_ur5_attv3'
    probs = case_h(name, 814)
    a = grads(run_batch(name, probs, _mse_inner)[0])
    b = grads(run_batch(name, probs, _mse_inner)[0])
    for k in SMOOTHER_TRAINABLE:
        assert torch.equal(a[k], b[k]), k


def _loss_case(key, name, probs):
    """training_loss against the same loss through forward_train per problem, and against the oracle."""
    ref = reference(key, name, probs, _mse_counted)
    m = make(name)
    m.train()
    targets = torch.cat([q['target'] for q in probs]).to(DEV)
    loss = m.training_loss(batch_of(probs), targets, [q['loop'] for q in probs])
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    loss.backward()
    m2, outs2 = run_per_problem(name, probs, _mse_counted)
    with torch.no_grad():
        want = _mse_counted(outs2, probs).item()
        want64 = _mse_counted(ref['o64'], probs).item()
    # a loss is a mean of squared differences of rows that sit within `atol` of the oracle's: d (a - t)^2 <= 2 |a - t| atol + atol^2
    worst = max((q['target'].double() - o).abs().max().item() for q, o in zip(probs, ref['o64']) if q['path'].shape[0] > 2)
    tol = 2 * worst * ref['atol'] + ref['atol'] ** 2 + 1e-5 * abs(want64)
    print('%s: training_loss %.6e, per problem %.6e, oracle %.6e (tol %.1e)' % (key, loss.item(), want, want64, tol))
    assert abs(loss.item() - want64) <= tol and abs(loss.item() - want) <= 2 * tol
    g, g2 = grads(m), grads(m2)
    for k in SMOOTHER_TRAINABLE:
        assert (g[k] - ref['g64'][k]).abs().max().item() <= ref['bars'][k], (key, k)
        assert (g[k] - g2[k]).abs().max().item() <= 2 * ref['bars'][k], (key, k)
    return loss


def test_training_loss_leaves_out_paths_without_interior():
    """Case 5a: a P = 2 problem in the batch is in neither the sum nor the divisor."""
    probs = ragged()
    assert sum(q['path'].shape[0] <= 2 for q in probs) == 1
    _loss_case('ragged_mse', 'smooth_2d_attv3', probs)


def test_training_loss_on_device_side_targets():
    """Case 5b: four short maze2 paths on a map of tests/golden/oracle_smooth_*.npz, samples classified by Maze2D, targets
    from oracle_smooth.smoothing_targets: a finite loss, gradients as through forward_train per problem."""
    from gnnmp import oracle_smooth as OS
    from gnnmp.maze2d import Maze2D
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    with np.load(os.path.join(here, 'oracle_smooth_p330.npz')) as f:
        grid, rec = f['map'], f['path'].astype(np.float32)
    env = Maze2D(grid[None], np.zeros((1, 2)), np.zeros((1, 2)))
    env.init_new_problem(0)
    assert len(rec) == 14
    gen = torch.Generator().manual_seed(MAZE_SEED)
    probs = []
    for lo, hi, loop in ((0, 6, 2), (4, 10, 3), (8, 14, 1), (2, 7, 2)):
        pts = (torch.rand(90, 2, generator=gen, dtype=torch.float64) * 2 - 1).float()
        ok = torch.tensor([bool(env._state_fp(p.double().numpy())) for p in pts])
        assert 10 < int(ok.sum()) < 80
        probs.append(dict(path=torch.from_numpy(rec[lo:hi].copy()), free=pts[ok], collided=pts[~ok], edge_index=chain_edges(hi - lo),
                          loop=loop))
    paths = torch.cat([q['path'] for q in probs]).to(DEV)
    ptr = np.cumsum([0] + [q['path'].shape[0] for q in probs])
    target, status = OS.smoothing_targets(paths, ptr, np.stack([grid] * 4), torch.Generator(device=DEV).manual_seed(3))
    assert target.shape == paths.shape and not any(int(s) & OS.STATUS_SKIPPED for s in status.cpu().tolist())
    for q, t in zip(probs, split(target.cpu(), probs)):
        q['target'] = t
    loss = _loss_case('maze2', 'smooth_2d_attv3', probs)
    assert bool(torch.isfinite(loss))


def test_errors():
    """Case 6."""
    probs = ragged()
    sb = batch_of(probs)
    m = make('smooth_2d_attv3')
    m.train()
    with pytest.raises(ValueError):
        m.forward_train_batch(sb, [1, 2, 3])
    with pytest.raises(ValueError):
        m.forward_train_batch(sb, [1, 0, 2, 2])
    with pytest.raises(ValueError):
        m.forward_train_batch(sb, 0)
    cpu = SmoothBatch([q['path'] for q in probs], [q['free'] for q in probs], [q['collided'] for q in probs],
                      [q['edge_index'] for q in probs], 'cpu')
    with pytest.raises(RuntimeError, match='GPU only'):
        m.forward_train_batch(cpu, 2)
    m.mlp_dtype = 'bf16'
    with pytest.raises(RuntimeError, match='fp32'):
        m.forward_train_batch(sb, 2)
    m.mlp_dtype = 'fp32'
    # the C ABI: the one-problem entry point still refuses a batch; the batched one names its argument errors
    from gnnmp.smoother import _cbatch
    L = _lib.lib()
    h = m._native(DEV, for_training=True)
    two = batch_of(probs[:2])
    cb = _cbatch(two)
    buf = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(two.path)
    st = torch.cuda.current_stream().cuda_stream
    assert L.gnnmp_smoother_train_forward(h, ctypes.byref(cb), 1, out.data_ptr(), None, buf.data_ptr(), buf.numel(), st) == ERR_DIMS
    need = ctypes.c_size_t()
    arr = lambda *v: (ctypes.c_int32 * len(v))(*v)  # noqa: E731
    assert L.gnnmp_smoother_train_batch_workspace_bytes(h, ctypes.byref(cb), None, ctypes.byref(need)) == ERR_NULL
    assert L.gnnmp_smoother_train_batch_workspace_bytes(h, ctypes.byref(cb), arr(2, 0), ctypes.byref(need)) == ERR_ARG
    assert L.gnnmp_smoother_train_batch_workspace_bytes(h, ctypes.byref(cb), arr(1, 2), ctypes.byref(need)) == ERR_ARG
    assert L.gnnmp_smoother_train_batch_workspace_bytes(h, ctypes.byref(cb), arr(2, 1), ctypes.byref(need)) == 0
    assert L.gnnmp_smoother_train_batch_forward(h, ctypes.byref(cb), arr(2, 1), out.data_ptr(), None, buf.data_ptr(), 256, st) \
        == ERR_WORKSPACE
    assert L.gnnmp_smoother_train_batch_forward(h, ctypes.byref(cb), arr(2, 1), None, None, buf.data_ptr(), buf.numel(), st) \
        == ERR_NULL
    mb = make('smooth_2d_attv3')
    mb.mlp_dtype = 'bf16'
    hb = mb._native(DEV)
    assert L.gnnmp_smoother_train_batch_workspace_bytes(hb, ctypes.byref(cb), arr(2, 1), ctypes.byref(need)) == ERR_DIMS
    torch.cuda.synchronize()
