"""NextNet3DTrain on the device against the unmodified reference's recorded losses and gradients
(tests/golden/next3d_train_*.npz): kuka7 at 0 / 1 / 2 / 20 rounds, kuka14 at 1 / 20 rounds.

  * pb_rep and y of the training forward are torch.equal to the inference network's (NextNet3D);
  * the loss: |loss - loss64| <= max(1e-4 |loss64|, 4 own) + 1e-6, own = |loss32 - loss64| of the reference (the rule of
    tests/test_next_train_gpu.py);
  * every parameter's gradient through the project's gradient bar (next3d_train_host.check_bar):
    |g - g64| <= max(1e-4 max|g64|, 4 own) + 1e-6, own = max|g32 - g64| of the reference's two recordings;
  * rows in a permuted order, a problem without rows, a problem_of_state outside [0, B), run-to-run bit equality, the empty call
    and the stale backward.
Run with -s for error / bar per tensor."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_model3d, next_train, next_train3d
import next3d_train_host as host

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = [(7, 0), (7, 1), (7, 2), (7, 20), (14, 1), (14, 20)]
_NETS = {}


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _net(dim):
    if dim not in _NETS:
        w = host.load_weights(dim)
        pd = host.FAMILIES[dim][1]
        _NETS[dim] = (next_train3d.NextNet3DTrain(dim, pd, device=DEV).load_state_dict(w), next_model3d.NextNet3D(dim, pd).load_state_dict(w))
    return _NETS[dim]


def _run(net, maps, goals, rows, of, ptr, actions, values, iters):
    """One forward and backward of train()'s loss -> (y, loss, {name: gradient tensor}, pb_rep)."""
    y = net.forward(_t(maps), _t(goals), _t(rows), _t(of, torch.int32), iters)
    loss = next_train.loss_from_outputs(y, _t(actions), _t(values), ptr)
    for p in net.parameters():
        p.grad = None
    loss.backward()
    return y.detach(), float(loss.detach()), {k: p.grad.detach().clone() for k, p in net.named_parameters()}, net.pb_rep


@pytest.mark.parametrize('dim,iters', CASES)
def test_forward_bits_loss_and_gradients_against_the_recorded_reference(dim, iters):
    net, plain = _net(dim)
    rec = host.load_case(dim)
    maps, goals, rows, of, ptr, actions, values = host.case_inputs(rec, iters)
    y, loss, grads, pb_rep = _run(net, maps, goals, rows, of, ptr, actions, values, iters)
    net.check_status()
    # the forward's bits
    pb_plain = plain.pb_forward(_t(maps), _t(goals), iters)
    assert torch.equal(pb_rep, pb_plain)
    assert torch.equal(y, plain.state_forward(_t(rows), _t(of, torch.int32), pb_plain))
    plain.check_status()
    # the loss
    l64, l32 = float(rec['loss64_i%d' % iters]), float(rec['loss32_i%d' % iters])
    own = abs(l32 - l64)
    print('kuka%d iters %2d: loss %.9g  reference fp64 %.9g  (reference fp32 off by %.2e)' % (dim, iters, loss, l64, own))
    assert abs(loss - l64) <= max(1e-4 * abs(l64), 4 * own) + 1e-6
    # the gradients
    g32, g64 = host.load_grads(dim, iters)
    assert set(grads) == set(g64)
    bad = host.check_bar(grads, g32, g64, 'kuka%d i%d' % (dim, iters))
    assert not bad, bad


def test_permuted_rows_a_problem_without_rows_and_run_to_run_bits():
    dim, iters = 7, 2
    net, _ = _net(dim)
    rec = host.load_case(dim)
    maps, goals, rows, of, ptr, actions, values = host.case_inputs(rec, 20)          # both problems, 13 rows
    y0, loss0, g0, _ = _run(net, maps, goals, rows, of, ptr, actions, values, iters)
    y1, loss1, g1, _ = _run(net, maps, goals, rows, of, ptr, actions, values, iters)
    assert torch.equal(y0, y1) and loss0 == loss1 and all(torch.equal(g0[k], g1[k]) for k in g0)      # two runs, the same bits

    # rows in a permuted order: y follows the permutation bit for bit; the gradient against the float64 restatement of the
    # same sum (the sum over the rows runs in another order, so not the same bits)
    perm = np.random.RandomState(3).permutation(rows.shape[0])
    dy = np.random.RandomState(4).standard_normal((rows.shape[0], dim + 1)).astype(np.float32)

    def weighted(order):
        y = net.forward(_t(maps), _t(goals), _t(rows[order]), _t(of[order], torch.int32), iters)
        for p in net.parameters():
            p.grad = None
        (y * _t(dy[order])).sum().backward()
        return y.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}

    ya, ga = weighted(np.arange(rows.shape[0]))
    yb, gb = weighted(perm)
    assert torch.equal(ya[perm], yb)
    w = host.load_weights(dim)
    pair = []
    for dtype in (torch.float32, torch.float64):
        lv = host.leaves(w, dtype)
        out = host.forward(lv, maps, goals, rows, of, iters)
        pair.append(host.grads_of((out * torch.from_numpy(dy).to(dtype)).sum(), lv))
    assert not host.check_bar(ga, pair[0], pair[1], 'rows in order')
    assert not host.check_bar(gb, pair[0], pair[1], 'rows permuted')

    # a problem without rows: three problems, the middle one (a copy of problem 0's map with another goal) has no row;
    # outputs and gradient bits equal the two-problem run
    maps3 = np.stack([maps[0], maps[0], maps[1]])
    goals3 = np.stack([goals[0], goals[1], goals[1]])
    of3 = np.where(of == 1, 2, 0).astype(np.int32)
    y3 = net.forward(_t(maps3), _t(goals3), _t(rows), _t(of3, torch.int32), iters)
    for p in net.parameters():
        p.grad = None
    (y3 * _t(dy)).sum().backward()
    g3 = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    net.check_status()
    assert torch.equal(y3.detach(), ya)
    # the rowless problem adds exact zeros to the problem-side sums, so the bits are those of the two-problem run
    assert all(torch.equal(g3[k], ga[k]) for k in ga), [k for k in ga if not torch.equal(g3[k], ga[k])]


def test_a_problem_index_out_of_range_is_reported_and_takes_no_part():
    dim, iters = 7, 1
    net, _ = _net(dim)
    rec = host.load_case(dim)
    maps, goals, rows, of, ptr, actions, values = host.case_inputs(rec, 20)
    dy = np.random.RandomState(5).standard_normal((rows.shape[0] + 2, dim + 1)).astype(np.float32)

    def run(rows_, of_, dy_):
        y = net.forward(_t(maps), _t(goals), _t(rows_), _t(of_, torch.int32), iters)
        for p in net.parameters():
            p.grad = None
        (torch.nan_to_num(y) * _t(dy_)).sum().backward()
        return y.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}

    keep = np.array([i for i in range(rows.shape[0] + 2) if i not in (4, 9)])
    rows_bad = np.insert(rows, [4, 8], rows[:2], axis=0)
    of_bad = np.insert(of, [4, 8], [2, -1]).astype(np.int32)                 # rows 4 and 9 of the longer batch: B and -1
    assert list(np.flatnonzero((of_bad < 0) | (of_bad >= 2))) == [4, 9]
    y_bad, g_bad = run(rows_bad, of_bad, dy)
    with pytest.raises(RuntimeError, match='outside'):
        net.check_status()
    y_ok, g_ok = run(rows_bad[keep], of_bad[keep], dy[keep])
    net.check_status()
    assert torch.isnan(y_bad[[4, 9]]).all()
    assert torch.equal(y_bad[keep], y_ok)
    assert all(torch.equal(g_bad[k], g_ok[k]) for k in g_ok), [k for k in g_ok if not torch.equal(g_bad[k], g_ok[k])]


def test_the_empty_call_and_the_stale_backward():
    dim = 7
    net, _ = _net(dim)
    rec = host.load_case(dim)
    maps, goals, rows, of, ptr, actions, values = host.case_inputs(rec, 1)
    empty = torch.empty(0, net.row, device=DEV)
    y = net.forward(_t(maps), _t(goals), empty, torch.empty(0, dtype=torch.int32, device=DEV), 1)
    assert tuple(y.shape) == (0, dim + 1)
    for p in net.parameters():
        p.grad = None
    y.sum().backward()
    assert all(p.grad is not None and not p.grad.any() for p in net.parameters())
    # no problems and no rows either
    y = net.forward(torch.empty(0, 15, 15, 15, device=DEV), torch.empty(0, net.row, device=DEV), empty,
                    torch.empty(0, dtype=torch.int32, device=DEV), 1)
    assert tuple(y.shape) == (0, dim + 1)
    with pytest.raises(ValueError):
        net.forward(torch.empty(0, 15, 15, 15, device=DEV), torch.empty(0, net.row, device=DEV), _t(rows), _t(of, torch.int32), 1)
    with pytest.raises(RuntimeError):
        net.forward(torch.from_numpy(maps), _t(goals), _t(rows), _t(of, torch.int32), 1)            # a CPU tensor: no fallback
    # backward after a later forward
    y_old = net.forward(_t(maps), _t(goals), _t(rows), _t(of, torch.int32), 1)
    net.forward(_t(maps), _t(goals), _t(rows), _t(of, torch.int32), 1).sum().backward()
    with pytest.raises(RuntimeError, match='later forward'):
        y_old.sum().backward()
    net.check_status()
