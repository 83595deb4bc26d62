"""gnnmp_episode_frontier_loss (gnnmp.explorer_replay.frontier_loss): train_explorer.py:172 and its gradient on the device.

    loss      |loss - l64| <= max(1e-4 |l64|, 4 |l32 - l64|) + 1e-6, l64 = frontier_loss_reference (float64 torch on the same
              float32 scores), l32 = the existing episodes.frontier_loss
    gradient  max |g - g64| <= max(1e-4 max |g64|, 4 own) + 1e-6, g64 float64 autograd, own = max |g32 - g64| of the torch
              float32 gradient
    dscores exactly 0 outside the frontiers and over the whole edge range of a problem that is not counted; a frontier of one
    entry gives loss and gradient exactly 0; two runs give the same bits; a score of 1000 outside every frontier changes nothing

Hand-made frontiers: lengths 1, 2, 63, 64, 65 (around one pass of the wave) and 1000 (several passes), the label at the first
and at the last position, one edge listed twice, one problem each with status != 0, frontier_len == 0 and label == -1; B = 1
and B = 70; scores over [-32, 12].  Then a real pipeline of 6 problems against episodes.frontier_loss."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import episodes as ep
from gnnmp import explorer_replay as er

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GARBAGE = 2 ** 30                       # what the unused slots of `frontier` hold
# (frontier length, label position: 'first' / 'last' / 'mid', kind)
MAIN = [(1, 'first', 'ok'), (2, 'last', 'ok'), (63, 'first', 'ok'), (64, 'last', 'ok'), (65, 'mid', 'ok'), (1000, 'last', 'ok'),
        (40, 'first', 'twice'), (9, 'mid', 'status'), (9, 'mid', 'empty'), (9, 'mid', 'nolabel'), (1000, 'first', 'twice')]
_CASES = {}


def _spec(name):
    if name == 'main':
        return MAIN, 1.0
    if name == 'B1':
        return [(65, 'mid', 'twice')], 1.0
    rng = np.random.RandomState(70)
    kinds = ['ok', 'ok', 'ok', 'twice', 'ok', 'status', 'ok', 'empty', 'ok', 'nolabel']
    return [(int(rng.randint(1, 131)), ['first', 'last', 'mid'][i % 3], kinds[i % len(kinds)]) for i in range(70)], 8.0


def _case(name):
    """The frontier dict, the scores, and the float64 / float32 torch values, computed once and left unchanged."""
    if name in _CASES:
        return _CASES[name]
    spec, divisor = _spec(name)
    rng = np.random.RandomState(len(spec))
    B = len(spec)
    counts = [n + 7 for n, _, _ in spec]                         # edges per problem: a few are in no frontier
    eptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    E = int(eptr[-1])
    frontier = np.full(2 * E + B, GARBAGE, dtype=np.int64)
    flen, label, status = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    listed = np.zeros(E, dtype=bool)
    outside = None
    for b, (n, where, kind) in enumerate(spec):
        ids = eptr[b] + rng.permutation(counts[b])[:n]
        if kind == 'twice' and n > 1:
            ids[n // 2] = ids[0]                                  # one edge listed twice
        frontier[2 * eptr[b] + b:2 * eptr[b] + b + n] = ids
        flen[b], label[b] = n, {'first': 0, 'last': n - 1, 'mid': n // 2}[where]
        if kind == 'status':
            status[b] = 2
        elif kind == 'empty':
            flen[b] = 0
        elif kind == 'nolabel':
            label[b] = -1
        else:
            listed[ids] = True
        if outside is None and kind in ('ok', 'twice'):
            outside = int(np.setdiff1d(np.arange(eptr[b], eptr[b + 1]), ids)[0])      # an edge of a counted problem in no frontier
    scores = torch.from_numpy(rng.uniform(-32.0, 12.0, E).astype(np.float32))
    i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).to(DEV)          # noqa: E731
    fr = {'frontier': i32(frontier), 'frontier_len': i32(flen), 'label': i32(label), 'status': i32(status), 'edge_ptr': i32(eptr),
          'total_edges': E}
    s64 = scores.to(DEV).double().requires_grad_(True)
    l64, t64, c64 = er.frontier_loss_reference(s64, fr, divisor)
    g64, = torch.autograd.grad(l64, s64)
    s32 = scores.to(DEV).requires_grad_(True)
    t32, ok32 = ep.frontier_loss(s32, fr)
    l32 = t32.sum() / divisor
    g32, = torch.autograd.grad(l32, s32)
    _CASES[name] = dict(spec=spec, divisor=divisor, eptr=eptr, fr=fr, scores=scores, listed=torch.from_numpy(listed).to(DEV),
                        outside=outside, l64=float(l64.detach()), t64=t64.detach(), c64=c64, g64=g64, l32=float(l32.detach()),
                        own=float((g32.double() - g64).abs().max()), ok32=ok32)
    return _CASES[name]


@pytest.mark.parametrize('name', ['main', 'B1', 'B70'])
def test_loss_and_gradient_against_float64(name):
    c = _case(name)
    scores = c['scores'].to(DEV).requires_grad_(True)
    loss, terms, counted = er.frontier_loss(scores, c['fr'], c['divisor'], return_terms=True)
    assert loss.dtype == torch.float32 and loss.shape == () and terms.dtype == torch.float32 and not terms.requires_grad
    assert counted.dtype == torch.bool and torch.equal(counted, c['c64']) and torch.equal(counted, c['ok32'])
    err, bar = abs(float(loss.detach()) - c['l64']), max(1e-4 * abs(c['l64']), 4 * abs(c['l32'] - c['l64'])) + 1e-6
    print('\n%s: loss %.9e, float64 %.9e, float32 torch %.9e, err %.2e, bar %.2e' % (name, float(loss.detach()), c['l64'], c['l32'], err, bar))
    assert err <= bar
    terr = float((terms.double() - c['t64']).abs().max())
    print('%s: terms max err %.2e against float64 (largest term %.3e)' % (name, terr, float(c['t64'].abs().max())))
    assert bool(((terms.double() - c['t64']).abs() <= 1e-6 * c['t64'].abs().clamp(min=1.0)).all())
    loss.backward()
    g = scores.grad
    gerr = float((g.double() - c['g64']).abs().max())
    gbar = max(1e-4 * float(c['g64'].abs().max()), 4 * c['own']) + 1e-6
    print('%s: gradient max err %.2e, own (torch float32) %.2e, bar %.2e' % (name, gerr, c['own'], gbar))
    assert gerr <= gbar
    assert not g[~c['listed']].any()                              # exactly 0 outside the frontiers
    for b, (n, _, kind) in enumerate(c['spec']):
        e0, e1 = int(c['eptr'][b]), int(c['eptr'][b + 1])
        if kind in ('status', 'empty', 'nolabel'):
            assert float(terms[b]) == 0.0 and not bool(counted[b]) and not g[e0:e1].any(), b
        elif n == 1:
            assert float(terms[b]) == 0.0 and bool(counted[b]) and not g[e0:e1].any(), b
    # the upstream gradient scales dscores; two runs give the same bits
    t1, c1, l1, d1, bad = er.frontier_loss_device(scores.detach(), c['fr'], c['divisor'])
    t2, c2, l2, d2, _ = er.frontier_loss_device(scores.detach(), c['fr'], c['divisor'])
    assert torch.equal(t1, t2) and torch.equal(c1, c2) and torch.equal(l1, l2) and torch.equal(d1, d2)
    assert torch.equal(t1, terms) and torch.equal(l1.reshape(()), loss.detach()) and torch.equal(d1, g)
    s2 = scores.detach().clone().requires_grad_(True)
    (er.frontier_loss(s2, c['fr'], c['divisor']) * 2.5).backward()
    assert torch.equal(s2.grad, d1 * torch.tensor(2.5, device=DEV))
    er.check_loss_status(bad)
    # a score of 1000 outside every frontier changes nothing
    far = scores.detach().clone()
    far[c['outside']] = 1000.0
    t3, c3, l3, d3, _ = er.frontier_loss_device(far, c['fr'], c['divisor'])
    assert torch.equal(t3, t1) and torch.equal(c3, c1) and torch.equal(l3, l1) and torch.equal(d3, d1)


def test_entry_outside_its_problem_is_reported_and_contributes_nothing():
    c = _case('main')
    fr = dict(c['fr'])
    frontier = fr['frontier'].clone()
    b = 3                                                         # 64 entries, the label at the last one
    off = 2 * int(c['eptr'][b]) + b
    frontier[off + 5] = int(c['eptr'][b + 1])                     # the next problem's first edge
    fr['frontier'] = frontier
    scores = c['scores'].to(DEV)
    terms, counted, loss, dscores, bad = er.frontier_loss_device(scores, fr, 1.0)
    short = dict(fr)
    lst = torch.cat([frontier[off:off + 5], frontier[off + 6:off + 64]])
    f2 = c['fr']['frontier'].clone()
    f2[off:off + 63] = lst
    short['frontier'] = f2
    short['frontier_len'] = c['fr']['frontier_len'].clone()
    short['frontier_len'][b] = 63
    short['label'] = c['fr']['label'].clone()
    short['label'][b] = 62
    l64, t64, _ = er.frontier_loss_reference(scores.double(), short, 1.0)
    assert abs(float(terms[b]) - float(t64[b])) <= 1e-6 * max(abs(float(t64[b])), 1.0) and bool(counted[b])
    assert float(dscores[int(c['eptr'][b + 1])]) == float(er.frontier_loss_device(scores, c['fr'], 1.0)[3][int(c['eptr'][b + 1])])
    with pytest.raises(RuntimeError, match='bad 1'):
        er.check_loss_status(bad)


def test_real_pipeline_matches_the_torch_loss():
    from test_episodes_gpu import draws, random_batch, run_pipeline
    rng0 = np.random.default_rng(8)
    g, pts, maps, scores, rng = random_batch(2, rng0.integers(100, 201, 6).tolist(), 16)
    goal, start, replay = draws(g, rng, unreachable_every=1000)
    paths, step, status, fr = run_pipeline(g, scores, goal, start, 1000, replay)
    sc = scores.clone()
    sc[0] = 1000.0
    ref, ok = ep.frontier_loss(sc, fr)
    loss, terms, counted = er.frontier_loss(sc.clone().requires_grad_(True), fr, return_terms=True)
    assert bool(ok.any()) and torch.equal(counted, ok)
    print('\nterms %s\ntorch %s' % (terms.tolist(), ref.tolist()))
    assert bool(((terms - ref).abs() <= 1e-6 * ref.abs().clamp(min=1.0)).all())
    assert bool(torch.isfinite(loss))
