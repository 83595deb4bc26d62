"""The plain-Python restatement of the explorer's training supervision (tests/episodes_host.py) reproduces every
episodes_* fixture recorded from the reference (tools/gen_golden_episodes.py) exactly, and the ctypes mirror of the new
episode struct matches include/gnnmp.h.  CPU only."""
import os
import re

import numpy as np
import pytest

from conftest import golden_files
import episodes_host as H

FILES = golden_files('episodes_')


def load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_fixtures_present():
    names = {os.path.basename(f)[len('episodes_'):-4] for f in FILES}
    assert {'maze2_model', 'maze3_model', 'maze2_ties', 'maze2_zeros', 'maze2_startgoal', 'maze2_cap', 'maze2_empty',
            'maze2_single', 'maze2_dupstart'} <= names


@pytest.mark.parametrize('path', FILES, ids=[os.path.basename(f) for f in FILES])
def test_restatement_matches_fixture(path):
    f = load(path)
    ei = f['edge_index'].astype(np.int64)
    N = f['points'].shape[0]
    free, cost = H.label_edges(f['points'], ei, f['map'])
    assert np.array_equal(free, f['edge_free'])
    assert np.array_equal(cost, f['edge_cost'])                 # bit-exact, +inf where blocked
    goal, start = int(f['goal']), int(f['start'])
    dist, prev, nv = H.shortest_paths(N, ei, cost, goal)
    assert np.array_equal(dist, f['dist']) and np.array_equal(prev, f['prev']) and nv == int(f['n_valid'])
    out = H.episode(N, ei, free, cost, f['scores'], goal, start, lambda step: int(f['replay_step']),
                    max_steps=int(f['max_steps']))
    assert out['status'] == int(f['status'])
    assert out['step'] == int(f['step'])
    assert np.array_equal(out['frontier'], f['frontier'].astype(np.int64))
    assert out['label'] == int(f['label'])


def test_fixture_cases_cover_the_quirks():
    f = {os.path.basename(p)[len('episodes_'):-4]: load(p) for p in FILES}
    assert int(f['maze2_single']['status']) == 1 and int(f['maze2_empty']['status']) == 2
    assert int(f['maze2_startgoal']['start']) == int(f['maze2_startgoal']['goal'])
    assert int(f['maze2_cap']['step']) == int(f['maze2_cap']['max_steps']) - 1
    assert int(f['maze3_model']['dim']) == 3
    z = f['maze2_zeros']['scores']
    assert (z == 0).any() and np.signbit(z[z == 0]).any()
    d = f['maze2_dupstart']
    cl = H._Clone(d['points'].shape[0], d['edge_index'].astype(np.int64), d['scores'], int(d['goal']))
    explored, _, _ = H._rollout(cl, d['edge_free'], int(d['start']), int(d['goal']), int(d['replay_step']), True)
    assert explored.count(int(d['start'])) == 2


def test_episode_struct_mirrors_the_header():
    import gnnmp  # noqa: F401
    from gnnmp import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gnnmp.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    body = re.search(r'typedef struct\s*\{([^{}]*)\}\s*gnnmp_episode_graphs;', text).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            fields.extend([decl.split(',')[0].split()[-1].lstrip('*')] + [x.strip().lstrip('*') for x in decl.split(',')[1:]])
    assert [f[0] for f in _lib.EpisodeGraphs._fields_] == fields


def test_draw_host_follows_the_reference_order():
    """gnnmp.episodes.draw_host makes the reference's numpy calls in its order (train_explorer.py:129, 133, 148, 165, 166-170):
    a goal for every problem, the other three draws only for problems that are not skipped, the replay step only after a
    successful explore -- checked against that sequence written out, with skipped problems of both kinds in the mix."""
    from gnnmp import episodes as ep
    cases = [load(p) for p in FILES if os.path.basename(p) in ('episodes_maze2_single.npz', 'episodes_maze2_empty.npz',
                                                               'episodes_maze2_model.npz', 'episodes_maze2_ties.npz')]
    graphs = []
    for c in cases:
        ei = c['edge_index'].astype(np.int64)
        graphs.append((c['points'].shape[0], ei, c['edge_free'], c['edge_cost'], c['scores']))

    def valid_of(b, goal):
        N, ei, _, cost, _ = graphs[b]
        return np.isfinite(H.shortest_paths(N, ei, cost, goal)[0])

    def step_of(b, goal, loop, start):
        N, ei, free, _, sc = graphs[b]
        step, status = H.explore(N, ei, free, sc, start, goal)
        return None if status else step

    kinds = set()
    for seed in range(6):
        np.random.seed(seed)
        got = ep.draw_host([g[0] for g in graphs], valid_of, step_of, 10)
        np.random.seed(seed)
        want = []
        for b, (N, ei, free, cost, sc) in enumerate(graphs):
            goal_index = np.random.choice(N)
            valid_node = valid_of(b, goal_index)
            if sum(valid_node) == 1:
                want.append((goal_index, None, None, None))
                continue
            current_loop = np.random.randint(1, 10)
            start_index = np.random.choice(np.arange(len(valid_node))[valid_node])
            step = step_of(b, goal_index, current_loop, start_index)
            if step is None:
                want.append((goal_index, current_loop, start_index, None))
                continue
            want.append((goal_index, current_loop, start_index, np.random.randint(0, step + 1)))
        assert [tuple(None if x is None else int(x) for x in w) for w in want] == got
        kinds |= {(w[1] is None, w[3] is None) for w in want}
    assert kinds == {(True, True), (False, True), (False, False)}


def test_frontier_loss_matches_log_softmax_on_fixtures():
    """gnnmp.episodes.frontier_loss (plain torch, so it runs here on CPU tensors) against the reference's expression
    -policy[frontier].log_softmax(0)[next_edge_idx] on every fixture with a frontier, batched, skipped problems included, and
    its gradient against autograd through that expression."""
    import torch
    from gnnmp import episodes as ep
    cs = [load(p) for p in FILES]
    eptr = np.concatenate([[0], np.cumsum([c['edge_index'].shape[1] for c in cs])])
    E, B = int(eptr[-1]), len(cs)
    frontier = torch.full((2 * E + B,), 123456789, dtype=torch.int32)          # junk beyond each problem's list
    for b, c in enumerate(cs):
        off = 2 * int(eptr[b]) + b
        frontier[off:off + len(c['frontier'])] = torch.from_numpy(c['frontier'].astype(np.int64) + int(eptr[b]))
    fr = {'frontier': frontier, 'frontier_len': torch.tensor([len(c['frontier']) for c in cs], dtype=torch.int32),
          'label': torch.tensor([int(c['label']) for c in cs], dtype=torch.int32),
          'status': torch.tensor([int(c['status']) for c in cs], dtype=torch.int32),
          'edge_ptr': torch.from_numpy(eptr.astype(np.int32)), 'total_edges': E}
    scores = torch.from_numpy(np.concatenate([c['scores'] for c in cs])).requires_grad_(True)
    losses, ok = ep.frontier_loss(scores, fr)
    ref = []
    for b, c in enumerate(cs):
        if int(c['status']) != 0:
            ref.append(torch.zeros(()))
            continue
        ids = torch.from_numpy(c['frontier'].astype(np.int64) + int(eptr[b]))
        ref.append(-scores[ids].log_softmax(dim=0)[int(c['label'])])
    ref = torch.stack(ref)
    assert ok.tolist() == [int(c['status']) == 0 for c in cs]
    assert bool(((losses - ref).abs() <= 1e-6 * ref.abs().clamp(min=1.0)).all())
    g1, = torch.autograd.grad(losses.sum(), scores)
    g2, = torch.autograd.grad(ref.sum(), scores)
    assert float((g1 - g2).abs().max()) <= 1e-5 * float(g2.abs().max()) + 1e-7
