"""Bit fingerprint of the training calls, for comparing two builds of the library (a refactor must not move a bit):
one line per tensor -- case, tensor name, sha256 of its fp32 bytes -- for the scores or output path, every parameter
gradient and, for the smoother, the BatchNorm running statistics the call updated; and per case the value of the matching
*_workspace_bytes call.  Run it in two checkouts with their own builds and diff the outputs:

    python tools/diag/train_bits.py > bits.txt

Cases: the smallest shapes where the row bookkeeping of the training path can go wrong (one graph below a tile, several
graphs across tiles, a loop count past TRAIN_BATCH_MAX_LOOP on the uniform call, ragged loop counts in caller order, the
smoother at loop 0 and on the ragged problems of tests/test_smoother_train_batch_gpu.py)."""
import ctypes
import hashlib
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
import gnnmp  # noqa: E402
from gnnmp import _lib  # noqa: E402
from gnnmp.smoother import SmoothBatch, _cbatch  # noqa: E402
from gnnmp.synth import ENVS, synth_graph  # noqa: E402
from gnnmp.weights import load_weights  # noqa: E402

DEV = 'cuda:0'
RAGGED_SIZES, RAGGED_LOOPS = (33, 64, 257, 100, 40), (2, 5, 1, 5, 3)       # tests/test_explorer_train_batch_gpu.py


def sha(t):
    return hashlib.sha256(t.detach().float().contiguous().cpu().numpy().tobytes()).hexdigest()


def report(case, out, named, ws_bytes):
    print('%s workspace_bytes %d' % (case, ws_bytes))
    print('%s out %s' % (case, sha(out)))
    for n, t in named:
        print('%s %s %s' % (case, n, sha(t)))
    sys.stdout.flush()


def explorer_case(case, env, sizes, k, seed0, loops, use_obstacles=True):
    """``loops``: an int -> train_scores, a sequence -> train_scores_batch.  Loss: sum(coef * scores), coef ~ N(0, 1)."""
    e = ENVS[env]
    m = gnnmp.EncoderProcessDecoder(e['workspace'], e['C'], e['d'], e['S'], use_obstacles=use_obstacles)
    m.load_state_dict(load_weights(e['ckpt']), strict=True)
    m.train()
    graphs = [synth_graph(env, n, k, seed=seed0 + i) for i, n in enumerate(sizes)]
    b = gnnmp.GraphBatch.from_graphs(graphs, e['S'], DEV)
    coef = torch.randn(b.total_edges, generator=torch.Generator().manual_seed(7), dtype=torch.float64).float().to(DEV)
    h, cb, need = m._native(DEV), m._cbatch(b), ctypes.c_size_t()
    if isinstance(loops, int):
        _lib.check(_lib.lib().gnnmp_explorer_train_workspace_bytes(h, ctypes.byref(cb), loops, ctypes.byref(need)), case)
        s = m.train_scores(b, loops)
    else:
        # the library takes the graphs longest loop first; the workspace depends on the batch's totals and max(loops) only
        order = sorted(range(len(sizes)), key=lambda g: -loops[g])
        host = [_lib.i32_array([x[g] for g in order]) for x in (loops, sizes, [g['edge_index'].shape[1] for g in graphs])]
        _lib.check(_lib.lib().gnnmp_explorer_train_batch_workspace_bytes(h, ctypes.byref(cb), *host, ctypes.byref(need)), case)
        s = m.train_scores_batch(b, list(loops))
    (s * coef).sum().backward()
    report(case, s, [(n, p.grad) for n, p in m.named_parameters() if p.grad is not None], need.value)


def smoother_problem(gen, C, P, F, Co, loop):
    """tests/test_smoother_autograd_scale_gpu.py _problem at lim = 1 (same draws in the same order), chain edges + self loops."""
    box = lambda n: (torch.rand(n, C, generator=gen, dtype=torch.float64) * 2 - 1).float()   # noqa: E731
    path, free, coll = box(P), box(F), box(Co)
    a, c = torch.arange(1, P), torch.arange(0, P - 1)
    ei = torch.cat((torch.stack((a, c)), torch.stack((c, a)), torch.stack((torch.arange(P),) * 2)), dim=1)
    return dict(path=path, free=free, collided=coll, edge_index=ei, loop=loop, target=box(P))


def smoother_case(case, probs, batched):
    m = gnnmp.ModelSmoother(workspace_size=3, config_size=2, embed_size=128, obs_size=6, scale=1.0)
    m.load_state_dict(load_weights('smooth_2d_attv3'), strict=True)
    m.train()
    sb = SmoothBatch([q['path'] for q in probs], [q['free'] for q in probs], [q['collided'] for q in probs],
                     [q['edge_index'] for q in probs], DEV)
    loops = [q['loop'] for q in probs]
    h, cb, need = m._native(DEV, for_training=True), _cbatch(sb), ctypes.c_size_t()
    if batched:
        order = sorted(range(len(probs)), key=lambda i: -loops[i])       # sizes do not depend on the problems' order
        _lib.check(_lib.lib().gnnmp_smoother_train_batch_workspace_bytes(h, ctypes.byref(cb), _lib.i32_array([loops[i] for i in order]),
                                                                         ctypes.byref(need)), case)
        out = m.forward_train_batch(sb, loops)
    else:
        q = probs[0]
        _lib.check(_lib.lib().gnnmp_smoother_train_workspace_bytes(h, ctypes.byref(cb), loops[0], ctypes.byref(need)), case)
        out = m.forward_train(path=q['path'].to(DEV), free=q['free'].to(DEV), collided=q['collided'].to(DEV),
                              edge_index=q['edge_index'].to(DEV), loop=loops[0])
    coef = torch.randn(out.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64).float().to(DEV)
    (out * coef).sum().backward()
    bn = m.node_code[1]
    named = [(n, p.grad) for n, p in m.named_parameters() if p.grad is not None]
    named += [('bn.running_mean', bn.running_mean), ('bn.running_var', bn.running_var), ('bn.num_batches_tracked', bn.num_batches_tracked)]
    report(case, out, named, need.value)


def main():
    big = _lib.TRAIN_BATCH_MAX_LOOP + 1
    explorer_case('explorer.uniform.maze2.N33.loop1', 'maze2', (33,), 4, 100, 1)
    explorer_case('explorer.uniform.maze2.N40-64-130.loop3', 'maze2', (40, 64, 130), 4, 100, 3)
    explorer_case('explorer.uniform.maze2.N33.loop%d' % big, 'maze2', (33,), 4, 100, big)
    explorer_case('explorer.uniform.kuka7.N33-257.loop2.obstacles', 'kuka7', (33, 257), 4, 300, 2, True)
    explorer_case('explorer.uniform.kuka7.N33-257.loop2.no-obstacles', 'kuka7', (33, 257), 4, 300, 2, False)
    explorer_case('explorer.batch.maze2.ragged', 'maze2', RAGGED_SIZES, 4, 200, RAGGED_LOOPS)
    explorer_case('explorer.batch.kuka7.ragged', 'kuka7', RAGGED_SIZES, 4, 200, RAGGED_LOOPS)
    for loop in (2, 0):
        gen = torch.Generator().manual_seed(5)
        smoother_case('smoother.one.P33.loop%d' % loop, [smoother_problem(gen, 2, 33, 60, 40, loop)], False)
    gen = torch.Generator().manual_seed(2)                               # RAGGED_SEED and ragged() of the batch test
    probs = [smoother_problem(gen, 2, P, F, Co, loop) for P, F, Co, loop in ((2, 50, 30, 3), (3, 4, 3, 1), (33, 60, 1, 4), (12, 40, 25, 2))]
    smoother_case('smoother.batch.ragged', probs, True)
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
