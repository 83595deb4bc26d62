"""A from-scratch torch restatement of the 3-D NEXT planning network's forward (the PPN of next_model/model3D.py, the arm
families): conv3d, an explicit LSTM cell and both attentions.  Differentiable, any dtype, any iters: the autograd oracle the
device backward is held to (a test helper like tests/next_train_host.py, not a fallback).  tests/test_next3d_train_host.py holds
it to gnnmp.next_model3d.pb_forward_host / state_forward_host in float64 and to the reference's recorded gradients."""
import os

import numpy as np
import torch
import torch.nn.functional as F

WIDTH, VOXELS, LATENT = 15, 3375, 64
_SHARE = (0, 2, 4, 6, 8, 10)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FAMILIES = {7: ('next_7', 3), 14: ('next_14', 6)}
RECORDED_ITERS = {7: (0, 1, 2, 20), 14: (1, 20)}


def leaves(state_dict, dtype, device='cpu'):
    """The trainable parameters as leaf tensors of ``dtype`` (``attention_s`` is ``attention_g``: listed once)."""
    out = {}
    for k, v in state_dict.items():
        if k.startswith('attention_s.'):
            continue
        v = torch.as_tensor(np.asarray(v.detach().cpu() if hasattr(v, 'detach') else v))
        out[k] = v.to(device=device, dtype=dtype).clone().requires_grad_(True)
    return out


def _rows(x, like, width):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).reshape(-1, width).to(device=like.device, dtype=like.dtype)


def attention(w, inp):
    """``inp`` [n, point_dim + dim] -> (a123 [n, 3375] in (i, j, k) order, a3 [n, 8]).  Voxel (i, j, k) enters the shared MLP as
    ``[point, j, i, k]``."""
    n, dtype = inp.shape[0], inp.dtype
    pd = w['attention_g.mlp_share.0.weight'].shape[1] - 3
    v = torch.arange(VOXELS, device=inp.device)
    i, j, k = v // (WIDTH * WIDTH), (v // WIDTH) % WIDTH, v % WIDTH
    x = torch.cat([inp[:, None, :pd].expand(n, VOXELS, pd),
                   torch.stack([j, i, k], dim=-1).to(dtype)[None].expand(n, VOXELS, 3)], dim=-1)
    for li, layer in enumerate(_SHARE):
        wt = w['attention_g.mlp_share.%d.weight' % layer]
        x = x @ wt.reshape(wt.shape[0], -1).T + w['attention_g.mlp_share.%d.bias' % layer]
        if li + 1 < len(_SHARE):
            x = torch.relu(x)
    a123 = torch.softmax(x[:, :, 0], dim=1)
    z = torch.relu(inp[:, pd:] @ w['attention_g.mlp.0.weight'].T + w['attention_g.mlp.0.bias'])
    a3 = torch.softmax(z @ w['attention_g.mlp.2.weight'].T + w['attention_g.mlp.2.bias'], dim=1)
    return a123, a3


def pb_forward(w, maps, goal_rows, iters=20):
    like = w['hidden.weight']
    width = w['attention_g.mlp.0.weight'].shape[1] + w['attention_g.mlp_share.0.weight'].shape[1] - 3
    maps = torch.as_tensor(np.asarray(maps, dtype=np.float32)).to(device=like.device, dtype=like.dtype).reshape(-1, 1, WIDTH, WIDTH, WIDTH)
    B = maps.shape[0]
    a123, a3 = attention(w, _rows(goal_rows, like, width))
    att = (a3[:, :, None] * a123[:, None, :]).reshape(B, 8, WIDTH, WIDTH, WIDTH)
    hl = F.conv3d(torch.cat([maps, att], dim=1), w['hidden.weight'], w['hidden.bias'], padding=1)
    h = F.conv3d(hl, w['h0.weight'], w['h0.bias'], padding=1)
    c = F.conv3d(hl, w['c0.weight'], w['c0.bias'], padding=1)
    for _ in range(int(iters)):
        x = F.conv3d(h, w['conv.weight'], w['conv.bias'], padding=1)
        gates = (torch.einsum('gc,ncijk->ngijk', w['lstm.weight_ih'], x) + torch.einsum('gc,ncijk->ngijk', w['lstm.weight_hh'], h)
                 + (w['lstm.bias_ih'] + w['lstm.bias_hh'])[None, :, None, None, None])
        gi, gf, gg, go = (gates[:, q * LATENT:(q + 1) * LATENT] for q in range(4))
        c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        h = torch.sigmoid(go) * torch.tanh(c)
    return h


def state_forward(w, rows, problem_of_state, pb_rep):
    like = w['hidden.weight']
    width = w['attention_g.mlp.0.weight'].shape[1] + w['attention_g.mlp_share.0.weight'].shape[1] - 3
    a123, a3 = attention(w, _rows(rows, like, width))
    of = torch.as_tensor(np.asarray(problem_of_state, dtype=np.int64)).reshape(-1).to(like.device)
    pb = pb_rep.reshape(-1, 8, 8, VOXELS)
    x = torch.einsum('sgcp,sp,sc->sg', pb[of], a123, a3)
    for layer in (0, 2, 4):
        x = x @ w['policy.%d.weight' % layer].T + w['policy.%d.bias' % layer]
        if layer != 4:
            x = torch.relu(x)
    return x


def forward(w, maps, goal_rows, rows, problem_of_state, iters=20):
    return state_forward(w, rows, problem_of_state, pb_forward(w, maps, goal_rows, iters))


def grads_of(loss, w):
    """{name: numpy gradient} of a scalar ``loss`` with respect to the leaves ``w`` (zeros where nothing flows)."""
    gs = torch.autograd.grad(loss, list(w.values()), allow_unused=True)
    return {k: (np.zeros(tuple(v.shape)) if g is None else g.detach().cpu().numpy().astype(np.float64)) for (k, v), g in zip(w.items(), gs)}


def check_bar(got, g32, g64, label, verbose=True):
    """The project's gradient bar (tests/test_explorer_autograd_gpu.py): per parameter tensor
    ``|g - g64| <= max(1e-4 max|g64|, 4 own) + 1e-6`` with ``own = max|g32 - g64|``.  Prints error / bar per tensor; returns the
    list of failing names."""
    bad = []
    for k in g64:
        g = np.asarray(got[k].detach().cpu() if hasattr(got[k], 'detach') else got[k], dtype=np.float64)
        own = np.abs(g32[k] - g64[k]).max()
        bar = max(1e-4 * np.abs(g64[k]).max(), 4 * own) + 1e-6
        err = np.abs(g - g64[k]).max()
        if verbose:
            print('%-22s %-34s max|g64| %.3e  own %.3e  err %.3e  bar %.3e  err/bar %.3f'
                  % (label, k, np.abs(g64[k]).max(), own, err, bar, err / bar))
        if not err <= bar:
            bad.append((k, err, bar))
    return bad


# ---- the recorded fixtures (tools/gen_golden_next3d_train.py)
def load_weights(dim):
    from gnnmp.next_model3d import load_npz_weights
    stem = os.path.join(GOLDEN, FAMILIES[dim][0] + '_weights')
    paths = [stem + '.npz'] + ([stem + '_b.npz'] if os.path.exists(stem + '_b.npz') else [])
    return load_npz_weights(*paths)


def load_case(dim):
    """The recorded inputs, labels and losses of a family as a dict of arrays."""
    with np.load(os.path.join(GOLDEN, 'next3d_train_kuka%d.npz' % dim)) as f:
        return {k: f[k] for k in f.files}


def load_grads(dim, iters):
    """(g32, g64) of a recorded case: the files are split by parameter name, the float64 set is g32 + the stored difference."""
    g32, d64 = {}, {}
    for part in 'abcdefgh':
        for kind, into in (('g32', g32), ('d64', d64)):
            path = os.path.join(GOLDEN, 'next3d_train_kuka%d_i%d_%s_%s.npz' % (dim, iters, kind, part))
            if os.path.exists(path):
                with np.load(path) as f:
                    into.update({k: f[k] for k in f.files})
    assert g32 and set(g32) == set(d64), 'next3d_train_kuka%d_i%d: fixture files missing' % (dim, iters)
    return ({k: v.astype(np.float64) for k, v in g32.items()}, {k: g32[k].astype(np.float64) + d64[k].astype(np.float64) for k in g32})


def case_inputs(rec, iters):
    """(maps, goal_rows, rows, problem_of_state, ptr, actions, values) of the recorded case at ``iters``: the 20-round cases hold
    both problems, the others problem 0 alone."""
    npb = 2 if iters == 20 else 1
    ptr = rec['path_ptr'][:npb + 1].astype(np.int64)
    n = int(ptr[-1])
    of = np.repeat(np.arange(npb, dtype=np.int32), np.diff(ptr))
    return (rec['maps'][:npb].astype(np.float32), rec['goals'][:npb], rec['rows'][:n], of, ptr,
            rec['actions'][:n].astype(np.float32), rec['values'][:n].astype(np.float32))
