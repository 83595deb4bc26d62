"""A from-scratch torch restatement of the NEXT planning network's forward (the PPN of next_model/model2D.py, dim 2 / 3):
conv2d, an explicit LSTM cell and both attentions.  Differentiable, any dtype: the autograd oracle a device backward will be
held to (a test helper like tests/train_ops_host.py, not a fallback).  tests/test_next_train_host.py holds it to
gnnmp.next_model.pb_forward_host / state_forward_host in float64 and to the reference's recorded gradients."""
import numpy as np
import torch
import torch.nn.functional as F

WIDTH, CELLS, LATENT = 15, 225, 64
_SHARE = (0, 2, 4, 6, 8, 10)


def leaves(state_dict, dtype, device='cpu'):
    """The trainable parameters as leaf tensors of ``dtype`` (``attention_s`` is ``attention_g``: listed once).  The tests keep
    them on the CPU."""
    out = {}
    for k, v in state_dict.items():
        if k.startswith('attention_s.'):
            continue
        v = torch.as_tensor(np.asarray(v.detach().cpu() if hasattr(v, 'detach') else v))
        out[k] = v.to(device=device, dtype=dtype).clone().requires_grad_(True)
    return out


def _scaled(x, dim, like):
    s = torch.as_tensor(np.asarray(x, dtype=np.float32)).reshape(-1, dim).to(device=like.device, dtype=like.dtype).clone()
    s[:, -1] = s[:, -1] / 0.4
    return s


def attention(w, s):
    """``s`` [n, dim], last coordinate divided -> (a12 [n, 225] in (row, column) order, a3 [n, 8])."""
    n, dtype = s.shape[0], s.dtype
    rows = torch.arange(CELLS, device=s.device) // WIDTH
    cols = torch.arange(CELLS, device=s.device) % WIDTH
    x = torch.stack([s[:, 0:1].expand(n, CELLS), s[:, 1:2].expand(n, CELLS), cols.to(dtype).expand(n, CELLS),
                     rows.to(dtype).expand(n, CELLS)], dim=-1)
    for li, layer in enumerate(_SHARE):
        wt = w['attention_g.mlp_share.%d.weight' % layer]
        x = x @ wt.reshape(wt.shape[0], -1).T + w['attention_g.mlp_share.%d.bias' % layer]
        if li + 1 < len(_SHARE):
            x = torch.relu(x)
    a12 = torch.softmax(x[:, :, 0], dim=1)
    z = torch.relu(s @ w['attention_g.mlp.0.weight'].T + w['attention_g.mlp.0.bias'])
    a3 = torch.softmax(z @ w['attention_g.mlp.2.weight'].T + w['attention_g.mlp.2.bias'], dim=1)
    return a12, a3


def pb_forward(w, maps, goals, iters=20):
    like = w['hidden.weight']
    dim = w['attention_g.mlp.0.weight'].shape[1]
    maps = torch.as_tensor(np.asarray(maps, dtype=np.float32)).to(device=like.device, dtype=like.dtype).reshape(-1, 1, WIDTH, WIDTH)
    B = maps.shape[0]
    a12, a3 = attention(w, _scaled(goals, dim, like))
    att = (a3[:, :, None] * a12[:, None, :]).reshape(B, 8, WIDTH, WIDTH)
    hl = F.conv2d(torch.cat([maps, att], dim=1), w['hidden.weight'], w['hidden.bias'], padding=1)
    h = F.conv2d(hl, w['h0.weight'], w['h0.bias'], padding=1)
    c = F.conv2d(hl, w['c0.weight'], w['c0.bias'], padding=1)
    for _ in range(int(iters)):
        x = F.conv2d(h, w['conv.weight'], w['conv.bias'], padding=1)
        gates = (torch.einsum('gc,nchw->nghw', w['lstm.weight_ih'], x) + torch.einsum('gc,nchw->nghw', w['lstm.weight_hh'], h)
                 + (w['lstm.bias_ih'] + w['lstm.bias_hh'])[None, :, None, None])
        gi, gf, gg, go = (gates[:, k * LATENT:(k + 1) * LATENT] for k in range(4))
        c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        h = torch.sigmoid(go) * torch.tanh(c)
    return h


def state_forward(w, states, problem_of_state, pb_rep):
    like = w['hidden.weight']
    dim = w['attention_g.mlp.0.weight'].shape[1]
    a12, a3 = attention(w, _scaled(states, dim, like))
    of = torch.as_tensor(np.asarray(problem_of_state, dtype=np.int64)).reshape(-1).to(like.device)
    pb = pb_rep.reshape(-1, 8, 8, CELLS)
    x = torch.einsum('sgcp,sp,sc->sg', pb[of], a12, a3)
    for layer in (0, 2, 4):
        x = x @ w['policy.%d.weight' % layer].T + w['policy.%d.bias' % layer]
        if layer != 4:
            x = torch.relu(x)
    return x


def forward(w, maps, goals, states, problem_of_state, iters=20):
    return state_forward(w, states, problem_of_state, pb_forward(w, maps, goals, iters))


def grads_of(loss, w):
    """{name: numpy gradient} of a scalar ``loss`` with respect to the leaves ``w`` (zeros where nothing flows)."""
    gs = torch.autograd.grad(loss, list(w.values()), allow_unused=True)
    return {k: (np.zeros(tuple(v.shape)) if g is None else g.detach().cpu().numpy().astype(np.float64)) for (k, v), g in zip(w.items(), gs)}


def oracle_pair(state_dict, maps, goals, states, problem_of_state, iters, loss_fn):
    """(loss32, g32, loss64, g64): the restatement in float32 and in float64 with ``loss_fn(y) -> scalar``."""
    out = []
    for dtype in (torch.float32, torch.float64):
        w = leaves(state_dict, dtype)
        loss = loss_fn(forward(w, maps, goals, states, problem_of_state, iters))
        out += [float(loss.detach()), grads_of(loss, w)]
    return tuple(out)


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
