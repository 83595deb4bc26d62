"""Host side of tests/test_train_ops_gpu.py: float64 restatements of the training operators (train_kernels.hip), the
rounding bound of an fp32 sum, the ragged test batch and the invariants of the padded geometry.  No GPU needed here.

The bound: with u = 2^-24, an fp32 sum of n products in ANY order, fused or not, obeys |err| <= gamma_n * sum |a_i| |b_i|,
gamma_n = (2n + 2) u / (1 - (2n + 2) u) (n multiplications and n additions, one rounding each, plus the final rounding and
one spare).  A `+=` onto an old value adds u |old|."""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    t = (2 * n + 2) * U
    return t / (1 - t)


# ---- the GEMM trio -----------------------------------------------------------------------------------------------
def linear_ref(X, W, b, relu):
    X, W = X.astype(np.float64), W.astype(np.float64)
    y = X @ W.T
    mag = np.abs(X) @ np.abs(W).T
    if b is not None:
        y = y + b.astype(np.float64)
        mag = mag + np.abs(b.astype(np.float64))
    if relu:
        y = np.maximum(y, 0)                                       # 1-Lipschitz: the bound of the pre-activation holds
    return y, gamma(X.shape[1]) * mag


def linear_dx_ref(dY, W, dX_old):
    dY, W = dY.astype(np.float64), W.astype(np.float64)
    y, bound = dY @ W, gamma(dY.shape[1]) * (np.abs(dY) @ np.abs(W))
    if dX_old is not None:
        y, bound = y + dX_old, bound + U * np.abs(dX_old.astype(np.float64))
    return y, bound


def linear_dw_ref(dY, X, dW_old, db_old):
    dY, X = dY.astype(np.float64), X.astype(np.float64)
    g = gamma(dY.shape[0])
    dW = dW_old.astype(np.float64) + dY.T @ X
    bW = g * (np.abs(dY).T @ np.abs(X)) + U * np.abs(dW_old.astype(np.float64))
    if db_old is None:
        return dW, bW, None, None
    db = db_old.astype(np.float64) + dY.sum(0)
    bb = g * np.abs(dY).sum(0) + U * np.abs(db_old.astype(np.float64))
    return dW, bW, db, bb


# the dispatch the launchers are documented to have (train_kernels.hip): pinned by the tests
def expected_path(op, K, O):
    mfma = {'LINEAR': O >= 8, 'LINEAR_DX': O >= 8 and K >= 8, 'LINEAR_DW': O >= 8 and K >= 4}[op]
    return 'mfma' if mfma else 'plain'


MODEL_PAIRS = [(4, 32), (8, 32), (14, 64), (28, 64), (56, 64), (32, 32), (64, 32), (96, 32), (128, 32), (160, 32), (320, 64), (5, 128),
               (9, 128), (17, 128), (128, 128), (384, 128), (128, 2), (128, 7), (128, 13), (128, 14), (32, 1), (64, 1)]
BOUNDARY_PAIRS = [(k, o) for k in (1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64) for o in (1, 7, 8, 9, 31, 32, 33)]
ROWS = (1, 31, 32, 33, 127, 128, 129, 257, 1025)
# every R meets these pairs (both sides of every dispatch threshold, K % 32 == 0 and != 0, K % 4 == 0 and != 0, pair groups that
# end mid-group and on a group boundary, the widest layer) ...
PAIRS_FOR_EVERY_R = [(1, 1), (3, 8), (4, 8), (7, 9), (8, 7), (31, 33), (32, 32), (33, 31), (14, 64), (96, 32), (128, 13), (384, 128)]
# ... and every pair meets these R (one row, a partly filled tile, one row into the second 128-row chunk, two chunks and one row)
ROWS_FOR_EVERY_PAIR = (1, 33, 129, 257)


def gemm_cases():
    seen, out = set(), []
    for R in ROWS:
        for K, O in PAIRS_FOR_EVERY_R:
            out.append((R, K, O))
    for K, O in MODEL_PAIRS + BOUNDARY_PAIRS:
        for R in ROWS_FOR_EVERY_PAIR:
            out.append((R, K, O))
    return [c for c in out if not (c in seen or seen.add(c))]


# ---- BatchNorm (training mode) -----------------------------------------------------------------------------------
BN_EPS = 1e-5


def bn_ref(x, gamma_, beta, relu, dy, dgamma_old, dbeta_old):
    """float64: y, (mean, invstd, unbiased variance -- the biased one when N == 1, the kernel's rule), dx, dgamma, dbeta."""
    x, g, b, dy = (a.astype(np.float64) for a in (x, gamma_, beta, dy))
    N = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    invstd = 1.0 / np.sqrt(var + BN_EPS)
    xhat = (x - mean) * invstd
    y = xhat * g + b
    if relu:
        y = np.maximum(y, 0)
    unb = ((x - mean) ** 2).sum(0) / (N - 1) if N > 1 else var
    s0, s1 = dy.sum(0), (dy * xhat).sum(0)
    dx = g * invstd / N * (N * dy - s0 - xhat * s1)
    return dict(y=y, mean=mean, invstd=invstd, var=unb, dx=dx, dgamma=dgamma_old.astype(np.float64) + s1,
                dbeta=dbeta_old.astype(np.float64) + s0)


def bn_torch32(x, gamma_, beta, relu, dy, dgamma_old, dbeta_old):
    """The same through torch's float32 CPU batch norm, forward and autograd (the reference pair's other half)."""
    import torch
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    gt = torch.from_numpy(gamma_.copy()).requires_grad_(True)
    bt = torch.from_numpy(beta.copy()).requires_grad_(True)
    y, mean, invstd = torch.native_batch_norm(xt, gt, bt, None, None, True, 0.1, BN_EPS)
    y.backward(torch.from_numpy(dy.copy()))
    N = x.shape[0]
    var = xt.detach().var(0, unbiased=True) if N > 1 else xt.detach().var(0, unbiased=False)
    yo = torch.relu(y.detach()) if relu else y.detach()
    return dict(y=yo.numpy(), mean=mean.detach().numpy(), invstd=invstd.detach().numpy(), var=var.numpy(), dx=xt.grad.numpy(),
                dgamma=(torch.from_numpy(dgamma_old) + gt.grad).numpy(), dbeta=(torch.from_numpy(dbeta_old) + bt.grad).numpy())


def bn_inputs(kind, N, D, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D)).astype(np.float32)
    if kind == 'cancel':                                          # mean 1e3, standard deviation 1e-2
        x = (1e3 + 1e-2 * x.astype(np.float64)).astype(np.float32)
    return dict(x=x, gamma=(1 + 0.5 * rng.standard_normal(D)).astype(np.float32), beta=rng.standard_normal(D).astype(np.float32),
                dy=rng.standard_normal((N, D)).astype(np.float32), dgamma_old=rng.standard_normal(D).astype(np.float32),
                dbeta_old=rng.standard_normal(D).astype(np.float32))


BN_TENSORS = ('y', 'mean', 'invstd', 'var', 'dx', 'dgamma', 'dbeta')
BN_D = (1, 32, 128)
BN_N = (1, 2, 255, 256, 257, 2100)
# The unit-scale inputs are held to 1e-5 * scale + 1e-6 with no `own` term where the batch variance is about 1.  With one row
# the variance is 0 and with two it is (x0 - x1)^2 / 4: invstd reaches 1 / sqrt(eps) = 316, y and dx are differences of nearly
# equal numbers times that factor, and the float32 reference itself misses 1e-5 * scale (3e-5 .. 2e-4 measured on the CPU
# pair).  Those two sizes keep the general bar max(1e-4 scale, 4 own) + 1e-6.
BN_TIGHT_N = (255, 256, 257, 2100)


def bn_pair(kind, N, D, relu):
    inp = bn_inputs(kind, N, D, seed=1000 * N + 10 * D + relu + (7 if kind == 'cancel' else 0))
    args = (inp['x'], inp['gamma'], inp['beta'], relu, inp['dy'], inp['dgamma_old'], inp['dbeta_old'])
    r64, r32 = bn_ref(*args), bn_torch32(*args)
    own = {k: float(np.max(np.abs(r32[k].astype(np.float64) - r64[k]))) for k in BN_TENSORS}
    scale = {k: float(np.max(np.abs(r64[k]))) for k in BN_TENSORS}
    return inp, r64, own, scale


# ---- the ragged batch of the geometry operators -------------------------------------------------------------------
def ragged_batch(C, seed):
    """Six graphs: a hub with 70 incoming and 70 outgoing edges; every edge three times; isolated nodes; no edges; one node
    with self loops; 257 nodes.  In every graph with >= 3 nodes two rows equal the goal exactly (the lower index must win)."""
    rng = np.random.default_rng(seed)
    graphs = []

    def rand_edges(n, e):
        return rng.integers(0, n, size=(2, e))

    hub = np.concatenate([np.stack([np.arange(1, 71), np.zeros(70, int)]), np.stack([np.zeros(70, int), np.arange(1, 71)]),
                          rand_edges(80, 60)], 1)
    graphs.append((80, hub[:, rng.permutation(hub.shape[1])]))
    tri = np.tile(rand_edges(20, 30), 3)
    graphs.append((20, tri[:, rng.permutation(90)]))
    graphs.append((40, rand_edges(10, 25)))                       # nodes 10 .. 39 isolated
    graphs.append((5, np.zeros((2, 0), int)))
    graphs.append((1, np.zeros((2, 3), int)))
    big = np.concatenate([rand_edges(257, 1000), np.stack([np.arange(0, 257, 9)] * 2)], 1)      # self loops among them
    graphs.append((257, big[:, rng.permutation(big.shape[1])]))
    node_ptr = np.cumsum([0] + [n for n, _ in graphs]).astype(np.int32)
    edge_ptr = np.cumsum([0] + [e.shape[1] for _, e in graphs]).astype(np.int32)
    v = rng.uniform(-1, 1, size=(node_ptr[-1], C)).astype(np.float32)
    goal = rng.uniform(-1, 1, size=(len(graphs), C)).astype(np.float32)
    goal_local = []
    for g, (n, _) in enumerate(graphs):
        if n >= 3:
            a, b = sorted(rng.choice(n, 2, replace=False))
            v[node_ptr[g] + a] = goal[g]
            v[node_ptr[g] + b] = goal[g]
        d = ((v[node_ptr[g]:node_ptr[g + 1]].astype(np.float64) - goal[g].astype(np.float64)) ** 2).sum(1)
        goal_local.append(int(np.argmin(d)))                     # first minimum: the oracle's torch.argmin / the kernel's lowest index
    return dict(C=C, G=len(graphs), sizes=[n for n, _ in graphs], node_ptr=node_ptr, edge_ptr=edge_ptr, v=v, goal=goal,
                edge_index=np.concatenate([e for _, e in graphs], 1).astype(np.int64), goal_local=goal_local)


def check_geometry(b, gd):
    """Invariants of the dumped geometry `gd` (arrays of gnnmp_train_geom) for the caller's batch `b`; the padding rules are
    not restated, only what every kernel relies on.  Returns per-slot / per-node views used by the references."""
    G, E = b['G'], b['edge_index'].shape[1]
    Npad, Epad = gd['n_pad'], gd['e_pad']
    npp, csr, row_beg, deg = gd['node_ptr_pad'], gd['csr'].reshape(Epad, 4), gd['row_beg'], gd['deg']
    assert Npad % 32 == 0 and Epad % 32 == 0 and npp[0] >= 0 and npp[G] <= Npad
    pad_of = np.full(b['node_ptr'][-1], -1)                      # caller node row -> padded node id
    for g in range(G):
        n = b['sizes'][g]
        assert npp[g] % 32 == 0 and npp[g + 1] - npp[g] >= n
        pad_of[b['node_ptr'][g]:b['node_ptr'][g + 1]] = npp[g] + np.arange(n)
        assert (gd['ntile_graph'][(npp[g] + np.arange(n)) >> 5] == g).all()
        assert gd['goal_node'][g] == npp[g] + b['goal_local'][g], (g, gd['goal_node'][g], npp[g], b['goal_local'][g])
    real = csr[:, 0] >= 0
    assert (csr[~real, 0] == -1).all()                           # pad slots are -1
    assert sorted(csr[real, 2].tolist()) == list(range(E))       # every caller column in exactly one non-pad slot
    col = csr[real, 2]
    gcol = np.searchsorted(b['edge_ptr'], col, side='right') - 1
    assert (csr[real, 0] == npp[gcol] + b['edge_index'][0, col]).all() and (csr[real, 1] == npp[gcol] + b['edge_index'][1, col]).all()
    assert int(deg.sum()) == E
    owner = np.full(Epad, -1)
    for n in np.nonzero(deg)[0]:
        s = slice(row_beg[n], row_beg[n] + deg[n])
        assert (owner[s] == -1).all() and (csr[s, 1] == n).all() and (np.diff(csr[s, 2]) > 0).all(), n
        owner[s] = n
    assert ((owner >= 0) == real).all()                          # the segments hold exactly the non-pad slots
    out_lists = []
    for n in range(Npad):
        lst = gd['out_slot'][gd['out_beg'][n]:gd['out_beg'][n] + gd['out_cnt'][n]]
        assert (lst == np.nonzero(csr[:, 0] == n)[0]).all(), n  # exactly the slots whose source is n, ascending
        out_lists.append(lst)
    assert int(gd['out_cnt'].sum()) == E
    return dict(pad_of=pad_of, real=real, csr=csr, owner=owner, out_lists=out_lists)


def segment_sum_ref(Npad, D, terms):
    """sum over (node, value rows) contributions in float64 with the absolute sum next to it: terms = [(node ids, rows)]"""
    acc, mag = np.zeros((Npad, D)), np.zeros((Npad, D))
    for nodes, rows in terms:
        np.add.at(acc, nodes, rows.astype(np.float64))
        np.add.at(mag, nodes, np.abs(rows.astype(np.float64)))
    return acc, mag


# ---- the batched smoother path: B problems per call, the prefix [0, A) active -------------------------------------
# Restated from the module, not from the kernels: nodes = cat(path, free / scale, collided / scale) with a one-hot kind
# (model_smoother.py:118-135), z = cat(x_j - x_i, x_j, x_i) summed into the target (:32-37), path[1:-1] = proposal[1:-1] (:139),
# every problem on its own rows.  A problem past its loop count (b >= A) takes no part: its outputs are left alone, zero, or
# its state handed through, as include/gnnmp.h says per operator.
SM_K = 10                                    # kNN edges per waypoint (model_smoother.py:125)
SEG_SIZES = ((2, 0, 0), (3, 4, 3), (33, 200, 60), (12, 244, 0), (2, 5, 4), (40, 1, 1))      # (P, F, Co) per problem
SEG_CALLER_EDGES = (0, 5, 100, 37, 0, 64)    # E_b of edge_ptr: only the slot layout depends on it
SEG_N_EDGES = (-1, 20, 300, 0, -1, 100)      # slots in use; -1 = the whole segment
SEG_ACTIVE = (6, 4, 1)
BAD_ID = 1 << 28


def round32(x):
    return (int(x) + 31) & ~31


def seg_layout(sizes, caller_edges):
    """Prefix arrays of a batch and where every problem's rows and edge slots start: node rows are stacked [path_b; free_b;
    collided_b] problem by problem, edge slots start at round32(edge_ptr[b] + 10 path_ptr[b]) + 32 b (the kNN stage's padded edge
    space); Ec = the slots the product's workspace holds."""
    sizes = np.asarray(sizes, np.int64).reshape(-1, 3)
    B = len(sizes)
    pp, fp, cp = (np.concatenate([[0], np.cumsum(sizes[:, i])]) for i in range(3))
    ep = np.concatenate([[0], np.cumsum(np.asarray(caller_edges, np.int64))])
    n0 = pp + fp + cp
    e0 = np.array([round32(ep[b] + SM_K * pp[b]) + 32 * b for b in range(B)], np.int64)
    Ec = round32(ep[B] + SM_K * pp[B] + 64 * B + 32)
    assert (np.diff(e0) >= 0).all() and e0[-1] < Ec
    s = dict(B=B, sizes=sizes, path_ptr=pp.astype(np.int32), free_ptr=fp.astype(np.int32), coll_ptr=cp.astype(np.int32),
             edge_ptr=ep.astype(np.int32), n0=n0, e0=e0, cap=np.append(e0[1:], Ec) - e0, P=int(pp[B]), F=int(fp[B]), Co=int(cp[B]),
             Nn=int(n0[B]), Ec=Ec)
    # node row of every path / free / collided row, problem and local index of every path row
    s['path_rows'] = np.concatenate([n0[b] + np.arange(sizes[b, 0]) for b in range(B)]).astype(np.int64)
    s['free_rows'] = np.concatenate([n0[b] + sizes[b, 0] + np.arange(sizes[b, 1]) for b in range(B)]).astype(np.int64)
    s['coll_rows'] = np.concatenate([n0[b] + sizes[b, 0] + sizes[b, 1] + np.arange(sizes[b, 2]) for b in range(B)]).astype(np.int64)
    s['path_b'] = np.repeat(np.arange(B), sizes[:, 0])
    s['path_local'] = np.concatenate([np.arange(p) for p in sizes[:, 0]]).astype(np.int64)
    s['node_b'] = np.repeat(np.arange(B), sizes.sum(1))
    s['slot_b'] = np.searchsorted(e0, np.arange(Ec), side='right') - 1
    return s


def seg_edges(s, n_edges, rng):
    """Edge slots of the layout `s`: problem b uses its first n_edges[b] slots (-1 = all of them), sources anywhere among its
    node rows, targets among its path rows except the last (a path row without an incoming edge); slots 0 and 1 are duplicates
    and, where there is room, 40 slots share one target.  Slots not in use hold an id nothing may follow."""
    B, Ec = s['B'], s['Ec']
    ne = np.array([s['cap'][b] if n_edges[b] < 0 else n_edges[b] for b in range(B)], np.int32)
    assert (ne <= s['cap']).all()
    src, dst = np.full(Ec, BAD_ID, np.int32), np.full(Ec, BAD_ID, np.int32)
    for b in range(B):
        P, N, n, e = int(s['sizes'][b, 0]), int(s['sizes'][b].sum()), int(ne[b]), int(s['e0'][b])
        src[e:e + n], dst[e:e + n] = rng.integers(0, N, n), rng.integers(0, max(P - 1, 1), n)
        if n >= 2:
            src[e + 1], dst[e + 1] = src[e], dst[e]
        if n >= 60 and P > 2:
            dst[e + 10:e + 50] = P // 2
    s = dict(s, n_edges=ne, e_src=src, e_dst=dst)
    s['used'] = np.arange(Ec) - s['e0'][s['slot_b']] < ne[s['slot_b']]
    return s


def seg_ragged_batch(seed):
    """The ragged batch of the segmented operators: N = 2 without samples; 293 node rows (the 256-stride row loops wrap, the path
    rows cross a 32-row tile); exactly 256 node rows and no edge; full, partly used and empty edge segments."""
    s = seg_edges(seg_layout(SEG_SIZES, SEG_CALLER_EDGES), SEG_N_EDGES, np.random.default_rng(seed))
    u = s['used']
    into = np.bincount(s['path_ptr'][s['slot_b'][u]] + s['e_dst'][u], minlength=s['P'])
    assert into.max() > 32 and (into == 0).any() and (s['n_edges'] == 0).any() and (s['n_edges'] == s['cap']).any()
    assert ((s['n_edges'] > 0) & (s['n_edges'] < s['cap'])).any() and (s['e_src'][~u] == BAD_ID).all()
    return s


def _seg_sel(s, A):
    """slots in use of active problems -> (slot ids, node row of the source, node row of the target, path row of the target)"""
    e = np.nonzero(s['used'] & (s['slot_b'] < A))[0]
    b = s['slot_b'][e]
    return e, s['n0'][b] + s['e_src'][e], s['n0'][b] + s['e_dst'][e], s['path_ptr'][b] + s['e_dst'][e]


def nodes_in_seg_ref(s, A, scale, cur, free_pts, coll, old):
    C = cur.shape[1]
    x = np.zeros((s['Nn'], C + 3), np.float32)
    x[s['path_rows'], :C], x[s['path_rows'], C] = cur, 1
    x[s['free_rows'], :C], x[s['free_rows'], C + 1] = free_pts / np.float32(scale), 1
    x[s['coll_rows'], :C], x[s['coll_rows'], C + 2] = coll / np.float32(scale), 1
    on = (s['node_b'] < A)[:, None]
    return np.where(on, x, old), np.broadcast_to(on, x.shape)


def msg_in_seg_ref(s, A, X):
    e, js, it, _ = _seg_sel(s, A)
    out = np.zeros((s['Ec'], 3 * X.shape[1]), np.float32)
    out[e] = np.concatenate([X[js] - X[it], X[js], X[it]], 1)
    return out


def msg_in_bwd_seg_ref(s, A, dZ):
    """float64 sum, absolute sum, largest number of edges at one node, rows the operator adds to"""
    D = dZ.shape[1] // 3
    e, js, it, _ = _seg_sel(s, A)
    z = dZ[e]
    acc, mag = segment_sum_ref(s['Nn'], D, [(js, z[:, :D]), (js, z[:, D:2 * D]), (it, z[:, 2 * D:]), (it, -z[:, :D])])
    fan = int((np.bincount(js, minlength=s['Nn']) + np.bincount(it, minlength=s['Nn'])).max()) if e.size else 1
    return acc, mag, fan, np.broadcast_to((s['node_b'] < A)[:, None], acc.shape)


def scatter_add_seg_ref(s, A, M):
    e, _, _, pt = _seg_sel(s, A)
    acc, mag = segment_sum_ref(s['P'], M.shape[1], [(pt, M[e])])
    return acc, mag, int(np.bincount(pt, minlength=s['P']).max()) if e.size else 1


def scatter_add_bwd_seg_ref(s, A, dS):
    e, _, _, pt = _seg_sel(s, A)
    out = np.zeros((s['Ec'], dS.shape[1]), np.float32)
    out[e] = dS[pt]
    return out


def add_path_seg_ref(s, A, X, Y, old):
    on = (s['path_b'] < A)[:, None]
    return np.where(on, X[s['path_rows']] + Y, old), np.broadcast_to(on, Y.shape)


def add_path_bwd_seg_ref(s, A, dH):
    out = np.zeros((s['Nn'], dH.shape[1]), np.float32)
    on = s['path_b'] < A
    out[s['path_rows'][on]] = dH[on]
    return out


def _seg_inner(s, A):
    return ((s['path_b'] < A) & (s['path_local'] >= 1) & (s['path_local'] <= s['sizes'][s['path_b'], 0] - 2))[:, None]


def path_update_seg_ref(s, A, prev, proposal):
    return np.where(_seg_inner(s, A), proposal, prev)


def path_update_bwd_seg_ref(s, A, d_next):
    inner = _seg_inner(s, A)
    return np.where(inner, d_next, np.float32(0)), np.where(inner, np.float32(0), d_next)


def coords_bwd_seg_ref(s, A, dXin, old):
    on = (s['path_b'] < A)[:, None]
    return np.where(on, old + dXin[s['path_rows'], :old.shape[1]], old), np.broadcast_to(on, old.shape)


def bn_seg_dgb_ref(part, dgamma_old, dbeta_old):
    """part [L, B, 2, D] -> float32 sums in the documented order: iterations last to first, problems ascending"""
    dg, db = dgamma_old.copy(), dbeta_old.copy()
    for it in range(part.shape[0] - 1, -1, -1):
        for b in range(part.shape[1]):
            dg, db = dg + part[it, b, 0], db + part[it, b, 1]
    return dg, db


# the one-problem forms (the module's own call), against which the segmented references are checked at B = 1
def sm_nodes_in_ref(cur, free_pts, coll, scale):
    P, F, Co, C = len(cur), len(free_pts), len(coll), cur.shape[1]
    info = np.zeros((P + F + Co, 3), np.float32)
    info[:P, 0], info[P:P + F, 1], info[P + F:, 2] = 1, 1, 1
    return np.concatenate([np.concatenate([cur, free_pts / np.float32(scale), coll / np.float32(scale)]), info], 1)


def sm_msg_in_ref(src, dst, n, X):
    out = np.zeros((len(src), 3 * X.shape[1]), np.float32)
    out[:n] = np.concatenate([X[src[:n]] - X[dst[:n]], X[src[:n]], X[dst[:n]]], 1)
    return out


def sm_path_update_ref(prev, proposal):
    out = prev.copy()
    out[1:-1] = proposal[1:-1]
    return out


# ---- the explorer's path with a loop count per graph -------------------------------------------------------------
def final_cat_ref(rows, NC, Hs):
    """rows[it] = rows of the graphs still running in iteration it (descending); Hs [n_it, rows[0], D].  Row n's graph ran
    L(n) = #{it: rows[it] > n} iterations, and the decoder reads cat(node_code, h after its last one) (model.py:143)."""
    n = np.arange(rows[0])
    L = (np.asarray(rows)[:, None] > n[None, :]).sum(0)
    return np.concatenate([NC, Hs[L - 1, n]], 1)


def seed_dh_ref(rows_next, d_dec, dXin):
    D = d_dec.shape[1]
    return np.where((np.arange(len(d_dec)) >= rows_next)[:, None], d_dec, dXin[:, 3 * D:4 * D])


FINAL_CAT_TABLES = ([256], [1280, 1024, 1024, 512, 256], [768] * 20 + [512] * 22 + [256] * 22)
DW_ORDER_PAIRS = ((32, 1), (8, 32), (160, 32), (128, 64))
DW_ORDER_ROWS = ((256, 256), (256, 2304), (1024, 2304), (300, 1300))
DW_BLOCK_ROWS = 128                          # rows per partial sum of LINEAR_DW's first stage (train_kernels.hip kDwRows)


def dw_slice_width(R):
    """blocks per slice of LINEAR_DW's second stage at R rows: eight slices over ceil(R / 128) partial sums"""
    return ((R + DW_BLOCK_ROWS - 1) // DW_BLOCK_ROWS + 7) // 8
