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
