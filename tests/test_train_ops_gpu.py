"""Every launcher of the training path (train_kernels.hip, `t_*` of kernels.hpp) on its own, through the test hook
gnnmp_train_op, against a float64 restatement of the same operation (tests/train_ops_host.py) at the shapes where the
kernels branch.  For every case:

  * all buffers of a case live in ONE device tensor that the whole module shares; every output sits between two guard bands
    of a sentinel, and after the call the entire image -- guards, inputs, the other outputs' surroundings -- must be
    unchanged outside the regions the operator may write;
  * the operator runs twice from the same image and must give identical bits ("no float atomics, fixed summation orders");
  * copies, gathers and differences are compared bit for bit with the float32 numpy restatement; sums obey the derived bound
    |err| <= gamma_n * sum |a_i| |b_i| (+ u |old| for a `+=`), element-wise, gamma_n = (2n + 2) u / (1 - (2n + 2) u), u = 2^-24;
  * BatchNorm has no closed-form bound: err <= max(1e-4 scale, 4 own) + 1e-6 per output tensor, own = torch's float32 CPU
    batch norm against float64, next to the ceilings of BN_CEIL below, and 1e-5 scale + 1e-6 without `own` on the unit-scale
    inputs with a batch variance near 1 (train_ops_host.BN_TIGHT_N).  The `cancel` inputs (column mean 1e3, standard
    deviation 1e-2) are the regression test of a fault this module found: with the column mean carried in float32 the kernels
    were 7.2e-3 off in y (bar 1.6e-3) and 0.38 off in dgamma (bar 0.31); they now carry it in double.

The launchers of the two batched paths (the `_seg` operators of the smoother, FINAL_CAT / SEED_DH / LINEAR_DW_ORDER of the
explorer) follow at the end of the file: their contracts -- problems past their loop count are absent, sums inside a problem keep
the one-problem kernel's order, R_order reproduces the longer call -- are bit-exact statements and are tested as such.

The worst err / bound per operator and the dispatch path of the three GEMM launchers are printed (pytest -s shows them;
profiles/train_ops_unit.txt is that output from the MI355X)."""
import ctypes

import numpy as np
import pytest
import torch

from gnnmp import _lib
import train_ops_host as H

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 512                                   # words on each side of an output (more than one row of any output here)
SENT = np.float32(-1.7e38).view(np.uint32)    # read by mistake it wrecks any sum; as an int32 it is a huge negative index
POOL_WORDS = 24 << 20

# worst err / scale per output tensor of t_bn_fwd / t_bn_bwd over all (N, D, relu) of a kind, measured on the MI355X; the
# ceilings are about 3x that.  `cancel`: columns with mean 1e3 and standard deviation 1e-2.
BN_CEIL = {
    ('unit', 'y'): 2e-7,            # measured 5.70e-8
    ('unit', 'mean'): 2e-7,         # measured 5.45e-8
    ('unit', 'invstd'): 2e-7,       # measured 5.79e-8
    ('unit', 'var'): 2e-7,          # measured 5.58e-8
    ('unit', 'dx'): 1.5e-4,         # measured 4.41e-5 (N = 2: dx is a difference of nearly equal numbers, scale 3e-5)
    ('unit', 'dgamma'): 3.5e-7,     # measured 1.10e-7
    ('unit', 'dbeta'): 2.5e-7,      # measured 8.04e-8
    ('cancel', 'y'): 2e-7,          # measured 5.52e-8
    ('cancel', 'mean'): 1e-7,       # measured 3.05e-8
    ('cancel', 'invstd'): 2e-7,     # measured 5.44e-8
    ('cancel', 'var'): 2e-7,        # measured 5.43e-8
    ('cancel', 'dx'): 2e-6,         # measured 7.01e-7
    ('cancel', 'dgamma'): 3e-7,     # measured 9.07e-8
    ('cancel', 'dbeta'): 3e-7,      # measured 9.06e-8
}

_pool = {}


@pytest.fixture(scope='module', autouse=True)
def release_device_memory():
    yield
    _pool.clear()
    _geoms.clear()
    torch.cuda.empty_cache()


def pool():
    if 't' not in _pool:
        _pool['t'] = torch.empty(POOL_WORDS, dtype=torch.int32, device=DEV)
    return _pool['t']


class Case:
    """Host image of one case's buffers (4-byte words, 64-word aligned), uploaded into the shared device tensor."""

    def __init__(self):
        self.parts, self.n, self.outs = [], 0, {}

    def _add(self, words):
        off = self.n
        self.parts.append(words)
        pad = -len(words) % 64
        if pad:
            self.parts.append(np.full(pad, SENT, np.uint32))
        self.n += len(words) + pad
        return off

    def inp(self, a):
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float32, np.int32)
        return self._add(a.reshape(-1).view(np.uint32)) if a.size else self._add(np.full(1, SENT, np.uint32))

    def out(self, name, init, writable=None):
        """An output region with its initial content (the sentinel when init is a shape) between two guard bands.
        writable: boolean mask of the elements the operator may write (default: all)."""
        if isinstance(init, tuple):
            dtype, init = init[0], np.full(init[1], SENT, np.uint32).view(init[0])
        init = np.ascontiguousarray(init)
        self._add(np.full(GUARD, SENT, np.uint32))
        off = self._add(init.reshape(-1).view(np.uint32))
        self._add(np.full(GUARD, SENT, np.uint32))
        self.outs[name] = (off, init.shape, init.dtype, writable)
        return off

    def run(self, launch):
        """launch(addr) enqueues the operator(s); addr(off) = device address of word `off`.  Twice from the same image:
        identical bits; nothing outside the writable regions changed.  Returns {name: array}."""
        host = np.concatenate(self.parts)
        assert host.size == self.n <= POOL_WORDS
        dev = pool()[:self.n]
        src = torch.from_numpy(host.view(np.int32))
        base = pool().data_ptr()
        got = []
        for _ in range(2):
            dev.copy_(src)
            launch(lambda off: base + 4 * int(off))
            got.append(dev.cpu().numpy().view(np.uint32))       # .cpu() waits for the stream
        assert np.array_equal(got[0], got[1]), 'two runs from the same image differ in %d words' % int((got[0] != got[1]).sum())
        res, rest = {}, got[0].copy()
        for name, (off, shape, dtype, writable) in self.outs.items():
            n = int(np.prod(shape))
            res[name] = got[0][off:off + n].view(dtype).reshape(shape).copy()
            w = np.ones(n, bool) if writable is None else writable.reshape(-1)
            rest[off:off + n][w] = host[off:off + n][w]
        bad = np.nonzero(rest != host)[0]
        assert bad.size == 0, 'words outside the writable regions changed, first at %d (outputs at %s)' % (
            int(bad[0]), {k: v[0] for k, v in self.outs.items()})
        return res


class Worst:
    """worst err / bound per operator, printed at the end of a test"""

    def __init__(self):
        self.w, self.fail = {}, []

    def bounded(self, op, what, got, ref, bound, tag=''):
        err = np.abs(got.astype(np.float64) - ref)
        assert np.isfinite(got).all(), (op, what)
        ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
        key = (op, tag)
        if ratio > self.w.get(key, (-1, None))[0]:
            self.w[key] = (ratio, what)
        if ratio > 1:
            self.fail.append((op, tag, what, ratio))

    def exact(self, op, what, got, ref):
        g, r = np.ascontiguousarray(got), np.ascontiguousarray(ref).astype(got.dtype)
        same = g.view(np.uint32) == r.view(np.uint32)
        self.w.setdefault((op, 'exact'), (0.0, 'bit equality'))
        if not same.all():
            self.fail.append((op, 'exact', what, int((~same).sum())))

    def report(self):
        for (op, tag), (ratio, what) in sorted(self.w.items()):
            print('[train_ops] %-20s %-6s worst err/bound %.3e at %s' % (op, tag, ratio, what))
        assert not self.fail, self.fail[:20]


def op(name, dims, bufs, geom=None, scalar=0.0):
    _lib.train_op(name, dims, bufs, geom, scalar, torch.cuda.current_stream().cuda_stream)


# ======================================================================================================================
# GEMM trio
# ======================================================================================================================
CASES = H.gemm_cases()
N_FULL = len(H.ROWS) * len(H.PAIRS_FOR_EVERY_R)           # these cases take every variant, the rest rotate through them


def _gemm_inputs(R, K, O, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return f(R, K), f(O, K), f(O), f(R, O), rng


def _paths(opname):
    seen = {}
    for R, K, O in CASES:
        p = _lib.train_op_path(opname, R, K, O)
        assert p == H.expected_path(opname, K, O), (opname, K, O, p)
        seen[p] = seen.get(p, 0) + 1
    print('[train_ops] %-20s dispatch: %s' % (opname, ', '.join('%s x %d' % kv for kv in sorted(seen.items()))))
    assert set(seen) == {'mfma', 'plain'}


def test_linear():
    w = Worst()
    _paths('LINEAR')
    for i, (R, K, O) in enumerate(CASES):
        X, W, b, _, _ = _gemm_inputs(R, K, O, i)
        for v in (range(4) if i < N_FULL else [i % 4]):
            bias, relu = v & 1, v >> 1
            c = Case()
            x, wt, bb = c.inp(X), c.inp(W), c.inp(b)
            y = c.out('Y', (np.float32, (R, O)))
            got = c.run(lambda a: op('LINEAR', [R, K, O, relu], [a(x), a(wt), a(bb) if bias else None, a(y)]))
            ref, bound = H.linear_ref(X, W, b if bias else None, relu)
            w.bounded('LINEAR', (R, K, O, 'bias' * bias, 'relu' * relu), got['Y'], ref, bound, _lib.train_op_path('LINEAR', R, K, O))
    w.report()


def test_linear_dx():
    w = Worst()
    _paths('LINEAR_DX')
    for i, (R, K, O) in enumerate(CASES):
        X, W, _, dY, rng = _gemm_inputs(R, K, O, 10000 + i)
        for acc in ((0, 1) if i < N_FULL else [i % 2]):
            c = Case()
            dy, wt = c.inp(dY), c.inp(W)
            dx = c.out('dX', X if acc else (np.float32, (R, K)))       # accumulate: onto random dX; else onto the sentinel
            got = c.run(lambda a: op('LINEAR_DX', [R, K, O, acc], [a(dy), a(wt), a(dx)]))
            ref, bound = H.linear_dx_ref(dY, W, X if acc else None)
            w.bounded('LINEAR_DX', (R, K, O, 'acc' * acc), got['dX'], ref, bound, _lib.train_op_path('LINEAR_DX', R, K, O))
    w.report()


def test_linear_dw():
    w = Worst()
    _paths('LINEAR_DW')
    for i, (R, K, O) in enumerate(CASES):
        X, W0, b0, dY, rng = _gemm_inputs(R, K, O, 20000 + i)
        for with_db in ((1, 0) if i < N_FULL else [i % 2]):
            c = Case()
            dy, x = c.inp(dY), c.inp(X)
            dw, db = c.out('dW', W0), c.out('db', b0, writable=np.full(O, bool(with_db)))      # onto random non-zero dW / db
            ns = _lib.train_dw_scratch_floats(R, K, O)
            sc = c.out('scratch', np.full(ns, np.nan, np.float32))                            # never read before written
            got = c.run(lambda a: op('LINEAR_DW', [R, K, O], [a(dy), a(x), a(dw), a(db) if with_db else None, a(sc)]))
            rW, bW, rb, bb = H.linear_dw_ref(dY, X, W0, b0 if with_db else None)
            path = _lib.train_op_path('LINEAR_DW', R, K, O)
            w.bounded('LINEAR_DW', (R, K, O, 'dW', 'db' * with_db), got['dW'], rW, bW, path)
            if with_db:
                w.bounded('LINEAR_DW', (R, K, O, 'db'), got['db'], rb, bb, path)
    w.report()


# ======================================================================================================================
# BatchNorm
# ======================================================================================================================
@pytest.mark.parametrize('kind', ['unit', 'cancel'])
def test_batchnorm(kind):
    worst = {k: (0.0, None) for k in H.BN_TENSORS}
    fail = []
    for D in H.BN_D:
        for N in H.BN_N:
            for relu in (0, 1):
                inp, r64, own, scale = H.bn_pair(kind, N, D, relu)
                c = Case()
                x, g, b, dy = c.inp(inp['x']), c.inp(inp['gamma']), c.inp(inp['beta']), c.inp(inp['dy'])
                y, st, dx = c.out('y', (np.float32, (N, D))), c.out('stats', (np.float32, (3, D))), c.out('dx', (np.float32, (N, D)))
                dg, db = c.out('dgamma', inp['dgamma_old']), c.out('dbeta', inp['dbeta_old'])

                def launch(a):
                    op('BN_FWD', [N, D, relu], [a(x), a(g), a(b), a(y), a(st)])
                    op('BN_BWD', [N, D], [a(x), a(dy), a(g), a(st), a(dx), a(dg), a(db)])      # the forward's own stats, as the product
                got = c.run(launch)
                got.update(mean=got['stats'][0], invstd=got['stats'][1], var=got['stats'][2])
                for k in H.BN_TENSORS:
                    assert np.isfinite(got[k]).all(), (k, N, D)
                    err = float(np.max(np.abs(got[k].astype(np.float64) - r64[k])))
                    bar = max(1e-4 * scale[k], 4 * own[k]) + 1e-6
                    rel = err / scale[k] if scale[k] > 0 else 0.0
                    if rel > worst[k][0]:
                        worst[k] = (rel, (N, D, relu, 'err %.3e own %.3e bar %.3e' % (err, own[k], bar)))
                    if err > bar:
                        fail.append((k, N, D, relu, 'err %.3e > bar %.3e (own %.3e, scale %.3e)' % (err, bar, own[k], scale[k])))
                    if kind == 'unit' and N in H.BN_TIGHT_N and err > 1e-5 * scale[k] + 1e-6:
                        fail.append((k, N, D, relu, 'err %.3e > 1e-5 scale + 1e-6 (scale %.3e)' % (err, scale[k])))
                    ceil = BN_CEIL[(kind, k)]
                    if ceil is not None and err > ceil * scale[k] + 1e-6:
                        fail.append((k, N, D, relu, 'err %.3e > ceiling %.1e x scale %.3e' % (err, ceil, scale[k])))
    for k in H.BN_TENSORS:
        print('[train_ops] BN %-6s %-7s worst err/scale %.3e at %s' % (kind, k, worst[k][0], worst[k][1]))
    assert not fail, fail[:20]


# ======================================================================================================================
# geometry operators on a ragged batch
# ======================================================================================================================
_geoms = {}


def geometry(D):
    """The dumped geometry of the ragged batch at (d, C) = (32, 2) / (64, 7): built once, kept on the device."""
    if D in _geoms:
        return _geoms[D]
    C = {32: 2, 64: 7}[D]
    b = H.ragged_batch(C, seed=D)
    L = _lib.lib()
    E = b['edge_index'].shape[1]
    shape = _lib.Batch(b['G'], int(b['node_ptr'][-1]), E, 0, 0, None, None, None, None, None, None, None)
    need = ctypes.c_size_t()
    _lib.check(L.gnnmp_train_geom_workspace_bytes(ctypes.byref(shape), C, ctypes.byref(need)), 'geom_workspace_bytes')
    ins = [b['v'].view(np.uint8).reshape(-1), b['goal'].view(np.uint8).reshape(-1), b['node_ptr'].view(np.uint8),
           b['edge_ptr'].view(np.uint8), np.ascontiguousarray(b['edge_index']).view(np.uint8).reshape(-1)]
    offs, o = [], (need.value + 255) & ~255
    for a in ins:
        offs.append(o)
        o += (a.size + 255) & ~255
    host = np.zeros(o, np.uint8)
    host[:need.value] = 0xA5                                     # junk where the workspace is: nothing may rely on zeros
    for a, off in zip(ins, offs):
        host[off:off + a.size] = a
    mem = torch.from_numpy(host).to(DEV)
    base = mem.data_ptr()
    assert base % 256 == 0
    batch = _lib.Batch(b['G'], int(b['node_ptr'][-1]), E, 0, 0, base + offs[0], base + offs[1], None, base + offs[4],
                       base + offs[2], base + offs[3], None)
    geom = _lib.TrainGeom()
    _lib.check(L.gnnmp_train_geom_build(ctypes.byref(batch), C, base, need.value, ctypes.byref(geom),
                                        torch.cuda.current_stream().cuda_stream), 'geom_build')
    dump = mem.cpu().numpy()

    def arr(ptr, n):
        off = ptr - base
        assert 0 <= off and off + 4 * n <= need.value
        return dump[off:off + 4 * n].view(np.int32).copy()
    Np, Ep = geom.n_pad, geom.e_pad
    gd = dict(n_pad=Np, e_pad=Ep, node_ptr_pad=arr(geom.node_ptr_pad, b['G'] + 1), ntile_graph=arr(geom.ntile_graph, Np // 32),
              goal_node=arr(geom.goal_node, b['G']), row_beg=arr(geom.row_beg, Np), deg=arr(geom.deg, Np), csr=arr(geom.csr, 4 * Ep),
              out_beg=arr(geom.out_beg, Np), out_cnt=arr(geom.out_cnt, Np), out_slot=arr(geom.out_slot, Ep))
    _geoms[D] = dict(b=b, geom=geom, gd=gd, mem=mem, D=D, C=C)
    return _geoms[D]


@pytest.mark.parametrize('D', [32, 64])
def test_geometry_invariants(D):
    G = geometry(D)
    b, gd = G['b'], G['gd']
    info = H.check_geometry(b, gd)
    assert gd['deg'].max() > 64 and gd['out_cnt'].max() > 64                    # the hub
    assert (gd['deg'][info['pad_of'][b['node_ptr'][2] + 10:b['node_ptr'][3]]] == 0).all()      # isolated nodes
    print('[train_ops] geometry d=%d: Npad %d Epad %d E %d max in-degree %d max out-degree %d' % (
        D, gd['n_pad'], gd['e_pad'], b['edge_index'].shape[1], gd['deg'].max(), gd['out_cnt'].max()))


@pytest.mark.parametrize('D', [32, 64])
def test_gathers_and_concatenations(D):
    G = geometry(D)
    b, gd, geom, C = G['b'], G['gd'], G['geom'], G['C']
    info = H.check_geometry(b, gd)
    Np, Ep, csr, real, pad_of = gd['n_pad'], gd['e_pad'], info['csr'], info['real'], info['pad_of']
    rng = np.random.default_rng(D + 1)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    w = Worst()
    # caller row / graph of every padded node
    row_of = np.full(Np, -1)
    row_of[pad_of] = np.arange(pad_of.size)
    graph_of = np.searchsorted(b['node_ptr'], np.maximum(row_of, 0), side='right') - 1
    v, goal = b['v'], b['goal']
    # node_in / edge_in
    ref = np.zeros((Np, 4 * C), np.float32)
    m = row_of >= 0
    vv, gg = v[row_of[m]], goal[graph_of[m]]
    dl = vv - gg
    ref[m] = np.concatenate([vv, gg, dl * dl, dl], 1)
    c = Case()
    o = c.out('out', (np.float32, (Np, 4 * C)))
    w.exact('NODE_IN', 'all', c.run(lambda a: op('NODE_IN', [], [a(o)], geom))['out'], ref)
    ref = np.zeros((Ep, 2 * C), np.float32)
    ref[real] = np.concatenate([v[row_of[csr[real, 0]]], v[row_of[csr[real, 1]]]], 1)
    c = Case()
    o = c.out('out', (np.float32, (Ep, 2 * C)))
    w.exact('EDGE_IN', 'all', c.run(lambda a: op('EDGE_IN', [], [a(o)], geom))['out'], ref)
    # h0 and its adjoint
    ge, dH0, dge_old = f(D), f(Np, D), f(D)
    ref = np.zeros((Np, D), np.float32)
    ref[gd['goal_node']] = ge
    c = Case()
    g_, o = c.inp(ge), c.out('H0', (np.float32, (Np, D)))
    w.exact('H0', 'all', c.run(lambda a: op('H0', [D], [a(g_), a(o)], geom))['H0'], ref)
    c = Case()
    d_, o = c.inp(dH0), c.out('dge', dge_old)
    got = c.run(lambda a: op('H0_BWD', [D], [a(d_), a(o)], geom))['dge']
    rows = dH0[gd['goal_node']].astype(np.float64)
    w.bounded('H0_BWD', 'all', got, dge_old + rows.sum(0), H.gamma(b['G']) * np.abs(rows).sum(0) + H.U * np.abs(dge_old))
    # concat / split on an odd row count
    R = 37
    parts4 = [f(R, D) for _ in range(4)]
    for parts in (2, 4):
        c = Case()
        offs = [c.inp(p) for p in parts4]
        o = c.out('out', (np.float32, (R, parts * D)))
        got = c.run(lambda a: op('CONCAT', [R, D, parts], [a(x) if i < parts else None for i, x in enumerate(offs)] + [a(o)]))
        w.exact('CONCAT', parts, got['out'], np.concatenate(parts4[:parts], 1))
        d_in, old = f(R, parts * D), f(R, D)
        for part in range(parts):
            for acc in (0, 1):
                c = Case()
                i_, o = c.inp(d_in), c.out('dst', old if acc else (np.float32, (R, D)))
                got = c.run(lambda a: op('SPLIT', [R, D, parts, part, acc], [a(i_), a(o)]))
                sl = d_in[:, part * D:(part + 1) * D]
                w.exact('SPLIT', (parts, part, acc), got['dst'], old + sl if acc else sl)
    # msg_in / pol_in and their adjoints
    X, EF, EC = f(Np, D), f(Ep, D), f(Ep, D)
    s, t = csr[real, 0], csr[real, 1]
    slots = np.nonzero(real)[0]
    # n of gamma_n for the adjoint gathers: the largest fan-in, the hub's in- or out-degree (70 + the random edges).  This is the
    # bar the test sets, not the rigorous worst case: msg_in_bwd sums 2 (deg + out_cnt) terms per element, about 280 at the hub, so
    # a chain of worst-case roundings could reach ~4x this bound; random roundings stay far below it (measured ratio <= 0.13), and a
    # dropped or doubled term is ~1 / 280 of the absolute sum against gamma_71 = 8.6e-6 of it.
    fan = int(max(gd['deg'].max(), gd['out_cnt'].max()))
    ref = np.zeros((Ep, 5 * D), np.float32)
    ref[real] = np.concatenate([X[s] - X[t], X[s], X[t], EF[real], EC[real]], 1)
    c = Case()
    x_, ef_, ec_, o = c.inp(X), c.inp(EF), c.inp(EC), c.out('out', (np.float32, (Ep, 5 * D)))
    w.exact('MSG_IN', 'all', c.run(lambda a: op('MSG_IN', [D], [a(x_), a(ef_), a(ec_), a(o)], geom))['out'], ref)
    dZ, dX_old, dEC_old = f(Ep, 5 * D), f(Np, D), f(Ep, D)
    c = Case()
    z_, dx_ = c.inp(dZ), c.out('dX', dX_old)
    dec_ = c.out('dEC', dEC_old, writable=np.repeat(real, D).reshape(Ep, D))
    got = c.run(lambda a: op('MSG_IN_BWD', [D], [a(z_), a(dx_), a(dec_)], geom))
    zr = dZ[slots]
    acc, mag = H.segment_sum_ref(Np, D, [(s, zr[:, :D]), (s, zr[:, D:2 * D]), (t, -zr[:, :D]), (t, zr[:, 2 * D:3 * D])])
    w.bounded('MSG_IN_BWD', 'dX', got['dX'], dX_old + acc, H.gamma(fan) * mag + H.U * np.abs(dX_old))
    ref = dEC_old.copy()
    ref[real] = dEC_old[real] + dZ[real][:, 4 * D:]
    w.exact('MSG_IN_BWD', 'dEC', got['dEC'], ref)
    Dn = f(Np, D)
    ref = np.zeros((Ep, 3 * D), np.float32)
    ref[real] = np.concatenate([Dn[s], Dn[s] - Dn[t], EF[real]], 1)
    c = Case()
    d_, ef_, o = c.inp(Dn), c.inp(EF), c.out('out', (np.float32, (Ep, 3 * D)))
    w.exact('POL_IN', 'all', c.run(lambda a: op('POL_IN', [D], [a(d_), a(ef_), a(o)], geom))['out'], ref)
    dP, dDn_old = f(Ep, 3 * D), f(Np, D)
    c = Case()
    p_, o = c.inp(dP), c.out('dDn', dDn_old)
    got = c.run(lambda a: op('POL_IN_BWD', [D], [a(p_), a(o)], geom))['dDn']
    pr = dP[slots]
    acc, mag = H.segment_sum_ref(Np, D, [(s, pr[:, :D]), (s, pr[:, D:2 * D]), (t, -pr[:, D:2 * D])])
    w.bounded('POL_IN_BWD', 'dDn', got, dDn_old + acc, H.gamma(fan) * mag + H.U * np.abs(dDn_old))
    # scores: CSR slot order <-> caller column order
    E = b['edge_index'].shape[1]
    sc, d_out = f(Ep), f(E)
    ref = np.empty(E, np.float32)
    ref[csr[real, 2]] = sc[real]
    c = Case()
    s_, o = c.inp(sc), c.out('out', (np.float32, (E,)))
    w.exact('SCORES_OUT', 'all', c.run(lambda a: op('SCORES_OUT', [], [a(s_), a(o)], geom))['out'], ref)
    ref = np.zeros(Ep, np.float32)
    ref[real] = d_out[csr[real, 2]]
    c = Case()
    d_, o = c.inp(d_out), c.out('d_slot', (np.float32, (Ep,)))
    w.exact('SCORES_IN', 'all', c.run(lambda a: op('SCORES_IN', [], [a(d_), a(o)], geom))['d_slot'], ref)
    w.report()


@pytest.mark.parametrize('D', [32, 64])
def test_segment_max(D):
    G = geometry(D)
    b, gd, geom = G['b'], G['gd'], G['geom']
    info = H.check_geometry(b, gd)
    Np, Ep, csr, real = gd['n_pad'], gd['e_pad'], info['csr'], info['real']
    rng = np.random.default_rng(D + 2)
    M = rng.standard_normal((Ep, D)).astype(np.float32)
    M[~real] = np.float32(9e9)                                   # pad slots must never win
    npp = gd['node_ptr_pad']
    # exact ties: duplicate edges (the tripled graph) carry identical rows ...
    key = {}
    for e in np.nonzero(real & (csr[:, 1] >= npp[1]) & (csr[:, 1] < npp[2]))[0]:
        M[e] = M[key.setdefault((csr[e, 0], csr[e, 1]), e)]
    # ... the hub's segment is all-equal, and graph 2's segments are negative throughout (the maximum is not 0)
    hub = int(np.argmax(gd['deg']))
    M[gd['row_beg'][hub]:gd['row_beg'][hub] + gd['deg'][hub]] = np.float32(-2.5)
    g2 = real & (csr[:, 1] >= npp[2]) & (csr[:, 1] < npp[3])
    M[g2] = -np.abs(M[g2]) - np.float32(0.5)
    A_ref, arg_ref = np.zeros((Np, D), np.float32), np.full((Np, D), -1, np.int32)
    for n in np.nonzero(gd['deg'])[0]:
        seg = M[gd['row_beg'][n]:gd['row_beg'][n] + gd['deg'][n]]
        k = np.argmax(seg, 0)                                    # first maximum in segment order
        A_ref[n], arg_ref[n] = seg[k, np.arange(D)], gd['row_beg'][n] + k
    assert (A_ref[hub] == -2.5).all() and (arg_ref[hub] == gd['row_beg'][hub]).all()
    w = Worst()
    c = Case()
    m_, a_, g_ = c.inp(M), c.out('A', (np.float32, (Np, D))), c.out('arg', (np.int32, (Np, D)))
    got = c.run(lambda a: op('SEGMENT_MAX', [D], [a(m_), a(a_), a(g_)], geom))
    w.exact('SEGMENT_MAX', 'A', got['A'], A_ref)
    w.exact('SEGMENT_MAX', 'arg', got['arg'], arg_ref)
    # backward: exactly dA at arg, every other slot of the zero-filled dM stays zero
    dA = rng.standard_normal((Np, D)).astype(np.float32)
    dM_ref = np.zeros((Ep, D), np.float32)
    nn, ff = np.nonzero(arg_ref >= 0)
    dM_ref[arg_ref[nn, ff], ff] = dA[nn, ff]
    c = Case()
    d_, g_, o = c.inp(dA), c.inp(arg_ref), c.out('dM', np.zeros((Ep, D), np.float32), writable=dM_ref != 0)
    got = c.run(lambda a: op('SEGMENT_MAX_BWD', [Np, D], [a(d_), a(g_), a(o)]))
    w.exact('SEGMENT_MAX_BWD', 'dM', got['dM'], dM_ref)
    w.report()


def test_relu_bwd_and_fill():
    rng = np.random.default_rng(5)
    w = Worst()
    n = 1001
    y, dy = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    y[:4] = [0.0, -0.0, 1e-45, -1e-45]
    c = Case()
    y_, o = c.inp(y), c.out('dy', dy, writable=~(y > 0))
    w.exact('RELU_BWD', n, c.run(lambda a: op('RELU_BWD', [n], [a(y_), a(o)]))['dy'], np.where(y > 0, dy, np.float32(0)))
    c = Case()
    o = c.out('x', (np.float32, (n,)))
    w.exact('FILL', n, c.run(lambda a: op('FILL', [n], [a(o)], scalar=2.5))['x'], np.full(n, 2.5, np.float32))
    w.report()


# ======================================================================================================================
# smoother gathers
# ======================================================================================================================
def _edge_list(Nn, n_edges, cap, rng):
    """cap slots, the first n_edges in use: duplicates, self loops, node Nn - 1 without an incoming edge; the slots beyond
    n_edges hold out-of-range ids that nothing may follow."""
    src, dst = rng.integers(0, Nn, cap).astype(np.int32), rng.integers(0, Nn - 1, cap).astype(np.int32)
    if n_edges >= 6:
        src[1], dst[1] = src[0], dst[0]                          # duplicate
        src[2] = dst[2] = 0                                      # self loops
        src[3] = dst[3] = 1
        src[4] = Nn - 1
    src[n_edges:], dst[n_edges:] = 1 << 28, 1 << 28
    return src, dst


@pytest.mark.parametrize('C', [2, 7, 14])
def test_smoother_gathers(C):
    rng = np.random.default_rng(100 + C)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    w = Worst()
    D = {2: 128, 7: 32, 14: 64}[C]
    for P in (2, 3, 33):
        F, Co, scale = 5, 4, 2.5
        Nn = P + F + Co
        cur, fr, co = f(P, C), f(F, C), f(Co, C)
        ref = np.zeros((Nn, C + 3), np.float32)
        ref[:P, :C], ref[P:P + F, :C], ref[P + F:, :C] = cur, fr / np.float32(scale), co / np.float32(scale)
        ref[:P, C], ref[P:P + F, C + 1], ref[P + F:, C + 2] = 1, 1, 1
        c = Case()
        a0, a1, a2, o = c.inp(cur), c.inp(fr), c.inp(co), c.out('out', (np.float32, (Nn, C + 3)))
        got = c.run(lambda a: op('SM_NODES_IN', [P, F, Co, C], [a(a0), a(a1), a(a2), a(o)], scalar=scale))
        w.exact('SM_NODES_IN', (P, C), got['out'], ref)
        # path update and the coordinate adjoints
        prev, prop = f(P, C), f(P, C)
        inner = np.zeros((P, 1), bool)
        inner[1:P - 1] = True
        c = Case()
        a0, a1, o = c.inp(prev), c.inp(prop), c.out('next', (np.float32, (P, C)))
        got = c.run(lambda a: op('SM_PATH_UPDATE', [P, C], [a(a0), a(a1), a(o)]))
        w.exact('SM_PATH_UPDATE', (P, C), got['next'], np.where(inner, prop, prev))
        dn = f(P, C)
        c = Case()
        a0, o1, o2 = c.inp(dn), c.out('dprop', (np.float32, (P, C))), c.out('dprev', (np.float32, (P, C)))
        got = c.run(lambda a: op('SM_PATH_UPDATE_BWD', [P, C], [a(a0), a(o1), a(o2)]))
        w.exact('SM_PATH_UPDATE_BWD', (P, C, 'proposal'), got['dprop'], np.where(inner, dn, np.float32(0)))
        w.exact('SM_PATH_UPDATE_BWD', (P, C, 'prev'), got['dprev'], np.where(inner, np.float32(0), dn))
        dXin, dprev_old = f(Nn, C + 3), f(P, C)
        c = Case()
        a0, o = c.inp(dXin), c.out('dprev', dprev_old)
        got = c.run(lambda a: op('SM_COORDS_BWD', [P, C], [a(a0), a(o)]))
        w.exact('SM_COORDS_BWD', (P, C), got['dprev'], dprev_old + dXin[:P, :C])
        n = P * C + 3
        x, y2 = f(n), f(n)
        c = Case()
        a0, a1, o = c.inp(x), c.inp(y2), c.out('out', (np.float32, (n,)))
        w.exact('ADD_ROWS', n, c.run(lambda a: op('ADD_ROWS', [n], [a(a0), a(a1), a(o)]))['out'], x + y2)
        c = Case()
        a0, o = c.inp(x), c.out('y', (np.float32, (n,)))
        w.exact('SCALE', n, c.run(lambda a: op('SCALE', [n], [a(a0), a(o)], scalar=scale))['y'], x * np.float32(scale))
        # edge-list operators: a full list, a partly used one, an empty one
        cap = 40
        for n_edges in (cap, 25, 0):
            src, dst = _edge_list(Nn, n_edges, cap, rng)
            s, t = src[:n_edges], dst[:n_edges]
            ne = np.array([n_edges], np.int32)
            X = f(Nn, D)
            ref = np.zeros((cap, 3 * D), np.float32)
            ref[:n_edges] = np.concatenate([X[s] - X[t], X[s], X[t]], 1)
            c = Case()
            n_, s_, t_, x_, o = c.inp(ne), c.inp(src), c.inp(dst), c.inp(X), c.out('out', (np.float32, (cap, 3 * D)))
            got = c.run(lambda a: op('SM_MSG_IN', [D, cap], [a(n_), a(s_), a(t_), a(x_), a(o)]))
            w.exact('SM_MSG_IN', (P, C, n_edges), got['out'], ref)
            dZ, dX_old = f(cap, 3 * D), f(Nn, D)
            zr = dZ[:n_edges]
            acc, mag = H.segment_sum_ref(Nn, D, [(s, zr[:, :D]), (s, zr[:, D:2 * D]), (t, zr[:, 2 * D:]), (t, -zr[:, :D])])
            fan = int((np.bincount(s, minlength=Nn) + np.bincount(t, minlength=Nn)).max()) if n_edges else 1
            c = Case()
            n_, s_, t_, z_, o = c.inp(ne), c.inp(src), c.inp(dst), c.inp(dZ), c.out('dX', dX_old)
            got = c.run(lambda a: op('SM_MSG_IN_BWD', [D, Nn], [a(n_), a(s_), a(t_), a(z_), a(o)]))
            w.bounded('SM_MSG_IN_BWD', (P, C, n_edges), got['dX'], dX_old + acc, H.gamma(fan) * mag + H.U * np.abs(dX_old))
            Mm, S_old = f(cap, D), f(Nn, D)
            acc, mag = H.segment_sum_ref(Nn, D, [(t, Mm[:n_edges])])
            fan = int(np.bincount(t, minlength=Nn).max()) if n_edges else 1
            assert n_edges == 0 or np.bincount(t, minlength=Nn)[Nn - 1] == 0           # a node without an incoming edge
            c = Case()
            n_, t_, m_, o = c.inp(ne), c.inp(dst), c.inp(Mm), c.out('S', S_old)
            got = c.run(lambda a: op('SM_SCATTER_ADD', [D, Nn], [a(n_), a(t_), a(m_), a(o)]))
            w.bounded('SM_SCATTER_ADD', (P, C, n_edges), got['S'], S_old + acc, H.gamma(fan) * mag + H.U * np.abs(S_old))
            dS = f(Nn, D)
            ref = np.zeros((cap, D), np.float32)
            ref[:n_edges] = dS[t]
            c = Case()
            n_, t_, d_, o = c.inp(ne), c.inp(dst), c.inp(dS), c.out('dM', (np.float32, (cap, D)))
            got = c.run(lambda a: op('SM_SCATTER_ADD_BWD', [D, cap], [a(n_), a(t_), a(d_), a(o)]))
            w.exact('SM_SCATTER_ADD_BWD', (P, C, n_edges), got['dM'], ref)
    w.report()


# ======================================================================================================================
# the batched smoother path: B problems per call, the prefix [0, A) active (the `_seg` launchers)
# ======================================================================================================================
# What an operator does with a problem past its loop count is stated through the writable masks and bit equality: "left alone"
# = outside the mask (the image check of Case.run), "zero" = +0.0 bit for bit, "handed through" = the input's bits.  The inputs of
# such problems, the edge slots not in use and the old contents of every `+=` target are random non-zero numbers.
def _seg_case(s):
    c = Case()
    return c, [c.inp(s[k]) for k in ('path_ptr', 'free_ptr', 'coll_ptr', 'edge_ptr')]


def _seg_dims(s, A, *rest):
    return [s['B'], A, s['P'], s['Nn'], s['Ec']] + list(rest)


def _problem(s, b):
    """node rows, path rows and edge slots of problem b"""
    return (slice(int(s['n0'][b]), int(s['n0'][b + 1])), slice(int(s['path_ptr'][b]), int(s['path_ptr'][b + 1])),
            slice(int(s['e0'][b]), int(s['e0'][b] + s['cap'][b])))


@pytest.mark.parametrize('D', [32, 128])
def test_segmented_feature_rows(D):
    s = H.seg_ragged_batch(D)
    rng = np.random.default_rng(300 + D)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)
    w = Worst()
    B, P, Nn, Ec = s['B'], s['P'], s['Nn'], s['Ec']
    X, dZ, dX_old, M, dS, Y, Hh_old = f(Nn, D), f(Ec, 3 * D), f(Nn, D), f(Ec, D), f(P, D), f(P, D), f(P, D)
    # the one-problem operators on every problem's own rows and edge segment: the summation order the segmented ones promise
    one_dx, one_S = [], []
    for b in range(B):
        nr, pr, er = _problem(s, b)
        ne = s['n_edges'][b:b + 1]
        c = Case()
        n_, s_, t_, z_, o = c.inp(ne), c.inp(s['e_src'][er]), c.inp(s['e_dst'][er]), c.inp(dZ[er]), c.out('dX', dX_old[nr])
        one_dx.append(c.run(lambda a: op('SM_MSG_IN_BWD', [D, nr.stop - nr.start], [a(n_), a(s_), a(t_), a(z_), a(o)]))['dX'])
        c = Case()
        n_, t_, m_, o = c.inp(ne), c.inp(s['e_dst'][er]), c.inp(M[er]), c.out('S', np.zeros((pr.stop - pr.start, D), np.float32))
        one_S.append(c.run(lambda a: op('SM_SCATTER_ADD', [D, pr.stop - pr.start], [a(n_), a(t_), a(m_), a(o)]))['S'])      # += onto 0
    for A in H.SEG_ACTIVE:
        dims = _seg_dims(s, A, D)
        node_on, path_on = s['node_b'] < A, s['path_b'] < A
        c, p = _seg_case(s)
        n_, s_, t_, x_ = c.inp(s['n_edges']), c.inp(s['e_src']), c.inp(s['e_dst']), c.inp(X)
        o = c.out('out', (np.float32, (Ec, 3 * D)))
        got = c.run(lambda a: op('SM_MSG_IN_SEG', dims, [a(q) for q in p] + [a(n_), a(s_), a(t_), a(x_), a(o)]))
        w.exact('SM_MSG_IN_SEG', (A, D), got['out'], H.msg_in_seg_ref(s, A, X))
        acc, mag, fan, mask = H.msg_in_bwd_seg_ref(s, A, dZ)
        c, p = _seg_case(s)
        n_, s_, t_, z_ = c.inp(s['n_edges']), c.inp(s['e_src']), c.inp(s['e_dst']), c.inp(dZ)
        o = c.out('dX', dX_old, writable=mask)
        got = c.run(lambda a: op('SM_MSG_IN_BWD_SEG', dims, [a(q) for q in p] + [a(n_), a(s_), a(t_), a(z_), a(o)]))['dX']
        w.bounded('SM_MSG_IN_BWD_SEG', (A, D), got[node_on], (dX_old + acc)[node_on], (H.gamma(fan) * mag + H.U * np.abs(dX_old))[node_on])
        for b in range(A):
            w.exact('SM_MSG_IN_BWD_SEG', (A, D, 'problem', b, 'against SM_MSG_IN_BWD'), got[_problem(s, b)[0]], one_dx[b])
        acc, mag, fan = H.scatter_add_seg_ref(s, A, M)
        c, p = _seg_case(s)
        n_, t_, m_ = c.inp(s['n_edges']), c.inp(s['e_dst']), c.inp(M)
        o = c.out('S', (np.float32, (P, D)))
        got = c.run(lambda a: op('SM_SCATTER_ADD_SEG', dims, [a(q) for q in p] + [a(n_), a(t_), a(m_), a(o)]))['S']
        w.bounded('SM_SCATTER_ADD_SEG', (A, D), got[path_on], acc[path_on], (H.gamma(fan) * mag)[path_on])
        w.exact('SM_SCATTER_ADD_SEG', (A, D, 'absent problems'), got[~path_on], np.zeros((int((~path_on).sum()), D), np.float32))
        for b in range(A):
            w.exact('SM_SCATTER_ADD_SEG', (A, D, 'problem', b, 'against SM_SCATTER_ADD'), got[_problem(s, b)[1]], one_S[b])
        c, p = _seg_case(s)
        n_, t_, d_ = c.inp(s['n_edges']), c.inp(s['e_dst']), c.inp(dS)
        o = c.out('dM', (np.float32, (Ec, D)))
        got = c.run(lambda a: op('SM_SCATTER_ADD_BWD_SEG', dims, [a(q) for q in p] + [a(n_), a(t_), a(d_), a(o)]))['dM']
        w.exact('SM_SCATTER_ADD_BWD_SEG', (A, D), got, H.scatter_add_bwd_seg_ref(s, A, dS))
        ref, mask = H.add_path_seg_ref(s, A, X, Y, Hh_old)
        c, p = _seg_case(s)
        x_, y_ = c.inp(X), c.inp(Y)
        o = c.out('out', Hh_old, writable=mask)
        got = c.run(lambda a: op('SM_ADD_PATH_SEG', dims, [a(q) for q in p] + [a(x_), a(y_), a(o)]))['out']
        w.exact('SM_ADD_PATH_SEG', (A, D), got, ref)
        c, p = _seg_case(s)
        d_ = c.inp(dS)
        o = c.out('dX', (np.float32, (Nn, D)))
        got = c.run(lambda a: op('SM_ADD_PATH_BWD_SEG', dims, [a(q) for q in p] + [a(d_), a(o)]))['dX']
        w.exact('SM_ADD_PATH_BWD_SEG', (A, D), got, H.add_path_bwd_seg_ref(s, A, dS))
    w.report()


@pytest.mark.parametrize('C', [2, 7, 14])
def test_segmented_coordinate_rows(C):
    s = H.seg_ragged_batch(C)
    rng = np.random.default_rng(400 + C)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)
    w = Worst()
    P, Nn, scale = s['P'], s['Nn'], 2.5
    cur, fr, co, Xin_old = f(P, C), f(s['F'], C), f(s['Co'], C), f(Nn, C + 3)
    prop, dn, dXin, dprev_old = f(P, C), f(P, C), f(Nn, C + 3), f(P, C)
    for A in H.SEG_ACTIVE:
        dims = _seg_dims(s, A, C)
        ref, mask = H.nodes_in_seg_ref(s, A, scale, cur, fr, co, Xin_old)
        c, p = _seg_case(s)
        a0, a1, a2 = c.inp(cur), c.inp(fr), c.inp(co)
        o = c.out('out', Xin_old, writable=mask)
        got = c.run(lambda a: op('SM_NODES_IN_SEG', dims, [a(q) for q in p] + [a(a0), a(a1), a(a2), a(o)], scalar=scale))['out']
        w.exact('SM_NODES_IN_SEG', (A, C), got, ref)
        c, p = _seg_case(s)
        a0, a1 = c.inp(cur), c.inp(prop)
        o = c.out('next', (np.float32, (P, C)))
        got = c.run(lambda a: op('SM_PATH_UPDATE_SEG', dims, [a(q) for q in p] + [a(a0), a(a1), a(o)]))['next']
        w.exact('SM_PATH_UPDATE_SEG', (A, C), got, H.path_update_seg_ref(s, A, cur, prop))
        c, p = _seg_case(s)
        a0 = c.inp(dn)
        o1, o2 = c.out('dprop', (np.float32, (P, C))), c.out('dprev', (np.float32, (P, C)))
        got = c.run(lambda a: op('SM_PATH_UPDATE_BWD_SEG', dims, [a(q) for q in p] + [a(a0), a(o1), a(o2)]))
        r1, r2 = H.path_update_bwd_seg_ref(s, A, dn)
        w.exact('SM_PATH_UPDATE_BWD_SEG', (A, C, 'proposal'), got['dprop'], r1)
        w.exact('SM_PATH_UPDATE_BWD_SEG', (A, C, 'prev'), got['dprev'], r2)
        ref, mask = H.coords_bwd_seg_ref(s, A, dXin, dprev_old)
        c, p = _seg_case(s)
        a0 = c.inp(dXin)
        o = c.out('dprev', dprev_old, writable=mask)
        got = c.run(lambda a: op('SM_COORDS_BWD_SEG', dims, [a(q) for q in p] + [a(a0), a(o)]))['dprev']
        w.exact('SM_COORDS_BWD_SEG', (A, C), got, ref)
    w.report()


@pytest.mark.parametrize('kind', ['unit', 'cancel'])
def test_segmented_batchnorm(kind):
    """Per active problem bit-equal to BN_FWD / BN_BWD on its rows alone (dgamma / dbeta from zero), and -- so that the test
    does not rest on the sibling kernel alone -- inside the bar of test_batchnorm against float64, own = torch's float32 result
    on the same rows.  Absent problems: y, stats and out_stats untouched, dx and part +0.0."""
    s = H.seg_ragged_batch(7)
    B, Nn, L, it = s['B'], s['Nn'], 3, 1
    w, fail = Worst(), []
    worst = {k: (0.0, None) for k in H.BN_TENSORS}
    for D in (32, 128):
        inp = H.bn_inputs(kind, Nn, D, seed=5000 + D + (7 if kind == 'cancel' else 0))
        rng = np.random.default_rng(D)
        f = lambda *sh: rng.standard_normal(sh).astype(np.float32)
        y_old, st_old, ost_old = f(Nn, D), f(B, 3, D), f(B, L, 2, D)
        zero = np.zeros(D, np.float32)
        stride = L * 2 * D
        for relu in (0, 1):
            one, r64, own, scale = [], [], [], []
            for b in range(B):
                nr = _problem(s, b)[0]
                N = nr.stop - nr.start
                c = Case()
                x, g, be, dy = c.inp(inp['x'][nr]), c.inp(inp['gamma']), c.inp(inp['beta']), c.inp(inp['dy'][nr])
                y, st, dx = c.out('y', (np.float32, (N, D))), c.out('stats', (np.float32, (3, D))), c.out('dx', (np.float32, (N, D)))
                dg, db = c.out('dgamma', zero), c.out('dbeta', zero)

                def launch(a):
                    op('BN_FWD', [N, D, relu], [a(x), a(g), a(be), a(y), a(st)])
                    op('BN_BWD', [N, D], [a(x), a(dy), a(g), a(st), a(dx), a(dg), a(db)])
                one.append(c.run(launch))
                args = (inp['x'][nr], inp['gamma'], inp['beta'], relu, inp['dy'][nr], zero, zero)
                r64.append(H.bn_ref(*args))
                r32 = H.bn_torch32(*args)
                own.append({k: float(np.max(np.abs(r32[k].astype(np.float64) - r64[b][k]))) for k in H.BN_TENSORS})
                scale.append({k: float(np.max(np.abs(r64[b][k]))) for k in H.BN_TENSORS})
            for A in H.SEG_ACTIVE:
                with_out = A != 4                                 # out_stats may be NULL
                node_on = np.broadcast_to((s['node_b'] < A)[:, None], (Nn, D))
                prob_on = np.arange(B) < A
                c, p = _seg_case(s)
                x, g, be, dy = c.inp(inp['x']), c.inp(inp['gamma']), c.inp(inp['beta']), c.inp(inp['dy'])
                y = c.out('y', y_old, writable=node_on)
                st = c.out('stats', st_old, writable=np.broadcast_to(prob_on[:, None, None], (B, 3, D)))
                om = np.zeros((B, L, 2, D), bool)
                om[:A, it] = with_out
                ost = c.out('out_stats', ost_old, writable=om)
                dx, part = c.out('dx', (np.float32, (Nn, D))), c.out('part', (np.float32, (B, 2, D)))

                def launch(a):
                    op('BN_SEG_FWD', _seg_dims(s, A, D, relu, stride), [a(q) for q in p] + [a(x), a(g), a(be), a(y), a(st),
                                                                                              a(ost + it * 2 * D) if with_out else None])
                    op('BN_SEG_BWD', _seg_dims(s, A, D), [a(q) for q in p] + [a(x), a(dy), a(g), a(st), a(dx), a(part)])
                got = c.run(launch)
                tag = (kind, A, D, relu)
                w.exact('BN_SEG_BWD', tag + ('dx of absent problems',), got['dx'][~node_on[:, 0]], np.zeros((int((~node_on[:, 0]).sum()), D), np.float32))
                w.exact('BN_SEG_BWD', tag + ('part of absent problems',), got['part'][A:], np.zeros((B - A, 2, D), np.float32))
                for b in range(A):
                    nr = _problem(s, b)[0]
                    o1 = one[b]
                    mine = dict(y=got['y'][nr], mean=got['stats'][b, 0], invstd=got['stats'][b, 1], var=got['stats'][b, 2], dx=got['dx'][nr],
                                dgamma=got['part'][b, 0], dbeta=got['part'][b, 1])
                    w.exact('BN_SEG_FWD', tag + (b, 'y'), mine['y'], o1['y'])
                    w.exact('BN_SEG_FWD', tag + (b, 'stats'), got['stats'][b], o1['stats'])
                    if with_out:
                        w.exact('BN_SEG_FWD', tag + (b, 'out_stats'), got['out_stats'][b, it], o1['stats'][[0, 2]])
                    w.exact('BN_SEG_BWD', tag + (b, 'dx'), mine['dx'], o1['dx'])
                    w.exact('BN_SEG_BWD', tag + (b, 'part'), got['part'][b], np.stack([o1['dgamma'], o1['dbeta']]))
                    for k in H.BN_TENSORS:
                        assert np.isfinite(mine[k]).all(), (k, tag, b)
                        err = float(np.max(np.abs(mine[k].astype(np.float64) - r64[b][k])))
                        bar = max(1e-4 * scale[b][k], 4 * own[b][k]) + 1e-6
                        rel = err / bar
                        if rel > worst[k][0]:
                            worst[k] = (rel, tag + (b, 'err %.3e own %.3e bar %.3e' % (err, own[b][k], bar)))
                        if err > bar:
                            fail.append((k, tag, b, 'err %.3e > bar %.3e (own %.3e, scale %.3e)' % (err, bar, own[b][k], scale[b][k])))
    for k in H.BN_TENSORS:
        print('[train_ops] BN_SEG %-6s %-7s worst err/bar %.3e at %s' % (kind, k, worst[k][0], worst[k][1]))
    assert not fail, fail[:20]
    w.report()


def test_segmented_batchnorm_dgamma_dbeta():
    w = Worst()
    L, B = 3, 6
    for D in (32, 128):
        rng = np.random.default_rng(600 + D)
        part, dg_old, db_old = (rng.standard_normal(sh).astype(np.float32) for sh in ((L, B, 2, D), (D,), (D,)))
        c = Case()
        p_, g_, b_ = c.inp(part), c.out('dgamma', dg_old), c.out('dbeta', db_old)
        got = c.run(lambda a: op('BN_SEG_DGB', [L, B, D], [a(p_), a(g_), a(b_)]))
        rg, rb = H.bn_seg_dgb_ref(part, dg_old, db_old)
        w.exact('BN_SEG_DGB', (D, 'dgamma'), got['dgamma'], rg)
        w.exact('BN_SEG_DGB', (D, 'dbeta'), got['dbeta'], rb)
    w.report()


# ======================================================================================================================
# the explorer's path with a loop count per graph
# ======================================================================================================================
@pytest.mark.parametrize('D', [32, 64])
def test_final_cat(D):
    w = Worst()
    for t, rows in enumerate(H.FINAL_CAT_TABLES):
        rng = np.random.default_rng(700 + D + t)
        n_it, R = len(rows), rows[0]
        stride = R * D + 192                                     # the slabs lie apart, the sentinel between them
        NC, Hs = rng.standard_normal((R, D)).astype(np.float32), rng.standard_normal((n_it, R, D)).astype(np.float32)
        slabs = np.full(n_it * stride, SENT, np.uint32).view(np.float32)
        for i in range(n_it):
            slabs[i * stride:i * stride + R * D] = Hs[i].reshape(-1)
        c = Case()
        n_, h_, o = c.inp(NC), c.inp(slabs), c.out('out', (np.float32, (R, 2 * D)))
        got = c.run(lambda a: op('FINAL_CAT', [D, stride, n_it] + list(rows), [a(n_), a(h_), a(o)]))['out']
        w.exact('FINAL_CAT', (D, n_it, R), got, H.final_cat_ref(rows, NC, Hs))
    w.report()


@pytest.mark.parametrize('D', [32, 64])
def test_seed_dh(D):
    w = Worst()
    R = 1024
    rng = np.random.default_rng(800 + D)
    d_dec, dXin = rng.standard_normal((R, D)).astype(np.float32), rng.standard_normal((R, 4 * D)).astype(np.float32)
    for nxt in (0, 256, 768, 1024):
        c = Case()
        d_, x_, o = c.inp(d_dec), c.inp(dXin), c.out('dH', (np.float32, (R, D)))
        got = c.run(lambda a: op('SEED_DH', [R, nxt, D], [a(d_), a(x_), a(o)]))['dH']
        w.exact('SEED_DH', (D, R, nxt), got, H.seed_dh_ref(nxt, d_dec, dXin))
    w.report()


def test_linear_dw_order():
    """dW / db of a call over the first R rows in the order of R_order rows: bit-equal to LINEAR_DW over R_order rows whose dY rows
    >= R are zero (X is random there), and inside LINEAR_DW's bound of float64.  Where the order changes the width of the second
    stage's slices the result is NOT that of LINEAR_DW at R rows: at least one case shows it."""
    w = Worst()
    seen, differs = set(), 0
    for i, (K, O) in enumerate(H.DW_ORDER_PAIRS):
        path = _lib.train_op_path('LINEAR_DW_ORDER', 256, K, O)
        assert path == H.expected_path('LINEAR_DW', K, O) == _lib.train_op_path('LINEAR_DW', 256, K, O)
        seen.add(path)
        for j, (R, Ro) in enumerate(H.DW_ORDER_ROWS):
            X, W0, b0, _, rng = _gemm_inputs(Ro, K, O, 30000 + 10 * i + j)
            dY = rng.standard_normal((R, O)).astype(np.float32)
            dY_all = np.concatenate([dY, np.zeros((Ro - R, O), np.float32)])

            def run(name, dims, dy_rows, x_rows):
                c = Case()
                dy, x, dw, db = c.inp(dy_rows), c.inp(x_rows), c.out('dW', W0), c.out('db', b0)
                sc = c.out('scratch', np.full(_lib.train_dw_scratch_floats(len(dy_rows), K, O), np.nan, np.float32))
                return c.run(lambda a: op(name, dims, [a(dy), a(x), a(dw), a(db), a(sc)]))
            got = run('LINEAR_DW_ORDER', [R, K, O, Ro], dY, X[:R])
            full = run('LINEAR_DW', [Ro, K, O], dY_all, X)
            w.exact('LINEAR_DW_ORDER', (R, Ro, K, O, 'dW'), got['dW'], full['dW'])
            w.exact('LINEAR_DW_ORDER', (R, Ro, K, O, 'db'), got['db'], full['db'])
            rW, bW, rb, bb = H.linear_dw_ref(dY, X[:R], W0, b0)
            w.bounded('LINEAR_DW_ORDER', (R, Ro, K, O, 'dW'), got['dW'], rW, bW, path)
            w.bounded('LINEAR_DW_ORDER', (R, Ro, K, O, 'db'), got['db'], rb, bb, path)
            if H.dw_slice_width(R) != H.dw_slice_width(Ro):
                plain = run('LINEAR_DW', [R, K, O], dY, X[:R])
                differs += int(not np.array_equal(plain['dW'].view(np.uint32), got['dW'].view(np.uint32)))
    assert seen == {'mfma', 'plain'}
    print('[train_ops] LINEAR_DW_ORDER      cases whose bits differ from LINEAR_DW over the R rows alone: %d' % differs)
    assert differs > 0
    w.report()
