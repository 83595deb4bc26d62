"""The oracle path smoother without a GPU: the host restatement (tests/oracle_smooth_host.py) against the recorded runs of
the unmodified reference (tests/golden/oracle_smooth_*.npz, tools/gen_golden_oracle_smooth.py) bit for bit -- paths,
float32 flags, lengths and collision-check counts after every stage -- and the C ABI's symbols and argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import gnnmp  # noqa: F401
from gnnmp import _lib

import oracle_smooth_host as H

FIX = H.fixtures()
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_NULL, ERR_DIMS, ERR_ARG = 0, -1, -2, -6


def test_the_issue_s_cases_are_all_recorded():
    assert len(FIX) >= 16
    ordinary = [n for n, f in FIX.items() if re.fullmatch(r'p\d+', n)]
    assert len(ordinary) >= 6 and all(5 <= len(FIX[n]['path']) <= 30 for n in ordinary)
    assert {len(FIX[n]['path']) for n in ('len1', 'len2', 'len3')} == {1, 2, 3}
    assert sum(1 for f in FIX.values() if not bool(f['in32'])) >= 2
    assert sum(1 for f in FIX.values() if not bool(f['ratio'])) >= 2
    assert {'keepall', 'drop3', 'f64end', 'abort'} <= set(FIX)
    assert int(FIX['abort']['status']) == H.STATUS_UNREACHABLE
    # mixed precision is real: a float32-input run ends with float32 end points and float64 waypoints between them
    # (a path pruned down to start -> goal is re-spaced between two float32 ends and stays float32 throughout)
    assert all(FIX[n]['result_is32'][0] and FIX[n]['result_is32'][-1] for n in ordinary)
    assert sum(1 for n in ordinary if not FIX[n]['result_is32'][1:-1].any()) >= 3
    assert sum(1 for n in ordinary if FIX[n]['result_is32'][1:-1].all()) >= 1


@pytest.mark.parametrize('name', sorted(FIX))
def test_host_restatement_equals_the_reference_bit_for_bit(name):
    fx = FIX[name]
    trace = []
    xy, f32, checks, status = H.smooth(fx['path'].astype(np.float64), bool(fx['in32']), fx['map'], fx['action'],
                                       node_idx=fx['node_idx'], iters=int(fx['iters']), random_iter=int(fx['random_iter']),
                                       prune_iter=int(fx['prune_iter']), ratio=bool(fx['ratio']), trace=trace)
    assert status == int(fx['status'])
    assert xy.shape == fx['result'].shape and xy.tobytes() == fx['result'].tobytes()
    assert (f32 == fx['result_is32']).all() and checks == int(fx['checks'])
    stages = H.fixture_stages(fx)
    assert len(stages) == len(trace) == 3 * int(fx['iters'])
    for (kind, _, sxy, s32, schecks), (hkind, hxy, h32, hchecks) in zip(stages, trace):
        assert kind == hkind and len(sxy) == len(hxy)
        assert sxy.tobytes() == hxy.tobytes() and (s32 == h32).all() and schecks == hchecks, (name, kind)


def test_device_form_index_rule_covers_its_range():
    for n in (3, 4, 17, H.CAP):
        idx = {H.node_index(u, n) for u in np.linspace(0.0, np.nextafter(1.0, 0.0), 4001)}
        assert idx == set(range(1, n - 1))


def test_stop_stages_and_status_bits():
    fx = FIX['drop3']
    args = (fx['path'].astype(np.float64), True, fx['map'], fx['action'])
    stages = H.fixture_stages(fx)
    for s, (kind, it, sxy, s32, schecks) in enumerate(stages):
        if kind == 'iter':
            continue
        xy, f32, checks, status = H.smooth(*args, node_idx=fx['node_idx'], iters=it + 1,
                                           stop=H.STOP_RANDOM if kind == 'random' else H.STOP_PRUNE)
        assert xy.tobytes() == sxy.tobytes() and (f32 == s32).all() and checks == schecks and status == 0
    dup = args[0].copy()
    dup[3] = dup[1]
    xy, _, checks, status = H.smooth(dup, True, fx['map'], fx['action'], node_idx=fx['node_idx'])
    assert status == H.STATUS_DUPLICATE and checks == 0 and xy.tobytes() == dup.tobytes()
    long = np.linspace(-0.9, 0.9, 2 * (H.CAP + 1)).reshape(-1, 2)
    assert H.smooth(long, True, fx['map'], fx['action'], node_idx=fx['node_idx'])[3] == H.STATUS_CAP


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_oracle_smooth_symbols_are_exported_and_mirrored():
    L = ctypes.CDLL(_lib.LIB_PATH)
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'gnnmp.h')).read(), flags=re.S)
    names = sorted(set(re.findall(r'\b(gnnmp_oracle_smooth[a-z0-9_]*)\s*\(', text)))
    assert names == ['gnnmp_oracle_smooth', 'gnnmp_oracle_smooth_limits']
    assert all(hasattr(L, n) for n in names)
    body = re.search(r'typedef struct\s*\{([^}]*)\}\s*gnnmp_oracle_smooth_batch;', text, flags=re.S).group(1)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            fields.extend(x.split()[-1].lstrip('*') for x in decl.split(','))
    assert [f[0] for f in _lib.OracleSmoothBatch._fields_] == fields
    a, b = ctypes.c_int32(), ctypes.c_int32()
    assert _lib.lib().gnnmp_oracle_smooth_limits(ctypes.byref(a), ctypes.byref(b)) == OK
    assert (a.value, b.value) == (H.CAP, 64)
    assert _lib.lib().gnnmp_oracle_smooth_limits(None, ctypes.byref(b)) == ERR_NULL


def test_oracle_smooth_rejects_bad_arguments_before_touching_the_device():
    """Fake non-null pointers: every case here must be refused by the argument checks, so nothing is dereferenced."""
    L = _lib.lib()
    P = 0x1000

    def batch(**kw):
        d = dict(n_paths=2, total_points=10, dim=2, width=15, iters=5, random_iter=100, prune_iter=100, ratio=1, stop=0,
                 path_ptr=P, paths=P, is32=None, maps=P, action=P, node_idx=P, u=None)
        d.update(kw)
        return _lib.OracleSmoothBatch(*[d[f[0]] for f in _lib.OracleSmoothBatch._fields_])

    def call(b, out=P, out32=P, out_len=P, checks=P, status=P):
        return L.gnnmp_oracle_smooth(ctypes.byref(b) if b is not None else None, out, out32, out_len, checks, status, None)

    assert call(None) == ERR_NULL
    for k in ('out', 'out32', 'out_len', 'checks', 'status'):
        assert call(batch(), **{k: None}) == ERR_NULL, k
    for k in ('path_ptr', 'paths', 'maps', 'action'):
        assert call(batch(**{k: None})) == ERR_NULL, k
    assert call(batch(node_idx=None, u=None)) == ERR_NULL                   # neither form of the index draws
    for dim in (0, 1, 3, 7):
        assert call(batch(dim=dim)) == ERR_DIMS
    for w in (0, -3, 65):
        assert call(batch(width=w)) == ERR_DIMS                              # a map the kernel cannot hold
    for kw in (dict(n_paths=-1), dict(total_points=-1), dict(iters=-1), dict(random_iter=-2), dict(prune_iter=-1),
               dict(stop=3), dict(stop=-1), dict(ratio=2)):
        assert call(batch(**kw)) == ERR_ARG, kw
    assert call(batch(n_paths=0, path_ptr=None, maps=None, paths=None, action=None, node_idx=None)) == OK   # empty batch
