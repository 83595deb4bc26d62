"""The oracle path smoother for the stick robot (MazeEnv(dim=3)) without a GPU: the host restatement
(tests/oracle_smooth3_host.py) against the recorded runs of the unmodified reference (tests/golden/oracle_smooth3_*.npz,
tools/gen_golden_oracle_smooth3.py) bit for bit -- paths, float32 flags, lengths and collision-check counts after every
stage --, what the recordings cover, the norm formulas the device kernel uses against numpy's, and the C ABI's new entry
point and its argument checks."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import gnnmp  # noqa: F401
from gnnmp import _lib

import oracle_smooth3_host as H3
import oracle_smooth_host as H

FIX = H3.fixtures()
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_NULL, ERR_DIMS, ERR_ARG = 0, -1, -2, -6
ENTRY = 'gnnmp_stick_oracle_smooth'


def host_run(fx, **kw):
    args = dict(node_idx=fx['node_idx'], iters=int(fx['iters']), random_iter=int(fx['random_iter']),
                prune_iter=int(fx['prune_iter']), ratio=bool(fx['ratio']))
    args.update(kw)
    return H3.smooth(fx['path'].astype(np.float64), bool(fx['in32']), fx['map'], fx['action'], **args)


def kept_sources(fx):
    """For every (random, prune) stage pair of a fixture: (indices the pruned waypoints had in the random stage's path,
    that path's float32 flags)."""
    st = H3.fixture_stages(fx)
    out = []
    for (k0, _, x0, f0, _), (k1, _, x1, _, _) in zip(st[:-1], st[1:]):
        if k0 == 'random' and k1 == 'prune':
            pos = {tuple(r): i for i, r in enumerate(x0)}
            out.append(([pos[tuple(r)] for r in x1], f0))
    return out


def test_the_issue_s_cases_are_all_recorded():
    assert len(FIX) >= 12
    assert all(f['path'].shape[1] == 3 and f['action'].shape[-1] == 3 and f['result'].shape[1] == 3 for f in FIX.values())
    assert all(int(f['status']) == 0 for f in FIX.values())                 # neither a tie nor identical waypoints
    assert sum(1 for f in FIX.values() if bool(f['in32'])) >= 6
    assert sum(1 for f in FIX.values() if not bool(f['in32'])) >= 1          # the all-float64 route
    assert sum(1 for f in FIX.values() if not bool(f['ratio'])) >= 1         # joint_smoother
    assert {len(FIX[n]['path']) for n in ('len1', 'len2', 'len3')} == {1, 2, 3}
    assert int(FIX['short']['iters']) < 5 and int(FIX['short']['random_iter']) < 100
    # a prune that keeps everything; one that drops >= 3 waypoints in a row
    assert any(len(src) == len(f0) for src, f0 in kept_sources(FIX['keepall']))
    assert any(b - a >= 4 for src, _ in kept_sources(FIX['drop3']) for a, b in zip(src[:-1], src[1:]))
    # a consecutive pair of the input with |dz| > 0.4: its edge is interpolated along the wrapped displacement
    fx = FIX['wrap']
    dz = np.abs(np.diff(fx['path'][:, 2].astype(np.float64)))
    assert len(fx['wrap_pairs']) >= 1 and (dz[fx['wrap_pairs']] > 0.4).all()
    # trials rejected because z left +-0.4 (recorded as [iteration, trial]; recomputed here)
    fx = FIX['zreject']
    assert len(fx['z_rejected']) >= 1
    assert H3.z_rejected_trials(fx['path'].astype(np.float64), True, fx['map'], fx['action'], fx['node_idx']) == \
        [tuple(r) for r in fx['z_rejected'].tolist()]
    # mixed float32 / float64 edge checks: float32-input runs in which a random stage leaves a float64 waypoint next to a
    # float32 one (the prune's edge checks between them follow)
    mixed = [n for n, f in FIX.items() if bool(f['in32']) and any(
        kind == 'random' and (s32[:-1] != s32[1:]).any() for kind, _, _, s32, _ in H3.fixture_stages(f))]
    assert len(mixed) >= 3, mixed


@pytest.mark.parametrize('name', sorted(FIX))
def test_host_restatement_equals_the_reference_bit_for_bit(name):
    fx = FIX[name]
    trace = []
    xyz, f32, checks, status = host_run(fx, trace=trace)
    assert status == int(fx['status']) == 0
    assert xyz.shape == fx['result'].shape and xyz.tobytes() == fx['result'].tobytes()
    assert (f32 == fx['result_is32']).all() and checks == int(fx['checks'])
    stages = H3.fixture_stages(fx)
    assert len(stages) == len(trace) == 3 * int(fx['iters'])
    for (kind, _, sxy, s32, schecks), (hkind, hxy, h32, hchecks) in zip(stages, trace):
        assert kind == hkind and len(sxy) == len(hxy)
        assert sxy.tobytes() == hxy.tobytes() and (s32 == h32).all() and schecks == hchecks, (name, kind)


def test_stop_stages_and_status_bits():
    fx = FIX['short']
    for kind, it, sxy, s32, schecks in H3.fixture_stages(fx):
        if kind == 'iter':
            continue
        xyz, f32, checks, status = host_run(fx, iters=it + 1, stop=H.STOP_RANDOM if kind == 'random' else H.STOP_PRUNE)
        assert xyz.tobytes() == sxy.tobytes() and (f32 == s32).all() and checks == schecks and status == 0
    dup = fx['path'].astype(np.float64)
    dup[3] = dup[1]
    xyz, _, checks, status = H3.smooth(dup, True, fx['map'], fx['action'], node_idx=fx['node_idx'])
    assert status == H.STATUS_DUPLICATE and checks == 0 and xyz.tobytes() == dup.tobytes()
    dup = fx['path'].astype(np.float64)
    dup[3, :2] = dup[1, :2]                                                  # same place, another orientation: no duplicate
    assert H3.smooth(dup, True, fx['map'], fx['action'], node_idx=fx['node_idx'], iters=1, random_iter=2)[3] == 0
    long = np.linspace(-0.3, 0.3, 3 * (H3.CAP + 1)).reshape(-1, 3)
    assert H3.smooth(long, True, fx['map'], fx['action'], node_idx=fx['node_idx'])[3] == H.STATUS_CAP


def test_stick_checker_rules():
    """The rules a recording pins only in sum, one at a time on an empty map."""
    env = H3.Maze3(np.zeros((15, 15), np.uint8))
    p32 = np.array([0.2, -0.3, 0.1], np.float32)
    a, b = H3.Maze3.ends(p32)
    assert a.dtype == b.dtype == np.float64                                  # float64 ends of a float32 state
    assert env.state_fp(p32) and env.count >= 2                              # both ends, then the bisection's midpoints
    one = env.count
    env.count = 0
    assert env.state_fp(p32.astype(np.float64)) and env.count == one         # the stick check ignores the state's dtype
    env.count = 0
    for bad in ([0.2, -0.3, 0.41], [0.2, -0.3, -0.4000001], [1.01, 0.0, 0.0]):
        assert not env.state_fp(np.array(bad)) and env.count == 0           # _valid_state first: nothing counted
        assert not env.edge_fp(np.array(bad), p32) and not env.edge_fp(p32, np.array(bad)) and env.count == 0
    assert not env.state_fp(np.array([0.95, 0.0, 0.0])) and env.count == 1  # first end counted, second out of the map
    # |dz| = 0.78 wraps to 0.02: K = int(0.02 / 0.015) = 1, no interpolated stick, only the two sticks themselves
    s, t = np.array([0.0, 0.0, 0.39]), np.array([0.0, 0.0, -0.39])
    env.count = 0
    assert env.state_fp(s) and env.state_fp(t)
    two = env.count
    env.count = 0
    assert env.edge_fp(s, t) and env.count == two
    # without the wrap the same |dz| inside the range is 52 steps
    env.count = 0
    assert env.edge_fp(np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.39])) and env.count > two + 2 * 20
    # dtype flows: the mixed pair takes the float64 flow on exactly upcast values
    s32, t32 = np.array([-0.5, 0.1, 0.3], np.float32), np.array([0.4, -0.2, -0.35], np.float32)
    counts = []
    for s, t in ((s32.astype(np.float64), t32.astype(np.float64)), (s32, t32.astype(np.float64)),
                 (s32.astype(np.float64), t32)):
        env.count = 0
        assert env.edge_fp(s, t)
        counts.append(env.count)
    assert counts[0] == counts[1] == counts[2]


def _fma(a, b, c):
    """round_to_nearest_even(a * b + c) of doubles, exactly."""
    r = Fraction(a) * Fraction(b) + Fraction(c)
    f = float(r)                                                             # Fraction -> float rounds correctly
    return f


def test_device_norm_formulas_equal_numpy_on_recorded_vectors():
    """np.linalg.norm of a 3-vector is the host BLAS's dot; the kernel restates it as float64 fma(d2, d2, fma(d1, d1,
    d0 * d0)) and float32 'squares rounded to float32, summed left to right in double, rounded once'.  Both against numpy
    on differences of recorded waypoints (float32 pairs from the inputs, float64 pairs from the stages)."""
    n32 = n64 = 0
    for fx in FIX.values():
        p = fx['path'].astype(np.float32)
        for a, b in zip(p[:-1], p[1:]):
            d = a - b
            sq = (d * d).astype(np.float32)
            acc = (np.float64(sq[0]) + np.float64(sq[1])) + np.float64(sq[2])
            assert np.sqrt(np.float32(acc)) == np.linalg.norm(d), (a, b)
            n32 += 1
        x = fx['stage_xy']
        for a, b in zip(x[:-1:7], x[1::7]):
            d = a - b
            acc = _fma(d[2], d[2], _fma(d[1], d[1], d[0] * d[0]))
            assert np.sqrt(np.float64(acc)) == np.linalg.norm(d), (a, b)
            n64 += 1
    assert n32 >= 50 and n64 >= 50


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_stick_entry_point_is_declared_exported_and_shares_the_batch_struct():
    L = ctypes.CDLL(_lib.LIB_PATH)
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'gnnmp.h')).read(), flags=re.S)
    decl = re.search(r'int\s+%s\s*\(([^)]*)\)' % ENTRY, text, flags=re.S)
    assert decl and decl.group(1).split(',')[0].split() == ['const', 'gnnmp_oracle_smooth_batch*', 'batch']
    assert hasattr(L, ENTRY)
    assert [f[0] for f in _lib.OracleSmoothBatch._fields_] == [
        'n_paths', 'total_points', 'dim', 'width', 'iters', 'random_iter', 'prune_iter', 'ratio', 'stop', 'path_ptr', 'paths',
        'is32', 'maps', 'action', 'node_idx', 'u']


def test_stick_entry_point_rejects_bad_arguments_before_touching_the_device():
    """Fake non-null pointers: every case here must be refused by the argument checks, so nothing is dereferenced.  The
    checks and their order are gnnmp_oracle_smooth's."""
    L = _lib.lib()
    P = 0x1000

    def batch(**kw):
        d = dict(n_paths=2, total_points=10, dim=3, width=15, iters=5, random_iter=100, prune_iter=100, ratio=1, stop=0,
                 path_ptr=P, paths=P, is32=None, maps=P, action=P, node_idx=P, u=None)
        d.update(kw)
        return _lib.OracleSmoothBatch(*[d[f[0]] for f in _lib.OracleSmoothBatch._fields_])

    def call(b, out=P, out32=P, out_len=P, checks=P, status=P, fn=ENTRY):
        return getattr(L, fn)(ctypes.byref(b) if b is not None else None, out, out32, out_len, checks, status, None)

    assert call(None) == ERR_NULL
    for k in ('out', 'out32', 'out_len', 'checks', 'status'):
        assert call(batch(), **{k: None}) == ERR_NULL, k
    for k in ('path_ptr', 'paths', 'maps', 'action'):
        assert call(batch(**{k: None})) == ERR_NULL, k
    assert call(batch(node_idx=None, u=None)) == ERR_NULL                   # neither form of the index draws
    for dim in (0, 1, 2, 7):
        assert call(batch(dim=dim)) == ERR_DIMS
    assert call(batch(dim=3), fn='gnnmp_oracle_smooth') == ERR_DIMS          # the point robot's entry point still refuses 3
    for w in (0, -3, 65):
        assert call(batch(width=w)) == ERR_DIMS                              # a map the kernel cannot hold
    assert call(batch(dim=2, n_paths=-1)) == ERR_DIMS                        # the order: dimensions before scalars
    for kw in (dict(n_paths=-1), dict(total_points=-1), dict(iters=-1), dict(random_iter=-2), dict(prune_iter=-1),
               dict(stop=3), dict(stop=-1), dict(ratio=2)):
        assert call(batch(**kw)) == ERR_ARG, kw
    assert call(batch(n_paths=0, path_ptr=None, maps=None, paths=None, action=None, node_idx=None)) == OK   # empty batch
