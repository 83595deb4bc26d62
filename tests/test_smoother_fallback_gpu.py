"""The flag-timeout fallback of the smoother's two d = 128 message kernels (sm_msg_split_kernel, sm_msg_stream_kernel), bit for bit.

An edge workgroup whose targets' flags do not arrive within its polling budget computes the target half b00 + (W_c - W_a) x_i
itself.  GNNMP_SM_FORCE_FALLBACK (read per forward call) makes the FORCE instantiations of the two kernels take that path without
polling: 1 = every edge tile (split) / edge round (stream), 2 = the even tiles / a workgroup's visits 0, 2, 4, ..., 3 = the odd
ones.  Target workgroups still run and publish, so a launch mixes both paths.  g_sm_fallbacks (gnnmp_debug_sm_fallbacks, bound here
with ctypes) counts the forced fallbacks taken, so a misspelt switch cannot pass vacuously.

GNNMP_SM_STREAM is read once per process: every case runs in two fresh child processes (this file as a script), one per value, one
at a time; a child walks the modes in-process and saves its outputs and counts with torch.save.  Shapes are the smallest at which
the bookkeeping can go wrong: ragged problems of 20-40 waypoints (one or two path tiles) plus problems of 2, 3 and 33 waypoints,
40-300 free and 10-200 collided samples (>= 10 in total: exactly 10 kNN in-edges per waypoint), chain edges, loops 1 and 3, and as
many problems as give the stream kernel more than two rounds per CU (so some workgroup goes fallback -> normal -> fallback in mode
2 and the opposite in mode 3: the slot parity of every round after a fallback round flips, 9 columns against 0)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from conftest import REPO, load_weights

pytestmark = pytest.mark.gpu

CKPT = {14: 'smooth_14d_attv3', 2: 'smooth_2d_attv3'}
K = 10                  # kNN in-edges per waypoint (kSmK)


def n_waypoints(i, layout):
    if layout == 'B':                                  # the second layout of the workspace-reuse runs: other counts, same C
        return 40 - (5 * i) % 21
    if i % 50 == 7:
        return 2
    if i % 50 == 19:
        return 3
    if i % 50 == 31:
        return 33
    return 20 + (11 * i) % 21


def problem(C, i, layout='A'):
    """Problem i of a layout: (path, free, collided, edge_index), its own generator, so the parent can rebuild single problems."""
    from gnnmp.planner import chain_edge_index
    gen = torch.Generator().manual_seed(7001 + 2 * i + (layout == 'B'))
    P = n_waypoints(i, layout)
    mk = lambda n: torch.rand(n, C, generator=gen) * 2 - 1  # noqa: E731
    return mk(P), mk(40 + (13 * i) % 261), mk(10 + (11 * i) % 191), chain_edge_index(P)


def edge_tiles(P):
    """32-edge tiles in use of a problem of P waypoints: 10 sample in-edges per waypoint + the chain's 3 P - 2 path-to-path edges
    (sources of the first are sample nodes, so nothing coalesces away)."""
    return (K * P + 3 * P - 2 + 31) // 32


def large_count(cus):
    """Smallest number of problems with sum_b ceil(10 P_b / 32) > 8 * 2 * CUs: more than two 8-tile rounds per resident edge
    workgroup of the stream kernel, whatever the path-to-path edges add."""
    n = tiles = 0
    while tiles <= 8 * 2 * cus or n < 60:
        tiles += (K * n_waypoints(n, 'A') + 31) // 32
        n += 1
    return n


# ------------------------------------------------------------------------------------------------------------------------------
# child process: `python test_smoother_fallback_gpu.py child <C> <case> <n_prob> <out>`
# ------------------------------------------------------------------------------------------------------------------------------
def _child(C, case, n_prob, out_path):
    import gnnmp
    from gnnmp import _lib
    from gnnmp.weights import load_weights as package_weights
    L = _lib.lib()
    L.gnnmp_debug_sm_fallbacks.restype = ctypes.c_int
    L.gnnmp_debug_sm_fallbacks.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]

    def fallbacks():
        v = ctypes.c_ulonglong(1 << 60)
        assert L.gnnmp_debug_sm_fallbacks(ctypes.byref(v), 1) == 0
        return int(v.value)

    def model():
        m = gnnmp.ModelSmoother(workspace_size=3, config_size=C, embed_size=128, obs_size=6).eval()
        m.load_state_dict(package_weights(CKPT[C]))
        if case == 'bf16':
            m.mlp_dtype = 'bf16'
        return m

    def batch(n, layout):
        ps = [problem(C, i, layout) for i in range(n)]
        return gnnmp.SmoothBatch([p[0] for p in ps], [p[1] for p in ps], [p[2] for p in ps], [p[3] for p in ps], 'cuda:0')

    def run(m, sb, loop, mode):
        if mode is None:
            os.environ.pop('GNNMP_SM_FORCE_FALLBACK', None)          # absent = off, like '0'
        else:
            os.environ['GNNMP_SM_FORCE_FALLBACK'] = str(mode)
        fallbacks()
        out = m.forward_batch(sb, loop)
        cnt = fallbacks()
        m.check_status(sb)                                           # the blocking read of this layout's status words
        return out.cpu(), cnt

    # workspaces come from torch.empty: leave NaN (non-zero as flags and counters) in the allocator's free blocks
    junk = torch.full((64 << 20,), float('nan'), device='cuda:0')
    del junk
    res = {}
    m = model()
    A = batch(n_prob, 'A')
    for loop in (1, 3):
        for mode in ((0, 1) if case == 'small' else (0, 1, 2, 3)):
            res['out_loop%d_mode%d' % (loop, mode)], res['cnt_loop%d_mode%d' % (loop, mode)] = \
                run(m, A, loop, None if (mode == 0 and loop == 3) else mode)
    if case == 'large':
        # one module, one stream, one workspace: A, then a smaller batch of another layout (its carve puts the flags, the target
        # rows and the tile counters elsewhere, over A's leftovers), then A again
        B = batch(n_prob // 3 + 5, 'B')
        for mode in (0, 2):
            res['reuse_a1_mode%d' % mode] = run(m, A, 3, mode)[0]
            res['reuse_b_mode%d' % mode] = run(m, B, 3, mode)[0]
            res['reuse_a2_mode%d' % mode] = run(m, A, 3, mode)[0]
            res['reuse_b_fresh_mode%d' % mode] = run(model(), B, 3, mode)[0]
    torch.save(res, out_path)


if __name__ == '__main__':
    assert sys.argv[1] == 'child'
    _child(int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), sys.argv[5])
    sys.exit(0)


# ------------------------------------------------------------------------------------------------------------------------------
CASES = [(14, 'large'), (2, 'large'), (14, 'small'), (2, 'small')]
LARGE = [c for c in CASES if c[1] == 'large']
SMALL_N = 37            # fewer rounds than CUs: one visit per workgroup of the stream kernel


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def n_problems(case):
    return large_count(cu_count()) if case == 'large' else SMALL_N


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """runs(C, case, stream) -> what the child of that case saved; every child runs once per module, one at a time.
    stream: '0' (split kernel), '1' (streamed-weights kernel), None (the library's own choice: the bf16 case)."""
    done = {}
    tmp = tmp_path_factory.mktemp('sm_fallback')

    def get(C, case, stream):
        key = (C, case, stream)
        if key not in done:
            out = str(tmp / ('c%d_%s_%s.pt' % key))
            env = dict(os.environ)
            env.pop('GNNMP_SM_FORCE_FALLBACK', None)
            env.pop('GNNMP_SM_STREAM', None)
            if stream is not None:
                env['GNNMP_SM_STREAM'] = stream
            subprocess.run([sys.executable, os.path.abspath(__file__), 'child', str(C), case, str(n_problems(case)), out],
                           check=True, env=env, timeout=300, cwd=REPO)
            done[key] = torch.load(out)
        return done[key]
    return get


def modes_of(case):
    return (0, 1) if case == 'small' else (0, 1, 2, 3)


def test_large_case_gives_three_visits():
    """sum_b ceil(10 P_b / 32) > 8 * 2 * CUs: the stream kernel's edge rounds outnumber twice its resident edge workgroups."""
    n = n_problems('large')
    waypoints = [n_waypoints(i, 'A') for i in range(n)]
    assert sum((K * P + 31) // 32 for P in waypoints) > 8 * 2 * cu_count()
    assert {2, 3, 33} <= set(waypoints) and min(w for w in waypoints if w > 3) == 20 and max(waypoints) == 40


@pytest.mark.parametrize('C,case', CASES)
def test_forced_fallback_same_bits(C, case, runs):
    """Every mode of the stream kernel and of the split kernel gives the bits of the unforced stream run, loops 1 and 3."""
    st, sp = runs(C, case, '1'), runs(C, case, '0')
    for loop in (1, 3):
        base = st['out_loop%d_mode0' % loop]
        assert bool(torch.isfinite(base).all())
        for mode in modes_of(case):
            k = 'out_loop%d_mode%d' % (loop, mode)
            assert bool(torch.isfinite(st[k]).all()) and bool(torch.isfinite(sp[k]).all()), k
            assert torch.equal(st[k], base), ('stream', k)
            assert torch.equal(sp[k], sp['out_loop%d_mode0' % loop]), ('split', k)
            assert torch.equal(sp[k], base), ('split vs stream', k)


@pytest.mark.parametrize('C,case', CASES)
def test_forced_fallback_counters(C, case, runs):
    """The forced fallbacks really ran: none in mode 0, one per edge tile in use (split) / per 8-tile round (stream) in mode 1, the
    even and the odd ones add up, three iterations take three times as many (the edge count per problem never changes: 10 sample
    in-edges per waypoint + the chain), and the stream child's count is rounds, not tiles."""
    st, sp = runs(C, case, '1'), runs(C, case, '0')
    cus, n = cu_count(), n_problems(case)
    tiles = sum(edge_tiles(n_waypoints(i, 'A')) for i in range(n))
    rounds = (tiles + 7) // 8
    cnt = lambda r, loop, mode: r['cnt_loop%d_mode%d' % (loop, mode)]  # noqa: E731
    for r in (st, sp):
        for loop in (1, 3):
            assert cnt(r, loop, 0) == 0
            assert cnt(r, loop, 1) > 0
            if case == 'large':
                assert cnt(r, loop, 2) > 0 and cnt(r, loop, 3) > 0
                assert cnt(r, loop, 2) + cnt(r, loop, 3) == cnt(r, loop, 1)
        for mode in modes_of(case)[1:]:
            assert cnt(r, 3, mode) == 3 * cnt(r, 1, mode), mode
    assert cnt(st, 1, 1) == (cnt(sp, 1, 1) + 7) // 8          # rounds against tiles: the stream child ran the stream kernel
    assert cnt(sp, 1, 1) == tiles and cnt(st, 1, 1) == rounds
    if case == 'large':
        # one resident edge workgroup per CU takes rounds w, w + CUs, w + 2 CUs, ...: round r is visit r // CUs of its workgroup
        assert rounds > 2 * cus                                 # some workgroup makes at least three visits
        odd = sum(1 for r in range(rounds) if (r // cus) & 1)
        assert cnt(st, 1, 3) == odd and cnt(st, 1, 2) == rounds - odd
    else:
        assert rounds < cus                                     # one visit each


@pytest.mark.parametrize('C,case', LARGE)
def test_forced_fallback_against_reference(C, case, runs):
    """So that 'all forms equally wrong' cannot pass: four problems of the all-fallback stream run (the first, a 33-waypoint one,
    a 3-waypoint one, the last) against the CPU oracle, at tests/test_smoother_parity.py's bar."""
    from oracle import ref_cpu
    out = runs(C, case, '1')['out_loop3_mode1']
    n = n_problems(case)
    waypoints = [n_waypoints(i, 'A') for i in range(n)]
    assert out.shape[0] == sum(waypoints)
    w = load_weights(CKPT[C])
    for i in (0, waypoints.index(33), waypoints.index(3), n - 1):
        path, free, coll, ei = problem(C, i)
        ref = ref_cpu.smoother_forward(w, path, free, coll, ei, loop=3)
        got = out[sum(waypoints[:i]):sum(waypoints[:i + 1])]
        assert torch.allclose(got, ref, rtol=1e-5, atol=1e-5), (i, (got - ref).abs().max())


def test_forced_fallback_bf16(runs):
    """bf16 operands: the split kernels (a batch under 2048 edge tiles of capacity), modes 1-3 equal mode 0 bitwise."""
    waypoints = [n_waypoints(i, 'A') for i in range(SMALL_N)]
    capacity = sum(3 * P - 2 for P in waypoints) + K * sum(waypoints) + 64 * SMALL_N + 32        # sm_carve's ecap
    assert (capacity + 31) // 32 < 2048
    r = runs(14, 'bf16', None)
    tiles = sum(edge_tiles(P) for P in waypoints)
    for loop in (1, 3):
        base = r['out_loop%d_mode0' % loop]
        assert bool(torch.isfinite(base).all())
        for mode in (1, 2, 3):
            assert torch.equal(r['out_loop%d_mode%d' % (loop, mode)], base), (loop, mode)
        assert r['cnt_loop%d_mode0' % loop] == 0
        assert r['cnt_loop%d_mode1' % loop] == loop * tiles
        assert r['cnt_loop%d_mode2' % loop] > 0 and r['cnt_loop%d_mode3' % loop] > 0
        assert r['cnt_loop%d_mode2' % loop] + r['cnt_loop%d_mode3' % loop] == r['cnt_loop%d_mode1' % loop]


@pytest.mark.parametrize('stream', ['1', '0'])
@pytest.mark.parametrize('C,case', LARGE)
def test_workspace_reuse_across_layouts(C, case, stream, runs):
    """Batch A, a smaller batch B of another layout, A again -- one module, one stream, one workspace, flags in play: B equals B
    from a fresh module and the second A the first, unforced and with every other tile / visit falling back."""
    r = runs(C, case, stream)
    for mode in (0, 2):
        a1, a2 = r['reuse_a1_mode%d' % mode], r['reuse_a2_mode%d' % mode]
        b, bf = r['reuse_b_mode%d' % mode], r['reuse_b_fresh_mode%d' % mode]
        assert bool(torch.isfinite(b).all())
        assert torch.equal(a1, r['out_loop3_mode0'])
        assert torch.equal(a2, a1), mode
        assert torch.equal(b, bf), mode
    assert torch.equal(r['reuse_b_mode2'], r['reuse_b_mode0'])
