#!/usr/bin/env python
"""Record the fixtures of the 3-D NEXT network (the arm families) under tests/golden/ from the UNMODIFIED reference
(next_model/model3D.py:PPN, environment/kuka_env.py:KukaEnv.obs_map), on the CPU:

  next_{7,14}_weights.npz                 the kuka7 (point_dim 3) and kuka14 (point_dim 6) checkpoints as arrays under their
                                          reference parameter names (split into ..._weights_b.npz by parameter name when one
                                          file would pass the size limit)
  next3d_kuka{7,14}_net.npz               three maps (two real kuka7 problems through the reference's own obs_map, one synthetic
                                          map that differs under every permutation of its axes), their goal rows, 24 state rows
                                          interleaved over problems 0 and 1 with y in fp32, in fp64 and in fp64 read out of the
                                          fp32 pb_rep
  next3d_kuka{7,14}_pb{0,1}_i20_f32.npz   pb_rep of problems 0 and 1 at iters = 20, fp32
  next3d_kuka{7,14}_pb0_i20_f64.npz       the same module in .double(), problem 0
  next3d_kuka{7,14}_pb0_i{0,1,2}_f{32,64}.npz   problem 0 at iters = 0, 1, 2

A network input row is [point (point_dim), state (dim)].  In the reference the point part is the end effector position(s) of
the state, which takes PyBullet's forward kinematics; PyBullet is not available where this runs, so the POINT PART OF EVERY ROW
IS DRAWN in the cube [-1, 1]^3 (cube corners included) and is NOT the state's end effector.  The network does not know the
difference: it sees point_dim + dim numbers.  States of the dim 7 family are the recorded start, goal and path configurations of
the two problems plus uniform draws; dim 14 uses uniform draws (the kuka7 maps serve both families: the map is 15^3 voxels either
way).

Runs only where the reference is present; its third-party imports resolve to tools/standins/.  What is written is data only.
Printed per fixture: the reference's own fp32-vs-fp64 error.
"""
import copy
import os
import pickle
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
os.environ.setdefault('CUDA_VISIBLE_DEVICES', '')
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, 'tools', 'standins'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

os.chdir(REF)
from environment.kuka_env import KukaEnv  # noqa: E402
from next_model.model3D import PPN  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
W = 15
FAMILIES = {7: ('next_7', 3), 14: ('next_14', 6)}
SIZE_LIMIT = 1 << 20                       # no committed file passes 1 MiB


def save(name, **arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < SIZE_LIMIT, '%s: %d bytes' % (name, size)
    print('  wrote %s (%d bytes)' % (name, size), flush=True)


def save_weights(stem, sd):
    arrays = {k: v.numpy() for k, v in sd.items()}
    try:
        save(stem + '_weights.npz', **arrays)
    except AssertionError:
        second = {k: v for k, v in arrays.items() if k.startswith(('c0.', 'conv.'))}
        save(stem + '_weights.npz', **{k: v for k, v in arrays.items() if k not in second})
        save(stem + '_weights_b.npz', **second)


def double_net(net):
    net64 = copy.deepcopy(net).double()
    net64.attention_g.coords = net64.attention_g.coords.double()
    return net64


def asymmetric_map():
    """Blocked voxels that no permutation of the three axes maps onto themselves."""
    m = np.zeros((W, W, W), dtype=np.float32)
    m[1:4, 2:9, 5:7] = 1
    m[10:14, 0:2, 3:12] = 1
    m[6, 11, 13] = 1
    for perm in ((0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        assert not np.array_equal(m, m.transpose(perm))
    return m


def real_maps(indices):
    with open('maze_files/kukas_7_3000.pkl', 'rb') as f:
        problems = pickle.load(f)
    out = []
    for i in indices:
        obstacles, start, goal, path = problems[i]
        occ = KukaEnv.obs_map(types.SimpleNamespace(obstacles=obstacles), W)[1]
        out.append((np.array(occ).astype(np.float32), np.asarray(start, dtype=np.float64), np.asarray(goal, dtype=np.float64),
                    [np.asarray(q, dtype=np.float64) for q in path]))
    return out


def points(rng, n, point_dim):
    """n drawn point parts; the first rows sit on cube corners."""
    p = rng.uniform(-1., 1., (n, point_dim))
    corners = np.array([[sx, sy, sz] for sx in (-1., 1.) for sy in (-1., 1.) for sz in (-1., 1.)])
    for i in range(min(n, 4)):
        p[i] = np.tile(corners[(3 * i + 1) % 8], point_dim // 3) if i % 2 == 0 else np.concatenate(
            [corners[(5 * i + k) % 8] for k in range(point_dim // 3)])
    return p


def family(dim):
    stem, pd = FAMILIES[dim]
    name = 'next3d_kuka%d' % dim
    sd = torch.load('data/weights/%s.pt' % stem, map_location='cpu')
    save_weights(stem, sd)
    net = PPN(False, env_width=W, cap=8, dim=dim, point_dim=pd)
    net.load_state_dict(sd)
    net.eval()
    net64 = double_net(net)
    rng = np.random.RandomState(300 + dim)
    real = real_maps((3, 11))
    maps = np.stack([real[0][0], real[1][0], asymmetric_map()])
    lim = np.abs(np.vstack([np.vstack([r[1], r[2]] + r[3]) for r in real])).max(axis=0)        # per joint, of the recorded configurations
    lim = np.resize(lim, dim)
    if dim == 7:
        goal_states = [real[0][2], real[1][2], rng.uniform(-lim, lim)]
        states = [real[b][k] for b in range(2) for k in (1, 2)] + [q for b in range(2) for q in real[b][3][1:-1][:3]]
    else:
        goal_states = [rng.uniform(-lim, lim) for _ in range(3)]
        states = []
    while len(states) < 24:
        states.append(rng.uniform(-lim, lim))
    goal_pts = points(rng, 3, pd)
    goal_pts[2] = np.tile([1., -1., 1.], pd // 3)                                          # a goal point at a cube corner
    goals = np.concatenate([goal_pts, np.array(goal_states)], axis=1).astype(np.float32)
    states = np.concatenate([points(rng, 24, pd), np.array(states[:24])], axis=1).astype(np.float32)
    of = np.array([(i * 7 + i // 3) % 2 for i in range(24)], dtype=np.int32)               # problems 0 and 1 interleaved
    print('%s: %d blocked voxels in the maps %s' % (name, int(maps.sum()), [int(m.sum()) for m in maps]))

    def pb(n, b, dtype):
        with torch.no_grad():
            return n.pb_forward(torch.from_numpy(goals[b:b + 1]).to(dtype), torch.from_numpy(maps[b:b + 1]).to(dtype))

    pb32 = [pb(net, b, torch.float32) for b in range(2)]
    pb64 = [pb(net64, b, torch.float64) for b in range(2)]
    with torch.no_grad():
        st = torch.from_numpy(states)
        y32 = np.stack([net.state_forward(st[i:i + 1], pb32[of[i]])[0].numpy() for i in range(24)])
        y64 = np.stack([net64.state_forward(st[i:i + 1].double(), pb64[of[i]])[0].numpy() for i in range(24)])
        y64_of32 = np.stack([net64.state_forward(st[i:i + 1].double(), pb32[of[i]].double())[0].numpy() for i in range(24)])
    save(name + '_net.npz', dim=dim, point_dim=pd, maps=maps.astype(np.uint8), goals=goals, states=states, problem_of_state=of,
         y32=y32, y64=y64, y64_of32=y64_of32)
    p32 = [p.reshape(64, W, W, W).numpy() for p in pb32]
    p64 = pb64[0].reshape(64, W, W, W).numpy()
    save(name + '_pb0_i20_f32.npz', pb_rep=p32[0])
    save(name + '_pb1_i20_f32.npz', pb_rep=p32[1])
    save(name + '_pb0_i20_f64.npz', pb_rep=p64)
    print('%s: own error pb_rep %.3e (max |.| %.3f), y %.3e (max |y| %.3f)'
          % (name, np.abs(p32[0] - p64).max(), np.abs(p64).max(), np.abs(y32 - y64).max(), np.abs(y64).max()))
    for it in (0, 1, 2):
        net.iters = net64.iters = it
        a = pb(net, 0, torch.float32).reshape(64, W, W, W).numpy()
        b = pb(net64, 0, torch.float64).reshape(64, W, W, W).numpy()
        save(name + '_pb0_i%d_f32.npz' % it, pb_rep=a)
        save(name + '_pb0_i%d_f64.npz' % it, pb_rep=b)
        print('%s: iters %d own error %.3e' % (name, it, np.abs(a - b).max()))
    net.iters = net64.iters = 20


def main():
    torch.set_num_threads(8)
    for dim in [int(a) for a in sys.argv[1:]] or sorted(FAMILIES):
        family(dim)


if __name__ == '__main__':
    main()
