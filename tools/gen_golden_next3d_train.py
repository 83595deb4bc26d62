#!/usr/bin/env python
"""Record the training fixtures of the 3-D NEXT network (the arm families) under tests/golden/ from the UNMODIFIED reference
(train_next.py's get_label and loss, next_model/model3D.py, environment/kuka_env.py:KukaEnv.interpolate), on the CPU.  For kuka7
(next_7, point_dim 3) and kuka14 (next_14, point_dim 6):

  next3d_train_kuka{7,14}.npz                  two problems -- problem 0 on the asymmetric map of gen_golden_next3d.asymmetric_map,
                                               problem 1 on a real kuka7 map -- their goal rows, a path of 5 and one of 8 states
                                               (steps both longer and shorter than RRT_EPS; one long step ends beyond a joint
                                               limit, so its interpolated state is clipped), the network input rows of the path
                                               states, the recorded pose_range and RRT_EPS, get_label's outputs (float64), and the
                                               loss of every case in fp32 and from the same module in .double()
  next3d_train_kuka{7,14}_i{R}_g32_{a..d}.npz  the per-parameter gradients of train()'s loss, fp32 module, split by parameter
                                               name (a: everything small, b: h0, c: c0, d: conv) so no file passes 1 MiB
  next3d_train_kuka{7,14}_i{R}_d64_{a..d}.npz  the .double() module's gradients minus the fp32 ones, stored in float32:
                                               g64 = g32 + d64 to 1e-7 of the DIFFERENCE

Cases: kuka7 at 0, 1, 2 rounds (problem 0 alone) and 20 rounds (both problems); kuka14 at 1 round (problem 0) and 20 rounds (both).

The loss is train()'s: per (problem, path) sample Model3D.set_problem, net_forward(path, use_np=False), MSELoss on the value
column plus MSELoss on the action columns, summed and divided by the number of problems.  get_label runs on a namespace that
carries the recorded pose_range and RRT_EPS with KukaEnv.interpolate bound to it.  As tools/gen_golden_next3d.py explains, the
point part of a network input row is the arm's end effector position, which takes PyBullet; here THE POINT PARTS ARE DRAWN in
[-1, 1]^3 and handed to the reference's Model3D through the namespace's get_robot_points.

Runs only where the reference is present; its third-party imports resolve to tools/standins/.  What is written is data only.
"""
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
os.environ.setdefault('CUDA_VISIBLE_DEVICES', '')
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, 'tools', 'standins'))
sys.path.insert(0, os.path.join(REPO, 'tools'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

os.chdir(REF)
from environment.kuka_env import KukaEnv  # noqa: E402
from next_model.model3D import Model3D  # noqa: E402
from train_next import get_label  # noqa: E402
from gen_golden_next3d import FAMILIES, asymmetric_map, double_net, points, real_maps, save  # noqa: E402

RRT_EPS = 0.5                              # environment/kuka_env.py
IIWA = np.array([2.96705972839, 2.09439510239, 2.96705972839, 2.09439510239, 2.96705972839, 2.09439510239, 3.05432619099])
CASES = {7: ((20, 2), (0, 1), (1, 1), (2, 1)), 14: ((20, 2), (1, 1))}
PARTS = (('b', 'h0.'), ('c', 'c0.'), ('d', 'conv.'))


def make_path(rng, n, hi, clip_at=None):
    """A polyline of n states inside the joint limits: steps longer than RRT_EPS, one shorter, and (clip_at) one long step that
    ends beyond the upper limit of joint 1."""
    dim = hi.shape[0]
    pts = [rng.uniform(-0.6, 0.6, dim) * hi]
    for _ in range(n - 1):
        pts.append(np.clip(pts[-1] + rng.uniform(-0.45, 0.45, dim), -hi, hi))
    pts[2] = pts[1] + rng.uniform(-0.05, 0.05, dim)                  # a short step
    if clip_at is not None:
        pts[clip_at][1] = hi[1] - 0.04
        pts[clip_at + 1] = pts[clip_at] + rng.uniform(-0.1, 0.1, dim)
        pts[clip_at + 1][1] = hi[1] + 0.5                            # a recorded state beyond the limit
    return np.array(pts)


def grads(net, loss):
    named = list(net.named_parameters())
    gs = torch.autograd.grad(loss, [p for _, p in named], allow_unused=True)
    return {k: (np.zeros(tuple(p.shape)) if g is None else g.detach().numpy()) for (k, p), g in zip(named, gs)}


def save_split(stem, arrays):
    rest = dict(arrays)
    for part, prefix in PARTS:
        sel = {k: rest.pop(k) for k in list(rest) if k.startswith(prefix)}
        save('%s_%s.npz' % (stem, part), **sel)
    save('%s_a.npz' % stem, **rest)


def family(dim):
    stem, pd = FAMILIES[dim]
    name = 'next3d_train_kuka%d' % dim
    hi = np.resize(IIWA, dim)
    pose_range = [(-v, v) for v in hi]
    rng = np.random.RandomState(500 + dim)
    maps = np.stack([asymmetric_map(), real_maps((3,))[0][0]])
    paths = [make_path(rng, 5, hi, clip_at=3), make_path(rng, 8, hi)]
    goal_states = [p[-1].copy() for p in paths]
    goal_states[0] = np.clip(goal_states[0], -hi, hi)
    pts = [points(rng, len(p), pd) for p in paths]
    goal_pts = points(rng, 2, pd)
    table = {}
    for p, q in zip(paths, pts):
        for s, x in zip(p, q):
            table[np.asarray(s, dtype=np.float64).tobytes()] = x
    for s, x in zip(goal_states, goal_pts):
        table[('goal', np.asarray(s, dtype=np.float64).tobytes())] = x

    env = types.SimpleNamespace(RRT_EPS=RRT_EPS, pose_range=pose_range, goal=False)
    env.interpolate = types.MethodType(KukaEnv.interpolate, env)

    def get_robot_points(state):
        key = np.asarray(state, dtype=np.float64).tobytes()
        return table[('goal', key)] if env.goal else table[key]
    env.get_robot_points = get_robot_points

    model = Model3D(env=env, cuda=False, dim=dim, point_dim=pd)
    model.net.load_state_dict(torch.load('data/weights/%s.pt' % stem, map_location='cpu'))
    net64 = double_net(model.net)
    probs = [dict(map=maps[b], goal_state=goal_states[b]) for b in range(2)]
    labels = [get_label(p, env) for p in paths]
    clipped = labels[0][0][3]
    assert np.linalg.norm(paths[0][4] - paths[0][3]) > RRT_EPS and abs(paths[0][3][1] + clipped[1] - hi[1]) < 1e-12, 'the clipped step'
    goal_rows = np.concatenate([goal_pts, np.array(goal_states)], axis=1).astype(np.float32)
    rows = np.concatenate([np.concatenate(pts), np.concatenate(paths)], axis=1).astype(np.float32)
    rec = dict(dim=dim, point_dim=pd, rrt_eps=RRT_EPS, lo=-hi, hi=hi, maps=maps.astype(np.uint8), goals=goal_rows, rows=rows,
               points=np.concatenate(pts), paths=np.concatenate(paths), path_ptr=np.array([0, 5, 13], dtype=np.int64),
               actions=np.concatenate([np.array(a) for a, _ in labels]), values=np.concatenate([np.array(v) for _, v in labels]))

    def loss_fp32(npb):
        total = 0.
        for pb, path, (action, value) in zip(probs[:npb], paths[:npb], labels[:npb]):
            env.goal = True
            model.set_problem(pb)
            env.goal = False
            action_pred, value_pred = model.net_forward(np.array(path), use_np=False)
            total = total + torch.nn.MSELoss()(torch.FloatTensor(value), value_pred) + torch.nn.MSELoss()(torch.FloatTensor(action), action_pred)
        return total / npb

    def loss_fp64(npb):
        total, at = 0., 0
        for b, (path, (action, value)) in enumerate(zip(paths[:npb], labels[:npb])):
            pb_rep = net64.pb_forward(torch.from_numpy(goal_rows[b:b + 1]).double(), torch.from_numpy(maps[b:b + 1]).double())
            y = net64.state_forward(torch.from_numpy(rows[at:at + len(path)]).double(), pb_rep)
            at += len(path)
            total = total + torch.nn.MSELoss()(torch.FloatTensor(value).double(), y[:, -1]) \
                + torch.nn.MSELoss()(torch.FloatTensor(action).double(), y[:, :dim])
        return total / npb

    for iters, npb in CASES[dim]:
        model.net.iters = net64.iters = iters
        l32, l64 = loss_fp32(npb), loss_fp64(npb)
        g32, g64 = grads(model.net, l32), grads(net64, l64)
        rec['loss32_i%d' % iters], rec['loss64_i%d' % iters] = float(l32.detach()), float(l64.detach())
        save_split('%s_i%d_g32' % (name, iters), {k: v.astype(np.float32) for k, v in g32.items()})
        save_split('%s_i%d_d64' % (name, iters), {k: (g64[k] - g32[k].astype(np.float64)).astype(np.float32) for k in g64})
        print('%s iters %2d: loss %.9g / %.15g' % (name, iters, rec['loss32_i%d' % iters], rec['loss64_i%d' % iters]), flush=True)
        for k in g64:
            m = np.abs(g64[k]).max()
            own = np.abs(g32[k] - g64[k]).max()
            print('    %-34s max|g64| %.3e  own %.3e  own / max %.2e' % (k, m, own, own / max(m, 1e-300)))
    model.net.iters = 20
    save(name + '.npz', **rec)


def main():
    torch.set_num_threads(8)
    for dim in [int(a) for a in sys.argv[1:]] or sorted(FAMILIES):
        family(dim)


if __name__ == '__main__':
    main()
