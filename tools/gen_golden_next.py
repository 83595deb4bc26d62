#!/usr/bin/env python
"""Record the NEXT fixtures under tests/golden/ from the UNMODIFIED reference (next_model/model2D.py, algorithm/tsa.py,
algorithm/search_tree.py, environment/maze_env.py), on the CPU:

  next_{2,3}_weights.npz          the two checkpoints as arrays under their reference parameter names
  next_net_maze{2,3}.npz          two real problems each: pb_rep at iters = 20 in fp32 and from the same module in .double(),
                                  and about 40 states (corners, limits, the goal, the init state, both problems interleaved)
                                  with y in fp32 and fp64
  next_net_maze{2,3}_iters.npz    one problem at iters = 0, 1, 2, fp32 and fp64
  next_plan_maze{2,3}_*.npz       recorded ``np.random.seed(s); torch.manual_seed(s); env.init_new_problem(i);
                                  model.set_problem(...); NEXT_plan(env, model, T, g_explore_eps=0.1, stop_when_success=True)``
                                  runs: every tree field and, in call order, every pred_value / policy query with its result
                                  (both wrapped at run time), and the network output behind every queried state in fp32
                                  and fp64

Runs only in the authoring container, like tools/gen_golden_rrtstar.py: the reference's third-party imports resolve to
tools/standins/.  What is written is data only.  Printed per planner case: guided iterations, guided iterations that collided,
successes reached through the guided branch, angle wraps inside env.step.
"""
import copy
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
os.environ.setdefault('CUDA_VISIBLE_DEVICES', '')
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, 'tools', 'standins'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

os.chdir(REF)
import algorithm.tsa as tsa  # noqa: E402
from environment import MazeEnv  # noqa: E402
from next_model.model2D import Model2D  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
T_MAX = 60
FILES = {2: 'maze_files/mazes_hard.npz', 3: 'maze_files/mazes_15_3_3000.npz'}


def load_model(env, dim):
    model = Model2D(env=env, cuda=False, dim=dim)
    sd = torch.load('data/weights/next_%d.pt' % dim, map_location='cpu')
    model.net.load_state_dict(sd)
    model.net.eval()
    return model, sd


def double_net(net):
    net64 = copy.deepcopy(net).double()
    net64.attention_g.coords = net64.attention_g.coords.double()
    return net64


def net_fixtures(dim, env, model, sd):
    np.savez_compressed(os.path.join(OUT, 'next_%d_weights.npz' % dim), **{k: v.numpy() for k, v in sd.items()})
    net, net64 = model.net, double_net(model.net)
    rng = np.random.RandomState(100 + dim)
    lim = np.array([1., 1., 0.4])[:dim]
    probs = [env.init_new_problem(i) for i in (3, 11)]
    maps = np.stack([p['map'] for p in probs]).astype(np.float32)
    goals = np.stack([p['goal_state'] for p in probs]).astype(np.float32)
    inits = np.stack([p['init_state'] for p in probs]).astype(np.float32)
    states, of = [], []
    for sx in (-1., 1.):
        for sy in (-1., 1.):
            states.append(np.concatenate([[sx, sy], rng.uniform(-0.4, 0.4, dim - 2)]))
    for k in range(dim):                                          # one coordinate at each limit
        for sgn in (-1., 1.):
            s = rng.uniform(-lim, lim)
            s[k] = sgn * lim[k]
            states.append(s)
    for b in range(2):
        states += [goals[b].astype(np.float64), inits[b].astype(np.float64)]
    while len(states) < 40:
        states.append(rng.uniform(-lim, lim))
    states = np.array(states, dtype=np.float32)
    of = np.array([(i * 7 + i // 3) % 2 for i in range(len(states))], dtype=np.int32)      # both problems interleaved
    of[4 + 2 * dim:8 + 2 * dim] = [0, 0, 1, 1]                                             # goal / init of their own problem
    with torch.no_grad():
        pb32 = [net.pb_forward(torch.from_numpy(goals[b:b + 1]), torch.from_numpy(maps[b:b + 1])) for b in range(2)]
        pb64 = [net64.pb_forward(torch.from_numpy(goals[b:b + 1]).double(), torch.from_numpy(maps[b:b + 1]).double()) for b in range(2)]
        y32 = np.stack([net.state_forward(torch.from_numpy(states[i:i + 1]), pb32[of[i]])[0].numpy() for i in range(len(states))])
        y64 = np.stack([net64.state_forward(torch.from_numpy(states[i:i + 1]).double(), pb64[of[i]])[0].numpy()
                        for i in range(len(states))])
        # the same states read out of the fp32 pb_rep by the double module: isolates the state kernel from pb_rep's error
        y64_of32 = np.stack([net64.state_forward(torch.from_numpy(states[i:i + 1]).double(), pb32[of[i]].double())[0].numpy()
                             for i in range(len(states))])
    p32 = np.stack([p.reshape(64, 15, 15).numpy() for p in pb32])
    p64 = np.stack([p.reshape(64, 15, 15).numpy() for p in pb64])
    np.savez_compressed(os.path.join(OUT, 'next_net_maze%d.npz' % dim), dim=dim, maps=maps, goals=goals, inits=inits, iters=20,
                        pb_rep32=p32, pb_rep64=p64, states=states, problem_of_state=of, y32=y32, y64=y64, y64_of32=y64_of32)
    print('next_net_maze%d: own error pb_rep %.3e (max |.| %.3f), y %.3e (max |y| %.3f)'
          % (dim, np.abs(p32 - p64).max(), np.abs(p64).max(), np.abs(y32 - y64).max(), np.abs(y64).max()))
    rec = dict(dim=dim, maps=maps[:1], goals=goals[:1])
    for it in (0, 1, 2):
        net.iters = net64.iters = it
        with torch.no_grad():
            a = net.pb_forward(torch.from_numpy(goals[:1]), torch.from_numpy(maps[:1])).reshape(1, 64, 15, 15).numpy()
            b = net64.pb_forward(torch.from_numpy(goals[:1]).double(), torch.from_numpy(maps[:1]).double()).reshape(1, 64, 15, 15).numpy()
        rec['pb_rep32_i%d' % it], rec['pb_rep64_i%d' % it] = a, b
        print('next_net_maze%d_iters: iters %d own error %.3e' % (dim, it, np.abs(a - b).max()))
    net.iters = 20
    np.savez_compressed(os.path.join(OUT, 'next_net_maze%d_iters.npz' % dim), **rec)


def run_plan(env, model, idx, seed, t_max):
    np.random.seed(seed)
    torch.manual_seed(seed)
    problem = env.init_new_problem(idx)
    model.set_problem(problem)
    dim = env.dim
    count = dict(guided=0, guided_collided=0, guided_success=0, wraps=0)
    q_kind, q_n, q_states, v_out, p_actions, p_priors = [], [], [], [], [], []
    real_value, real_policy, real_expand, real_step = model.pred_value, model.policy, tsa.expand, env.step

    def pred_value(states):
        r = real_value(states)
        a = np.asarray(states, dtype=np.float64).reshape(-1, dim)
        q_kind.append(0), q_n.append(a.shape[0]), q_states.append(a.copy()), v_out.append(np.asarray(r, dtype=np.float32).reshape(-1))
        return r

    def policy(state, k=1):
        actions, priors = real_policy(state=state, k=k)
        a = np.asarray(state, dtype=np.float64).reshape(-1, dim)
        q_kind.append(1), q_n.append(a.shape[0]), q_states.append(a.copy())
        p_actions.append(np.array(actions, dtype=np.float32)), p_priors.append(np.array(priors, dtype=np.float64))
        return actions, priors

    def expand(*a, **kw):
        r = real_expand(*a, **kw)
        count['guided'] += 1
        count['guided_collided'] += not r[2]
        count['guided_success'] += bool(r[3])
        return r

    def step(state, action=None, new_state=None, check_collision=True):
        if dim == 3:
            z = (state + action)[2] if action is not None else new_state[2]
            count['wraps'] += bool(np.abs(z) > 0.4)
        return real_step(state, action=action, new_state=new_state, check_collision=check_collision)

    model.pred_value, model.policy, tsa.expand, env.step = pred_value, policy, expand, step
    try:
        tree, success, i = tsa.NEXT_plan(env=env, model=model, T=t_max, g_explore_eps=0.1, stop_when_success=True, UCB_type='kde')
    finally:
        tsa.expand = real_expand
        del model.pred_value, model.policy, env.step
    states = np.asarray(tree.states, dtype=np.float64)
    # the whole network output behind every query, query by query in the recorded batch shapes: fp32 as the run saw it, and
    # from the same module in .double()
    net64 = double_net(model.net)
    y32, y64, row = [], [], 0
    with torch.no_grad():
        pb64 = net64.pb_forward(model.goal_state.double(), model.maze_map.double())
        for n in q_n:
            st = np.concatenate(q_states)[row:row + n]
            row += n
            y32.append(model.net.state_forward(torch.FloatTensor(st), model.pb_rep).numpy())
            y64.append(net64.state_forward(torch.FloatTensor(st).double(), pb64).numpy())
    y32, y64 = np.concatenate(y32), np.concatenate(y64)
    is_value = np.repeat(np.array(q_kind) == 0, q_n)
    assert np.array_equal(y32[is_value, -1], np.concatenate(v_out)), 'the recorded values are not the network output'
    walk = []
    if tree.in_goal_region[-1]:
        cur = len(states) - 1
        while True:
            walk.append(cur)
            if cur == 0:
                break
            cur = tree.rewired_parents[cur]
        walk.reverse()
    par = lambda xs: np.array([-1 if x is None else x for x in xs], dtype=np.int32)      # noqa: E731
    k = p_actions[0].shape[0] if p_actions else 10
    return dict(dim=dim, map=problem['map'].astype(np.float64), init_state=np.asarray(problem['init_state'], dtype=np.float64),
                goal_state=np.asarray(problem['goal_state'], dtype=np.float64), seed=seed, t_max=t_max, index=idx,
                states=states, parents=par(tree.parents), rewired_parents=par(tree.rewired_parents),
                expanded_by_rrt=par([None if x is None else int(x) for x in tree.expanded_by_rrt]).astype(np.int8),
                freesp=np.array(tree.freesp, dtype=bool), in_goal_region=np.array(tree.in_goal_region, dtype=bool),
                costs=np.array(tree.costs, dtype=np.float64), path_lengths=np.array(tree.path_lengths, dtype=np.float64),
                cumulated_collision_checks=np.array(tree.cumulated_collision_checks, dtype=np.int64),
                visits=np.array(tree.visits, dtype=np.int64), state_values=np.array(tree.state_values, dtype=np.float32),
                w=np.array(tree.w, dtype=np.float64), w_sum=float(tree.w_sum), success=bool(success), i=int(i),
                path_ids=np.array(walk, dtype=np.int32), q_kind=np.array(q_kind, dtype=np.uint8), q_n=np.array(q_n, dtype=np.int32),
                q_states=np.concatenate(q_states), v_out=np.concatenate(v_out), y32=y32, y64=y64,
                p_actions=np.array(p_actions, dtype=np.float32).reshape(-1, k, dim),
                p_priors=np.array(p_priors, dtype=np.float64).reshape(-1, k), **count)


def plan_fixtures(dim, env, model, max_runs=60):
    need = {'guided_success', 'exhausted', 'guided_collided'} | ({'wraps'} if dim == 3 else set())
    kept = 0
    for idx in range(max_runs):
        if not need or kept >= 4:
            break
        rec = run_plan(env, model, idx, 2000 + idx, T_MAX)
        has = set()
        if rec['success'] and rec['guided_success']:
            has.add('guided_success')
        if not rec['success']:
            has.add('exhausted')
        if rec['guided_collided']:
            has.add('guided_collided')
        if rec['wraps']:
            has.add('wraps')
        print('maze%d idx %3d seed %d: n=%3d i=%3d success=%d guided=%2d guided_collided=%2d guided_success=%d wraps=%d queries=%d%s'
              % (dim, idx, rec['seed'], rec['states'].shape[0], rec['i'], rec['success'], rec['guided'], rec['guided_collided'],
                 rec['guided_success'], rec['wraps'], len(rec['q_kind']), '  <- kept' if has & need else ''), flush=True)
        new = has & need
        if new - {'guided_collided'} or (new and need == {'guided_collided'}):
            np.savez_compressed(os.path.join(OUT, 'next_plan_maze%d_t%d_i%d.npz' % (dim, T_MAX, idx)), **rec)
            need -= has
            kept += 1
    if need:
        raise SystemExit('maze%d: no recorded run with %s' % (dim, sorted(need)))


def main():
    torch.set_num_threads(4)
    what = sys.argv[1:] or ['net', 'plan']
    for dim in (2, 3):
        env = MazeEnv(dim=dim, map_file=FILES[dim])
        model, sd = load_model(env, dim)
        if 'net' in what:
            net_fixtures(dim, env, model, sd)
        if 'plan' in what:
            plan_fixtures(dim, env, model)


if __name__ == '__main__':
    main()
