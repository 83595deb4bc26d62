"""The tie rules of csrc/rrt_tree.hpp on the device -- rrt_nearest's first minimum (a strided scan per lane, then a wave
minimum of (distance bits, id)), pass 1's strict ``<`` against the running minimum behind a pre-filter per group of 64, pass
2's strict ``<`` -- on the draw blocks of tests/golden/rrtstar_lattice_*.npz, where distances and costs tie exactly: through
gnnmp_rrtstar_plan against the recorded runs of the reference, and through gnnmp_next_plan with g_explore_eps = 1 (wave 0 of
the guided loop runs the same steps) against gnnmp.next_plan.plan_host on the same block.  The host tests
(test_rrtstar_ties_host.py) show that each rule, swapped for its neighbour, moves these fields on these inputs.  Reads only
tests/golden/ and the package."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_plan, rrtstar

from test_rrtstar_host import assert_same_tree
from test_rrtstar_gpu import tree_of
from test_rrtstar_ties_host import LATTICE, lattice_host, load_lattice

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def plan_blocks(recs):
    """The problems ``recs`` (one robot, one t_max) as ONE batch through gnnmp_rrtstar_plan with their stored blocks ->
    (the per-problem words [6, B], the tree tensors on the host)."""
    t_max = int(recs[0]['t_max'])
    f64 = lambda key: torch.from_numpy(np.stack([np.asarray(r[key], dtype=np.float64) for r in recs])).to(DEV)      # noqa: E731
    out = rrtstar.rrtstar_plan(f64('map'), f64('init_state'), f64('goal_state'), f64('raw'), t_max, False)
    torch.cuda.synchronize()
    return out['small'].cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items() if k not in ('small', 'workspace')}


def check(small, host, b, rec, what):
    got = tree_of(small, host, b)
    ties = {k: int(rec[k]) for k in ('nearest_ties', 'nearest_ties_far', 'parent_ties', 'parent_ties_late', 'rewire_ties')}
    print('%s: %d nodes, status %d, used %d (recorded %d), checks %d (recorded %d), rewired %d (recorded %d); ties on this input: %s'
          % (what, got['states'].shape[0], small[5, b], got['draws'], int(rec['draws']), got['cumulated_collision_checks'][-1],
             rec['cumulated_collision_checks'][-1], int((got['parents'] != got['rewired_parents']).sum()), int(rec['rewired']), ties))
    assert small[5, b] == 0, what
    assert_same_tree(got, rec, what)                                     # every tree field, ``draws`` = used included
    assert got['draws'] == int(rec['draws']) == rec['raw'].size


@pytest.mark.parametrize('name', LATTICE)
def test_lattice_block_equals_reference(name):
    """t_max 70: ties among the lanes of one pass (and one pair of equidistant nodes 64 ids apart); 300: ties within a lane
    across strides, more than 64 near nodes, pass-1 ties in a later group than the first improvement; one tree on each side
    of lds_nodes(); a map with a blocked pocket, where collided nodes take part in pass 2.  Both robots."""
    rec = load_lattice(name)
    lds = rrtstar.lds_nodes()
    assert int(rec['t_max']) in (70, 300, lds - 2, lds) and int(rec['nearest_ties_far']) > 0
    small, host = plan_blocks([rec])
    check(small, host, 0, rec, name)


@pytest.mark.parametrize('dim', [2, 3])
def test_batches_of_lattice_blocks(dim):
    """The same block twice in one batch, and two problems in both orders: each tree is the recorded one."""
    a, b = load_lattice('lattice_maze%d_t300' % dim), load_lattice('lattice_maze%d_pocket_t300' % dim)
    for order in ((a, a), (a, b), (b, a)):
        small, host = plan_blocks(list(order))
        for i, rec in enumerate(order):
            check(small, host, i, rec, 'maze%d batch slot %d' % (dim, i))


@pytest.mark.parametrize('t_max', [70, 300])
@pytest.mark.parametrize('dim', [2, 3])
def test_next_plan_rrt_branch_on_the_lattice(dim, t_max):
    """gnnmp_next_plan with g_explore_eps = 1: every iteration is wave 0's RRT step on the stored block.  Against
    next_plan.plan_host(raw=...) on the device model: every field bit for bit, ``w`` within the derived bar of the guided
    loop's tests -- and the tree fields it shares with RRT* are the reference's recorded ones."""
    from test_next_plan_device_gpu import _model
    from test_next_plan_edges_gpu import check_tree
    name = 'lattice_maze%d_t%d' % (dim, t_max)
    rec = load_lattice(name)
    pr = dict(map=rec['map'], init_state=rec['init_state'], goal_state=rec['goal_state'])
    model = _model(dim)
    k = 10
    eps = torch.zeros(1, 1, k, dim)                                      # no guided iteration reads it
    model.set_problem(pr)
    want = next_plan.plan_host(pr, 0, next_plan.NoiseModel(model, eps[0]), t_max=t_max, g_explore_eps=1.0, stop_when_success=False,
                               k=k, raw=rec['raw'])
    model.check_status()
    assert want['stats']['guided'] == 0 and all(want['stats'][key] == int(rec[key]) for key in
                                                ('nearest_ties', 'nearest_ties_far', 'parent_ties', 'rewire_ties'))
    assert_same_tree(want, lattice_host(name), name + ': next_plan.plan_host against rrtstar.plan_host')
    f64 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64)[None]).to(DEV)      # noqa: E731
    net = model.net
    with torch.cuda.device(DEV):
        maps, init64, goal64 = f64(rec['map']), f64(rec['init_state']), f64(rec['goal_state'])
        pb_rep = net.pb_forward(maps.to(torch.float32), goal64.to(torch.float32))
        out = next_plan.next_plan_device(maps, init64, goal64, f64(rec['raw']), pb_rep, net._weights(torch.device(DEV)), eps.to(DEV),
                                         t_max, False, 1.0, 1.0, k)
        torch.cuda.synchronize()
        small = out['small'].cpu().numpy()
        host = {key: v.cpu().numpy() for key, v in out.items() if key != 'small'}
    net.check_status()
    n, plen = int(small[0, 0]), int(small[4, 0])
    flags, pts = host['flags'][0, :n], host['states'][0, :n]
    ids = host['path'][0, :plen].astype(np.int64)
    got = {'states': pts, 'parents': host['parents'][0, :n].astype(np.int64), 'rewired_parents': host['rewired_parents'][0, :n].astype(np.int64),
           'freesp': (flags & 1).astype(bool), 'in_goal_region': (flags & 2).astype(bool), 'costs': host['costs'][0, :n],
           'path_lengths': host['path_lengths'][0, :n], 'cumulated_collision_checks': host['cumulated_checks'][0, :n],
           'success': bool(small[1, 0]), 'i': int(small[2, 0]), 'path_ids': ids, 'path': pts[ids], 'draws': int(small[3, 0]),
           'expanded_by_rrt': host['expanded_by_rrt'][0, :n], 'state_values': host['state_values'][0, :n], 'w': host['w'][0, :n],
           'w_sum': float(host['w_sum'][0]), 'visits': host['visits'][0, :n].astype(np.int64), 'guided': int(small[6, 0]),
           'status': int(small[5, 0])}
    check_tree(got, want, name + ' through gnnmp_next_plan')
    assert_same_tree(got, rec, name + ' through gnnmp_next_plan against the recorded run')
