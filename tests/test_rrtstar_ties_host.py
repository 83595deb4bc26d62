"""The three tie rules of RRT* -- first minimum in the nearest-node search, strict ``<`` in both rewiring passes -- on inputs
that tie: the reference's runs on draw blocks of a dyadic lattice (tests/golden/rrtstar_lattice_*.npz, written by
tools/gen_golden_rrtstar.py), where equal distances and equal costs are equal bit for bit.  gnnmp.rrtstar.plan_host on the
stored block must give the recorded tree in every field, every tie counter must be above zero on every input, and each rule,
swapped for its neighbour, must move a compared field -- otherwise the inputs would not tell the rules apart.  No GPU."""
import glob
import os

import numpy as np
import pytest

from gnnmp import rrtstar

from test_rrtstar_host import GOLDEN, assert_same_tree, problem_of

LATTICE = sorted(os.path.basename(p)[len('rrtstar_'):-len('.npz')] for p in glob.glob(os.path.join(GOLDEN, 'rrtstar_lattice_*.npz')))
TIE_COUNTERS = ('nearest_ties', 'nearest_ties_far', 'parent_ties', 'rewire_ties')
_RECS, _HOST = {}, {}


def load_lattice(name):
    if name not in _RECS:
        with np.load(os.path.join(GOLDEN, 'rrtstar_%s.npz' % name)) as f:
            _RECS[name] = {k: f[k] for k in f.files}
    return _RECS[name]


def lattice_host(name):
    """plan_host on the stored block, once per fixture: shared with the GPU tests and left unchanged."""
    if name not in _HOST:
        rec = load_lattice(name)
        _HOST[name] = rrtstar.plan_host(problem_of(rec), 0, t_max=int(rec['t_max']), stop_when_success=bool(rec['stop_when_success']),
                                        raw=rec['raw'])
    return _HOST[name]


def test_fixture_list():
    """Both robots at 70 and 300 iterations, on both sides of the device's LDS node count (1024 nodes = t_max 1023) and on a
    map with a blocked pocket; all run to t_max; every block is on the lattice and draws no goal sample."""
    recs = {n: load_lattice(n) for n in LATTICE}
    for dim in (2, 3):
        t = sorted(int(r['t_max']) for r in recs.values() if int(r['dim']) == dim)
        assert 70 in t and 300 in t and t[-2] + 1 < 1024 < t[-1] + 1, t
        assert any(int(r['dim']) == dim and int(r['collided_second_pass']) > 0 for r in recs.values())
    for name, r in recs.items():
        raw = r['raw'].reshape(int(r['t_max']), 2 + int(r['dim']))
        assert np.array_equal(raw * 64, np.round(raw * 64)) and (raw[:, 0] >= rrtstar.MODEL_EPS).all(), name
        assert not bool(r['stop_when_success']) and r['states'].shape[0] == int(r['t_max']) + 1, name
        assert int(r['draws']) == raw.size, name
        if int(r['dim']) == 3:
            assert int(r['wrap_edges']) > 0, name                     # edges whose angle gap goes the short way round
        if int(r['t_max']) >= 300:
            assert int(r['max_near']) > 64, name                      # rewiring passes of more than one group of 64
        if int(r['t_max']) >= 300 and 'pocket' not in name:
            assert int(r['parent_ties_late']) > 0, name               # pass-1 ties in a later group than the first improvement


@pytest.mark.parametrize('name', LATTICE)
def test_plan_host_equals_reference_on_the_lattice(name):
    rec, got = load_lattice(name), lattice_host(name)
    assert_same_tree(got, rec, name)
    assert got['draws'] == int(rec['draws'])
    for key in ('direct_steer', 'collided_second_pass', 'goal_rechecks'):
        assert got['stats'][key] == int(rec[key]), key
    assert int((got['parents'] != got['rewired_parents']).sum()) == int(rec['rewired'])
    assert got['stats']['rewired'] == int(rec['second_pass_rewires'])
    # the ties are there: a later change of the inputs cannot quietly remove them
    for key in TIE_COUNTERS + ('parent_ties_late',):
        assert got['stats'][key] == int(rec[key]), key
    for key in TIE_COUNTERS:
        assert got['stats'][key] > 0, (name, key)


def last_minimum(d):
    return len(d) - 1 - int(np.argmin(np.asarray(d)[::-1]))


MUTATIONS = {'nearest: last minimum instead of first': ('nearest_index', last_minimum),
             'pass 1: <= instead of <': ('parent_improves', lambda cost_new, min_cost: cost_new <= min_cost),
             'pass 2: <= instead of <': ('neighbor_improves', lambda cost_new, cost_j: cost_new <= cost_j)}
# the inputs every mutation runs on (the two long trees of a robot differ in two iterations: one mutation each is enough there)
SHORT = [n for n in LATTICE if int(load_lattice(n)['t_max']) <= 300]


def moved_fields(name, monkeypatch, attr, rule):
    """Tree fields of ``name`` that differ from the recorded run when ``rrtstar.attr`` is ``rule`` (a run that ends in a
    cycle of rewired parents, which the reference would never leave, counts as moved)."""
    rec = load_lattice(name)
    with monkeypatch.context() as mp:
        mp.setattr(rrtstar, attr, rule)
        try:
            got = rrtstar.plan_host(problem_of(rec), 0, t_max=int(rec['t_max']), stop_when_success=False, raw=rec['raw'])
        except RuntimeError:
            return ['path_ids']
    return [k for k in rrtstar.TREE_FIELDS if not np.array_equal(np.asarray(got[k]), np.asarray(rec[k]))]


@pytest.mark.parametrize('mutation', sorted(MUTATIONS))
def test_every_mutated_rule_moves_a_field(mutation, monkeypatch):
    """Sensitivity: each rule swapped for its neighbour changes a compared field on an input of either robot -- and on
    every short input, so that none of them is dead weight for that rule."""
    attr, rule = MUTATIONS[mutation]
    moved = {n: moved_fields(n, monkeypatch, attr, rule) for n in SHORT}
    print(mutation, {n: m[:4] for n, m in moved.items()})
    for dim in (2, 3):
        assert any(m for n, m in moved.items() if int(load_lattice(n)['dim']) == dim), (mutation, dim)
    assert all(moved.values()), (mutation, [n for n, m in moved.items() if not m])


@pytest.mark.parametrize('name', [n for n in LATTICE if n not in SHORT])
def test_the_long_inputs_are_moved_too(name, monkeypatch):
    attr, rule = MUTATIONS['nearest: last minimum instead of first']
    assert moved_fields(name, monkeypatch, attr, rule), name


def test_seeded_runs_are_untouched_by_the_raw_argument():
    """``raw=`` with the block a seed gives is the seeded run."""
    rec = load_lattice(SHORT[0])
    pr = problem_of(rec)
    a = rrtstar.plan_host(pr, 11, t_max=40, stop_when_success=False)
    b = rrtstar.plan_host(pr, 0, t_max=40, stop_when_success=False,
                          raw=np.random.RandomState(11).random_sample(rrtstar.draws_per_problem(40, int(rec['dim']))))
    assert_same_tree(a, b, 'seed against its block')
    with pytest.raises(ValueError):
        rrtstar.plan_host(pr, 0, t_max=40, raw=np.zeros(5))
