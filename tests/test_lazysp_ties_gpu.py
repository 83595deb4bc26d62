"""The tie rules of the device's Dijkstra (csrc/lazysp_kernels.hip: least key, lowest id among equal keys through a strided
scan and a two-step wave minimum, strict ``alt < dist[v]``) on the lattice runs of tests/golden/lazysp_lattice_*.npz, where
keys and relaxed distances tie exactly: the explicit round loop over the C entry points on the stored draws, against the
recorded runs of the reference.  The host tests (test_lazysp_ties_host.py) show that each rule, swapped for its neighbour,
moves a compared field of every one of these runs.  Reads only tests/golden/ and the package."""
import numpy as np
import pytest

import gnnmp  # noqa: F401
from gnnmp import _lib, lazysp

from test_lazysp_gpu import run_abi
from test_lazysp_host import assert_same_plan
from test_lazysp_ties_host import LATTICE, lattice_host, load_lattice

pytestmark = pytest.mark.gpu


def test_the_runs_reach_the_scan_and_lds_boundaries():
    """Dijkstra on 63, 64, 65 and 129 nodes (one lane short of a scan pass, a full one, one lane into the second, into the
    third) and on each side of gnnmp_lazysp_lds_nodes()."""
    lds = _lib.lib().gnnmp_lazysp_lds_nodes()
    sizes = {int(row[0]) for n in LATTICE for row in load_lattice(n)['rounds']}
    assert {63, 64, 65, 129, lds, lds + 1} <= sizes


@pytest.mark.parametrize('name', LATTICE)
def test_lattice_run_equals_reference(name):
    """Every field of the recorded run -- ``rounds``, ``invalid_order`` and ``dijkstra_runs`` among them -- and the pair list
    in the order of the checks (plan_host's ``checked_order``; plan_host itself equals the recording in the host tests)."""
    rec = load_lattice(name)
    got, _ = run_abi(rec, attempts=rec['attempts'])
    print('%s: N %d, status %d, checks %d (recorded %d), dijkstra runs %d (recorded %d), pairs %d, path %d nodes (recorded %d), rounds %s; '
          'ties on this input: extractions %d, relaxations %d'
          % (name, got['samples'].shape[0], got['status'], got['checks'], int(rec['checks']), got['dijkstra_runs'], int(rec['dijkstra_runs']),
             got['n_pairs'], len(got['path_ids']), len(rec['path_ids']), got['rounds'].tolist(), int(rec['extract_ties']), int(rec['relax_ties'])))
    assert got['status'] == 0
    assert_same_plan(got, rec, name)
    order = lattice_host(name)['checked_order']
    assert np.array_equal(got['pairs'], order[:, :2]) and np.array_equal(got['pair_state'], order[:, 2])
    if 'closed' in name:                                                 # never solved: pairs are carried through every round
        assert len(rec['rounds']) > 1 and int(rec['rounds'][0, 2]) + int(rec['rounds'][0, 3]) > 0


def test_seven_rounds_beside_an_untouched_slot():
    """The run of seven rounds in a store of two slots: the same result, and no round writes into the other slot."""
    rec = load_lattice('lattice_b9_t63_closed')
    got, store = run_abi(rec, attempts=rec['attempts'], spare_slot=True)
    assert got['status'] == 0
    assert_same_plan(got, rec, 'with a spare slot')
    assert bool((store.pairs[1] == -7).all()) and bool((store.pair_state[1] == 9).all()) and bool((store.pool[1] == -7.0).all())
    assert lazysp.rounds_pair_cap(int(rec['batch']), int(rec['t_max']), int(rec['k'])) >= got['n_pairs']
