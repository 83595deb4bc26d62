"""Front of the forward, obstacle launch: the rows of the double-precision node role and everything behind them do not depend on
how many 64-row groups a workgroup of that role takes (GNNMP_F64_GROUPS: 1, 4, several 256-row blocks in a row).  The switch is
read when a module's native handle is created, so every setting gets its own module; all comparisons are bit for bit inside one
process."""
import contextlib
import os

import pytest
import torch

import gnnmp
from gnnmp.synth import synth_graph
from conftest import load_weights

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@contextlib.contextmanager
def environ(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def model(mlp_dtype='fp32'):
    m = gnnmp.EncoderProcessDecoder(2, 2, 32, 2).eval()
    m.load_state_dict(load_weights('weights_maze'))
    m.mlp_dtype = mlp_dtype
    return m


def graphs_of(sizes, n_obs, seed):
    """maze2 graphs (k = 4) with the given node counts; obstacle counts cycle through n_obs"""
    out = []
    gen = torch.Generator().manual_seed(seed)
    for i, n in enumerate(sizes):
        g = synth_graph('maze2', n, 4, seed=seed + i, n_obs=min(n_obs[i % len(n_obs)], 225))
        if n_obs[i % len(n_obs)] > 225:                           # more obstacles than the grid has cells: free-standing points
            g['obstacles'] = torch.rand(n_obs[i % len(n_obs)], 2, generator=gen) - 0.5
        out.append(g)
    return out


def run(graphs, mlp_dtype='fp32', loop=2, **env):
    """(scores, rows of the fp64 node role) of one forward under the given switches"""
    with environ(**env):
        m = model(mlp_dtype)
        b = gnnmp.GraphBatch.from_graphs(graphs, 2, DEV)
        s = m.forward_batch(b, loop)
        m0 = m.debug_tap(b, 4)
        m.check_status()
        torch.cuda.synchronize()
    return s.cpu().numpy().tobytes(), m0.cpu().numpy().tobytes()


# (node counts, obstacle counts): 1, 3 and 9 graphs; N = 40, 256, 300, 1000; O = 5, 33, 116 and 300 (three chunks of 128 in the
# fp64 role, which rebuilds its operands per chunk and group).  With 8 / 16 groups a workgroup runs from one graph into the next
# wherever the padded sizes (256, 256, 512, 1024 rows) are no multiple of its 512 / 1024 rows.
BATCHES = {
    'one': ([300], [33]),
    'three': ([40, 1000, 256], [5, 116, 33]),
    'nine': ([300, 40, 256, 1000, 40, 300, 256, 40, 1000], [116, 5, 33]),
    'chunks': ([300, 40, 256], [300, 5, 300]),
}


@pytest.mark.parametrize('name', list(BATCHES))
def test_rows_do_not_depend_on_the_groups_per_workgroup(name):
    sizes, n_obs = BATCHES[name]
    graphs = graphs_of(sizes, n_obs, seed=40)
    ref = run(graphs, GNNMP_F64_GROUPS=1)
    for groups in (4, 8, 16, None):                              # None: the launch's own choice
        got = run(graphs, GNNMP_F64_GROUPS=groups)
        assert got[1] == ref[1], ('M0', groups)
        assert got[0] == ref[0], ('scores', groups)


def test_launch_choice_on_a_batch_beyond_one_round():
    """More 256-row blocks in use than the device keeps workgroups of the obstacle launch resident (two per CU at d = 32): 260
    graphs of 300 nodes = 520 blocks.  The launch then weighs blocks per workgroup against resident rounds; whatever it picks,
    the rows are those of one block per workgroup."""
    graphs = graphs_of([300] * 4, [33, 116], seed=50) * 65
    ref = run(graphs, GNNMP_F64_GROUPS=4)
    assert run(graphs) == ref
    assert run(graphs, GNNMP_F64_GROUPS=12) == ref


@pytest.mark.parametrize('mlp_dtype', ['fp32', 'bf16x3'])
def test_both_double_precision_modes(mlp_dtype):
    """fp32 and bf16x3 operands both run the double-precision node role (bf16 does not)."""
    graphs = graphs_of([40, 300, 256], [5, 116, 33], seed=60)
    ref = run(graphs, mlp_dtype, GNNMP_F64_GROUPS=1)
    assert run(graphs, mlp_dtype, GNNMP_F64_GROUPS=8) == ref
    assert run(graphs, mlp_dtype) == ref


def test_training_forward_is_unchanged():
    """The training path stops after the pre kernels and takes node_free_code / edge_free_code (om_nodes / om_edges) from them:
    its scores move with any change of those rows."""
    graphs = graphs_of([40, 300, 256], [5, 116, 33], seed=70)

    def train(**env):
        with environ(**env):
            m = model()
            b = gnnmp.GraphBatch.from_graphs(graphs, 2, DEV)
            with torch.no_grad():
                s = m.train_scores(b, 2)
            torch.cuda.synchronize()
        return s.cpu().numpy().tobytes()
    ref = train(GNNMP_F64_GROUPS=1)
    assert train() == ref
    assert train(GNNMP_F64_GROUPS=8) == ref
