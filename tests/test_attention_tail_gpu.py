"""The obstacle-attention loop of the exact-fp32 pre kernels around its last tile (attention_block, explorer_kernels.hip).

The fp32 kernels peel the one obstacle tile that can hold padding: full tiles run unmasked through the 16-MFMA PV chain, the
last tile starts its logit chain from a per-graph 0 / -inf vector kept in LDS and runs 4, 8, 12 or 16 PV MFMAs.  None of this
may change a bit of the scores.  Cases (70-node k = 4 maze2 graphs, loop 2, one per obstacle count):

  SMALL    O <= 128, the LDS-resident kernels: every PV length 1..4 on the last tile, 1 to 4 tiles, exactly full last tiles.
  CHUNKED  O > 128, pre_kernel streaming the K/V tiles in chunks: only the final chunk has a partial tile.
  kuka7    d = 64 (two feature tiles per row), its own 5 boxes and 40 boxes.
  ragged   a batch mixing obstacle counts, against the per-graph calls.

tests/golden/attention_tail_maze2_fp32.npz holds the scores of the SMALL and CHUNKED cases (key `O<count>`) as commit a667573
("Maze planner on the device: resample rounds for a whole batch at once"), the last one with the masked form inside the loop,
computed them on an MI355X; test_recorded_bits pins later changes of the loop to those bits.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_weights
import gnnmp
from gnnmp.synth import ENVS, synth_graph
from parity_bar import assert_fp32_parity, explorer_oracle_pair

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

SMALL = [1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 57, 64, 65, 97, 104, 105, 116, 120, 121, 128]
CHUNKED = [129, 136, 137, 160, 300]
FIXTURE = os.path.join(GOLDEN, 'attention_tail_maze2_fp32.npz')
LOOP = 2


def make_model(env):
    e = ENVS[env]
    m = gnnmp.EncoderProcessDecoder(e['workspace'], e['C'], e['d'], e['S']).eval()       # mlp_dtype: the fp32 default
    m.load_state_dict(load_weights(e['ckpt']), strict=True)
    return m


def to_dev(g):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in g.items()}


def tail_graph(n_obs):
    """70 nodes, k = 4, `n_obs` obstacles.  The maze grid has 225 cells: beyond that the obstacles are uniform points of the
    same box, as in test_explorer_parity.test_obstacle_counts."""
    g = synth_graph('maze2', 70, 4, seed=4000 + n_obs, n_obs=min(n_obs, 225))
    if n_obs > 225:
        g['obstacles'] = torch.rand(n_obs, 2, generator=torch.Generator().manual_seed(n_obs)) - 0.5
    assert g['obstacles'].shape[0] == n_obs
    return g


@functools.lru_cache(maxsize=None)
def maze_model():
    return make_model('maze2')


@functools.lru_cache(maxsize=None)
def maze_scores(n_obs):
    """GPU scores of one case, computed once and shared by the parity and the recorded-bits test."""
    d = to_dev(tail_graph(n_obs))
    return maze_model().edge_scores(d['goal'], LOOP, d['v'], d['obstacles'], d['edge_index']).cpu()


@pytest.mark.parametrize('n_obs', SMALL + CHUNKED)
def test_oracle_parity(n_obs):
    g = tail_graph(n_obs)
    ref32, ref64 = explorer_oracle_pair(load_weights('weights_maze'), g, LOOP)
    assert_fp32_parity(maze_scores(n_obs), ref32, ref64, 'maze2 O=%d' % n_obs)


@pytest.mark.parametrize('n_obs', SMALL + CHUNKED)
def test_recorded_bits(n_obs):
    with np.load(FIXTURE) as f:
        want = torch.from_numpy(f['O%d' % n_obs])
    assert torch.equal(maze_scores(n_obs), want)


@pytest.mark.parametrize('n_obs', [5, 40])
def test_d64_fp32(n_obs):
    g = synth_graph('kuka7', 64, 4, seed=77, n_obs=n_obs)
    d = to_dev(g)
    s = make_model('kuka7').edge_scores(d['goal'], LOOP, d['v'], d['obstacles'], d['edge_index']).cpu()
    ref32, ref64 = explorer_oracle_pair(load_weights('weights_kuka'), g, LOOP)
    assert_fp32_parity(s, ref32, ref64, 'kuka7 O=%d' % n_obs)


def test_ragged_batch_equals_single():
    counts = [116, 57, 128, 1, 90, 33]
    graphs = [tail_graph(o) for o in counts]
    m = maze_model()
    b = gnnmp.GraphBatch.from_graphs(graphs, 2, DEV)
    parts = b.split_edges(m.forward_batch(b, LOOP))
    for o, g, p in zip(counts, graphs, parts):
        d = to_dev(g)
        s1 = m.edge_scores(d['goal'], LOOP, d['v'], d['obstacles'], d['edge_index'])
        assert torch.equal(s1, p), 'O=%d' % o
