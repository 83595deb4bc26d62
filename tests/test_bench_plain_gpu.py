"""A plain bench.py run (no --full): the headline line only, exactly --steps timed steps, and --dump-outputs writing what the
timed path computed -- the per-edge scores of the batch, equal to the same forward called here on the same seeded problems."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, load_weights

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_and_dumps_the_scores(tmp_path):
    out_dir = tmp_path / 'dump'
    r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1', '--graphs', '8',
                        '--dump-outputs', str(out_dir)], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert line['unit'] == 'graphs/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0
    assert abs(line['value'] - 8 / (line['ms_per_step'] * 1e-3)) <= 1e-3 * line['value']
    # what moved behind --full is not in a plain line
    assert 'roofline' not in line and 'cpu_baseline' not in line
    assert not {'stage_ms_per_step', 'strong_leg', 'single_graph_us', 'planner', 'other_configs_gpu'} & set(line['config'])
    assert os.listdir(out_dir) == ['scores.npy']
    got = np.load(out_dir / 'scores.npy')

    import torch
    import gnnmp
    from gnnmp.synth import ENVS, synth_batch_gpu
    dev = torch.device('cuda:0')
    e = ENVS['maze2']
    model = gnnmp.EncoderProcessDecoder(e['workspace'], e['C'], e['d'], e['S']).eval()
    model.load_state_dict(load_weights(e['ckpt']), strict=True)
    graphs = synth_batch_gpu('maze2', 1000, 8, 8, dev, seed0=1234)
    want = model.forward_batch(gnnmp.GraphBatch.from_graphs(graphs, e['S'], dev), 5).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape == (sum(int(g['edge_index'].shape[1]) for g in graphs),)
    assert np.array_equal(got, want)
