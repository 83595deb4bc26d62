"""Host steering of the smoothing stage for the stick robot: planner.smooth_step over maze2d.Maze3D against
tests/golden/steer3_*.npz, recorded from the unmodified reference's proposed_path_smootherv2 over MazeEnv(dim=3)
(tools/gen_golden_steer3.py) -- the yardstick the device kernel (tests/test_stick_steer_gpu.py) is held to."""
import os

import numpy as np
import pytest

from conftest import golden_files
from gnnmp import planner
from gnnmp.maze2d import Maze3D

def _load(path):
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


ALL = golden_files('steer3_')
CASES = [p for p in ALL if not bool(_load(p)['raised'])]           # assert_z: the reference raised, no result to compare


def test_every_case_is_there():
    names = {os.path.basename(p)[len('steer3_'):-len('.npz')] for p in ALL}
    assert names == {'len2', 'len3', 'noop', 'arrive', 'revert', 'zwrap_disp', 'zwrap_state', 'zwrap_edge', 'invalid_near',
                     'out_of_map', 'long_edge_64', 'long_edge_65', 'long_edge_150', 'long_edge_2pass', 'fail_first', 'fail_lane63', 'fail_pass2',
                     'assert_z', 'p12_0', 'p12_1'}


@pytest.mark.parametrize('path', CASES, ids=[os.path.basename(p)[7:-4] for p in CASES])
def test_smooth_step_reproduces_the_reference(path):
    c = _load(path)
    env = Maze3D(c['map'].astype(np.float64)[None], np.zeros((1, 3)), np.zeros((1, 3)))
    env.init_new_problem(0)
    env.collision_check_count = 0
    old = [r.copy() for r in c['old_path']]
    out = planner.smooth_step(old, c['new_path'].copy(), env)
    out = np.array(out, dtype=np.float32).reshape(-1, 3)
    assert out.tobytes() == c['result'].tobytes(), np.abs(out - c['result']).max()
    assert env.collision_check_count == int(c['checks'])
