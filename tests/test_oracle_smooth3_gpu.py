"""gnnmp.oracle_smooth for the stick robot on the device (-m gpu): runs every test function of
tests/oracle_smooth3_gpu_cases.py -- the dim = 3 fixtures alone and after every recorded stage, ragged batches, 1024 paths
against one by one, device-form draws, random paths against the host restatement, trials that turn on the last bit of a
float32 norm, per-path error statuses, the public wrappers, the training targets -- in a child process each, and passes
when the child's pytest does.

Why a child: as for tests/test_oracle_smooth_gpu.py.  The cases make thousands of small device allocations and
read-backs; run inside the suite's process they change its allocator state for every module that follows, and
test_smoother_autograd_scale_gpu.py::test_ur5_long_path_odd_caller_edges depends on that state."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ['test_every_fixture_alone_final_and_every_stage', 'test_all_fixtures_as_one_ragged_batch',
         'test_batch_of_1024_equals_one_by_one_and_repeats', 'test_device_form_draws_reproduce_the_replay_and_draw_device',
         'test_random_paths_on_synthetic_maps_equal_the_host_restatement',
         'test_float32_norm_rounding_decides_a_trial',
         'test_bad_paths_get_a_status_and_leave_the_others_alone', 'test_public_wrappers_and_dtype_routes',
         'test_smoothing_targets_are_float32_rows_of_three']


def test_the_case_list_is_complete():
    src = open(os.path.join(REPO, 'tests', 'oracle_smooth3_gpu_cases.py')).read()
    assert sorted(re.findall(r'^def (test_\w+)\(', src, flags=re.M)) == sorted(CASES)


@pytest.mark.parametrize('case', CASES)
def test_oracle_smooth3_gpu(case):
    r = subprocess.run([sys.executable, '-m', 'pytest', 'tests/oracle_smooth3_gpu_cases.py::' + case, '-m', 'gpu', '-q', '-s',
                        '-p', 'no:cacheprovider'], cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode(errors='replace')
    print(out[-6000:])
    assert r.returncode == 0, 'the child pytest failed (exit %d); its output is above' % r.returncode
    assert ' passed' in out and ' skipped' not in out and ' failed' not in out, 'the child did not run its tests'
