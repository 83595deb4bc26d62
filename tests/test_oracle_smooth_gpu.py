"""gnnmp.oracle_smooth on the device (-m gpu): runs every test function of tests/oracle_smooth_gpu_cases.py -- the fixtures
alone and after every recorded stage, ragged batches, 2048 paths against one by one, device-form draws, per-path error
statuses, targets into the smoother's training loss -- in a child process each, and passes when the child's pytest does.

Why a child: the cases make thousands of small device allocations and read-backs.  Run inside the suite's process they
change its allocator state and buffer addresses for every module that follows, and
test_smoother_autograd_scale_gpu.py::test_ur5_long_path_odd_caller_edges, whose summation order (and with it its error,
0.63 to 1.06 of its bar over the runs measured) depends on that state, went over its bar.  A process of their own leaves
the suite's process as it was found."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ['test_every_fixture_alone_final_and_every_stage', 'test_all_fixtures_as_one_ragged_batch',
         'test_batch_of_2048_equals_one_by_one_and_repeats', 'test_device_form_draws_reproduce_the_replay_and_draw_device',
         'test_bad_paths_get_a_status_and_leave_the_others_alone', 'test_public_wrappers_and_dtype_routes',
         'test_smoothing_targets_feed_the_training_loss']


def test_the_case_list_is_complete():
    src = open(os.path.join(REPO, 'tests', 'oracle_smooth_gpu_cases.py')).read()
    import re
    assert sorted(re.findall(r'^def (test_\w+)\(', src, flags=re.M)) == sorted(CASES)


@pytest.mark.parametrize('case', CASES)
def test_oracle_smooth_gpu(case):
    r = subprocess.run([sys.executable, '-m', 'pytest', 'tests/oracle_smooth_gpu_cases.py::' + case, '-m', 'gpu', '-q', '-s',
                        '-p', 'no:cacheprovider'], cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors='replace')
    print(out[-6000:])
    assert r.returncode == 0, 'the child pytest failed (exit %d); its output is above' % r.returncode
    assert ' passed' in out and ' skipped' not in out and ' failed' not in out, 'the child did not run its tests'
