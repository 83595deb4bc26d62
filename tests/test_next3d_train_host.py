"""The host side of 3-D NEXT training, no GPU: the torch restatement (tests/next3d_train_host.py) against the float64 numpy
oracle of gnnmp.next_model3d and against the unmodified reference's recorded losses and gradients
(tests/golden/next3d_train_*.npz, tools/gen_golden_next3d_train.py), and gnnmp.next_train3d.path_labels against the reference's
own get_label outputs, the clipped step included."""
import numpy as np
import pytest
import torch

import gnnmp  # noqa: F401
from gnnmp import next_model3d, next_train, next_train3d
import next3d_train_host as host


@pytest.mark.parametrize('dim', [7, 14])
def test_restatement_equals_the_numpy_oracle_in_float64(dim):
    w = host.load_weights(dim)
    rec = host.load_case(dim)
    maps, goals, rows, of, ptr, _, _ = host.case_inputs(rec, 20)
    lv = host.leaves(w, torch.float64)
    for iters in (0, 2):
        with torch.no_grad():
            pb = host.pb_forward(lv, maps, goals, iters)
            y = host.state_forward(lv, rows, of, pb).numpy()
        pb_np = next_model3d.pb_forward_host(w, maps, goals, iters)
        y_np = next_model3d.state_forward_host(w, rows, of, pb_np)
        assert np.abs(pb.numpy() - pb_np).max() <= 1e-10 * max(1., np.abs(pb_np).max()), iters
        assert np.abs(y - y_np).max() <= 1e-10 * max(1., np.abs(y_np).max()), iters


@pytest.mark.parametrize('dim,iters', [(7, 0), (7, 1), (7, 2), (7, 20), (14, 1), (14, 20)])
def test_restatement_reproduces_the_recorded_reference_gradients(dim, iters):
    w = host.load_weights(dim)
    rec = host.load_case(dim)
    maps, goals, rows, of, ptr, actions, values = host.case_inputs(rec, iters)
    g32, g64 = host.load_grads(dim, iters)
    lv = host.leaves(w, torch.float64)
    y = host.forward(lv, maps, goals, rows, of, iters)
    loss = next_train.loss_from_outputs(y, torch.from_numpy(actions).double(), torch.from_numpy(values).double(), ptr)
    l64 = float(rec['loss64_i%d' % iters])
    assert abs(float(loss.detach()) - l64) <= 1e-9 * abs(l64)
    got = host.grads_of(loss, lv)
    assert set(got) == set(g64) == set(next_train3d.param_shapes(dim, host.FAMILIES[dim][1]))
    for k in g64:
        # g64 is stored as g32 + a float32 difference: exact to 1e-7 of the difference
        tol = 1e-9 * np.abs(g64[k]).max() + 2e-7 * np.abs(g64[k] - g32[k]).max()
        assert np.abs(got[k] - g64[k]).max() <= tol, (k, np.abs(got[k] - g64[k]).max(), tol)


@pytest.mark.parametrize('dim', [7, 14])
def test_path_labels_equal_the_recorded_get_label(dim):
    rec = host.load_case(dim)
    actions, values = next_train3d.path_labels(rec['paths'], rec['path_ptr'], float(rec['rrt_eps']), rec['lo'], rec['hi'])
    assert np.array_equal(actions, rec['actions'].astype(np.float32)) and np.array_equal(values, rec['values'].astype(np.float32))
    # the recorded case holds a step longer than RRT_EPS whose interpolated state is clipped at a joint limit ...
    p, eps = rec['paths'], float(rec['rrt_eps'])
    assert np.linalg.norm(p[4] - p[3]) > eps and p[4][1] > rec['hi'][1]
    assert p[3][1] + rec['actions'][3][1] == rec['hi'][1]
    # ... so without the limits the labels differ there, and only there
    free, _ = next_train3d.path_labels(rec['paths'], rec['path_ptr'], eps)
    differs = np.flatnonzero((free != actions).any(axis=1))
    assert list(differs) == [3]
    # a short step is kept whole, the last state of a path has a zero action, the values end at zero
    ptr = rec['path_ptr']
    assert np.array_equal(actions[1], (p[2] - p[1]).astype(np.float32)) and np.linalg.norm(p[2] - p[1]) < eps
    assert not actions[ptr[1:] - 1].any() and not values[ptr[1:] - 1].any()
    with pytest.raises(ValueError):
        next_train3d.path_labels(rec['paths'], [0, 5], eps)
    with pytest.raises(ValueError):
        next_train3d.param_shapes(16, 3)
    with pytest.raises(ValueError):
        next_train3d.param_shapes(7, 4)
