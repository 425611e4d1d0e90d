"""GPU: the device backend of pinn_amd.anomaly (csrc/pinn_iforest.hip) against tests/golden/g_iforest.npz (scikit-learn's
trees and scores) and against the package's host backend (numpy, the same state machine and draws).

Gates: the shared checks of tests/test_anomaly_host.py.  Depth sums, trees and subsamples are compared bit for
bit; scores within 4 units in the last place (two for numpy's power, two for the device's exp2); the ROC curve of the
fixture's forest is equal because the generator holds the two classes' scores at least 1e-12 apart.  Every comparison
prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from test_anomaly_host import (FIT_CASES, check_determinism, check_edge_cases, check_evaluate, check_fixture, check_monitor, check_own_fit,
                               check_scoring_shapes, check_threshold_edges, draw_rows, fixture_forest, held_out_rows, host, results_array,
                               same_forest, ulps)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(golden):
    return golden("g_iforest.npz")


@pytest.fixture(scope="module")
def A():
    from pinn_amd import anomaly
    return anomaly


@pytest.fixture(scope="module")
def T():
    from pinn_amd import detection
    return detection


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_fixture_forest_on_device(G, A, T):
    check_fixture(G, A, T, "device")
    check_fixture(G, A, T, "device", dev)
    f = fixture_forest(G, A, "a", "device")
    out = f.score_samples(dev(results_array(G)), columns=[11, 12], row_index=dev(held_out_rows(G)))
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64
    assert isinstance(f.predict(results_array(G), columns=[11, 12]), np.ndarray)


def test_threshold_edges_on_device(G, A):
    check_threshold_edges(G, A, "device", dev)


def test_both_kernel_variants_and_row_counts_agree(G, A):
    """Nodes staged through LDS and nodes read from global memory; one and four rows per thread (the switch is at 4 x 512 x 1024
    rows): the same depth sums bit for bit.  The deep forest has trees of up to 999 nodes, so its groups hold few trees."""
    arr = results_array(G)
    X = arr[held_out_rows(G)][:, [11, 12]]
    big = dev(np.tile(X, (1700, 1))[:4 * 512 * 1024 + 77])
    for tag in ("a", "b"):
        f = fixture_forest(G, A, tag, "device")
        want = fixture_forest(G, A, tag, "host").depth_sums(X)
        for variant in (0, 1):
            assert host(f.depth_sums(dev(X), variant=variant)).tobytes() == want.tobytes()
            got = f.depth_sums(big, variant=variant)
            ref = dev(want).repeat(1700)[:big.shape[0]]
            assert bool(torch.equal(got, ref)), (tag, variant)


@pytest.mark.parametrize("n,D,n_trees", FIT_CASES)
def test_own_fit_equals_the_host(A, n, D, n_trees):
    check_own_fit(A, "device", n, D, n_trees, dev if (n + D) % 2 else None)


def test_scoring_shapes_on_device(A):
    check_scoring_shapes(A, "device")
    check_scoring_shapes(A, "device", dev)


def test_edge_cases_on_device(A):
    check_edge_cases(A, "device")
    check_edge_cases(A, "device", dev)


def test_determinism_on_device(A):
    check_determinism(A, "device", dev)


def test_fit_reads_rows_in_place(A):
    X = draw_rows(900, 4, 21)
    arr = np.zeros((1200, 22))
    cols, idx = [11, 12, 0, 8], np.random.default_rng(3).permutation(1200)[:900]
    arr[np.ix_(idx, cols)] = X
    a = A.DeviceIsolationForest(7, random_state=8, backend="device").fit(dev(arr), columns=cols, row_index=dev(idx))
    b = A.DeviceIsolationForest(7, random_state=8, backend="device").fit(dev(X))
    c = A.DeviceIsolationForest(7, random_state=8, backend="host").fit(arr, columns=cols, row_index=idx)
    assert same_forest(a, b) and same_forest(a, c) and a.max_samples_ == 256


def test_evaluate_feature_groups_on_device(G, A, T):
    d = check_evaluate(G, A, T, "device", dev)
    h = check_evaluate(G, A, T, "host")
    assert same_forest(d[0]["iforest"], h[0]["iforest"]) and d[0]["auc_unsup"] == h[0]["auc_unsup"]
    assert int(ulps(d[0]["anomaly_score"], h[0]["anomaly_score"]).max()) <= 4
    assert np.array_equal(host(d[0]["fpr_unsup"]), h[0]["fpr_unsup"]) and np.array_equal(host(d[0]["tpr_unsup"]), h[0]["tpr_unsup"])
    assert isinstance(d[0]["anomaly_score"], torch.Tensor) and d[0]["anomaly_score"].is_cuda


def test_monitor_on_device(G, A):
    check_monitor(G, A, "device")
    check_monitor(G, A, "device", dev)
