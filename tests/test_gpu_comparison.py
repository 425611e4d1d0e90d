"""GPU: the device backend of pinn_amd.comparison (csrc/pinn_cluster.hip) against tests/golden/g_cluster.npz and against
the package's host backend (float64 numpy, the same state machines).

Gates (from the reference's own sensitivity and the arithmetic, not from what the kernels give): the fixture
gates of tests/test_comparison_host.py; one Lloyd iteration on drawn data: labels equal, every sum within 1e-12 x the sum
of its absolute terms; Ward on drawn data: children_ equal, heights within 1e-12 relative, at most 3 (n - 1) chain steps.
The drawn cases are first held to the fixture tool's margin conditions on the host's series (at most 3 redraws).
In-place and gathered reads, repeated calls and chunked diagnosis are compared bit for bit.  Every comparison prints its
maxima before it asserts."""
import numpy as np
import pytest
import torch

from test_comparison_host import (blobs, check_diagnoser, check_duplicates, check_empty_cluster, check_metrics, check_offset, check_own_start,
                                  check_posteriors, host, lloyd_case, ward_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(golden):
    return golden("g_cluster.npz")


@pytest.fixture(scope="module")
def P():
    from pinn_amd import comparison
    return comparison


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_device_matches_reference_fixture(G, P):
    k, w = check_posteriors(G, P, "device")
    for a in (k["y_pred"], k["y_prob"], k["model"].cluster_centers_, k["model"].labels_, w["model"].labels_, w["model"].cluster_means_):
        assert isinstance(a, np.ndarray)
    tk, tw = check_posteriors(G, P, "device", dev)
    for a in (tk["y_pred"], tk["y_prob"], tk["cluster_class_prob"], tk["model"].cluster_centers_, tk["model"].labels_, tw["model"].labels_,
              tw["model"].cluster_means_):
        assert isinstance(a, torch.Tensor) and a.is_cuda
    assert host(tk["model"].cluster_centers_).tobytes() == k["model"].cluster_centers_.tobytes()
    assert host(tw["model"].cluster_means_).tobytes() == w["model"].cluster_means_.tobytes()
    assert tw["model"].distances_.tobytes() == w["model"].distances_.tobytes()
    km = k["model"]
    assert np.array_equal(km.predict(G["X_tr"]), G["km_labels"]) and km.strict_ in (True, False) and km.tol_abs_ > 0
    e_t = abs(km.tol_abs_ - P.host_tolerance(G["X_tr"], 1e-4)) / km.tol_abs_
    print("tol_abs on the device against numpy's variance: %.3e (gate 1e-13)" % e_t)
    assert e_t <= 1e-13


def test_device_own_start(G, P):
    check_own_start(G, P, "device")
    check_own_start(G, P, "device", dev)


LLOYD_CASES = [(n, K, Dm) for n in (1, 127, 128, 129, 2049, 100003) for K in (1, 2, 20, 32) for Dm in (1, 4, 8)]


@pytest.mark.parametrize("n,K,Dm", LLOYD_CASES)
def test_one_lloyd_iteration_against_the_host(P, n, K, Dm):
    X, c0, h = lloyd_case(P, n, K, Dm)
    d = P.lloyd_iteration(X, c0, backend="device")
    assert np.array_equal(d["labels"], h["labels"])
    err = np.abs(d["sums"] - h["sums"])
    ratio = (err / np.where(h["abs_sums"] > 0, h["abs_sums"], 1.0)).max()
    e_c = np.abs(d["centres"] - h["centres"]).max() / max(np.abs(h["centres"]).max(), 1e-300)
    e_i = abs(d["inertia"] - h["inertia"]) / max(h["inertia"], 1e-300)
    e_t = abs(d["tol_abs"] - h["tol_abs"]) / max(h["tol_abs"], 1e-300)
    print("n=%d K=%d D=%d: sums %.3e x sum|terms| (gate 1e-12), centres %.3e, inertia %.3e, tol_abs %.3e (gates 1e-12)" % (n, K, Dm, ratio, e_c, e_i, e_t))
    assert np.all(err <= 1e-12 * h["abs_sums"])
    assert e_c <= 1e-12 and e_i <= 1e-12 and e_t <= 1e-12
    assert abs(d["shift"] - h["shift"]) <= 1e-12 * max(h["shift"], 1e-300) + 1e-24


WARD_CASES = [(n, Dm) for n in (2, 3, 129, 1025, 2049) for Dm in (1, 4, 8)]


@pytest.mark.parametrize("n,Dm", WARD_CASES)
def test_ward_against_the_host(P, n, Dm):
    X, h = ward_case(P, n, Dm)
    d = P.DeviceWard(min(16, n), backend="device").fit(X)
    e = np.max(np.abs(d.distances_ - h.distances_) / h.distances_)
    print("n=%d D=%d: heights %.3e (gate 1e-12), steps %d host %d (bound %d)" % (n, Dm, e, d.n_steps_, h.n_steps_, 3 * (n - 1)))
    assert np.array_equal(d.children_, h.children_) and np.array_equal(d.labels_, h.labels_)
    assert e <= 1e-12 and d.n_steps_ <= 3 * (n - 1)
    e_m = np.abs(d.cluster_means_ - h.cluster_means_).max() / np.abs(h.cluster_means_).max()
    assert e_m <= 1e-13, e_m


def test_device_properties(G, P):
    check_duplicates(P, "device")
    check_duplicates(P, "device", dev)
    check_offset(P, "device")
    check_empty_cluster(P, "device")
    check_empty_cluster(P, "device", dev)
    check_diagnoser(G, P, "device")
    check_diagnoser(G, P, "device", dev)


def test_in_place_and_gathered_reads_equal_the_packed_copy_and_calls_repeat(G, P):
    X = G["X_tr"]
    n = len(X)
    rng = np.random.default_rng(4)
    full = rng.normal(0.0, 1.0, (n + 300, 11))
    where = rng.permutation(n + 300)[:n]
    full[where[:, None], [9, 2, 5, 0]] = X
    cols, ridx = [9, 2, 5, 0], dev(where.astype(np.int64))
    t_full, t_X = dev(full), dev(X)
    a = P.DeviceKMeans(20, init=G["km_init"], backend="device").fit(t_X)
    b = P.DeviceKMeans(20, init=G["km_init"], backend="device").fit(t_full, columns=cols, row_index=ridx)
    c = P.DeviceKMeans(20, init=G["km_init"], backend="device").fit(t_X)
    for m in (b, c):
        assert host(m.cluster_centers_).tobytes() == host(a.cluster_centers_).tobytes() and host(m.labels_).tobytes() == host(a.labels_).tobytes()
        assert m.inertia_ == a.inertia_ and m.n_iter_ == a.n_iter_
    assert host(b.predict(t_full, columns=cols, row_index=ridx)).tobytes() == host(a.predict(t_X)).tobytes()
    wa = P.DeviceWard(16, backend="device").fit(t_X)
    wb = P.DeviceWard(16, backend="device").fit(t_full, columns=cols, row_index=ridx)
    wc = P.DeviceWard(16, backend="device", chunk=97).fit(t_X)           # another chunking of the queue: the same steps
    for m in (wb, wc):
        assert m.distances_.tobytes() == wa.distances_.tobytes() and m.children_.tobytes() == wa.children_.tobytes()
        assert host(m.cluster_means_).tobytes() == host(wa.cluster_means_).tobytes() and m.n_steps_ == wa.n_steps_
    # a gather index outside the array reads nothing: it gets no cluster, NaN and adds nothing to a sum
    bad = torch.cat([ridx[:50], torch.tensor([-1, n + 300], device="cuda")])
    r = P.assign_clusters(t_full, a.cluster_centers_, None, cols, bad, "device", want=("cluster", "dist2"))
    assert host(r["cluster"])[50:].tolist() == [-1, -1] and np.all(np.isnan(host(r["dist2"])[50:]))
    assert np.array_equal(host(r["cluster"])[:50], host(a.predict(t_X))[:50])
    it_ok = P.lloyd_iteration(t_full, G["km_init"], columns=cols, row_index=ridx[:50], backend="device")
    it_bad = P.lloyd_iteration(t_full, G["km_init"], columns=cols, row_index=bad, backend="device")
    assert host(it_bad["sums"]).tobytes() == host(it_ok["sums"]).tobytes() and host(it_bad["labels"])[50:].tolist() == [-1, -1]


def test_limits_and_compare_methods_on_the_device(G, P):
    X, _ = blobs(200, 4, 9, 1)
    with pytest.raises(NotImplementedError):
        P.DeviceKMeans(33, init=np.zeros((33, 4)), backend="device").fit(X[:, :4])
    with pytest.raises(NotImplementedError):
        P.DeviceKMeans(4, init=np.zeros((4, 9)), backend="device").fit(X)
    with pytest.raises(NotImplementedError):
        P.DeviceWard(4, backend="device").fit(X)
    from pinn_amd import _lib
    lib = _lib.load()
    assert lib.pinn_km_state_bytes(100, 33, 4) == 0 and lib.pinn_km_workspace_bytes(100, 4, 9) == 0 and lib.pinn_ward_state_bytes(100, 9) == 0
    Xa = np.concatenate([G["X_tr"], G["X_te"]])
    ya = np.concatenate([G["y_tr"], G["y_te"]])
    n_tr = len(G["y_tr"])
    split = (np.arange(n_tr), n_tr + np.arange(len(G["y_te"])))
    r = P.compare_methods(dev(Xa), dev(ya), split=split, backend="device", method_args={"KMeans": {"init": G["km_init"]}})
    assert list(r) == ["split", "GMM", "Sup_LR", "KMeans", "Agglo"]
    assert np.array_equal(r["KMeans"]["y_pred"], G["km_y_pred"]) and np.array_equal(r["Agglo"]["y_pred"], G["ward_y_pred"])
    check_metrics(r["KMeans"], G["km_metrics"], "compare_methods KMeans, device")
    check_metrics(r["Agglo"], G["ward_metrics"], "compare_methods Agglo, device")
    with pytest.raises(NotImplementedError):
        P.compare_methods(dev(Xa), dev(ya), methods=("Spectral",), split=split, backend="device")
