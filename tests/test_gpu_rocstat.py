"""GPU: the device backend of pinn_amd.rocstat (csrc/pinn_rocstat.hip) against the package's host backend, which
tests/test_rocstat_host.py holds to the definitions.

Gates: everything the kernels produce is an integer and every float is an exact rational rounded once on the host, so the two
backends agree bit for bit: components, group numbers, U2, the 128-bit cross sums, the covariance and every resample of the
bootstrap.  The one statistical gate is the host test's: the bootstrap variances within 5 sqrt(2 / (B - 1)) of DeLong's."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import rocstat_cases as RC
import test_rocstat_host as H
from rocstat_cases import SIZES, VARIANTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def R():
    from pinn_amd import rocstat
    return rocstat


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def check_against_host(R, y, s, n_boot=6, seed=11, boot=True):
    """Components, covariance and bootstrap of one input on both backends, device tensors in."""
    hc = R.auc_components(y, s, backend="host")
    dc = R.auc_components(dev(y), dev(s), backend="device")
    assert (dc["n_pos"], dc["n_neg"]) == (hc["n_pos"], hc["n_neg"]) and np.array_equal(dc["U2"], hc["U2"])
    assert np.array_equal(dc["n_groups"], hc["n_groups"])
    for key in ("a", "b", "pos_rows", "neg_rows", "group"):
        assert dc[key].is_cuda and host(dc[key]).dtype == hc[key].dtype and np.array_equal(host(dc[key]), hc[key]), key
    if hc["n_pos"] >= 2 and hc["n_neg"] >= 2:
        hd, dd = R.delong_covariance(y, s, backend="host"), R.delong_covariance(dev(y), dev(s), backend="device")
        for key in ("auc", "cov", "S10", "S01"):
            assert dd[key].tobytes() == hd[key].tobytes(), key
    if boot:
        hb = R.bootstrap_auc(y, s, n_boot=n_boot, random_state=seed, first=3, backend="host")
        db = R.bootstrap_auc(dev(y), dev(s), n_boot=n_boot, random_state=seed, first=3, backend="device")
        assert db["U2_boot"].is_cuda and db["auc_boot"].is_cuda and db["U2_boot"].dtype == torch.int64
        assert np.array_equal(host(db["U2_boot"]), hb["U2_boot"]) and host(db["auc_boot"]).tobytes() == hb["auc_boot"].tobytes()
        assert db["cov_boot"].tobytes() == hb["cov_boot"].tobytes() and db["ci"].tobytes() == hb["ci"].tobytes()


@pytest.mark.parametrize("m,n", SIZES)
def test_host_cases_bit_for_bit(R, m, n):
    for variant in VARIANTS:
        y, s = RC.make_case(m, n, variant, K=2)
        check_against_host(R, y, s)


@pytest.mark.parametrize("N", [255, 256, 257, 513])
def test_scan_tile_edges(R, N):
    assert R.SCAN_TILE == 256
    for variant in ("continuous", "quarter"):
        y, s = RC.make_case(N // 3, N - N // 3, variant, K=3)
        check_against_host(R, y, s)


@pytest.mark.parametrize("K", [8, 1])
def test_five_thousand_rows(R, K):
    y, s = RC.make_case(1700, 3300, "continuous", K=K)
    check_against_host(R, y, s, n_boot=4)
    y, s = RC.make_case(1700, 3300, "eighth", K=K)
    check_against_host(R, y, s, n_boot=4)


@pytest.mark.parametrize("N", [12288, 12289])
def test_histogram_switch_between_lds_and_workspace(R, N):
    """Continuous scores: as many groups as rows, just below and just above what a workgroup counts in LDS; and the second
    classifier's few groups bring the workgroup back to LDS after a pass through the workspace."""
    assert R.BOOT_LDS_GROUPS == 12288
    y, s = RC.make_case(N // 4, N - N // 4, "continuous", K=2)
    s = s.copy()
    s[1] = np.round(s[1] * 8) / 8
    c = R.auc_components(y, s, backend="host")
    assert c["n_groups"][0] == N and c["n_groups"][1] < 200
    check_against_host(R, y, s, n_boot=5)
    # chunks of two resamples under a small workspace cap give the same resamples
    whole = R.bootstrap_auc(dev(y), dev(s), n_boot=5, random_state=11, backend="device")
    capped = R.bootstrap_auc(dev(y), dev(s), n_boot=5, random_state=11, backend="device", workspace_cap=2 * 4 * 12544)
    assert torch.equal(whole["U2_boot"], capped["U2_boot"])


def test_cross_sums_carry(R):
    """300 rows of values near 2^31..2^32: every product is near 2^63..2^64, so the low word wraps inside a workgroup's
    reduction and again when the two workgroups' partials are added; values near 2^40 need the high half of the product."""
    rng = np.random.default_rng(5)
    for lo, hi in ((1 << 31, 1 << 32), ((1 << 32) - 1000, 1 << 32), (1 << 39, 1 << 40), (0, 50)):
        comp = rng.integers(lo, hi, size=(3, 300), dtype=np.int64)
        P = R.component_cross_sums(dev(comp), backend="device")
        want = [[sum(int(x) * int(v) for x, v in zip(comp[k], comp[l])) for l in range(3)] for k in range(3)]
        assert P == want, (lo, hi)
        if lo >= 1 << 31:
            assert want[0][0] >> 64 > 0
    big = rng.integers(1 << 31, 1 << 32, size=(8, 70001), dtype=np.int64)               # the block cap: a workgroup takes several tiles
    assert R.component_cross_sums(dev(big), backend="device") == R.component_cross_sums(big, backend="host")


def test_same_bytes_devices_and_auto(R):
    y, s = RC.make_case(130, 127, "quarter", K=3)
    ty, ts = dev(y), dev(s)
    one, two = R.bootstrap_auc(ty, ts, n_boot=64, random_state=3), R.bootstrap_auc(ty, ts, n_boot=64, random_state=3)      # auto
    assert one["U2_boot"].is_cuda and torch.equal(one["U2_boot"], two["U2_boot"]) and torch.equal(one["auc_boot"], two["auc_boot"])
    c1, c2 = R.auc_components(ty, ts), R.auc_components(ty, ts)
    assert all(c1[k].is_cuda and torch.equal(c1[k], c2[k]) for k in ("a", "b", "group", "pos_rows", "neg_rows"))
    assert R.delong_covariance(ty, ts)["cov"].tobytes() == R.delong_covariance(ty, ts)["cov"].tobytes()
    # a host array through the device backend comes back as host arrays, with the host backend's values
    hb, db = R.bootstrap_auc(y, s, n_boot=8, backend="host"), R.bootstrap_auc(y, s, n_boot=8, backend="device")
    assert isinstance(db["U2_boot"], np.ndarray) and np.array_equal(db["U2_boot"], hb["U2_boot"])
    assert isinstance(R.auc_components(y, s, backend="device")["a"], np.ndarray)
    assert R.delong_test(ty, ts[0], ts[1])["p"] == R.delong_test(y, s[0], s[1], backend="host")["p"]
    assert R.compare_aucs(ty, ts)["p_holm"].tobytes() == R.compare_aucs(y, s, backend="host")["p_holm"].tobytes()
    with pytest.raises(ValueError):
        R.auc_components(ty, torch.where(ts > 2.0, torch.full_like(ts, float("nan")), ts))
    with pytest.raises(NotImplementedError):
        R.delong_covariance(ty, torch.cat([ts, ts, ts]))


def test_bootstrap_against_delong_on_the_device(R):
    H.check_bootstrap_against_delong(R, "device", wrap=dev)


def test_feature_groups_stay_on_the_device(R, golden, monkeypatch):
    from pinn_amd import detection as T
    from test_detection_host import Case
    c = Case(golden("g_lr.npz"), T, "b1")
    results = dev(np.nan_to_num(c.results, nan=0.0, posinf=0.0, neginf=0.0))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ev = T.evaluate_feature_groups(results, backend="device", split=(c.idx_tr, c.idx_te), unsupervised=True)
    assert all(e["p_fault"].is_cuda for e in ev)
    real = R._as_numpy

    def no_large_copies(x, dtype=None):
        assert not (isinstance(x, torch.Tensor) and x.is_cuda and x.numel() >= len(c.idx_te)), "a score vector was copied to the host"
        return real(x, dtype)

    monkeypatch.setattr(R, "_as_numpy", no_large_copies)
    table = R.compare_feature_groups(ev, n_boot=32)
    assert list(table) == list(T.FEATURE_GROUPS) + ["unsup"]
    for e in ev:
        assert table[e["spec"]]["auc"] == e["auc"]
    assert table["unsup"]["auc"] == ev[0]["auc_unsup"]
    monkeypatch.undo()
    again = R.compare_feature_groups([dict(e, p_fault=host(e["p_fault"]), anomaly_score=None) for e in ev], n_boot=32, backend="host")
    for e in ev:
        assert again[e["spec"]]["ci"] == table[e["spec"]]["ci"] and again[e["spec"]]["boot_ci"] == table[e["spec"]]["boot_ci"]


def test_example_prints_the_inference(R):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fault_detection.py"), "--inference", "--normal-rows", "4000",
                          "--fault-rows", "300"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "DeLong" in out.stdout and "Holm" in out.stdout and "bootstrap" in out.stdout
    assert out.stdout.rstrip().splitlines()[-1].split()[0] == str(4000 + 12 * 300)       # the replay still runs to the last chunk
