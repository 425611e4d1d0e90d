"""CPU: pinn_amd.rocstat's host backend against the definitions (tests/rocstat_cases.py): DeLong's components and covariance
exactly, the paired test and Holm's adjustment, the keying of the bootstrap, the bootstrap against DeLong, the feature-group
table, the argument errors and the host checks of the three entry points.

Gates: integers are equal; a float is the exact rational rounded once, so it is equal bit for bit; the bootstrap variances
lie within a relative 5 sqrt(2 / (B - 1)) of DeLong's, the sampling error of a variance from B near-normal draws at 5 s.e."""
import ctypes
import math
import warnings
from fractions import Fraction

import numpy as np
import pytest

import rocstat_cases as RC
from rocstat_cases import SIZES, VARIANTS


@pytest.fixture(scope="module")
def R():
    from pinn_amd import rocstat
    return rocstat


@pytest.mark.parametrize("m,n", SIZES)
def test_components_equal_the_double_loop(R, m, n):
    from pinn_amd import detection
    for variant in VARIANTS:
        y, s = RC.make_case(m, n, variant, K=2)
        c = R.auc_components(y, s, backend="host")
        A, B = RC.brute_components(y, s)
        assert c["n_pos"] == m and c["n_neg"] == n and c["a"].dtype == np.int64 and c["b"].dtype == np.int64
        assert c["a"].tolist() == A and c["b"].tolist() == B, variant
        assert np.array_equal(c["pos_rows"], np.flatnonzero(y == 1)) and np.array_equal(c["neg_rows"], np.flatnonzero(y == 0))
        for k in range(2):
            U2 = detection.roc_counts(y, s[k], backend="host", curve=False)["U2"]
            assert sum(A[k]) == sum(B[k]) == int(c["U2"][k]) == U2, (variant, k)
            # rows of one group share a score, rows of different groups do not, and the numbering ascends with the score
            g = c["group"][k]
            order = np.argsort(s[k], kind="stable")
            assert np.all(np.diff(g[order]) == (np.diff(s[k][order]) != 0)) and g[order][0] == 0 and c["n_groups"][k] == g.max() + 1


def semi_definite_after_shift(M, shift):
    """True when no eigenvalue of the float64 matrix M lies below -shift, decided exactly: M + shift I, taken as rationals,
    is eliminated symmetrically; a negative pivot, or a zero pivot with anything left in its row, means indefinite.
    eigvalsh errs by about eps |M|, a hundred times the shift asked for here, so it cannot decide this for a rank-deficient M
    (K classifiers on fewer than K rows of a class)."""
    K = M.shape[0]
    A = [[Fraction(float(M[i, j])) + (Fraction(shift) if i == j else 0) for j in range(K)] for i in range(K)]
    for i in range(K):
        if A[i][i] < 0 or (A[i][i] == 0 and any(A[i][c] != 0 for c in range(i + 1, K))):
            return False
        if A[i][i] == 0:
            continue
        for r in range(i + 1, K):
            f = A[r][i] / A[i][i]
            for c in range(i, K):
                A[r][c] -= f * A[i][c]
    return True


@pytest.mark.parametrize("K", [1, 3, 8])
def test_covariance_is_the_textbook_definition_rounded_once(R, K):
    for (m, n), variant in [((7, 13), "quarter"), ((60, 180), "eighth"), ((130, 127), "continuous"), ((2, 2), "continuous")]:
        y, s = RC.make_case(m, n, variant, K=K)
        theta, cov = RC.textbook_cov(*RC.brute_components(y, s))
        d = R.delong_covariance(y, s, backend="host")
        want = np.array([[float(v) for v in row] for row in cov])
        assert d["cov"].tobytes() == want.tobytes() and d["auc"].tobytes() == np.array([float(t) for t in theta]).tobytes()
        assert np.array_equal(d["cov"], d["cov"].T) and d["cov"].shape == (K, K)
        assert np.allclose(d["cov"], d["S10"] / m + d["S01"] / n, rtol=1e-13, atol=1e-300)
        ev = np.linalg.eigvalsh(d["cov"])
        print("K=%d (%d, %d) %s: smallest eigenvalue by eigvalsh %.3e, trace %.3e" % (K, m, n, variant, ev[0], np.trace(d["cov"])))
        assert semi_definite_after_shift(d["cov"], 1e-18 * float(np.trace(d["cov"])))


def test_degenerate_scores_have_zero_variance(R):
    for (m, n) in SIZES:
        y, s = RC.make_case(m, n, "equal", K=2)
        d = R.delong_covariance(y, s, backend="host")
        assert np.all(d["auc"] == 0.5) and not d["cov"].any()
        y, s = RC.make_case(m, n, "separated", K=2)
        d = R.delong_covariance(y, s, backend="host")
        assert np.all(d["auc"] == 1.0) and not d["cov"].any()
        assert R.auc_ci(y, s[0], backend="host") == (1.0, 1.0, 1.0)
        assert R.auc_ci(y, s[0], method="logit", backend="host") == (1.0, 1.0, 1.0)       # falls back to "delong"


def test_delong_test_holm_and_intervals(R):
    y, s = RC.make_case(60, 180, "eighth", K=3, shifts=[1.5, 1.0, 0.3])
    same = R.delong_test(y, s[0], s[0].copy(), backend="host")
    assert same["p"] == 1.0 and same["diff"] == 0.0 and same["var_diff"] == 0.0 and math.isnan(same["z"])
    ab, ba = R.delong_test(y, s[0], s[2], backend="host"), R.delong_test(y, s[2], s[0], backend="host")
    assert ab["diff"] == -ba["diff"] and ab["z"] == -ba["z"] and ab["p"] == ba["p"] and ab["var_diff"] == ba["var_diff"]
    assert ab["diff"] > 0 and 0.0 < ab["p"] < 1e-3
    theta, cov = RC.textbook_cov(*RC.brute_components(y, s[[0, 2]]))
    var = cov[0][0] + cov[1][1] - 2 * cov[0][1]
    assert ab["var_diff"] == float(var) and ab["diff"] == float(theta[0] - theta[1])
    assert ab["z"] == float(theta[0] - theta[1]) / math.sqrt(float(var)) and ab["p"] == math.erfc(abs(ab["z"]) / math.sqrt(2.0))
    # zero variance with a difference: all scores equal against perfect separation
    y2, eq = RC.make_case(7, 13, "equal")
    sep = np.where(y2 == 1, 2.0, -2.0)
    r = R.delong_test(y2, sep, eq[0], backend="host")
    assert r["var_diff"] == 0.0 and r["diff"] == 0.5 and r["z"] == math.inf and r["p"] == 0.0
    r = R.delong_test(y2, eq[0], sep, backend="host")
    assert r["z"] == -math.inf and r["p"] == 0.0
    # all pairs, Holm against the reference in rocstat_cases
    y8, s8 = RC.make_case(130, 127, "quarter", K=5, shifts=[1.2, 1.1, 0.9, 0.5, 0.45])
    c = R.compare_aucs(y8, s8, names=list("abcde"), backend="host")
    pairs = [(k, l) for k in range(5) for l in range(k + 1, 5)]
    want = RC.holm_reference([c["p"][k, l] for k, l in pairs])
    assert [c["p_holm"][k, l] for k, l in pairs] == want and np.array_equal(c["p_holm"], c["p_holm"].T)
    assert np.all(c["p_holm"] >= c["p"]) and np.array_equal(c["diff"], -c["diff"].T) and c["names"] == list("abcde")
    for k, l in pairs:
        t = R.delong_test(y8, s8[k], s8[l], backend="host")
        assert (t["diff"], t["z"], t["p"]) == (c["diff"][k, l], c["z"][k, l], c["p"][k, l])
    z95 = 1.959963984540054
    for k in range(5):
        a, lo, hi = R.auc_ci(y8, s8[k], backend="host")
        assert a == c["auc"][k] and (lo, hi) == tuple(c["ci"][k]) and abs((hi - lo) / 2 - z95 * c["se"][k]) <= 1e-12
        a, lo, hi = R.auc_ci(y8, s8[k], method="logit", backend="host")
        assert 0.0 < lo < a < hi < 1.0
    ys, ss = RC.make_case(2, 2, "continuous", seed=3)                                  # a wide interval stays inside (0, 1)
    a, lo, hi = R.auc_ci(ys, ss[0], method="logit", level=0.999, backend="host")
    assert (a in (0.0, 1.0)) or 0.0 < lo <= a <= hi < 1.0


def test_bootstrap_keying(R):
    y, s = RC.make_case(7, 13, "quarter", K=3)
    seed = 20261019
    one = R.bootstrap_auc(y, s, n_boot=5, random_state=seed, backend="host")
    two = R.bootstrap_auc(y, s, n_boot=5, random_state=seed, backend="host")
    assert one["U2_boot"].dtype == np.int64 and one["U2_boot"].shape == (5, 3)
    assert one["U2_boot"].tobytes() == two["U2_boot"].tobytes() and one["auc_boot"].tobytes() == two["auc_boot"].tobytes()
    assert np.array_equal(one["auc_boot"], one["U2_boot"] / (2 * 7 * 13))
    for r in range(5):
        for k in range(3):
            assert int(one["U2_boot"][r, k]) == RC.brute_resample_u2(y, s[k], seed, r), (r, k)
    # a resample depends on (seed, number) only: splitting, the number of classifiers and another seed
    head = R.bootstrap_auc(y, s, n_boot=2, random_state=seed, backend="host")
    tail = R.bootstrap_auc(y, s, n_boot=3, first=2, random_state=seed, backend="host")
    assert np.array_equal(np.concatenate([head["U2_boot"], tail["U2_boot"]]), one["U2_boot"])
    alone = R.bootstrap_auc(y, s[0], n_boot=5, random_state=seed, backend="host")
    assert np.array_equal(alone["U2_boot"][:, 0], one["U2_boot"][:, 0]) and alone["U2_boot"].shape == (5, 1)
    other = R.bootstrap_auc(y, s, n_boot=5, random_state=seed + 1, backend="host")
    assert not np.array_equal(other["U2_boot"], one["U2_boot"])
    assert [int(v) for v in R.bootstrap_draws(seed, 3, 1, 7)] == RC.philox_draws(seed, 3, 1, 7)
    y1, s1 = np.array([0, 1]), np.array([0.5, 0.5])                                    # one row of each class is enough here
    assert np.all(R.bootstrap_auc(y1, s1, n_boot=4, backend="host")["U2_boot"] == 1)


BOOT_CASE = dict(m=60, n=180, variant="eighth", K=3, shifts=[1.5, 1.0, 0.3], n_boot=2000, seed=7)


def check_bootstrap_against_delong(R, backend, wrap=lambda a: a):
    """Two independent routes to one quantity: the variances of the AUCs and of the first pairwise difference."""
    c = BOOT_CASE
    y, s = RC.make_case(c["m"], c["n"], c["variant"], K=c["K"], shifts=c["shifts"])
    d = R.delong_covariance(y, s, backend="host")
    b = R.bootstrap_auc(wrap(y), wrap(s), n_boot=c["n_boot"], random_state=c["seed"], backend=backend)
    band = 5.0 * math.sqrt(2.0 / (c["n_boot"] - 1))
    ratios = [b["cov_boot"][k, k] / d["cov"][k, k] for k in range(c["K"])]
    ratios.append((b["cov_boot"][0, 0] + b["cov_boot"][1, 1] - 2 * b["cov_boot"][0, 1]) / (d["cov"][0, 0] + d["cov"][1, 1] - 2 * d["cov"][0, 1]))
    print("bootstrap / DeLong variances (%s): %s, band %.3f" % (backend, ", ".join("%.4f" % r for r in ratios), band))
    assert all(abs(r - 1.0) <= band for r in ratios)
    for k in range(c["K"]):                        # the percentile interval brackets the estimate and is about 2 z se wide
        assert b["ci"][k, 0] < d["auc"][k] < b["ci"][k, 1]
    assert b["diff_ci"][0, 2, 0] > 0 and np.allclose(b["diff_ci"][0, 2], -b["diff_ci"][2, 0][::-1], rtol=1e-12)
    return b


def test_bootstrap_against_delong(R):
    b = check_bootstrap_against_delong(R, "host")
    y, s = RC.make_case(60, 180, "eighth", K=3, shifts=[1.5, 1.0, 0.3])
    a, lo, hi = R.auc_ci(y, s[0], method="bootstrap", n_boot=2000, random_state=7, backend="host")
    assert (a, lo, hi) == (b["auc"][0], b["ci"][0, 0], b["ci"][0, 1])


def test_compare_feature_groups(R, golden):
    from pinn_amd import detection as T
    from test_detection_host import Case
    c = Case(golden("g_lr.npz"), T, "b1")
    results = np.nan_to_num(c.results, nan=0.0, posinf=0.0, neginf=0.0)        # every group keeps the same rows: one split serves all
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ev = T.evaluate_feature_groups(results, backend="host", split=(c.idx_tr, c.idx_te), unsupervised=True)
        table = R.compare_feature_groups(ev, n_boot=50, random_state=1, backend="host")
        assert list(table) == list(T.FEATURE_GROUPS) + ["unsup"]
        for e in ev:
            row = table[e["spec"]]
            assert row["auc"] == e["auc"] and row["ci"][0] <= row["auc"] <= row["ci"][1] and row["boot_ci"][0] <= row["boot_ci"][1]
            assert set(row["p_holm"]) == set(table) - {e["spec"]}
        assert table["unsup"]["auc"] == ev[0]["auc_unsup"]
        assert table["epi,res"]["diff"]["res"] == -table["res"]["diff"]["epi,res"]
        plain = R.compare_feature_groups(ev[:2], backend="host")
        assert "boot_ci" not in plain["epi,res"] and list(plain) == list(T.FEATURE_GROUPS[:2]) + ["unsup"]
        # a group evaluated on another split (the same rows in another order is another pairing)
        odd = T.evaluate_feature_groups(results, feature_groups=[T.FEAT_GRP3], backend="host", split=(c.idx_tr, c.idx_te[::-1].copy()))
        with pytest.raises(ValueError, match="'res'"):
            R.compare_feature_groups([ev[0], ev[1], odd[0]], backend="host")


def test_argument_errors(R):
    y, s = RC.make_case(7, 13, "continuous", K=2)
    bad = s.copy()
    bad[1, 3] = np.nan
    with pytest.raises(ValueError):
        R.auc_components(y, bad, backend="host")
    bad[1, 3] = np.inf
    with pytest.raises(ValueError):
        R.delong_covariance(y, bad, backend="host")
    with pytest.raises(ValueError):
        R.bootstrap_auc(y, bad, n_boot=2, backend="host")
    with pytest.raises(ValueError):
        R.auc_components(y[:-1], s, backend="host")
    with pytest.raises(ValueError):
        R.delong_covariance(y, np.zeros((0, 20)), backend="host")
    with pytest.raises(ValueError):
        R.delong_test(y, s[0], s[1][:-1], backend="host")
    one_pos = np.zeros(20, dtype=np.int64)
    one_pos[4] = 1
    for fn in (R.auc_components, R.delong_covariance, lambda *a, **k: R.compare_aucs(*a, **k)):
        with pytest.raises(ValueError):
            fn(one_pos, s, backend="host")
        with pytest.raises(ValueError):
            fn(1 - one_pos, s, backend="host")
    with pytest.raises(ValueError):
        R.auc_ci(one_pos, s[0], backend="host")
    assert R.bootstrap_auc(one_pos, s, n_boot=3, backend="host")["U2_boot"].shape == (3, 2)
    with pytest.raises(ValueError):
        R.bootstrap_auc(np.zeros(20, dtype=np.int64), s, n_boot=3, backend="host")
    with pytest.raises(ValueError):
        R.bootstrap_auc(y, s, n_boot=0, backend="host")
    with pytest.raises(ValueError):
        R.auc_ci(y, s[0], method="wald", backend="host")
    with pytest.raises(ValueError):
        R.auc_ci(y, s[0], level=1.0, backend="host")
    with pytest.raises(ValueError):
        R.compare_aucs(y, s, names=["one"], backend="host")
    with pytest.raises(ValueError):
        R.auc_components(np.arange(20), s, backend="host")                          # not binary and no pos_label
    assert R.auc_components(np.where(y == 1, 5, 2), s, pos_label=5, backend="host")["n_pos"] == 7
    # nine score vectors: the host takes them, the device kernels are not built for them
    import pinn_amd
    assert pinn_amd.delong_covariance is R.delong_covariance and pinn_amd.compare_feature_groups is R.compare_feature_groups
    nine = np.concatenate([s] * 5)[:9]
    assert R.delong_covariance(y, nine, backend="host")["cov"].shape == (9, 9)
    with pytest.raises(NotImplementedError):
        R.delong_covariance(y, nine, backend="device")


def test_cross_sums_on_the_host(R):
    rng = np.random.default_rng(5)
    for lo, hi in ((1 << 31, 1 << 32), (1 << 39, 1 << 40), (0, 50)):
        comp = rng.integers(lo, hi, size=(3, 300), dtype=np.int64)
        P = R.component_cross_sums(comp, backend="host")
        for k in range(3):
            for l in range(3):
                assert P[k][l] == sum(int(x) * int(v) for x, v in zip(comp[k], comp[l]))


def test_limits_and_null_pointers_on_the_c_side():
    """Host-side checks of the three entry points: no GPU is needed, every call fails before a launch."""
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib, rocstat
    lib = _lib.load(build_if_missing=False)
    E_ARG, E_WS = -1, -3
    assert lib.pinn_abi_version() == 2
    assert (_lib.AUC_MAX_SCORES, _lib.AUC_TILE, _lib.AUC_BOOT_LDS_GROUPS, _lib.AUC_DRAW_BOOT) == (rocstat.MAX_SCORES, rocstat.SCAN_TILE,
                                                                                                rocstat.BOOT_LDS_GROUPS, rocstat.DRAW_BOOT)
    one, big = ctypes.c_void_p(0x1000), 1 << 40
    assert lib.pinn_auc_components_workspace_bytes(1000, 4) > 0
    for n, K in ((0, 1), (-1, 1), (10, 0), (10, 9), (1 << 31, 1)):
        assert lib.pinn_auc_components_workspace_bytes(n, K) == 0
        assert lib.pinn_auc_components(one, one, one, n, K, one, one, one, one, big, None) == E_ARG
    for hole in range(7):
        ptrs = [one] * 7
        ptrs[hole] = None
        assert lib.pinn_auc_components(ptrs[0], ptrs[1], ptrs[2], 1000, 4, ptrs[3], ptrs[4], ptrs[5], ptrs[6], big, None) == E_ARG, hole
    assert lib.pinn_auc_components(one, one, one, 1000, 4, one, one, one, one, lib.pinn_auc_components_workspace_bytes(1000, 4) - 1, None) == E_WS
    assert lib.pinn_auc_components(one, one, one, 1000, 4, one, one, ctypes.c_void_p(0x1002), one, big, None) == E_ARG    # alignment

    assert lib.pinn_auc_cross_sums_workspace_bytes(300, 3) > 0 and lib.pinn_auc_cross_sums_workspace_bytes(300, 9) == 0
    assert lib.pinn_auc_cross_sums_workspace_bytes(0, 3) == 0
    assert lib.pinn_auc_cross_sums(None, 300, 300, 3, one, one, big, None) == E_ARG
    assert lib.pinn_auc_cross_sums(one, 300, 300, 3, None, one, big, None) == E_ARG
    assert lib.pinn_auc_cross_sums(one, 300, 300, 3, one, None, big, None) == E_ARG
    assert lib.pinn_auc_cross_sums(one, 299, 300, 3, one, one, big, None) == E_ARG                   # rows beyond the leading dimension
    assert lib.pinn_auc_cross_sums(one, 300, 300, 9, one, one, big, None) == E_ARG
    assert lib.pinn_auc_cross_sums(one, 300, 300, 3, one, one, 16, None) == E_WS

    small, large = (ctypes.c_longlong * 2)(100, 12288), (ctypes.c_longlong * 2)(100, 12289)
    assert lib.pinn_auc_bootstrap_workspace_bytes(10, 2, small) == 0                                  # both histograms fit in LDS
    per = lib.pinn_auc_bootstrap_workspace_bytes(1, 2, large)
    assert per >= 12289 * 4 and lib.pinn_auc_bootstrap_workspace_bytes(10, 2, large) == 10 * per
    assert lib.pinn_auc_bootstrap_workspace_bytes(10, 9, large) == 0 and lib.pinn_auc_bootstrap_workspace_bytes(10, 2, None) == 0
    args = (10000, 10000, 2)
    assert lib.pinn_auc_bootstrap(None, one, *args, large, 1, 0, 10, one, one, big, None) == E_ARG
    assert lib.pinn_auc_bootstrap(one, None, *args, large, 1, 0, 10, one, one, big, None) == E_ARG
    assert lib.pinn_auc_bootstrap(one, one, *args, None, 1, 0, 10, one, one, big, None) == E_ARG
    assert lib.pinn_auc_bootstrap(one, one, *args, large, 1, 0, 10, None, one, big, None) == E_ARG
    assert lib.pinn_auc_bootstrap(one, one, *args, large, 1, 0, 10, one, None, big, None) == E_ARG     # a workspace is needed here
    assert lib.pinn_auc_bootstrap(one, one, *args, large, 1, 0, 10, one, one, 10 * per - 1, None) == E_WS
    assert lib.pinn_auc_bootstrap(one, one, *args, large, 1, 0, 0, one, one, big, None) == E_ARG
    assert lib.pinn_auc_bootstrap(one, one, *args, large, 1, (1 << 32) - 5, 10, one, one, big, None) == E_ARG
    assert lib.pinn_auc_bootstrap(one, one, 0, 10000, 2, large, 1, 0, 10, one, one, big, None) == E_ARG
    assert lib.pinn_auc_bootstrap(one, one, 100, 100, 2, large, 1, 0, 10, one, one, big, None) == E_ARG  # more groups than rows
