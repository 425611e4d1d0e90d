"""CPU: pinn_amd.anomaly (the isolation forest of reference script 02) on its host backend against tests/golden/g_iforest.npz
(scikit-learn 1.7.2's trees and scores, tools/make_golden_iforest.py), and the shared checks tests/test_gpu_anomaly.py runs on
the device.

Gates (none comes from what the code under test gives).  A given forest: depth sums bit-equal between the
backends and the numpy reading of the device block; host scores bit-equal to the fixture (the same numpy expressions),
device scores within 4 units in the last place (two for each side's power function); predictions equal wherever
|decision| > 1e-15; the ROC curve equal (rates are quotients of the same integers, the generator holds the scores of the two
classes at least 1e-12 apart) and the area within len(fpr) 2^-50 of scikit-learn's trapezoid sum (its rounding, as in
test_detection_host).  Own fit: host and device trees and subsamples bit-equal; the invariants of an isolation tree; the mean
depth per tree statistically indistinguishable from scikit-learn's over 16 seeds x 200 trees and 200 probe rows.
Every comparison prints its figures before it asserts."""
import warnings

import numpy as np
import pytest

TRAIN_ROWS, DIMS, TREES = (1, 2, 3, 255, 256, 257, 1000), (1, 2, 8), (1, 3, 200)
SCORE_ROWS = (1, 63, 64, 65, 257, 4099)
# every listed size of every axis: the full cross at 1 and 3 trees; 200 trees where the subsample is 1, below, at and above a
# wave, at max_samples_ = 256 and past it, with every D
FIT_CASES = [(n, D, T) for n in TRAIN_ROWS for D in DIMS for T in (1, 3)] + [(1, 1, 200), (3, 2, 200), (255, 8, 200), (256, 2, 200),
                                                                              (257, 1, 200), (1000, 8, 200), (2, 8, 200)]
K_SIGMA = 4.5          # fixed before any run (the issue's figure): 200 rows x 2 (1 - Phi(4.5)) = 1.4e-3 family-wise under a normal
                       # law; with the standard error taken from 2 x 16 seeds (Student, 30 degrees) about 2e-2: the gate is
                       # stricter than the 1e-3 asked for, and the seeds are fixed, so it cannot flicker


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


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def ulps(a, b):
    """Distance in units of the last place between float64 arrays of one sign."""
    a, b = np.ascontiguousarray(host(a), dtype=np.float64), np.ascontiguousarray(host(b), dtype=np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


def fixture_trees(G, tag):
    o = G[tag + "_offsets"]
    return [tuple(G[tag + "_" + k][o[i]:o[i + 1]] for k in ("feature", "threshold", "left", "right", "n_node")) for i in range(len(o) - 1)]


def fixture_forest(G, A, tag, backend):
    return A.DeviceIsolationForest.from_arrays(fixture_trees(G, tag), int(G[tag + "_max_samples"]), float(G[tag + "_offset"]), n_features=2,
                                               backend=backend)


def results_array(G):
    a = np.zeros((G["results_cols"].shape[0], 22))
    a[:, G["col_ids"]] = G["results_cols"].astype(np.float64)
    return a


def held_out_rows(G):
    return G["kept"].astype(np.int64)[G["idx_te"].astype(np.int64)]


def apply_tree(tree, X32):
    """Leaf of every float32 row, by the float64 comparison (independent of the package)."""
    feature, threshold, left, right, _ = tree
    node = np.zeros(len(X32), dtype=np.int64)
    for i in range(len(X32)):
        k = 0
        while feature[k] >= 0:
            k = left[k] if float(X32[i, feature[k]]) <= threshold[k] else right[k]
        node[i] = k
    return node


def draw_rows(n, D, seed, constant_col=True):
    """n rows, D features: a bulk, a few outliers, some duplicated rows, and (D = 8) one constant column."""
    rng = np.random.default_rng([seed, n, D])
    X = rng.normal(size=(n, D)) * np.linspace(1.0, 0.2, D)
    X[rng.random(n) < 0.05] *= 4.0
    if n >= 8:
        X[n // 2:n // 2 + 3] = X[0]
    if D == 8 and constant_col:
        X[:, 3] = 0.75
    return X


# ---------------------------------------------------------------------------------------------- shared checks
def check_fixture(G, A, T, backend, wrap=None):
    arr = results_array(G)
    data = wrap(arr) if wrap else arr
    cols, rows = [int(c) for c in G["cols"]], held_out_rows(G)
    for tag in ("a", "b"):
        f = fixture_forest(G, A, tag, backend)
        ref = fixture_forest(G, A, tag, "host")
        sums, want = host(f.depth_sums(data, columns=cols, row_index=rows)), ref.depth_sums(arr, columns=cols, row_index=rows)
        block = A.block_depth_sums(f._block, arr[rows][:, cols])
        s = host(f.score_samples(data, columns=cols, row_index=rows))
        d = host(f.decision_function(data, columns=cols, row_index=rows))
        p = host(f.predict(data, columns=cols, row_index=rows))
        u = int(ulps(s, G[tag + "_score"]).max())
        sure = np.abs(G[tag + "_decision"]) > 1e-15
        print("forest %s on %s: %d trees, block %d bytes, depth sums equal the host's: %s, the block's reading: %s, scores within %d ulp of "
              "scikit-learn's (gate %d), %d of %d rows with |decision| > 1e-15" % (tag, backend, len(f.trees_), f._block.nbytes, sums.tobytes() ==
              want.tobytes(), block.tobytes() == want.tobytes(), u, 0 if backend == "host" else 4, sure.sum(), sure.size))
        assert sums.tobytes() == want.tobytes() and block.tobytes() == want.tobytes()
        assert u <= (0 if backend == "host" else 4)
        assert int(ulps(d, s - float(G[tag + "_offset"])).max()) == 0
        assert np.array_equal(p[sure], G[tag + "_pred"].astype(np.int64)[sure]) and set(np.unique(p)) <= {-1, 1}
        assert f.max_samples_ == int(G[tag + "_max_samples"]) and f.offset_ == float(G[tag + "_offset"]) and f.n_features_in_ == 2
        if tag == "a":
            truth = G["truth"].astype(np.int64)
            score = -f.score_samples(data, columns=cols, row_index=rows)
            area = T.auc_score(wrap(truth) if wrap else truth, score, pos_label=1, backend=backend)
            exact = T.auc_score(truth, -G["a_score"], pos_label=1, backend="host")
            fpr, tpr, thr = T.roc_curve(wrap(truth) if wrap else truth, score, pos_label=1, backend=backend)
            bound = len(G["a_fpr"]) * 2.0 ** -50
            print("  AUC %.15f, from the fixture's scores %.15f, scikit-learn's trapezoid sum %.15f (difference %.3e, gate %.3e)"
                  % (area, exact, float(G["a_auc"]), abs(area - float(G["a_auc"])), bound))
            assert area == exact and abs(area - float(G["a_auc"])) <= bound
            assert np.array_equal(host(fpr), G["a_fpr"]) and np.array_equal(host(tpr), G["a_tpr"])
            assert int(ulps(host(thr)[1:], G["a_thr"][1:]).max()) <= (0 if backend == "host" else 4)


def check_threshold_edges(G, A, backend, wrap=None):
    """Rows whose float32 value is floor32(threshold) of a node, and the next float32 above it: the decisions of the packed
    float32 thresholds must be those of the float64 comparison."""
    for tag in ("a", "b"):
        f, ref = fixture_forest(G, A, tag, backend), fixture_forest(G, A, tag, "host")
        rng = np.random.default_rng(7)
        base = results_array(G)[held_out_rows(G)][:, [int(c) for c in G["cols"]]]
        rows = []
        for tree in ref.trees_[:40]:
            inner = np.flatnonzero(tree[0] >= 0)
            for k in rng.choice(inner, size=min(6, inner.size), replace=False):
                t32 = A.floor32(tree[1][k])
                for v in (t32, np.nextafter(t32, np.float32(np.inf)), np.nextafter(t32, np.float32(-np.inf))):
                    r = base[rng.integers(len(base))].copy()
                    r[tree[0][k]] = float(v)
                    rows.append(r)
                assert float(t32) <= tree[1][k] < float(np.nextafter(t32, np.float32(np.inf)))
        X = np.array(rows)
        got = host(f.depth_sums(wrap(X) if wrap else X))
        want = ref.depth_sums(X)
        block = A.block_depth_sums(ref._block, X)
        print("threshold edges, forest %s on %s: %d rows on or next to a float32 threshold, sums equal: %s, the block's reading: %s"
              % (tag, backend, len(X), got.tobytes() == want.tobytes(), block.tobytes() == want.tobytes()))
        assert got.tobytes() == want.tobytes() and block.tobytes() == want.tobytes()


def check_invariants(A, forest, X):
    """The invariants of an isolation tree, for every tree of a fitted forest and its own subsample."""
    m, n = forest.max_samples_, X.shape[0]
    limit = A.max_depth_of(m)
    assert limit == int(np.ceil(np.log2(max(m, 2))))
    assert forest.samples_.shape == (len(forest.trees_), m) and forest.samples_.dtype == np.int64
    for tree, pos in zip(forest.trees_, forest.samples_):
        feature, threshold, left, right, n_node = tree
        assert np.unique(pos).size == m and pos.min() >= 0 and pos.max() < n
        inner = feature >= 0
        assert n_node[0] == m and np.array_equal(n_node[inner], n_node[left[inner]] + n_node[right[inner]])
        assert np.array_equal(left[inner], np.flatnonzero(inner) + 1)                       # pre-order
        assert np.all(feature[~inner] == -2) and np.all(threshold[~inner] == -2.0) and np.all(left[~inner] == -1) and np.all(right[~inner] == -1)
        depth = A.tree_depths(left, right)
        assert depth.max() <= limit
        Xs = X[pos].astype(np.float32)
        leaf = apply_tree(tree, Xs)
        assert np.array_equal(np.bincount(leaf, minlength=len(feature))[~inner], n_node[~inner])
        for k in np.flatnonzero(~inner & (n_node > 1) & (depth < limit)):
            assert np.all(Xs[leaf == k] == Xs[leaf == k][0])
        for k in np.flatnonzero(inner):                                                     # never a feature that is constant on the node
            col = Xs[np.isin(leaf, subtree_leaves(tree, k)), feature[k]]
            assert col.min() <= threshold[k] < col.max()


def subtree_leaves(tree, k):
    out, stack = [], [k]
    while stack:
        v = stack.pop()
        if tree[0][v] < 0:
            out.append(v)
        else:
            stack += [tree[2][v], tree[3][v]]
    return out


def same_forest(f, g):
    return (len(f.trees_) == len(g.trees_) and all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for s, t in zip(f.trees_, g.trees_)
                                                  for a, b in zip(s, t)) and f.samples_.tobytes() == g.samples_.tobytes())


def check_own_fit(A, backend, n, D, T, wrap=None):
    X = draw_rows(n, D, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = A.DeviceIsolationForest(T, random_state=11, backend=backend).fit(wrap(X) if wrap else X)
        ref = f if backend == "host" else A.DeviceIsolationForest(T, random_state=11, backend="host").fit(X)
    assert f.max_samples_ == min(256, n) and f.offset_ == -0.5 and f.n_features_in_ == D and len(f.trees_) == T
    assert same_forest(f, ref), "host and device trees differ"
    if T <= 3 or backend == "host":
        check_invariants(A, f, X)
    if D == 8:
        assert all(not np.any(t[0] == 3) for t in f.trees_), "a constant column was chosen"
    return f, X


def check_scoring_shapes(A, backend, wrap=None):
    X = draw_rows(700, 4, 5)
    f = A.DeviceIsolationForest(50, random_state=2, backend=backend).fit(wrap(X) if wrap else X)
    ref = A.DeviceIsolationForest(50, random_state=2, backend="host").fit(X)
    assert same_forest(f, ref)
    big = draw_rows(max(SCORE_ROWS), 4, 6)
    whole = ref.depth_sums(big)
    for n in SCORE_ROWS:
        got = host(f.depth_sums(wrap(big[:n]) if wrap else big[:n]))
        assert got.tobytes() == whole[:n].tobytes(), n
        s = host(f.score_samples(wrap(big[:n]) if wrap else big[:n]))
        assert int(ulps(s, ref.score_samples(big[:n])).max()) <= (0 if backend == "host" else 4)
    # chunked scoring equals whole scoring, bit for bit on one backend
    full = host(f.score_samples(wrap(big) if wrap else big))
    parts = np.concatenate([host(f.score_samples(wrap(big[i:i + 1000]) if wrap else big[i:i + 1000])) for i in range(0, len(big), 1000)])
    assert parts.tobytes() == full.tobytes()
    # rows read in place from a [n, 22] array with a gather list equal the packed copy
    arr = np.zeros((len(big), 22))
    cols = [11, 12, 3, 5]
    arr[:, cols] = big
    idx = np.random.default_rng(0).permutation(len(big))[:3000]
    a = host(f.score_samples(wrap(arr) if wrap else arr, columns=cols, row_index=wrap(idx) if wrap else idx))
    b = host(f.score_samples(wrap(big[idx]) if wrap else big[idx]))
    pa = host(f.predict(wrap(arr) if wrap else arr, columns=cols, row_index=wrap(idx) if wrap else idx))
    assert a.tobytes() == b.tobytes() and np.array_equal(pa, np.where(a - f.offset_ >= 0, 1, -1))
    return f


def check_edge_cases(A, backend, wrap=None):
    w = wrap if wrap else (lambda v: v)
    # identical training rows: one leaf per tree, every score -0.5
    same = np.tile(np.array([[0.3, -1.2, 5.0]]), (300, 1))
    f = A.DeviceIsolationForest(20, random_state=1, backend=backend).fit(w(same))
    assert all(len(t[0]) == 1 and t[4][0] == 256 for t in f.trees_)
    probe = np.concatenate([same[:5], np.random.default_rng(1).normal(size=(70, 3))])
    assert np.all(host(f.score_samples(w(probe))) == -0.5) and np.all(host(f.predict(w(probe))) == 1)
    # one training row: depth 0 and c(1) = 0, scikit-learn's exponent -1
    one = A.DeviceIsolationForest(3, random_state=1, backend=backend).fit(w(same[:1]))
    assert one.max_samples_ == 1 and np.all(host(one.score_samples(w(probe))) == -0.5)
    # a gather index outside the array and a row that is not finite score NaN and predict -1
    X = draw_rows(400, 2, 9)
    f = A.DeviceIsolationForest(10, random_state=4, backend=backend).fit(w(X))
    idx = np.array([0, 5, 400, -1, 399, 1 << 40])
    s = host(f.score_samples(w(X), row_index=w(idx)))
    assert np.array_equal(np.isnan(s), [False, False, True, True, False, True])
    assert np.array_equal(host(f.predict(w(X), row_index=w(idx)))[[2, 3, 5]], [-1, -1, -1])
    bad = X[:6].copy()
    bad[1, 0], bad[3, 1], bad[4, 0] = np.nan, np.inf, 1e300              # 1e300 is infinite as a float32
    s = host(f.score_samples(w(bad)))
    assert np.array_equal(np.isnan(s), [False, True, False, True, True, False]) and np.all(np.isnan(host(f.depth_sums(w(bad)))) == np.isnan(s))
    with pytest.raises(ValueError):
        A.DeviceIsolationForest(5, max_samples=6, random_state=4, backend=backend).fit(w(bad))
    # contamination as a number: the percentile of the training scores, on the host
    c = A.DeviceIsolationForest(30, contamination=0.1, random_state=4, backend=backend).fit(w(X))
    assert c.offset_ == float(np.percentile(host(c.score_samples(w(X))), 10.0)) and abs(np.mean(host(c.predict(w(X))) == -1) - 0.1) < 0.02
    assert np.array_equal(host(c.fit_predict(w(X))), host(c.predict(w(X))))
    # sizes beyond the limits
    for make in (lambda: A.DeviceIsolationForest(1025, backend=backend).fit(w(X)),
                 lambda: A.DeviceIsolationForest(5, max_samples=1025, backend=backend).fit(w(draw_rows(1100, 2, 1))),
                 lambda: A.DeviceIsolationForest(5, backend=backend).fit(w(draw_rows(50, 9, 1))),
                 lambda: A.DeviceIsolationForest(5, max_features=0.5), lambda: A.DeviceIsolationForest(5, bootstrap=True)):
        with pytest.raises(NotImplementedError):
            make()
    deep = (np.r_[np.zeros(1024, dtype=np.int64), np.full(1025, -2)], np.r_[np.arange(1024.0), np.full(1025, -2.0)],
            np.r_[2 * np.arange(1024) + 1, np.full(1025, -1)], np.r_[2 * np.arange(1024) + 2, np.full(1025, -1)], np.ones(2049, dtype=np.int64))
    with pytest.raises(NotImplementedError):
        A.DeviceIsolationForest.from_arrays([deep], 256)


def check_determinism(A, backend, wrap=None):
    w = wrap if wrap else (lambda v: v)
    X = draw_rows(600, 3, 12)
    f1 = A.DeviceIsolationForest(12, random_state=5, backend=backend).fit(w(X))
    f2 = A.DeviceIsolationForest(12, random_state=5, backend=backend).fit(w(X))
    f3 = A.DeviceIsolationForest(12, random_state=6, backend=backend).fit(w(X))
    f4 = A.DeviceIsolationForest(5, random_state=5, backend=backend).fit(w(X))
    assert same_forest(f1, f2) and not same_forest(f1, f3)
    assert f1.samples_[:5].tobytes() == f4.samples_.tobytes() and all(a.tobytes() == b.tobytes() for s, t in zip(f1.trees_[:5], f4.trees_)
                                                                      for a, b in zip(s, t))
    assert not np.array_equal(f1.samples_[0], f1.samples_[1])


def same_result(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a:
        if k == "clf":
            assert host(a[k].named_steps["logreg"].coef_).tobytes() == host(b[k].named_steps["logreg"].coef_).tobytes()
        elif k == "metrics":
            assert all(np.array_equal(a[k][m], b[k][m]) for m in a[k])
        elif isinstance(a[k], (str, list, int, float)):
            assert a[k] == b[k], k
        else:
            assert host(a[k]).tobytes() == host(b[k]).tobytes(), k


def check_evaluate(G, A, T, backend, wrap=None):
    arr = results_array(G)
    data = wrap(arr) if wrap else arr
    split = (G["idx_tr"].astype(np.int64), G["idx_te"].astype(np.int64))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = T.evaluate_feature_groups(data, feature_groups=(T.FEAT_GRP1, T.FEAT_GRP3), split=split, backend=backend)
        off = T.evaluate_feature_groups(data, feature_groups=(T.FEAT_GRP1, T.FEAT_GRP3), split=split, backend=backend, unsupervised=False)
        given = T.evaluate_feature_groups(data, feature_groups=(T.FEAT_GRP1, T.FEAT_GRP3), split=split, backend=backend,
                                          unsupervised=fixture_forest(G, A, "a", backend))
        own = T.evaluate_feature_groups(data, feature_groups=(T.FEAT_GRP1, T.FEAT_GRP3), split=split, backend=backend, unsupervised=True,
                                        random_state=42)
    for a, b in zip(plain, off):
        same_result(a, b)
    new = {"auc_unsup", "fpr_unsup", "tpr_unsup", "thresholds_unsup", "anomaly_score", "iforest"}
    for res in (given, own):
        assert set(res[0]) - set(plain[0]) == new and set(res[1]) == set(plain[1])
        same_result({k: v for k, v in res[0].items() if k not in new}, plain[0])
    g = given[0]
    bound = len(G["a_fpr"]) * 2.0 ** -50
    print("evaluate_feature_groups on %s: auc_unsup %.15f with the fixture's forest (scikit-learn %.15f, gate %.3e), %.6f with the own fit"
          % (backend, g["auc_unsup"], float(G["a_auc"]), bound, own[0]["auc_unsup"]))
    assert abs(g["auc_unsup"] - float(G["a_auc"])) <= bound
    assert np.array_equal(host(g["fpr_unsup"]), G["a_fpr"]) and np.array_equal(host(g["tpr_unsup"]), G["a_tpr"])
    assert int(ulps(host(g["anomaly_score"]), -G["a_score"]).max()) <= (0 if backend == "host" else 4)
    o = own[0]
    assert 0.5 < o["auc_unsup"] < 1.0 and len(o["iforest"].trees_) == 200 and o["iforest"].max_samples_ == int(G["n_fit"])
    assert np.array_equal(np.sort(np.unique(o["iforest"].samples_)), np.arange(int(G["n_fit"])))
    return own


def check_monitor(G, A, backend, wrap=None):
    arr = results_array(G)
    arr = arr[np.isfinite(arr[:, 12])]
    f = fixture_forest(G, A, "a", backend)
    whole = A.AnomalyMonitor(f, backend=backend).update(wrap(arr) if wrap else arr)
    mon = A.AnomalyMonitor(f, features=[11, 12], backend=backend)
    parts = [mon.update(wrap(arr[i:i + 333]) if wrap else arr[i:i + 333]) for i in range(0, len(arr), 333)]
    assert mon.n_seen == len(arr) and mon.columns == [11, 12]
    assert np.concatenate([host(p[0]) for p in parts]).tobytes() == host(whole[0]).tobytes()
    assert np.array_equal(np.concatenate([host(p[1]) for p in parts]), host(whole[1]))
    assert np.array_equal(host(whole[0]), -host(f.score_samples(wrap(arr) if wrap else arr, columns=[11, 12])))


# ---------------------------------------------------------------------------------------------- host tests
def test_restated_arithmetic(A):
    n = np.array([0, 1, 2, 3, 79, 256, 1000])
    c = A.average_path_length(n)
    assert c[0] == c[1] == 0.0 and c[2] == 1.0 and c[3] == 2.0 * (np.log(2.0) + np.euler_gamma) - 2.0 * 2.0 / 3.0
    assert [A.max_depth_of(m) for m in (1, 2, 3, 4, 5, 79, 255, 256, 257, 1000, 1024)] == [1, 1, 2, 2, 3, 7, 8, 8, 9, 10, 10]
    rng = np.random.default_rng(0)
    t = np.concatenate([rng.normal(size=2000), rng.normal(size=2000).astype(np.float32).astype(np.float64), [0.0, -0.0, 1e300, -1e300, 1e-60]])
    f = A.floor32(t)
    with np.errstate(over="ignore"):
        up = np.nextafter(f, np.float32(np.inf))
    assert f.dtype == np.float32 and np.all(f.astype(np.float64) <= t) and np.all((up.astype(np.float64) > t) | np.isinf(f))
    # Philox4x32-10: the known-answer vectors of the Random123 distribution
    assert [int(v) for v in A.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(v) for v in A.philox4x32_10(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)] == \
        [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    for n_pos, m in ((1, 1), (2, 2), (3, 3), (5, 4), (700, 256), (70000, 1024)):
        p = A.subsample_positions(9, 4, m, n_pos)
        assert np.unique(p).size == m and p.min() >= 0 and p.max() < n_pos
    full = np.stack([A.subsample_positions(9, t, 64, 64) for t in range(50)])
    assert all(np.array_equal(np.sort(r), np.arange(64)) for r in full) and len({r.tobytes() for r in full}) == 50


def test_fixture_forest_on_host(G, A, T):
    check_fixture(G, A, T, "host")
    a = fixture_forest(G, A, "a", "host")
    assert int(G["b_max_depth"]) == 10 and max(A.tree_depths(t[2], t[3]).max() for t in fixture_forest(G, A, "b", "host").trees_) == 10
    hdr = a._block[:16].view(np.int64)
    assert hdr[0] == 0x49464f52 and hdr[1] == 200 and hdr[3] == 2 and hdr[5] == int(G["a_offsets"][-1])
    assert a._block.nbytes == 8 * (16 + 16384 + 2 * 513 + int(hdr[5])) and hdr[2] == np.diff(G["a_offsets"]).max()


def test_threshold_edges_on_host(G, A):
    check_threshold_edges(G, A, "host")


def test_from_sklearn_fresh_fit(A):
    ens = pytest.importorskip("sklearn.ensemble")
    rng = np.random.default_rng(77)
    X, Xt = rng.normal(size=(900, 3)), rng.normal(size=(500, 3)) * 2.0
    for kw in ({"n_estimators": 60}, {"n_estimators": 5, "max_samples": 700}, {"n_estimators": 20, "contamination": 0.05}):
        est = ens.IsolationForest(random_state=int(rng.integers(1 << 30)), **kw).fit(X)
        f = A.DeviceIsolationForest.from_sklearn(est, backend="host")
        assert f.score_samples(Xt).tobytes() == est.score_samples(Xt).tobytes() and np.array_equal(f.predict(Xt), est.predict(Xt))
        assert f.decision_function(Xt).tobytes() == est.decision_function(Xt).tobytes()
        assert A.block_depth_sums(f._block, Xt).tobytes() == f.depth_sums(Xt).tobytes()


@pytest.mark.parametrize("n,D,n_trees", FIT_CASES)
def test_own_fit_invariants(A, n, D, n_trees):
    check_own_fit(A, "host", n, D, n_trees)


def test_own_fit_covers_every_listed_size():
    assert {c[0] for c in FIT_CASES} == set(TRAIN_ROWS) and {c[1] for c in FIT_CASES} == set(DIMS) and {c[2] for c in FIT_CASES} == set(TREES)
    assert {c[0] for c in FIT_CASES if c[2] == 200} >= {1, 255, 256, 257, 1000} and {c[1] for c in FIT_CASES if c[2] == 200} == set(DIMS)


def test_scoring_shapes_on_host(A):
    check_scoring_shapes(A, "host")


def test_edge_cases_on_host(A):
    check_edge_cases(A, "host")


def test_determinism_on_host(A):
    check_determinism(A, "host")


def test_max_samples_as_in_scikit_learn(A):
    X = draw_rows(500, 2, 1)
    assert A.DeviceIsolationForest(2, max_samples=100, random_state=0, backend="host").fit(X).max_samples_ == 100
    assert A.DeviceIsolationForest(2, max_samples=0.5, random_state=0, backend="host").fit(X).max_samples_ == 250
    with pytest.warns(UserWarning):
        assert A.DeviceIsolationForest(2, max_samples=900, random_state=0, backend="host").fit(X).max_samples_ == 500
    assert A.DeviceIsolationForest(2, random_state=0, backend="host").fit(X[:100]).max_samples_ == 100
    with pytest.raises(RuntimeError):
        A.DeviceIsolationForest(2).score_samples(X)
    import pinn_amd
    assert pinn_amd.DeviceIsolationForest is A.DeviceIsolationForest and pinn_amd.AnomalyMonitor is A.AnomalyMonitor


def test_own_fit_against_scikit_learns_distribution(A):
    """Mean depth per tree at 200 probe rows, 16 seeds x 200 trees a side: |difference| <= K_SIGMA standard errors at every row.
    scikit-learn against scikit-learn on disjoint seeds runs first and must pass, or the inputs are wrong.
    Measured with scikit-learn 1.7.2: worst ratio 2.16 scikit-learn against itself, 2.56 and 2.60 own fit against its two sets."""
    ens = pytest.importorskip("sklearn.ensemble")
    rng = np.random.default_rng(20260)
    X = np.concatenate([rng.normal(size=(600, 2)) * [1.0, 0.5], rng.normal(size=(100, 2)) * 0.3 + [2.0, 1.0]])
    probe = np.concatenate([rng.normal(size=(100, 2)) * [1.0, 0.5], rng.uniform(-5, 5, size=(100, 2))])
    S = 16

    def sk(seed):
        est = ens.IsolationForest(n_estimators=200, random_state=seed).fit(X)
        return A.DeviceIsolationForest.from_sklearn(est, backend="host").depth_sums(probe) / 200

    def own(seed):
        return A.DeviceIsolationForest(200, random_state=seed, backend="host").fit(X).depth_sums(probe) / 200

    def worst(a, b):
        se = np.sqrt(a.var(axis=0, ddof=1) / len(a) + b.var(axis=0, ddof=1) / len(b))
        return float(np.max(np.abs(a.mean(axis=0) - b.mean(axis=0)) / se))
    sk1, sk2 = np.stack([sk(s) for s in range(S)]), np.stack([sk(1000 + s) for s in range(S)])
    r0 = worst(sk1, sk2)
    print("scikit-learn against scikit-learn: worst ratio %.3f (gate %.1f)" % (r0, K_SIGMA))
    assert r0 <= K_SIGMA, "the inputs of the test are wrong, not the gate"
    mine = np.stack([own(s) for s in range(S)])
    r1, r2 = worst(mine, sk1), worst(mine, sk2)
    print("own fit against scikit-learn: worst ratios %.3f and %.3f (gate %.1f)" % (r1, r2, K_SIGMA))
    assert r1 <= K_SIGMA and r2 <= K_SIGMA


def test_evaluate_feature_groups_on_host(G, A, T):
    check_evaluate(G, A, T, "host")


def test_monitor_on_host(G, A):
    check_monitor(G, A, "host")
