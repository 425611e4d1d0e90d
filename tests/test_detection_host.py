"""CPU: pinn_amd.detection (reference script 02) on its host backend against tests/golden/g_lr.npz, which
tools/make_golden_lr.py recorded from the reference's own functions and scikit-learn 1.7.2 at two tolerances.

Gates (from the reference or the arithmetic, none from what the code gives): scaler sums within 1e-12 x the sum of
their absolute terms, counts exact; predict_proba / decision_function with the reference's parameters atol 1e-12; a fit at
the default tol has max |grad F| / sum sw <= 1e-4 by the test's own numpy; a fit at tol = 1e-12 lies within 0.1 dc / 0.1 dp
of the reference at tol = 1e-13 (dc, dp: how far the reference at its defaults is from that), predicts the same class outside
the rows the fixture calls close, and its AUC is within q / (P N); ROC arrays bit-equal.  The check functions take the
backend, so tests/test_gpu_detection.py runs the same gates on the device.  Every comparison prints its maxima first."""
import ctypes
import warnings

import numpy as np
import pytest

CASES = ["b1", "b2", "b3", "b4", "f1", "f2", "f3", "f4"]
BINARY = "normal:0 | fault:1,2,3,4,5,6,7,8,9,10,11,12"
FIVE = "正常:0 | 水淹:1,2,3 | 氧饥饿:4,5,6 | 膜干:7,8,9 | 氢饥饿:10,11,12"


@pytest.fixture(scope="module")
def G(golden):
    return golden("g_lr.npz")


@pytest.fixture(scope="module")
def T():
    from pinn_amd import detection
    return detection


class Case:
    """One fixture case: the results array, the rows and classes of its split, the reference's numbers."""

    def __init__(self, G, T, name):
        self.name = name
        self.g = {k[len(name) + 1:]: v for k, v in G.items() if k.startswith(name + "_")}
        twin = name[0] + str(int(name[1]) - 2) if int(name[1]) > 2 else name
        self.idx_tr, self.idx_te = G[twin + "_idx_tr"].astype(np.int64), G[twin + "_idx_te"].astype(np.int64)
        n = G["results_cols"].shape[0]
        self.results = np.zeros((n, 22))
        self.results[:, G["col_ids"]] = G["results_cols"].astype(np.float64)
        self.cols = [int(c) for c in self.g["cols"]]
        self.kept = np.setdiff1d(np.arange(n), self.g["dropped"])
        self.spec = BINARY if name[0] == "b" else FIVE
        self.label_map, self.names = T.build_label_mapper(T.parse_group_spec(self.spec))
        self.C = len(self.names)
        det = self.results[self.kept, 17].astype(np.int64)
        self.y = np.array([self.label_map[int(d)] for d in det])
        self.rows_tr, self.rows_te = self.kept[self.idx_tr], self.kept[self.idx_te]
        self.y_tr, self.y_te = self.y[self.idx_tr], self.y[self.idx_te]
        self.truth = (self.y_te != 0).astype(np.int64)
        self.delta = 0.1 * float(self.g["dp"])


def full_params(coef, intercept):
    """[C, D] and [C] of scikit-learn's shapes (two classes: one row, W = (-coef, +coef))."""
    coef, intercept = np.asarray(coef), np.asarray(intercept).reshape(-1)
    return (np.concatenate([-coef, coef]), np.concatenate([-intercept, intercept])) if coef.shape[0] == 1 else (coef, intercept)


def np_objective(X, y, C, mean, scale, coef, intercept, balanced=True):
    """The test's own F, max |grad F| / sum sw, and per gradient entry the sum of the absolute terms / sum sw."""
    W, b = full_params(coef, intercept)
    Z = (X - mean) / scale
    count = np.bincount(y, minlength=C)
    sw = (len(y) / (C * count))[y] if balanced else np.ones(len(y))
    s = Z @ W.T + b
    m = s.max(axis=1, keepdims=True)
    lse = np.log(np.exp(s - m).sum(axis=1)) + m[:, 0]
    p = np.exp(s - lse[:, None])
    F = (sw * (lse - s[np.arange(len(y)), y])).sum() + 0.5 * (W ** 2).sum()
    R = p.copy()
    R[np.arange(len(y)), y] -= 1.0
    R *= sw[:, None]
    gW, gb = R.T @ Z + W, R.sum(axis=0)
    aW, ab = np.abs(R).T @ np.abs(Z) + np.abs(W), np.abs(R).sum(axis=0)
    return F, max(np.abs(gW).max(), np.abs(gb).max()) / sw.sum(), max(aW.max(), ab.max()) / sw.sum()


def set_params(T, clf, case, tag, backend):
    """The pipeline with the reference's scaler and coefficients copied in."""
    g = case.g
    sc, lr = clf.named_steps["scaler"], clf.named_steps["logreg"]
    sc._set(g["mean"].copy(), g["var"].copy(), g["scale"].copy(), len(case.idx_tr))
    lr.coef_, lr.intercept_, lr.classes_, lr.n_features_in_ = g[tag + "_coef"].copy(), g[tag + "_intercept"].copy(), np.arange(case.C), len(case.cols)
    lr._model = None
    return clf


def reference_roc(truth, score):
    """scikit-learn's roc_curve rules written out group by group: (fps, tps, thresholds) with the origin, after drop_intermediate."""
    order = np.argsort(score, kind="mergesort")[::-1]       # scikit-learn's order: equal scores in reverse input order
    s, t = score[order], truth[order]
    fps, tps, thr, tp, fp = [], [], [], 0, 0
    for i in range(len(s)):
        tp += int(t[i])
        fp += 1 - int(t[i])
        if i == len(s) - 1 or s[i] != s[i + 1]:
            fps.append(fp), tps.append(tp), thr.append(s[i])
    if len(fps) > 2:
        keep = [0] + [k for k in range(1, len(fps) - 1) if fps[k + 1] - 2 * fps[k] + fps[k - 1] or tps[k + 1] - 2 * tps[k] + tps[k - 1]] + [len(fps) - 1]
        fps, tps, thr = [fps[k] for k in keep], [tps[k] for k in keep], [thr[k] for k in keep]
    return np.array([0] + fps), np.array([0] + tps), np.array([np.inf] + thr)


def exact_auc(truth, score):
    """U2 / (2 P N) from Python integers: U2 = 2 #(positive above negative) + #(equal pairs); the nearest float64."""
    pos, neg = np.sort(score[truth == 1]), np.sort(score[truth == 0])
    below = np.searchsorted(neg, pos, side="left")
    equal = np.searchsorted(neg, pos, side="right") - below
    U2 = 2 * int(below.sum()) + int(equal.sum())
    return U2 / (2 * len(pos) * len(neg)), U2


# ------------------------------------------------------------------------------------------------ shared checks
def check_scaler(G, T, name, backend, wrap=lambda a: a):
    c = Case(G, T, name)
    X = c.results[c.rows_tr][:, c.cols]
    sc = T.DeviceStandardScaler(backend=backend).fit(wrap(c.results), columns=c.cols, row_index=wrap(c.rows_tr))
    mean, var, scale = (np.asarray(T._as_numpy(a)) for a in (sc.mean_, sc.var_, sc.scale_))
    n = len(c.rows_tr)
    e_m = np.abs(mean - c.g["mean"]) * n / np.abs(X).sum(axis=0)
    e_v = np.abs(var - c.g["var"]) * n / ((X - c.g["mean"]) ** 2).sum(axis=0)
    print("%s %s scaler: mean %.3e var %.3e of the sums of absolute terms (gate 1e-12), scale %.3e" %
          (name, backend, e_m.max(), e_v.max(), np.abs(scale / c.g["scale"] - 1).max()))
    assert sc.n_samples_seen_ == n and e_m.max() <= 1e-12 and e_v.max() <= 1e-12 and np.abs(scale / c.g["scale"] - 1).max() <= 1e-12


def check_reference_parameters(G, T, name, backend, wrap=lambda a: a):
    c = Case(G, T, name)
    for tag in ("t", "d"):
        clf = set_params(T, T.build_classifier(balanced=True, backend=backend), c, tag, backend)
        kw = dict(columns=c.cols, row_index=wrap(c.rows_te))
        proba, pred = T._as_numpy(clf.predict_proba(wrap(c.results), **kw)), T._as_numpy(clf.predict(wrap(c.results), **kw))
        if tag == "t":
            e = np.abs(proba - c.g["t_proba"]).max()
            top = np.sort(c.g["t_proba"], axis=1)
            sure = top[:, -1] - top[:, -2] >= 2 * c.delta
            print("%s %s tight parameters: predict_proba %.3e (gate 1e-12), predict differs on %d of %d sure rows" %
                  (name, backend, e, (pred != c.g["t_pred"])[sure].sum(), sure.sum()))
            assert e <= 1e-12 and np.array_equal(pred[sure], c.g["t_pred"][sure])
            if "t_decision" in c.g:
                e = np.abs(T._as_numpy(clf.decision_function(wrap(c.results), **kw)) - c.g["t_decision"]).max()
                print("   decision_function %.3e (gate 1e-12)" % e)
                assert e <= 1e-12
        else:
            e = np.abs(proba[:, 0] - c.g["d_proba0"]).max()
            print("%s %s default parameters: P(normal) %.3e (gate 1e-12)" % (name, backend, e))
            assert e <= 1e-12


def fit_case(T, c, backend, wrap=lambda a: a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # a fit that does not converge fails the test
        return T.build_classifier(balanced=True, backend=backend, **kw).fit(wrap(c.results), wrap(c.y_tr), columns=c.cols, row_index=wrap(c.rows_tr))


def check_default_fit(G, T, name, backend, wrap=lambda a: a):
    c = Case(G, T, name)
    clf = fit_case(T, c, backend, wrap)
    lr, sc = clf.named_steps["logreg"], clf.named_steps["scaler"]
    X = c.results[c.rows_tr][:, c.cols]
    F, gmax, _ = np_objective(X, c.y_tr, c.C, T._as_numpy(sc.mean_), T._as_numpy(sc.scale_), T._as_numpy(lr.coef_), T._as_numpy(lr.intercept_))
    print("%s %s default fit: %d Newton iterations, %d passes, max |grad F| / sum sw = %.3e (gate 1e-4; reference %.3e)" %
          (name, backend, lr.n_iter_, lr.n_passes_, gmax, c.g["g_default"]))
    assert lr.converged_ and gmax <= 1e-4
    assert T._as_numpy(lr.coef_).shape == ((1, len(c.cols)) if c.C == 2 else (c.C, len(c.cols)))


def check_tight_fit(G, T, name, backend, wrap=lambda a: a, **kw):
    c = Case(G, T, name)
    clf = fit_case(T, c, backend, wrap, tol=1e-12, **kw)
    lr = clf.named_steps["logreg"]
    e_c = max(np.abs(T._as_numpy(lr.coef_) - c.g["t_coef"]).max(), np.abs(T._as_numpy(lr.intercept_) - c.g["t_intercept"]).max())
    args = dict(columns=c.cols, row_index=wrap(c.rows_te))
    proba, pred = T._as_numpy(clf.predict_proba(wrap(c.results), **args)), T._as_numpy(clf.predict(wrap(c.results), **args))
    pf = 1.0 - proba[:, 0]
    area = T.auc_score(c.truth, pf, backend="host")
    bound = int(c.g["q"]) / (int(c.g["n_pos"]) * int(c.g["n_neg"]))
    print("%s %s fit at tol 1e-12: %d iterations, %d passes; coef / intercept %.3e (gate 0.1 dc = %.3e); AUC %.6f vs %.6f, |d| %.3e (gate %.3e)"
          % (name, backend, lr.n_iter_, lr.n_passes_, e_c, 0.1 * c.g["dc"], area, c.g["t_auc"], abs(area - c.g["t_auc"]), bound))
    assert lr.converged_ and e_c <= 0.1 * c.g["dc"] and abs(area - float(c.g["t_auc"])) <= bound
    if "t_proba" in c.g:
        e_p = np.abs(proba - c.g["t_proba"]).max()
        top = np.sort(c.g["t_proba"], axis=1)
        sure = top[:, -1] - top[:, -2] >= 2 * c.delta
        print("   predict_proba %.3e (gate 0.1 dp = %.3e); predict differs on %d of %d sure rows" %
              (e_p, 0.1 * c.g["dp"], (pred != c.g["t_pred"])[sure].sum(), sure.sum()))
        assert e_p <= 0.1 * c.g["dp"] and np.array_equal(pred[sure], c.g["t_pred"][sure])
    if name in ("b3", "b4"):                                  # one feature: the score is monotone in it, the curve is the same
        r = T.roc_counts(wrap(c.truth), wrap(pf), pos_label=1, backend=backend)
        fps, tps = T._as_numpy(r["fps"]), T._as_numpy(r["tps"])
        print("   one feature: %d curve points, reference %d" % (len(fps) - 1, len(c.g["roc_fps"])))
        assert np.array_equal(fps[1:], c.g["roc_fps"]) and np.array_equal(tps[1:], c.g["roc_tps"])
    return clf


def fixture_scores(c):
    return c.g["t_p_fault"] if "t_p_fault" in c.g else 1.0 - c.g["t_proba"][:, 0]


def check_roc(T, truth, score, backend, wrap=lambda a: a, fixture=None, label=""):
    fps0, tps0, thr0 = reference_roc(truth, score)
    r = T.roc_counts(wrap(truth), wrap(score), pos_label=1, backend=backend)
    fpr, tpr, thr = (T._as_numpy(a) for a in T.roc_curve(wrap(truth), wrap(score), pos_label=1, backend=backend))
    fps, tps = T._as_numpy(r["fps"]), T._as_numpy(r["tps"])
    if fixture is not None:
        assert np.array_equal(fps0[1:], fixture["roc_fps"]) and np.array_equal(tps0[1:], fixture["roc_tps"]) and np.array_equal(thr0[1:], fixture["roc_thr"])
    P, N = int(truth.sum()), int(len(truth) - truth.sum())
    area, want = T.auc(fpr, tpr), exact_auc(truth, score)
    got = T.auc_score(wrap(truth), wrap(score), pos_label=1, backend=backend)
    print("%s %s ROC: %d points, %d distinct scores, auc(fpr, tpr) - exact %.3e (gate %.3e), auc_score - exact %.3e (gate 0)" %
          (label, backend, len(fps), r["n_distinct"], area - want[0], len(fps) * 2.0 ** -50, got - want[0]))
    assert np.array_equal(fps, fps0) and np.array_equal(tps, tps0) and thr.tobytes() == thr0.tobytes()
    assert fpr.tobytes() == (fps0 / N).tobytes() and tpr.tobytes() == (tps0 / P).tobytes()
    assert r["n_pos"] == P and r["n_neg"] == N and r["U2"] == want[1]
    assert got == want[0] and abs(area - want[0]) <= len(fps) * 2.0 ** -50
    if fixture is not None:
        assert abs(area - float(fixture["t_auc"])) <= len(fps) * 2.0 ** -50


def check_far_start(G, T, backend, wrap=lambda a: a):
    c = Case(G, T, "b1")
    trace = []
    clf = T.build_classifier(balanced=True, backend=backend, tol=1e-12, coef_init=np.array([[4.0, -3.0]]), intercept_init=[2.5], chunk=1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        clf.fit(wrap(c.results), wrap(c.y_tr), columns=c.cols, row_index=wrap(c.rows_tr), trace=trace)
    lr = clf.named_steps["logreg"]
    e_c = max(np.abs(T._as_numpy(lr.coef_) - c.g["t_coef"]).max(), np.abs(T._as_numpy(lr.intercept_) - c.g["t_intercept"]).max())
    print("%s far start: %d iterations in %d passes, F over the accepted points %s, coef / intercept %.3e (gate %.3e)" %
          (backend, lr.n_iter_, lr.n_passes_, np.array(trace), e_c, 0.1 * c.g["dc"]))
    assert lr.n_passes_ > lr.n_iter_ + 1, "no proposed point was rejected: the start is not far enough to test the line search"
    # F does not increase from one accepted point to the next.  Next to the minimum the decrease of F is smaller than the
    # rounding of its own sum of n terms, which the acceptance rule allows for (4 n eps F): that is the bound here.
    slack = 4 * len(c.y_tr) * np.finfo(float).eps * np.array(trace[:-1])
    assert np.all(np.diff(trace) <= slack) and trace[-1] < trace[0] and lr.converged_ and e_c <= 0.1 * c.g["dc"]
    # the accepted values are what the test's own numpy computes at the final point
    sc = clf.named_steps["scaler"]
    F = np_objective(c.results[c.rows_tr][:, c.cols], c.y_tr, c.C, T._as_numpy(sc.mean_), T._as_numpy(sc.scale_), T._as_numpy(lr.coef_),
                     T._as_numpy(lr.intercept_))[0]
    assert abs(F - lr.loss_) <= 1e-12 * abs(F) * len(c.y_tr)


def check_degenerate(T, backend, wrap=lambda a: a):
    rng = np.random.default_rng(3)
    X = rng.normal(size=(300, 3))
    X[:, 1] = 7.25
    y = (X[:, 0] + 0.5 * rng.normal(size=300) > 0).astype(np.int64)
    with pytest.raises(ValueError):
        T.build_classifier(backend=backend).fit(wrap(X), wrap(np.zeros(300, dtype=np.int64)))
    clf = T.build_classifier(backend=backend).fit(wrap(X), wrap(y))
    scale, coef = T._as_numpy(clf.named_steps["scaler"].scale_), T._as_numpy(clf.named_steps["logreg"].coef_)
    print("%s constant feature: scale_ %s coef_ %s" % (backend, scale, coef))
    assert scale[1] == 1.0 and coef[0, 1] == 0.0 and coef.shape == (1, 3)
    assert np.array_equal(T._as_numpy(clf.named_steps["logreg"].classes_), [0, 1])


# ------------------------------------------------------------------------------------------------ host tests
def test_names_defaults_and_parsing(G, T):
    assert (T.FEAT_GRP1, T.FEAT_GRP2, T.FEAT_GRP3, T.FEAT_GRP4) == ("epi,res", "x0,x3,x4,x5", "res", "y_true")
    assert (T.DEFAULT_TEST_SIZE, T.DEFAULT_RANDOM_STATE, T.DEFAULT_BALANCED) == (0.9, 49, True) and T.INDEX["label"] == 17
    for r, spec in enumerate(G["feat_specs"]):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            try:
                got, err = T.parse_features(str(spec)), 0
            except KeyError:
                got, err = None, 1
            except ValueError:
                got, err = None, 2
        assert err == G["feat_error"][r], spec
        if got is not None:
            want = [int(v) for v in G["feat_result"][r] if v != -99]
            assert got == want and int(len(w) > 0) == G["feat_warns"][r], spec
    groups = T.parse_group_spec("正常:0 | 故障:1,2,3,4,5,6,7,8,9 ,10,11,12")
    assert groups == T.parse_group_spec(T.DEFAULT_GROUP_SPEC) == {"normal": [0], "fault": list(range(1, 13))}
    assert list(T.parse_group_spec(FIVE)) == ["normal", "flooding", "oxygen_starvation", "membrane_drying", "hydrogen_starvation"]
    assert list(T.parse_group_spec(FIVE, translate=False))[0] == "正常"
    import pinn_amd
    assert pinn_amd.DeviceLogisticRegression is T.DeviceLogisticRegression and pinn_amd.roc_curve is T.roc_curve


@pytest.mark.parametrize("name", CASES)
def test_extract_and_scaler(G, T, name):
    c = Case(G, T, name)
    X, y, kept = T.extract_X_y(c.results, c.cols, c.label_map, return_index=True, backend="host")
    assert np.array_equal(kept, c.kept) and np.array_equal(y, c.y) and len(kept) == len(c.results) - len(c.g["dropped"])
    assert np.array_equal(np.bincount(c.y_tr, minlength=c.C), c.g["count"])
    check_scaler(G, T, name, "host")


@pytest.mark.parametrize("name", ["b1", "f2"])
def test_reference_parameters(G, T, name):
    check_reference_parameters(G, T, name, "host")


@pytest.mark.parametrize("name", CASES)
def test_default_fit_meets_the_stopping_rule(G, T, name):
    check_default_fit(G, T, name, "host")


@pytest.mark.parametrize("name", CASES)
def test_tight_fit_against_the_tight_reference(G, T, name):
    clf = check_tight_fit(G, T, name, "host")
    lr = clf.named_steps["logreg"]
    c = Case(G, T, name)
    assert np.array_equal(lr.class_count_, c.g["count"]) and abs(lr.class_weight_ @ lr.class_count_ - len(c.y_tr)) < 1e-9


@pytest.mark.parametrize("name", ["b1", "f2", "b3", "b4"])
def test_roc_on_the_fixture_scores(G, T, name):
    c = Case(G, T, name)
    s = fixture_scores(c)
    check_roc(T, c.truth, s, "host", fixture=c.g, label=name)
    check_roc(T, c.truth, np.round(s, 3), "host", label=name + " ties")
    check_roc(T, c.truth, np.full(len(s), 0.25), "host", label=name + " all equal")
    check_roc(T, c.truth, np.round(s - 0.5, 0), "host", label=name + " signed zeros")
    fpr, tpr, thr = T.roc_curve(c.truth, s, pos_label=1, drop_intermediate=False, backend="host")
    assert len(fpr) == len(np.unique(s)) + 1 and thr[0] == np.inf and abs(T.auc(fpr, tpr) - float(c.g["t_auc"])) <= len(fpr) * 2.0 ** -50
    assert abs(T.auc(fpr[::-1], tpr[::-1]) - T.auc(fpr, tpr)) <= len(fpr) * 2.0 ** -50          # a decreasing x gives the same area
    with pytest.raises(ValueError):
        T.auc_score(np.ones(5, dtype=int), np.arange(5.0), backend="host")
    with pytest.raises(ValueError):
        T.roc_curve(np.array([0, 1, 2]), np.arange(3.0), backend="host")


def test_stratified_split_properties(T):
    rng = np.random.default_rng(0)
    y = rng.choice(5, size=1403, p=[0.55, 0.2, 0.1, 0.1, 0.05])
    tr, te = T.stratified_split(y, 0.9, 49)
    assert tr.dtype == np.int64 and len(np.intersect1d(tr, te)) == 0 and np.array_equal(np.sort(np.concatenate([tr, te])), np.arange(len(y)))
    assert np.all(np.abs(np.bincount(y[te], minlength=5) - 0.9 * np.bincount(y, minlength=5)) <= 1.0)
    assert abs(len(te) - 0.9 * len(y)) <= 1.0
    tr2, te2 = T.stratified_split(y, 0.9, 49)
    assert np.array_equal(tr, tr2) and np.array_equal(te, te2)
    assert not np.array_equal(te, T.stratified_split(y, 0.9, 50)[1])
    with pytest.raises(ValueError):
        T.stratified_split(y, 1.0)


def test_far_start_rejects_a_step_and_reaches_the_same_optimum(G, T):
    check_far_start(G, T, "host")


def test_degenerate_input(T):
    check_degenerate(T, "host")


def test_unsupported_arguments(T):
    for kw in (dict(penalty="l1"), dict(solver="saga"), dict(multi_class="ovr"), dict(class_weight={0: 1.0})):
        with pytest.raises(NotImplementedError):
            T.DeviceLogisticRegression(**kw)
    with pytest.raises(NotImplementedError):
        T.DeviceLogisticRegression().fit(np.zeros((4, 1)), np.array([0, 1, 0, 1]), sample_weight=np.ones(4))
    with pytest.raises(ValueError):
        T.DeviceLogisticRegression(backend="gpu")
    assert T.limits_ok(5, 8) and T.limits_ok(13, 4) and T.limits_ok(2, 1) and not T.limits_ok(13, 5) and not T.limits_ok(14, 1) and not T.limits_ok(2, 9)


def test_limits_and_null_pointers_on_the_c_side():
    """Host-side checks of the entry points: no GPU is needed, every call fails before a launch."""
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    lib = _lib.load(build_if_missing=False)
    E_ARG, E_WS = -1, -3
    assert (_lib.LR_MAX_CLASSES, _lib.LR_MAX_FEAT, _lib.LR_MAX_HESS) == (13, 8, 1365)
    for C in range(1, 16):
        for D in range(0, 11):
            inside = 2 <= C <= 13 and 1 <= D <= 8 and (C * (C + 1) // 2) * ((D + 1) * (D + 2) // 2) <= 1365
            assert (lib.pinn_lr_state_bytes(C, D) > 0) == inside and (lib.pinn_lr_workspace_bytes(100, C, D) > 0) == inside
            if C <= 5 and D <= 8 or C <= 13 and D <= 4:
                assert inside == (C >= 2 and D >= 1)
    one = ctypes.c_void_p(0x1000)
    cols = (ctypes.c_int * 4)(0, 1, 2, 3)
    big = 1 << 30
    assert lib.pinn_lr_newton(one, 22, 10, cols, 4, None, 10, one, 14, 1, 1e-4, 1.0, 1, one, one, big, None) == E_ARG      # 14 classes
    assert lib.pinn_lr_newton(one, 22, 10, cols, 4, None, 10, one, 5, 1, 1e-4, 1.0, 1, None, one, big, None) == E_ARG
    assert lib.pinn_lr_newton(one, 22, 10, cols, 4, None, 10, None, 5, 1, 1e-4, 1.0, 1, one, one, big, None) == E_ARG
    assert lib.pinn_lr_newton(one, 22, 10, cols, 4, None, 10, one, 5, 1, 1e-4, 1.0, 1, one, None, big, None) == E_ARG
    assert lib.pinn_lr_newton(one, 22, 10, cols, 4, None, 10, one, 5, 1, 1e-4, 1.0, 1, one, one, 64, None) == E_WS
    assert lib.pinn_lr_newton(one, 22, 10, cols, 4, None, 10, one, 5, 1, 1e-4, 0.0, 1, one, one, big, None) == E_ARG        # no penalty
    assert lib.pinn_lr_newton(None, 22, 10, cols, 4, None, 10, one, 5, 1, 1e-4, 1.0, 1, one, one, big, None) == E_ARG
    assert lib.pinn_lr_scaler(one, 22, 10, cols, 4, None, 10, one, 5, 1, None, one, big, None) == E_ARG
    assert lib.pinn_lr_scaler(one, 22, 10, cols, 4, None, 10, one, 5, 1, one, one, 64, None) == E_WS
    assert lib.pinn_lr_scaler(one, 3, 10, cols, 4, None, 10, one, 5, 1, one, one, big, None) == E_ARG                     # column 3 of 3
    assert lib.pinn_lr_pass(one, 22, 10, cols, 4, None, 10, one, 5, one, None, big, None) == E_ARG
    assert lib.pinn_lr_pass(one, 22, 10, cols, 4, None, 10, one, 5, one, one, 64, None) == E_WS
    assert lib.pinn_lr_posterior(one, 22, 10, cols, 4, None, 10, 5, None, 0, one, None, None, None, None) == E_ARG
    assert lib.pinn_lr_posterior(one, 22, 10, cols, 4, None, 10, 5, one, 5, one, None, None, None, None) == E_ARG         # normal class 5 of 5
    assert lib.pinn_lr_posterior(one, 22, 10, cols, 9, None, 10, 5, one, 0, one, None, None, None, None) == E_ARG         # 9 features
    assert lib.pinn_lr_roc(one, one, 10, 1, None, None, None, None, None, None, one, big, None) == E_ARG
    assert lib.pinn_lr_roc(one, one, 10, 1, one, None, None, None, None, None, None, big, None) == E_ARG
    assert lib.pinn_lr_roc(one, one, 10, 1, one, None, None, None, None, None, one, 64, None) == E_WS
    assert lib.pinn_lr_roc(one, one, 0, 1, one, None, None, None, None, None, one, big, None) == E_ARG
    assert lib.pinn_lr_roc_workspace_bytes(10) > 0 and lib.pinn_lr_roc_workspace_bytes(-1) == 0


def test_evaluate_feature_groups_and_the_online_detector(G, T):
    c1 = Case(G, T, "b1")
    res = T.evaluate_feature_groups(c1.results, backend="host", tol=1e-12, split=None)
    assert [r["spec"] for r in res] == list(T.FEATURE_GROUPS) and res[0]["class_names"] == ["normal", "fault"]
    for r in res:
        assert 0.5 < r["auc"] < 1.0 and abs(r["n_test"] - 0.9 * (r["n_test"] + r["n_train"])) <= 1 and r["metrics"]["confusion_matrix"].sum() == r["n_test"]
        assert abs(T.auc(r["fpr"], r["tpr"]) - r["auc"]) <= len(r["fpr"]) * 2.0 ** -50
    for name in ("b1", "b2", "f1", "f4"):                     # the reference's own split
        c = Case(G, T, name)
        r = T.evaluate_feature_groups(c.results, feature_groups=[",".join(str(k) for k in c.cols)], group_spec=c.spec, split=(c.idx_tr, c.idx_te),
                                      backend="host", tol=1e-12)[0]
        bound = int(c.g["q"]) / (int(c.g["n_pos"]) * int(c.g["n_neg"]))
        wrong = int(np.abs(r["metrics"]["confusion_matrix"] - c.g["t_cm"]).sum())
        print("%s evaluate: AUC %.6f vs %.6f (gate %.3e), confusion matrix differs by %d entries (close rows: %d)" %
              (name, r["auc"], c.g["t_auc"], bound, wrong, round(float(c.g["close"]) * r["n_test"])))
        assert abs(r["auc"] - float(c.g["t_auc"])) <= bound and wrong <= 2 * round(float(c.g["close"]) * r["n_test"])
    # online: chunk by chunk equals the whole
    clf = res[0]["clf"]
    det = T.FaultDetector(clf, features=T.FEAT_GRP1, normal_class=0, backend="host")
    rows = c1.results[c1.kept]
    parts = [det.update(rows[i:i + 333]) for i in range(0, len(rows), 333)]
    pf = np.concatenate([p[0] for p in parts])
    assert det.n_seen == len(rows) and pf.tobytes() == (1.0 - clf.predict_proba(rows, columns=c1.cols)[:, 0]).tobytes()
    assert np.array_equal(np.concatenate([p[1] for p in parts]), clf.predict(rows, columns=c1.cols))


def test_script_05_baseline_and_coefficients(G, T):
    c = Case(G, T, "f2")
    X_tr, X_te = c.results[c.rows_tr][:, c.cols], c.results[c.rows_te][:, c.cols]
    pred = T.run_supervised_lr(X_tr, c.y_tr, X_te, backend="host", tol=1e-12)
    top = np.sort(c.g["t_proba"], axis=1)
    sure = top[:, -1] - top[:, -2] >= 2 * c.delta
    assert np.array_equal(pred[sure], c.g["t_pred"][sure])
    m = T.compute_macro_metrics(c.y_te, pred)
    assert set(m) == {"accuracy", "macro_precision", "macro_recall", "macro_f1"} and abs(m["accuracy"] - (pred == c.y_te).mean()) < 1e-15
    clf = T.build_classifier(balanced=True, backend="host").fit(X_tr, c.y_tr)
    ex = T.explain_coefficients(clf, c.cols, c.names, topn=2)
    assert len(ex) == 5 and ex[0]["class"] == "normal" and len(ex[0]["positive"]) == 2 and ex[0]["positive"][0][1] >= ex[0]["positive"][1][1]
    assert {n for n, _ in ex[0]["positive"]} <= {"x0", "x3", "x4", "x5"} and T.explain_coefficients(clf, c.cols, c.names, topn=0) == []


def test_fresh_draw_against_scikit_learn(T):
    sk = pytest.importorskip("sklearn")
    from sklearn.linear_model import LogisticRegression
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler
    rng = np.random.default_rng(77)
    for C, D in ((2, 2), (5, 4), (3, 8)):
        n = 600
        y = rng.integers(C, size=n)
        X = rng.normal(size=(n, D)) * rng.uniform(0.5, 3.0, D) + 0.5 * y[:, None] * rng.normal(size=D) + 4.0
        Xt = rng.normal(size=(2000, D)) * 2.0 + 4.0
        fits = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for tag, kw in (("d", {}), ("t", dict(tol=1e-13, max_iter=100000))):
                fits[tag] = Pipeline([("s", StandardScaler()), ("l", LogisticRegression(multi_class="multinomial", class_weight="balanced", **kw))]).fit(X, y)
        dp = np.abs(fits["d"].predict_proba(Xt) - fits["t"].predict_proba(Xt)).max()
        dc = max(np.abs(fits["d"][1].coef_ - fits["t"][1].coef_).max(), np.abs(fits["d"][1].intercept_ - fits["t"][1].intercept_).max())
        clf = T.build_classifier(balanced=True, backend="host", tol=1e-12).fit(X, y)
        lr = clf.named_steps["logreg"]
        e_c = max(np.abs(lr.coef_ - fits["t"][1].coef_).max(), np.abs(lr.intercept_ - fits["t"][1].intercept_).max())
        pt = fits["t"].predict_proba(Xt)
        e_p = np.abs(clf.predict_proba(Xt) - pt).max()
        top = np.sort(pt, axis=1)
        sure = top[:, -1] - top[:, -2] >= 0.2 * dp
        print("scikit-learn %s, C=%d D=%d: coef %.3e (gate 0.1 dc = %.3e), proba %.3e (gate 0.1 dp = %.3e)" % (sk.__version__, C, D, e_c, 0.1 * dc, e_p, 0.1 * dp))
        assert e_c <= 0.1 * dc and e_p <= 0.1 * dp and np.array_equal(clf.predict(Xt)[sure], fits["t"].predict(Xt)[sure])
        assert np.abs(clf.named_steps["scaler"].scale_ - fits["t"][0].scale_).max() <= 1e-12 * fits["t"][0].scale_.max()
