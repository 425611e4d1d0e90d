"""CPU: the host backend of pinn_amd.svm (float64 numpy, the device's state machine) against tests/golden/g_svm.npz
(scikit-learn's SVC as script 05 runs it, solved to tol = 1e-12 by tools/make_golden_svm.py) on the split of g_cluster.npz.
The checkers and the drawn cases are shared with tests/test_gpu_svm.py.

Gates (from the problem's convexity and the number format, never from what the code under test returns):
1. the optimality certificate, computed here in numpy from alpha_, coef_ and intercept_: 0 <= alpha <= c to 1e-12 c,
   |t'alpha| <= 1e-12 sum alpha, |coef_ - V'alpha| <= 1e-12 sum |terms|, 0 <= primal - dual <= 1e-10 max(1, primal), and
   dual_gap_ equal to that difference within 1e-12 primal;
2. strong convexity, 1/2 |w - w*|^2 <= primal(w, b) - primal*, gives |coef_ - ref_coef|_2 <= sqrt(2 gap) + sqrt(2 ref_gap) from
   the two certificates alone; at a row that is free in the reference (alpha well inside (0, c)) both solutions have
   t (w.z + b) = 1 up to their margin residuals r, so |b - b_ref| <= coefficient bound |z|_2 + |r| + |r_ref|;
3. with eps = coefficient bound |z|_2 + intercept bound per pair, predictions equal the reference's on every row whose
   pairwise values all exceed eps in magnitude; at most 1 % of the rows may be left out.
Every comparison prints its maxima before it asserts."""
import warnings

import numpy as np
import pytest

METRICS = ("accuracy", "macro_precision", "macro_recall", "macro_f1")
FREE = 1e-4          # a row counts as free with alpha this fraction of c inside (0, c): eight orders above the solvers' complementarity


@pytest.fixture(scope="module")
def G(golden):
    g = golden("g_cluster.npz")
    g.update({"svm_" + k: v for k, v in golden("g_svm.npz").items()})
    return g


@pytest.fixture(scope="module")
def S():
    from pinn_amd import svm
    return svm


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def pairs_of(C):
    return [(a, b) for a in range(C) for b in range(a + 1, C)]


def balanced(y, C):
    return len(y) / (C * np.bincount(y, minlength=C).astype(np.float64))


def model_wb(m):
    """(w [P, D], b [P]) positive for the pair's first class: scikit-learn negates coef_ and intercept_ for two classes."""
    sign = -1.0 if len(host(m.class_weight_)) == 2 else 1.0
    return sign * host(m.coef_), sign * host(m.intercept_)


def pair_rows(y, alpha, a, b):
    """(row positions, t, alpha) of the pair, the rows of class a first."""
    ia, ib = np.nonzero(y == a)[0], np.nonzero(y == b)[0]
    return (np.concatenate([ia, ib]), np.concatenate([np.ones(len(ia)), -np.ones(len(ib))]),
            np.concatenate([alpha[ia, b - 1], alpha[ib, a]]))


def objectives(Z, y, c_row, alpha, w, b, C):
    """Per pair (primal, dual) in float64 numpy."""
    out = []
    for p, (a, bb) in enumerate(pairs_of(C)):
        idx, t, al = pair_rows(y, alpha, a, bb)
        v = (al * t) @ Z[idx]
        out.append((0.5 * float(w[p] @ w[p]) + float(np.sum(c_row[idx] * np.maximum(0.0, 1.0 - t * (Z[idx] @ w[p] + b[p])))),
                    float(al.sum()) - 0.5 * float(v @ v)))
    return np.array(out)


def check_certificate(m, Z, y, cw, C_pen, what):
    """Gate 1 on a fitted model; Z the standardised rows, y class indices, cw the class weights.  Returns gap [P], primal [P]."""
    C = len(cw)
    alpha, (w, b) = host(m.alpha_), model_wb(m)
    c_row = C_pen * cw[y]
    assert alpha.shape == (len(y), C - 1) and w.shape == (C * (C - 1) // 2, Z.shape[1]) and np.isfinite(alpha).all() and np.isfinite(w).all()
    e_lo, e_hi, e_t, e_w = 0.0, 0.0, 0.0, 0.0
    for p, (a, bb) in enumerate(pairs_of(C)):
        idx, t, al = pair_rows(y, alpha, a, bb)
        e_lo, e_hi = max(e_lo, float(np.max(-al / c_row[idx]))), max(e_hi, float(np.max(al / c_row[idx] - 1.0)))
        e_t = max(e_t, abs(float(t @ al)) / float(al.sum()))
        terms = (al * t)[:, None] * Z[idx]
        e_w = max(e_w, float(np.max(np.abs(w[p] - terms.sum(axis=0)) / np.maximum(np.abs(terms).sum(axis=0), 1e-300))))
    obj = objectives(Z, y, c_row, alpha, w, b, C)
    primal, gap = obj[:, 0], obj[:, 0] - obj[:, 1]
    e_g = float(np.max(np.abs(host(m.dual_gap_) - gap) / primal))
    print("%s: alpha below 0 %.1e, above c %.1e, |t'alpha| / sum %.1e, coef - V'alpha %.1e (gates 1e-12); gap / max(1, primal) in "
          "[%.2e, %.2e] (gate 0..1e-10), dual_gap_ off by %.1e primal (gate 1e-12), iterations %s"
          % (what, e_lo, e_hi, e_t, e_w, float(np.min(gap / np.maximum(1.0, primal))), float(np.max(gap / np.maximum(1.0, primal))), e_g,
             list(host(m.n_iter_))))
    assert bool(np.all(host(m.converged_)))
    assert e_lo <= 1e-12 and e_hi <= 1e-12 and e_t <= 1e-12 and e_w <= 1e-12
    assert np.all(gap >= 0.0) and np.all(gap <= 1e-10 * np.maximum(1.0, primal))
    assert e_g <= 1e-12
    return gap, primal


def bounds_against(Z, y, c_row, C, w, b, gap, r_w, r_b, r_alpha, r_gap, what, need_intercept=True):
    """Gate 2 against a reference solution (r_w, r_b, r_alpha, r_gap).  Returns (coefficient bound [P], intercept bound [P]);
    the intercept bound is inf where the reference has no free row."""
    cb, ib, e_c, e_b = np.zeros(len(w)), np.full(len(w), np.inf), 0.0, 0.0
    for p, (a, bb) in enumerate(pairs_of(C)):
        cb[p] = np.sqrt(2.0 * max(gap[p], 0.0)) + np.sqrt(2.0 * max(r_gap[p], 0.0))
        d = float(np.linalg.norm(w[p] - r_w[p]))
        e_c = max(e_c, d)
        assert d <= cb[p], (what, p, d, cb[p])
        idx, t, al = pair_rows(y, r_alpha, a, bb)
        inside = np.minimum(al, c_row[idx] - al) / c_row[idx]
        i = int(np.argmax(inside))
        if inside[i] >= FREE:
            zi = Z[idx[i]]
            ib[p] = cb[p] * np.linalg.norm(zi) + abs(t[i] * (zi @ w[p] + b[p]) - 1.0) + abs(t[i] * (zi @ r_w[p] + r_b[p]) - 1.0)
            e_b = max(e_b, abs(b[p] - r_b[p]))
            assert abs(b[p] - r_b[p]) <= ib[p], (what, p, abs(b[p] - r_b[p]), ib[p])
    print("%s: coef off by at most %.3e (bounds %.3e .. %.3e), intercept by %.3e (bounds %.3e .. %.3e)"
          % (what, e_c, cb.min(), cb.max(), e_b, ib.min(), ib.max()))
    assert not need_intercept or np.isfinite(ib).all()
    return cb, ib


def decided_rows(Zt, r_dec, cb, ib):
    """Rows whose every pairwise reference value exceeds eps = coefficient bound |z|_2 + intercept bound."""
    eps = np.linalg.norm(Zt, axis=1)[:, None] * cb[None, :] + ib[None, :]
    return np.all(np.abs(r_dec) > eps, axis=1)


def settled_rows(Zt, r_dec, cb, ib, C):
    """Where a pair has no free row in the reference its intercept has no bound (eps = inf) and its vote is open on every row.
    Returns (keep, near): keep marks the rows whose prediction is the same however their open votes (|value| <= eps) fall,
    which holds every row of decided_rows; near marks the rows with a value within a finite eps of zero."""
    eps = np.linalg.norm(Zt, axis=1)[:, None] * cb[None, :] + ib[None, :]
    open_ = ~(np.abs(r_dec) > eps)
    pairs, keep = pairs_of(C), np.ones(len(Zt), dtype=bool)
    for i in np.nonzero(open_.any(axis=1))[0]:
        base, op, winners = np.zeros(C, dtype=np.int64), np.nonzero(open_[i])[0], set()
        for p in np.nonzero(~open_[i])[0]:
            base[pairs[p][0 if r_dec[i, p] > 0 else 1]] += 1
        for bits in range(1 << len(op)):
            v = base.copy()
            for q, p in enumerate(op):
                v[pairs[p][(bits >> q) & 1]] += 1
            winners.add(int(v.argmax()))
        keep[i] = len(winners) == 1
    return keep, (open_ & np.isfinite(eps)).any(axis=1)


def check_predictions(pred, r_pred, keep, what, limit=0.01, near=None):
    """Equal predictions on the rows of `keep`; at most `limit` of the rows may lie within eps of a boundary (`near`; without
    it, every row outside `keep` counts)."""
    near = ~keep if near is None else near
    left = float(np.mean(near))
    print("%s: %d of %d rows within eps of a boundary (gate %.0f %%), %d compared, %d of them differ"
          % (what, int(near.sum()), len(keep), 100 * limit, int(keep.sum()), int((pred[keep] != r_pred[keep]).sum())))
    assert left <= limit and keep.any()
    assert np.array_equal(pred[keep], r_pred[keep])


def own_decision(Z, w, b, C):
    dec = Z @ w.T + b
    votes = np.zeros((len(Z), C), dtype=np.int64)
    for p, (a, bb) in enumerate(pairs_of(C)):
        votes[:, a] += dec[:, p] > 0
        votes[:, bb] += ~(dec[:, p] > 0)
    return dec, votes.argmax(axis=1)


def check_fixture(G, S, backend, to=lambda a: a):
    """Gates 1-3 of a fit of the fixture's training rows; returns the pipeline."""
    pipe = S.build_svm_classifier(backend).fit(to(G["X_tr"]), to(G["y_tr"]))
    m, sc = pipe.named_steps["svc"], pipe.named_steps["scaler"]
    y, C = G["y_tr"], 4
    e_s = max(np.abs(host(sc.mean_) - G["svm_mean"]).max() / np.abs(G["svm_mean"]).max(), np.abs(host(sc.scale_) / G["svm_scale"] - 1.0).max())
    print("scaler against scikit-learn's: %.3e (gate 1e-13)" % e_s)
    assert e_s <= 1e-13
    Z, Zt = (G["X_tr"] - G["svm_mean"]) / G["svm_scale"], (G["X_te"] - G["svm_mean"]) / G["svm_scale"]
    cw = balanced(y, C)
    assert np.abs(host(m.class_weight_) / cw - 1.0).max() <= 1e-15 and np.array_equal(host(m.classes_), np.arange(4))
    gap, primal = check_certificate(m, Z, y, cw, 0.05, "fixture, " + backend)
    w, b = model_wb(m)
    cb, ib = bounds_against(Z, y, 0.05 * cw[y], C, w, b, gap, G["svm_coef"], G["svm_intercept"], G["svm_alpha"], G["svm_ref_gap"],
                            "fixture against scikit-learn, " + backend)
    keep = decided_rows(Zt, G["svm_dec_te"], cb, ib)
    y_pred = host(pipe.predict(to(G["X_te"])))
    check_predictions(y_pred, G["svm_pred_tight"], keep, "fixture, tol = 1e-12")
    check_predictions(y_pred, G["svm_pred_default"], keep, "fixture, libsvm's default tol")
    dec = host(pipe.decision_function(to(G["X_te"]), shape="ovo"))
    e_d = np.abs(dec - G["svm_dec_te"]).max()
    print("decision values off by at most %.3e (largest eps %.3e)" % (e_d, (np.linalg.norm(Zt, axis=1)[:, None] * cb + ib).max()))
    assert np.all(np.abs(dec - G["svm_dec_te"]) <= np.linalg.norm(Zt, axis=1)[:, None] * cb[None, :] + ib[None, :])
    sup = host(m.n_support_)
    print("n_support_ %s, scikit-learn's %s" % (list(sup), list(G["svm_n_support"])))
    assert sup.shape == (4,) and np.abs(sup - G["svm_n_support"]).max() <= 2          # alpha at the edge of 1e-8 c is libsvm's own error
    pos, al = m.pair_alpha(1, 3)
    idx, _, al_own = pair_rows(y, host(m.alpha_), 1, 3)
    order = np.argsort(idx)
    assert np.array_equal(host(pos), idx[order]) and np.array_equal(host(al), al_own[order])
    return pipe


def svm_blobs(n, C, Dm, seed, spread=1.6, offset=0.0, apart=None):
    """n rows around C centres `apart` from each other along the first feature, overlapping enough that bounded support
    vectors exist; every class has rows."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, spread, (C, Dm))
    # no two classes on top of each other; with one feature a pair of overlapping small classes often has no free row (its
    # intercept is then pinned by a kink, which the gates cannot bound), so there the classes are drawn apart
    centres[:, 0] += ((2.5 if Dm > 1 else 6.0) if apart is None else apart) * rng.permutation(C)
    # unequal class sizes: with equal bounds on both sides of a pair the intercept can be free in an interval (no free row)
    share = rng.permutation(np.arange(1.0, C + 1.0))
    y = rng.permutation(np.concatenate([np.arange(C), rng.choice(C, n - C, p=share / share.sum())]))
    X = centres[y] + rng.normal(0.0, 1.0, (n, Dm)) * rng.uniform(0.5, 1.5, Dm)
    return X + offset, y.astype(np.int64)


def drawn_case(S, n, C, Dm, **svc_args):
    """A draw whose host solution has a free row in every pair and leaves at most 1 % of its own rows (none of fewer than
    100) within eps of a pairwise boundary; at most 3 redraws.  Returns X, y, the host pipeline and its certificate."""
    # a handful of rows, or separated classes on one feature: a bound that the support vectors stay inside of
    svc_args = {"C": 1000.0 if Dm == 1 else (10.0 if n <= 16 else 1.0), "class_weight": "balanced", **svc_args}
    for seed in range(4):
        X, y = svm_blobs(n, C, Dm, 1000 * n + 10 * C + Dm + 7919 * seed)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            pipe = S.build_svm_classifier("host", **svc_args).fit(X, y)
        m, sc = pipe.named_steps["svc"], pipe.named_steps["scaler"]
        Z = (X - sc.mean_) / sc.scale_
        cw = balanced(y, C) if m.class_weight == "balanced" else np.ones(C)
        c_row = m.C * cw[y]
        w, b = model_wb(m)
        free = all((np.minimum(al, c_row[idx] - al) / c_row[idx]).max() >= FREE
                   for idx, _, al in (pair_rows(y, m.alpha_, a, bb) for a, bb in pairs_of(C)))
        if not free:
            continue
        gap, _ = check_certificate(m, Z, y, cw, m.C, "drawn %d x %d, %d classes, host" % (n, Dm, C))
        cb, ib = bounds_against(Z, y, c_row, C, w, b, gap, w, b, m.alpha_, gap, "the host against itself")
        dec, _ = own_decision(Z, w, b, C)
        if np.mean(~decided_rows(Z, dec, cb, ib)) <= 0.01:
            return X, y, pipe, (Z, cw, c_row, w, b, gap, dec)
    raise AssertionError("no draw met the margin condition")


OVERLAPPING = [(129, 2), (2049, 4)]


def overlapping_case(S, n, C, backend, to=lambda a: a):
    """One feature, the classes 2.5 apart with spread 1 and C = 1: every pair has rows at the bound alpha = c, and often no free
    row, so the intercept sits in a kink and has no bound.  Gate 1 on the fit; returns what gate 2 needs for w."""
    X, y = svm_blobs(n, C, 1, 77 * n + C, apart=2.5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pipe = S.build_svm_classifier(backend, C=1.0).fit(to(X), to(y))
    m, sc = pipe.named_steps["svc"], pipe.named_steps["scaler"]
    Z, cw = (X - host(sc.mean_)) / host(sc.scale_), balanced(y, C)
    gap, _ = check_certificate(m, Z, y, cw, 1.0, "overlapping %d x 1, %d classes, %s" % (n, C, backend))
    alpha, c_row = host(m.alpha_), cw[y]
    at_c = [int((al >= (1.0 - 1e-6) * c_row[idx]).sum()) for idx, _, al in (pair_rows(y, alpha, a, b) for a, b in pairs_of(C))]
    print("rows at the bound per pair: %s" % at_c)
    assert min(at_c) >= 2                     # a property of the draw: with classes 2.5 apart about a tenth of a pair's rows
    w, b = model_wb(m)
    return Z, y, c_row, w, b, alpha, gap


@pytest.mark.parametrize("n,C", OVERLAPPING)
def test_one_feature_overlapping_on_the_host(S, n, C):
    overlapping_case(S, n, C, "host")


# ---------------------------------------------------------------------------------------------- tests
def test_host_matches_reference_fixture(G, S):
    pipe = check_fixture(G, S, "host")
    assert isinstance(pipe.named_steps["svc"].coef_, np.ndarray)
    y_pred = S.run_supervised_svm_rbf(G["X_tr"], G["y_tr"], G["X_te"], backend="host")
    assert np.array_equal(y_pred, pipe.predict(G["X_te"]))


def test_compare_methods_with_and_without_device_extras(G, S):
    from pinn_amd import comparison as P
    import pinn_amd
    X, y = np.concatenate([G["X_tr"], G["X_te"]]), np.concatenate([G["y_tr"], G["y_te"]])
    n_tr = len(G["y_tr"])
    split = (np.arange(n_tr), n_tr + np.arange(len(G["y_te"])))
    assert P.METHODS == ("GMM", "Sup_LR", "KMeans", "Agglo")
    with pytest.raises(NotImplementedError, match="device_extras"):
        P.compare_methods(X, y, methods=("KMeans", "Sup_SVM"), split=split, backend="host")
    with pytest.raises(NotImplementedError):
        P.compare_methods(X, y, methods=("Spectral",), split=split, backend="host", extra=P.device_extras("host"))
    r = P.compare_methods(X, y, methods=("Sup_LR", "Sup_SVM"), split=split, backend="host", extra=pinn_amd.device_extras("host"))
    assert list(r) == ["split", "Sup_LR", "Sup_SVM"]
    lo, hi = G["svm_acc_range"]
    e = max(abs(r["Sup_SVM"][k] - v) for k, v in zip(METRICS, G["svm_svm_metrics"]))
    print("Sup_SVM: accuracy %.4f (the reference's %.4f), metrics differ by %.3e (gate: the fixture's accuracy range %.4f)"
          % (r["Sup_SVM"]["accuracy"], G["svm_svm_metrics"][0], e, hi - lo))
    assert e <= hi - lo and r["Sup_SVM"]["accuracy"] >= lo - (hi - lo)


def test_votes_ties_and_decision_shapes(G, S):
    m = S.DeviceLinearSVC(backend="host")
    # three classes, values chosen by hand: a cycle 0 beats 1, 1 beats 2, 2 beats 0 ties at one vote each -> class 0
    m._w, m._b = np.zeros((3, 1)), np.array([1.0, -1.0, 1.0])
    m.coef_, m.intercept_, m.class_weight_, m.classes_, m.n_features_in_ = m._w, m._b, np.ones(3), np.array([5, 7, 9]), 1
    assert np.array_equal(m.predict(np.zeros((2, 1))), [5, 5])
    m._b = np.array([-1.0, -1.0, 0.0])                     # 1 beats 0, 2 beats 0, value 0 is a vote for the second class: 2 wins
    m.intercept_ = m._b
    assert np.array_equal(m.predict(np.zeros((1, 1))), [9])
    # "ovr" is scikit-learn's transform of the recorded pairwise values; "ovo" the values themselves
    dec = G["svm_dec_te"]
    ovr = S.ovr_decision_function(dec, 4)
    conf = np.zeros((len(dec), 4))
    votes = np.zeros((len(dec), 4))
    for p, (a, b) in enumerate(pairs_of(4)):
        conf[:, a] += dec[:, p]
        conf[:, b] -= dec[:, p]
        votes[:, a] += dec[:, p] >= 0
        votes[:, b] += dec[:, p] < 0
    want = votes + conf / (3 * (np.abs(conf) + 1))
    assert np.abs(ovr - want).max() <= 1e-15 and np.array_equal(ovr.argmax(axis=1), G["svm_pred_tight"])
    pipe = S.build_svm_classifier("host").fit(G["X_tr"], G["y_tr"])
    assert pipe.decision_function(G["X_te"]).shape == (450, 4) and pipe.decision_function(G["X_te"], shape="ovo").shape == (450, 6)
    two = S.DeviceLinearSVC(backend="host").fit(G["X_tr"][G["y_tr"] < 2], G["y_tr"][G["y_tr"] < 2])
    d2 = two.decision_function(G["X_te"])
    assert d2.shape == (450,) and two.coef_.shape == (1, 4) and np.array_equal(two.predict(G["X_te"]), (d2 >= 0).astype(np.int64) * (d2 != 0))


NAMED = ("separable", "single_row_class", "unequal_balanced", "unequal_dict", "large_offset", "duplicates", "coincident")


def named_case(name):
    """X, y, constructor arguments of DeviceLinearSVC."""
    rng = np.random.default_rng(len(name))
    if name == "separable":
        y = np.arange(300) % 2
        return rng.normal(0.0, 1.0, (300, 3)) + 12.0 * y[:, None], y, {"C": 1.0, "class_weight": None}
    if name == "single_row_class":
        X, y = svm_blobs(201, 3, 4, 5)
        keep = np.concatenate([np.nonzero(y != 1)[0], np.nonzero(y == 1)[0][:1]])
        return X[keep], y[keep], {"C": 1.0, "class_weight": None}
    if name.startswith("unequal"):
        y = np.concatenate([np.zeros(5, dtype=np.int64), np.ones(500, dtype=np.int64)])
        X = rng.normal(0.0, 1.0, (505, 2)) + 1.5 * y[:, None]
        return X, y, {"C": 0.5, "class_weight": "balanced" if name.endswith("balanced") else {0: 20.0, 1: 0.5}}
    if name == "large_offset":
        X, y = svm_blobs(400, 3, 4, 11)
        return X + 1e6, y, {"C": 0.2, "class_weight": "balanced"}
    if name == "duplicates":
        X, y = svm_blobs(150, 3, 2, 13)
        return np.concatenate([X, X]), np.concatenate([y, y]), {"C": 0.3, "class_weight": None}
    X, y = svm_blobs(120, 2, 3, 17)
    X = np.concatenate([X, rng.normal(3.0, 1.0, (60, 3))])
    return np.concatenate([X, X[:120]]), np.concatenate([y, np.full(60, 3), np.full(120, 2)]), {"C": 1.0, "class_weight": None}      # classes 2 = 0 and 1 together


def weights_of(args, y, C):
    cwa = args.get("class_weight")
    return balanced(y, C) if cwa == "balanced" else (np.array([cwa.get(k, 1.0) for k in range(C)]) if isinstance(cwa, dict) else np.ones(C))


def check_named(S, name, backend, to=lambda a: a):
    """Gate 1 on the named case; returns what the device test compares with the host."""
    X, y, args = named_case(name)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pipe = S.build_svm_classifier(backend, **args).fit(to(X), to(y))
    m, sc = pipe.named_steps["svc"], pipe.named_steps["scaler"]
    classes = np.unique(y)
    yi, C = np.searchsorted(classes, y), len(classes)
    cw = weights_of(args, yi, C)
    Z = (X - host(sc.mean_)) / host(sc.scale_)
    gap, primal = check_certificate(m, Z, yi, cw, m.C, "%s, %s" % (name, backend))
    w, b = model_wb(m)
    alpha, c_row = host(m.alpha_), m.C * cw[yi]
    if name == "separable":
        top = float(np.max(alpha / c_row[:, None]))
        print("separable: largest alpha / c %.3e" % top)
        assert top < 0.5 and np.array_equal(host(pipe.predict(to(X))), y)
    if name == "single_row_class":
        assert host(m.n_support_)[1] == 1
    if name == "large_offset":
        centred = S.build_svm_classifier("host", **args).fit(X - 1e6, y).named_steps["svc"]
        w0, b0 = model_wb(centred)
        Z0 = (X - 1e6 - (X - 1e6).mean(axis=0)) / (X - 1e6).std(axis=0)
        g0, _ = check_certificate(centred, Z0, yi, cw, m.C, "large_offset, centred on the host")
        bounds_against(Z0, yi, c_row, C, w, b, gap, w0, b0, centred.alpha_, g0, "offset 1e6 against the centred problem")
    if name == "coincident":
        p = pairs_of(C).index((0, 2))
        # class 2 holds the rows of classes 0 and 1 together: the pair (0, 2) has every row of class 0 on both sides.  The
        # certificate and finiteness are asked of it; two identical sets, where w = 0, are check_identical_classes
        print("class 0 inside class 2: |w| %.3e, intercept %.3e" % (np.linalg.norm(w[p]), b[p]))
    return X, y, args, pipe, (Z, yi, cw, c_row, w, b, gap)


@pytest.mark.parametrize("name", NAMED)
def test_named_cases_on_the_host(S, name):
    check_named(S, name, "host")


def check_identical_classes(S, backend, to=lambda a: a):
    """Two classes with identical rows: w = 0 within the gate (1/2 |w|^2 <= gap, as w* = 0), everything finite; the intercept
    is not gated."""
    X, _ = svm_blobs(90, 2, 3, 23)
    X, y = np.concatenate([X, X]), np.concatenate([np.zeros(90, dtype=np.int64), np.ones(90, dtype=np.int64)])
    m = S.DeviceLinearSVC(C=0.7, backend=backend).fit(to(X), to(y))
    gap, _ = check_certificate(m, X, y, np.ones(2), 0.7, "identical classes, " + backend)
    w, b = model_wb(m)
    print("identical classes: |w| %.3e (gate %.3e), intercept %.3e" % (np.linalg.norm(w[0]), np.sqrt(2 * gap[0]), b[0]))
    assert np.linalg.norm(w[0]) <= np.sqrt(2 * gap[0]) and np.isfinite(b).all() and np.isfinite(host(m.alpha_)).all()
    assert np.isfinite(host(m.decision_function(to(X)))).all()


def test_identical_classes_on_the_host(S):
    check_identical_classes(S, "host")


@pytest.mark.parametrize("n,C,Dm", [(4, 2, 1), (127, 3, 4), (129, 8, 8), (2049, 4, 4)])
def test_drawn_cases_on_the_host(S, n, C, Dm):
    X, y, pipe, _ = drawn_case(S, n, C, Dm)
    assert pipe.predict(X).shape == (n,)


def test_arguments(G, S):
    with pytest.raises(NotImplementedError):
        S.DeviceLinearSVC(kernel="rbf")
    with pytest.raises(NotImplementedError):
        S.DeviceLinearSVC(break_ties=True)
    for bad in ({"C": 0.0}, {"C": -1.0}, {"gap_tol": 0.0}, {"backend": "cpu"}, {"class_weight": "even"}, {"decision_function_shape": "x"}):
        with pytest.raises(ValueError):
            S.DeviceLinearSVC(**bad)
    m = S.DeviceLinearSVC(tol=1e-3, max_iter=-1, random_state=3, backend="host")
    assert (m.C, m.kernel, m.decision_function_shape, m.break_ties) == (1.0, "linear", "ovr", False)
    with pytest.raises(RuntimeError):
        m.predict(G["X_te"])
    X, y = G["X_tr"][:200], G["y_tr"][:200]
    with pytest.raises(NotImplementedError):
        m.fit(np.zeros((20, 9)), np.arange(20) % 2)                     # features
    with pytest.raises(NotImplementedError):
        m.fit(np.random.default_rng(0).normal(size=(90, 2)), np.arange(90) % 9)      # classes
    with pytest.raises(ValueError):
        m.fit(X, np.zeros(200))                                        # one class
    with pytest.raises(ValueError):
        m.fit(X, y[:-1])
    Xb = X.copy()
    Xb[17, 2] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        m.fit(Xb, y)
    with pytest.raises(NotImplementedError):
        m.fit(X, y, sample_weight=np.ones(200))
    with pytest.warns(UserWarning, match="did not reach"):
        S.DeviceLinearSVC(max_iter=2, backend="host").fit(X, y)
    with pytest.raises(ValueError):
        S.DeviceLinearSVC(backend="host").fit(X, y).pair_alpha(2, 1)
    import pinn_amd
    for name in ("DeviceLinearSVC", "run_supervised_svm_rbf", "build_svm_classifier", "SVMDiagnoser", "device_extras"):
        assert callable(getattr(pinn_amd, name))
    import inspect
    assert "sklearn" not in inspect.getsource(S)                      # the package never imports scikit-learn


def test_diagnoser_chunks_on_the_host(G, S):
    pipe = S.build_svm_classifier("host").fit(G["X_tr"], G["y_tr"])
    res = np.zeros((len(G["X_te"]), 22))
    res[:, 13:17] = G["X_te"]
    d = S.SVMDiagnoser(pipe)
    got = np.concatenate([d.update(res[i:i + 100]) for i in range(0, len(res), 100)])
    assert d.n_seen == len(res) and np.array_equal(got, pipe.predict(G["X_te"]))


def test_state_layout_is_the_header_s(S):
    """Every PINN_SVM_* constant of include/pinn_hip.h has its equal in _lib.py, which is where svm.py takes them from."""
    import os
    import re
    from pinn_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pinn_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define PINN_(SVM_[A-Z_]+) (\d+)$", text, flags=re.M)}
    assert len(defs) >= 39 and {"SVM_RANGE", "SVM_P_RW", "SVM_ST_N"} <= set(defs)
    assert {k: getattr(_lib, k, None) for k in defs} == defs
    assert (S.MAX_FEAT, S.MAX_CLASSES, S._HDR, S._PW, S._P_W, S._P_BETA) == tuple(defs[k] for k in (
        "SVM_MAX_FEAT", "SVM_MAX_CLASSES", "SVM_ST_HEADER", "SVM_PAIR_WORDS", "SVM_P_W", "SVM_P_BETA"))
