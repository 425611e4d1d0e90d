"""CPU: the host backend of pinn_amd.ksvm (float64 numpy, the device's state machine) against tests/golden/g_ksvm.npz
(scikit-learn's RBF-kernel SVC solved to tol = 1e-12 by tools/make_golden_ksvm.py) on the split of g_cluster.npz.  The
checkers and the drawn cases are shared with tests/test_gpu_ksvm.py.

Gates (from the problem's convexity and the number format, never from what the code under test returns):
1. the certificate at the default tol: every pair converges with violation_ <= tol; primal - dual recomputed here from a
   dense numpy Gram matrix agrees with dual_gap_ to 1e-12 x the sum of the absolute terms and is <= 2 sum(c) tol (each row's
   complementarity term is at most c_i times the violation once b lies between the two bounds); |t'alpha| <= 1e-13 sum alpha;
2. in the RKHS 1/2 |w - w*|^2 <= gap and K(x, x) = 1, so the decision values without intercept of two approximate
   solutions differ by at most sqrt(2 g_1) + sqrt(2 g_2): dual_gap_ and the fixture's ref_gap, no added factor;
3. the intercept (the primal is not strictly convex in b, so there is no clean bound) within ten times the larger of
   libsvm's own agreement between tol = 1e-10 and 1e-12 and sqrt(2 ref_gap) 1e-3; predictions equal the fixture's on every
   test row whose pairwise values all exceed bound 2 plus that allowance; at most 1 % of the rows may be left out;
4. n_support_ and, on every row whose alpha the fixture has outside (1e-6 c, (1 - 1e-6) c), the supports; dual_coef_ in
   scikit-learn's layout and signs.
Every comparison prints its maxima before it asserts."""
import warnings

import numpy as np
import pytest

METRICS = ("accuracy", "macro_precision", "macro_recall", "macro_f1")


@pytest.fixture(scope="module")
def G(golden):
    g = golden("g_cluster.npz")
    g.update({"k_" + k: v for k, v in golden("g_ksvm.npz").items()})
    return g


@pytest.fixture(scope="module")
def K():
    from pinn_amd import ksvm
    return ksvm


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same(a):
    return a


def pairs_of(C):
    return [(a, b) for a in range(C) for b in range(a + 1, C)]


def balanced(y, C):
    return len(y) / (C * np.bincount(y, minlength=C).astype(np.float64))


def gram(A, B, gamma):
    return np.exp(-gamma * ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=-1))


def pair_rows(y, alpha, a, b):
    """(row positions ascending, t, alpha) of the pair."""
    idx = np.nonzero((y == a) | (y == b))[0]
    first = y[idx] == a
    return idx, np.where(first, 1.0, -1.0), np.where(first, alpha[idx, b - 1], alpha[idx, a])


def model_parts(m):
    """(alpha [n, C - 1], b [P] positive for the pair's first class, class weights) as host arrays."""
    cw = host(m.class_weight_)
    sign = -1.0 if len(cw) == 2 else 1.0
    return host(m.alpha_), sign * host(m.intercept_), cw


def check_certificate(m, Z, yi, what, tol=None):
    """Gate 1 on a fitted model; Z the standardised rows, yi class indices.  Returns the dense gaps."""
    alpha, b, cw = model_parts(m)
    C, tol = len(cw), m.tol if tol is None else tol
    assert m.converged_.all() and (m.violation_ <= tol).all(), (what, m.converged_, m.violation_)
    gaps = np.zeros(len(b))
    worst = [0.0, 0.0, 0.0]
    for p, (ca, cb) in enumerate(pairs_of(C)):
        idx, t, al = pair_rows(yi, alpha, ca, cb)
        c = m.C * cw[yi[idx]]
        assert (al >= 0).all() and (al <= c).all(), what
        Kv = gram(Z[idx], Z[idx], m.gamma_) @ (al * t)
        quad = float((al * t) @ Kv)
        hinge = float(np.sum(c * np.maximum(0.0, 1.0 - t * (Kv + b[p]))))
        gaps[p] = (0.5 * quad + hinge) - (al.sum() - 0.5 * quad)
        scale = abs(quad) + hinge + al.sum()
        worst[0] = max(worst[0], abs(gaps[p] - m.dual_gap_[p]) / scale)
        worst[1] = max(worst[1], gaps[p] / (2.0 * c.sum() * tol))
        worst[2] = max(worst[2], abs(float(np.sum(t * al))) / al.sum())
    print("%s: dual_gap_ against the dense gap %.3e of the absolute terms (gate 1e-12), gap %.3e of 2 sum(c) tol (gate 1), "
          "|t'alpha| %.3e sum alpha (gate 1e-13); violation %.3e, iterations %s"
          % (what, worst[0], worst[1], worst[2], float(np.max(m.violation_)), list(m.n_iter_)))
    assert worst[0] <= 1e-12 and worst[1] <= 1.0 and worst[2] <= 1e-13
    return gaps


def own_decision(m, Zx, yi):
    """(values [n, P], sum of the absolute terms [n, P]) from the model's public attributes, the class indices yi of the rows it
    was fitted on and a dense Gram matrix."""
    cw = host(m.class_weight_)
    C = len(cw)
    flip = -1.0 if C == 2 else 1.0
    coef, b = flip * host(m.dual_coef_).T, flip * host(m.intercept_)
    sv, sup = host(m.support_vectors_), host(m.support_)
    cls = np.asarray(yi)[sup]
    Kx = gram(Zx, sv, m.gamma_)
    dec, mag = np.zeros((len(Zx), len(b))), np.zeros((len(Zx), len(b)))
    for p, (ca, cb) in enumerate(pairs_of(C)):
        w = np.where(cls == ca, coef[:, cb - 1], 0.0) + np.where(cls == cb, coef[:, ca], 0.0)
        dec[:, p], mag[:, p] = Kx @ w + b[p], Kx @ np.abs(w) + abs(b[p])
    return dec, mag


def check_decision(m, pipe_or_model, X, Zx, yi, what, **kw):
    """decision_function against the dense computation (1e-12 x the absolute terms), votes and predict outside that distance of 0."""
    dec, mag = own_decision(m, Zx, yi)
    got = host(pipe_or_model.decision_function(X, shape="ovo", **kw))
    C = len(host(m.class_weight_))
    if C == 2:
        got = -got[:, None]
    e = float(np.max(np.abs(got - dec) / mag))
    print("%s: decision values off by %.3e of their absolute terms (gate 1e-12)" % (what, e))
    assert got.shape == dec.shape and e <= 1e-12
    keep = (np.abs(dec) > 1e-12 * mag).all(axis=1)
    votes = np.zeros((len(Zx), C), dtype=np.int64)
    for p, (ca, cb) in enumerate(pairs_of(C)):
        votes[:, ca] += dec[:, p] > 0
        votes[:, cb] += ~(dec[:, p] > 0)
    pred = host(pipe_or_model.predict(X, **kw))
    assert np.array_equal(pred[keep], host(m.classes_)[votes.argmax(axis=1)][keep]), what
    return dec, keep


def fixture_fit(K, G, backend, ci, to=same):
    return K.build_kernel_svm_classifier(backend, C=float(G["k_C"][ci])).fit(to(G["X_tr"]), to(G["y_tr"]))


def check_fixture(K, G, backend, ci, to=same):
    """Gates 1-4 at the fixture's C number ci.  Returns the pipeline."""
    what = "fixture, C = %g, %s" % (G["k_C"][ci], backend)
    pipe = fixture_fit(K, G, backend, ci, to)
    m, sc = pipe.named_steps["svc"], pipe.named_steps["scaler"]
    y = G["y_tr"]
    Z, Zt = (G["X_tr"] - host(sc.mean_)) / host(sc.scale_), (G["X_te"] - host(sc.mean_)) / host(sc.scale_)
    assert abs(m.gamma_ - G["k_gamma"][ci]) <= 1e-14 * m.gamma_
    check_certificate(m, Z, y, what)
    # gate 2
    icpt = host(m.intercept_)
    dec = host(pipe.decision_function(to(G["X_te"]), shape="ovo"))
    bound = np.sqrt(2.0 * np.maximum(m.dual_gap_, 0.0)) + np.sqrt(2.0 * G["k_ref_gap"][ci])
    d = np.abs((dec - icpt) - (G["k_dec_te"][ci] - G["k_intercept"][ci])).max(axis=0)
    print("%s: decision values without intercept differ by %s from the reference's (bounds %s)" % (what, d, bound))
    assert (d <= bound).all()
    # gate 3
    allow = 10.0 * np.maximum(G["k_intercept_agreement"][ci], np.sqrt(2.0 * G["k_ref_gap"][ci]) * 1e-3)
    di = np.abs(icpt - G["k_intercept"][ci])
    print("%s: intercepts differ by %s from the reference's (libsvm at tol 1e-10 against 1e-12: %.3e; allowed %s)"
          % (what, di, G["k_intercept_agreement"][ci], allow))
    assert (di <= allow).all()
    assert G["k_pred_checked"][ci] == 1
    keep = (np.abs(G["k_dec_te"][ci]) > (bound + allow)[None, :]).all(axis=1)
    pred = host(pipe.predict(to(G["X_te"])))
    print("%s: %d of %d test rows lie within the bounds of a boundary; predictions differ on %d of the others"
          % (what, (~keep).sum(), len(keep), (pred[keep] != G["k_pred"][ci][keep]).sum()))
    assert (~keep).mean() <= 0.01 and np.array_equal(pred[keep], G["k_pred"][ci][keep])
    # gate 4
    n, C = len(y), 4
    sup_ref = G["k_support"][ci]
    sup_ref, coef_ref = sup_ref[sup_ref >= 0], G["k_dual_coef_sup"][ci][:(sup_ref >= 0).sum()]
    a_ref, s_ref = np.zeros((n, C - 1)), np.zeros((n, C - 1))
    a_ref[sup_ref], s_ref[sup_ref] = np.abs(coef_ref), np.sign(coef_ref)
    c = (m.C * host(m.class_weight_))[y][:, None]
    at_0, at_c = a_ref <= 1e-6 * c, a_ref >= (1.0 - 1e-6) * c
    alpha = host(m.alpha_)
    assert (alpha[at_0] <= (1e-6 * c * np.ones_like(alpha))[at_0]).all() and (alpha[at_c] >= ((1.0 - 1e-6) * c * np.ones_like(alpha))[at_c]).all()
    decided = (at_0 | at_c).all(axis=1)
    is_sup = np.zeros(n, dtype=bool)
    is_sup[host(m.support_)] = True
    ref_sup = np.zeros(n, dtype=bool)
    ref_sup[sup_ref] = True
    assert np.array_equal(is_sup[decided], ref_sup[decided]) and np.array_equal(m.n_support_, G["k_n_support"][ci])
    assert (np.diff(host(m.support_)) > 0).all()
    dc = host(m.dual_coef_)
    assert dc.shape == (C - 1, len(host(m.support_))) and np.array_equal(np.abs(dc.T), alpha[host(m.support_)])
    both = is_sup & ref_sup
    mine = np.zeros((n, C - 1))
    mine[host(m.support_)] = dc.T
    big = both[:, None] & (a_ref > 1e-6 * c) & (alpha > 0)
    assert big.sum() > 100 and np.array_equal(np.sign(mine[big]), s_ref[big])
    assert np.array_equal(host(m.support_vectors_), Z[host(m.support_)]) or np.abs(host(m.support_vectors_) - Z[host(m.support_)]).max() <= 1e-12
    return pipe


# ---------------------------------------------------------------------------------------------- drawn and named cases
def blobs(m, C, D, seed, spread=1.2):
    """m rows per class around C centres, overlapping enough that bounded support vectors exist, in shuffled order."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, spread, (C, D))
    centres[:, 0] += 2.0 * rng.permutation(C)
    y = rng.permutation(np.repeat(np.arange(C), m))
    return centres[y] + rng.normal(0.0, 1.0, (len(y), D)), y.astype(np.int64)


def check_model(K, X, y, backend, what, to=same, **args):
    """Fit with a scaler, then gate 1 and the decision values against the dense computation.  Returns (pipeline, Z, yi)."""
    pipe = K.build_kernel_svm_classifier(backend, **args).fit(to(X), to(y))
    m, sc = pipe.named_steps["svc"], pipe.named_steps["scaler"]
    Z = (X - host(sc.mean_)) / host(sc.scale_)
    yi = np.searchsorted(np.unique(y), y)
    check_certificate(m, Z, yi, what)
    check_decision(m, pipe, to(X), Z, yi, what)
    return pipe, Z, yi


def all_at_bound_case():
    """Two classes of equal size on top of each other and a small C: every margin t f stays below 1, so every alpha ends at c."""
    rng = np.random.default_rng(11)
    X = rng.normal(0.0, 1.0, (12, 2))
    return X, np.arange(12) % 2


NAMED = {
    "two_classes": lambda: blobs(40, 2, 3, 1) + ({"C": 1.0},),
    "one_feature": lambda: blobs(60, 3, 1, 2) + ({"C": 0.5},),
    "eight_features": lambda: blobs(50, 3, 8, 3) + ({"C": 1.0},),
    "eight_classes": lambda: blobs(20, 8, 3, 4) + ({"C": 1.0},),
    "gamma_float": lambda: blobs(40, 3, 2, 5) + ({"C": 1.0, "gamma": 0.7},),
    "gamma_auto": lambda: blobs(40, 3, 2, 6) + ({"C": 1.0, "gamma": "auto"},),
    "dict_weights": lambda: blobs(40, 3, 2, 7) + ({"C": 1.0, "class_weight": {0: 2.0, 1: 0.5}},),
}


def one_row_class_case():
    X, y = blobs(30, 3, 2, 8)
    keep = np.concatenate([np.nonzero(y != 1)[0], np.nonzero(y == 1)[0][:1]])
    keep.sort()
    return X[keep], y[keep]


def duplicates_case():
    X, y = blobs(25, 2, 2, 9)
    X[np.nonzero(y == 1)[0][:5]] = X[np.nonzero(y == 0)[0][:5]]            # the same row in both classes of the pair
    return X, y


def check_named(K, name, backend, to=same):
    X, y, args = NAMED[name]()
    pipe, Z, yi = check_model(K, X, y, backend, name + ", " + backend, to, **args)
    m = pipe.named_steps["svc"]
    C = len(np.unique(y))
    assert len(m.n_iter_) == C * (C - 1) // 2 and host(m.alpha_).shape == (len(y), C - 1)
    if name == "eight_classes":
        assert len(m.n_iter_) == 28
    if name == "gamma_float":
        assert m.gamma_ == 0.7
    if name == "gamma_auto":
        assert m.gamma_ == 1.0 / X.shape[1]
    if name == "dict_weights":
        assert np.array_equal(host(m.class_weight_), [2.0, 0.5, 1.0])
        assert (host(m.alpha_)[yi == 1] <= 0.5).all() and host(m.alpha_)[yi == 0].max() > 1.0
    if name == "two_classes":
        # scikit-learn's convention: the value is positive for classes_[1], dual_coef_ and intercept_ are the negated pair model
        dec = host(pipe.decision_function(to(X)))
        assert dec.shape == (len(y),) and np.array_equal(host(pipe.predict(to(X))) == 1, dec >= 0)
        assert (host(m.dual_coef_)[0][yi[host(m.support_)] == 0] < 0).all() and (host(m.dual_coef_)[0][yi[host(m.support_)] == 1] > 0).all()
        assert ((host(pipe.predict(to(X))) == y).mean()) > 0.7
    return pipe, Z, yi


# ---------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("ci", [0, 1])
def test_host_matches_reference_fixture(G, K, ci):
    pipe = check_fixture(K, G, "host", ci)
    m = pipe.named_steps["svc"]
    for a in (m.support_, m.support_vectors_, m.dual_coef_, m.intercept_, m.alpha_, m.class_weight_, pipe.predict(G["X_te"])):
        assert isinstance(a, np.ndarray)
    ia, al = m.pair_alpha(1, 3)
    assert np.array_equal(ia, np.nonzero((G["y_tr"] == 1) | (G["y_tr"] == 3))[0]) and al.shape == ia.shape
    if ci == 0:
        assert np.array_equal(K.run_supervised_svm_kernel(G["X_tr"], G["y_tr"], G["X_te"], backend="host"), pipe.predict(G["X_te"]))
        ovr = pipe.decision_function(G["X_te"])
        assert ovr.shape == (len(G["y_te"]), 4) and np.array_equal(ovr.argmax(axis=1), pipe.predict(G["X_te"]))


@pytest.mark.parametrize("name", list(NAMED))
def test_named_cases(K, name):
    check_named(K, name, "host")


def test_a_class_of_one_row(K):
    X, y = one_row_class_case()
    pipe, Z, yi = check_model(K, X, y, "host", "a class of one row", C=1.0)
    assert pipe.named_steps["svc"].n_support_[1] == 1


def check_duplicates(K, backend, to=same):
    X, y = duplicates_case()
    pipe, Z, yi = check_model(K, X, y, backend, "duplicate rows, " + backend, to, C=1.0)
    return pipe, X, y


def test_duplicate_rows_take_the_tau_branch(K):
    pipe, X, y = check_duplicates(K, "host")
    trace = []
    sc = pipe.named_steps["scaler"]
    K.DeviceKernelSVC(C=1.0, class_weight="balanced", backend="host").fit(X, y, scaler=sc, trace=trace)
    hit = [e for e in trace[0] if (X[e[0]] == X[e[1]]).all()]
    assert hit, "no working set of two identical rows"


def check_all_at_bound(K, backend, to=same):
    X, y = all_at_bound_case()
    m = K.DeviceKernelSVC(C=0.01, gamma=0.5, backend=backend).fit(to(X), to(y))
    alpha, b, cw = model_parts(m)
    assert np.array_equal(alpha, np.full((12, 1), 0.01)) and m.converged_.all() and (m.n_iter_ == 6).all()
    t = np.where(y == 0, 1.0, -1.0)
    f = gram(X, X, 0.5) @ (alpha[:, 0] * t)
    assert (np.abs(f) < 0.12).all()                               # |f| <= sum alpha: every margin t (f + b) < 1 for |b| < 0.88
    tG = f - t                                                    # t G = f - t
    rho = 0.5 * (tG[t < 0].min() + tG[t > 0].max())               # all rows at c: the midpoint of libsvm's two bounds
    print("all alpha at the bound, %s: intercept %.17g, the midpoint rule gives %.17g" % (backend, b[0], -rho))
    assert abs(b[0] + rho) <= 1e-14 and (t * (f + b[0]) < 1).all()
    check_certificate(m, X, y, "all alpha at the bound, " + backend)
    return m


def test_all_alpha_at_the_bound_uses_the_midpoint(K):
    check_all_at_bound(K, "host")


def test_gamma_scale(K):
    X, y = blobs(30, 3, 4, 12)
    X = 3.0 * X + 5.0
    m = K.DeviceKernelSVC(backend="host").fit(X, y)
    assert abs(m.gamma_ * (4 * X.var()) - 1.0) <= 1e-14
    sc = K.DeviceStandardScaler(backend="host").fit(X)
    Z = (X - sc.mean_) / sc.scale_
    m = K.DeviceKernelSVC(backend="host").fit(X, y, scaler=sc)
    assert abs(m.gamma_ * (4 * Z.var()) - 1.0) <= 1e-14 and abs(m.gamma_ - 0.25) <= 1e-14


def test_max_iter_warns(K):
    X, y = blobs(40, 3, 2, 13)
    with pytest.warns(UserWarning, match="did not reach tol"):
        m = K.DeviceKernelSVC(max_iter=3, backend="host").fit(X, y)
    assert not m.converged_.any() and (m.n_iter_ == 3).all() and (m.violation_ > m.tol).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        K.DeviceKernelSVC(backend="host").fit(X, y)


def check_arguments(K, backend, to=same):
    X, y = blobs(20, 2, 2, 14)
    for bad in ({"kernel": "linear"}, {"kernel": "poly"}, {"probability": True}, {"break_ties": True}):
        with pytest.raises(NotImplementedError):
            K.DeviceKernelSVC(**bad)
    for bad in ({"gamma": -1.0}, {"gamma": "median"}, {"C": 0.0}, {"tol": 0.0}, {"chunk": 0}, {"max_iter": 0}, {"backend": "cpu"},
                {"class_weight": "even"}, {"decision_function_shape": "ovx"}):
        with pytest.raises(ValueError):
            K.DeviceKernelSVC(**bad)
    m = K.DeviceKernelSVC(backend=backend, shrinking=False, random_state=3)
    with pytest.raises(NotImplementedError):
        m.fit(to(X), to(y), sample_weight=np.ones(len(y)))
    with pytest.raises(NotImplementedError):
        m.fit(to(np.zeros((20, 9))), to(np.arange(20) % 2))
    with pytest.raises(NotImplementedError):
        m.fit(to(np.random.default_rng(0).normal(size=(90, 2))), to(np.arange(90) % 9))
    with pytest.raises(ValueError):
        m.fit(to(X), to(y[:-1]))
    with pytest.raises(ValueError):
        m.fit(to(X), to(np.zeros(len(y), dtype=np.int64)))
    with pytest.raises(RuntimeError):
        m.predict(to(X))
    Xn = X.copy()
    Xn[7, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        m.fit(to(Xn), to(y))
    m.fit(to(X), to(y))
    with pytest.raises(ValueError):
        m.predict(to(X[:, :1]))
    with pytest.raises(ValueError):
        m.pair_alpha(1, 0)


def test_arguments_and_limits(K):
    check_arguments(K, "host")


def test_compare_methods_runs_the_kernel_machine(G, K):
    from pinn_amd import comparison as P
    import pinn_amd
    assert pinn_amd.DeviceKernelSVC is K.DeviceKernelSVC and pinn_amd.kernel_extras is P.kernel_extras
    X, y = np.concatenate([G["X_tr"], G["X_te"]]), np.concatenate([G["y_tr"], G["y_te"]])
    n_tr = len(G["y_tr"])
    split = (np.arange(n_tr), n_tr + np.arange(len(G["y_te"])))
    with pytest.raises(ValueError):
        P.compare_methods(X, y, methods=("Sup_SVM_RBF",), split=split, backend="host")
    r = P.compare_methods(X, y, methods=("Sup_LR", "Sup_SVM", "Sup_SVM_RBF"), split=split, backend="host",
                          extra={**P.device_extras("host"), **P.kernel_extras("host")})
    e = max(abs(r["Sup_SVM_RBF"][k] - v) for k, v in zip(METRICS, G["k_metrics"][0]))
    print("Sup_SVM_RBF: accuracy %.4f, metrics differ by %.3e from the reference's" % (r["Sup_SVM_RBF"]["accuracy"], e))
    assert list(r) == ["split", "Sup_LR", "Sup_SVM", "Sup_SVM_RBF"] and e <= 1e-12
    assert list(G["k_metric_names"]) == list(METRICS) and P.METHODS == ("GMM", "Sup_LR", "KMeans", "Agglo")


def test_online_diagnoser_on_the_host(G, K):
    n_te = len(G["y_te"])
    res = np.zeros((n_te, 22))
    pipe = fixture_fit(K, G, "host", 1)
    d = K.KernelSVMDiagnoser(pipe, features=[13, 14, 15, 16])
    res[:, 13:17] = G["X_te"]
    got = np.concatenate([d.update(res[i:i + 128]) for i in range(0, n_te, 128)])
    assert d.n_seen == n_te and np.array_equal(got, pipe.predict(G["X_te"]))


def test_state_layout_is_the_header_s(K):
    """Every PINN_KSVM_* constant of include/pinn_hip.h has its equal in _lib.py, which is where ksvm.py takes them from."""
    import os
    import re
    from pinn_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pinn_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define PINN_(KSVM_[A-Z_]+) (\d+)\b", text, flags=re.M)}
    assert len(defs) == 24 and {"KSVM_RANGE", "KSVM_P_VIOLATION", "KSVM_SV_TILE"} <= set(defs)
    assert {k: getattr(_lib, k, None) for k in defs} == defs
    assert (K.MAX_FEAT, K.MAX_CLASSES, K._HDR, K._PW, K.SV_TILE) == tuple(defs[k] for k in (
        "KSVM_MAX_FEAT", "KSVM_MAX_CLASSES", "KSVM_ST_HEADER", "KSVM_PAIR_WORDS", "KSVM_SV_TILE"))
