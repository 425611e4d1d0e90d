"""GPU: the device backend of pinn_amd.detection (csrc/pinn_lr.hip) against tests/golden/g_lr.npz and against the package's
host backend (float64 numpy).

Gates (from the reference, the arithmetic or the device itself, none from what the kernels give): the fixture
gates of tests/test_detection_host.py, run on the device; one row pass: every loss, gradient and Hessian sum within 1e-12 x
the sum of its absolute terms; a full fit at tol = 1e-10: max |grad F| / sum sw by the test's numpy <= tol + 1e-12 x (sum
of the absolute terms of that gradient entry) / sum sw; in-place and gathered reads, repeated calls, chunked posteriors and
the online detector bit for bit; the ROC arrays bit-equal with the rules written out in Python and the area equal to the
exact rational.  Every comparison prints its maxima before it asserts."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import test_detection_host as H
from test_detection_host import CASES, Case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(golden):
    return golden("g_lr.npz")


@pytest.fixture(scope="module")
def T():
    from pinn_amd import detection
    return detection


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if isinstance(a, np.ndarray) else a


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def synthetic(n, C, D, seed):
    rng = np.random.default_rng(seed)
    y = rng.integers(C, size=n)
    y[:C] = np.arange(C)
    X = rng.normal(size=(n, D)) * rng.uniform(0.5, 3.0, D) + 0.4 * y[:, None] * rng.normal(size=D) + rng.normal(size=D) * 5.0
    return X, y.astype(np.int64)


@pytest.mark.parametrize("name", CASES)
def test_scaler_and_counts(G, T, name):
    H.check_scaler(G, T, name, "device")
    H.check_scaler(G, T, name, "device", wrap=dev)


@pytest.mark.parametrize("name", ["b1", "f2"])
def test_reference_parameters(G, T, name):
    H.check_reference_parameters(G, T, name, "device")
    H.check_reference_parameters(G, T, name, "device", wrap=dev)


@pytest.mark.parametrize("name", CASES)
def test_default_fit_meets_the_stopping_rule(G, T, name):
    H.check_default_fit(G, T, name, "device", wrap=dev)


@pytest.mark.parametrize("name", CASES)
def test_tight_fit_against_the_tight_reference(G, T, name):
    """tol = 1e-12: the decrease of F falls below the rounding of its sum before the gradient test is met; without the
    floor in the acceptance rule this fit halves its step until it stalls."""
    clf = H.check_tight_fit(G, T, name, "device", wrap=dev)
    lr = clf.named_steps["logreg"]
    c = Case(G, T, name)
    assert isinstance(lr.coef_, torch.Tensor) and lr.coef_.is_cuda and np.array_equal(host(lr.class_count_), c.g["count"])
    clf_np = H.check_tight_fit(G, T, name, "device", chunk=1)
    assert isinstance(clf_np.named_steps["logreg"].coef_, np.ndarray)
    assert clf_np.named_steps["logreg"].coef_.tobytes() == host(lr.coef_).tobytes(), "numpy in and tensor in, chunks of 1 and 4 passes"


SHAPES = [(1, 2, 1), (127, 2, 2), (128, 5, 8), (129, 13, 4), (2049, 5, 4), (2049, 2, 8), (100003, 13, 4), (100003, 5, 8), (1000000, 2, 2)]


@pytest.mark.parametrize("n,C,D", SHAPES)
def test_one_row_pass_against_the_host(T, n, C, D):
    X, y = synthetic(max(n, C), C, D, seed=n + C + D)
    X, y = X[:n], y[:n]
    rng = np.random.default_rng(n)
    theta = rng.normal(0.0, 0.7, (C, D + 1))
    sc = T.DeviceStandardScaler(backend="host").fit(X) if n > 1 else None
    lr_h, lr_d = (T.DeviceLogisticRegression(class_weight="balanced", backend=b) for b in ("host", "device"))
    S, A = lr_h.pass_sums(X, y, theta, scaler=sc, want_abs=True)
    Sd = lr_d.pass_sums(dev(X), dev(y), theta, scaler=sc)
    assert Sd.shape == (T.n_pass_sums(C, D),) and Sd.is_cuda
    Sd = host(Sd)
    rel = np.abs(Sd - S) / np.where(A > 0, A, 1.0)
    P = C * (D + 1)
    print("n=%d C=%d D=%d: loss %.3e gradient %.3e Hessian %.3e of the sums of absolute terms (gate 1e-12)" %
          (n, C, D, rel[0], rel[1:1 + P].max(), rel[1 + P:].max()))
    assert np.all(np.isfinite(Sd)) and rel.max() <= 1e-12
    assert host(lr_d.pass_sums(dev(X), dev(y), theta, scaler=sc)).tobytes() == Sd.tobytes()


@pytest.mark.parametrize("n,C,D", [(2049, 5, 4), (100003, 2, 2), (100003, 5, 8), (2049, 13, 4)])
def test_full_fit_meets_its_tolerance(T, n, C, D):
    X, y = synthetic(n, C, D, seed=n + C)
    tol = 1e-10
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        clf = T.build_classifier(balanced=True, backend="device", tol=tol).fit(dev(X), dev(y))
    lr, sc = clf.named_steps["logreg"], clf.named_steps["scaler"]
    F, gmax, amax = H.np_objective(X, y, C, host(sc.mean_), host(sc.scale_), host(lr.coef_), host(lr.intercept_))
    print("n=%d C=%d D=%d: %d Newton iterations, %d passes, max |grad F| / sum sw = %.3e by numpy, %.3e by the device (gate %.3e)" %
          (n, C, D, lr.n_iter_, lr.n_passes_, gmax, lr.grad_max_, tol + 1e-12 * amax))
    assert lr.converged_ and lr.grad_max_ <= tol and gmax <= tol + 1e-12 * amax
    assert abs(F - lr.loss_) <= 1e-12 * abs(F)
    # against the host backend: the same minimiser
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ch = T.build_classifier(balanced=True, backend="host", tol=tol).fit(X, y)
    e = np.abs(host(lr.coef_) - ch.named_steps["logreg"].coef_).max()
    print("   coef_ device - host %.3e" % e)
    assert e <= 1e-6          # both gradients are below 1e-10 sum sw and the curvature along any direction is above 1e-4 sum sw


def test_in_place_gather_repeats_and_chunks_bit_for_bit(G, T):
    c = Case(G, T, "f2")
    res = dev(c.results)
    rows_tr, rows_te = dev(c.rows_tr), dev(c.rows_te)
    kw = dict(balanced=True, backend="device", tol=1e-10)
    a = T.build_classifier(**kw).fit(res, dev(c.y_tr), columns=c.cols, row_index=rows_tr)
    b = T.build_classifier(**kw).fit(res, dev(c.y_tr), columns=c.cols, row_index=rows_tr)
    packed = res[rows_tr][:, c.cols].contiguous()
    p = T.build_classifier(**kw).fit(packed, dev(c.y_tr))
    wide = torch.zeros(res.shape[0], 40, dtype=torch.float64, device="cuda")[:, 3:25]       # a view with a larger leading dimension
    wide.copy_(res)
    w = T.build_classifier(**kw).fit(wide, dev(c.y_tr), columns=c.cols, row_index=rows_tr)
    for other, what in ((b, "second call"), (p, "packed rows"), (w, "leading dimension 40")):
        for step, attr in (("logreg", "coef_"), ("logreg", "intercept_"), ("scaler", "mean_"), ("scaler", "scale_")):
            assert host(getattr(other.named_steps[step], attr)).tobytes() == host(getattr(a.named_steps[step], attr)).tobytes(), (what, attr)
        assert other.named_steps["logreg"].n_iter_ == a.named_steps["logreg"].n_iter_
    whole = a.predict_proba(res, columns=c.cols, row_index=rows_te)
    assert host(whole).tobytes() == host(a.predict_proba(res[rows_te][:, c.cols].contiguous())).tobytes()
    for chunk in (1, 127, 128, 500):
        parts = torch.cat([a.predict_proba(res, columns=c.cols, row_index=rows_te[i:i + chunk]) for i in range(0, len(c.rows_te), chunk)])
        assert host(parts).tobytes() == host(whole).tobytes(), chunk
    # a gather index outside the array reads nothing: NaN and -1 out, nothing added to a fit
    bad = torch.cat([rows_te[:5], torch.tensor([-1, res.shape[0]], device="cuda")])
    r = a.named_steps["logreg"]._posterior(res, c.cols, bad, a.named_steps["scaler"], 0, ("proba", "pred", "p_fault", "decision"))
    assert torch.isnan(r["proba"][5:]).all() and torch.isnan(r["p_fault"][5:]).all() and (r["pred"][5:] == -1).all()
    assert host(r["proba"][:5]).tobytes() == host(whole[:5]).tobytes()
    # the online detector: chunk by chunk, one launch each
    det = T.FaultDetector(a, features=c.cols, normal_class=0)
    rows = res[dev(c.kept)]
    outs = [det.update(rows[i:i + 333]) for i in range(0, rows.shape[0], 333)]
    proba = a.predict_proba(rows, columns=c.cols)
    assert host(torch.cat([o[0] for o in outs])).tobytes() == host(1.0 - proba[:, 0]).tobytes()
    assert torch.equal(torch.cat([o[1] for o in outs]), a.predict(rows, columns=c.cols)) and det.n_seen == rows.shape[0]


def test_far_start_rejects_a_step_and_reaches_the_same_optimum(G, T):
    H.check_far_start(G, T, "device", wrap=dev)


def test_degenerate_input(T):
    H.check_degenerate(T, "device", wrap=dev)


def test_limits(T):
    from pinn_amd import _lib
    lib = _lib.load()
    X, y = synthetic(400, 13, 5, seed=1)
    with pytest.raises(NotImplementedError):
        T.build_classifier(backend="device").fit(dev(X), dev(y))
    with pytest.raises(NotImplementedError):
        T.build_classifier(backend="device").fit(dev(np.concatenate([X, X], axis=1)[:, :9]), dev(y % 2))     # 9 features
    t = dev(X)
    cols = (ctypes.c_int * 5)(0, 1, 2, 3, 4)
    st = torch.zeros(4096, dtype=torch.float64, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    rc = lib.pinn_lr_newton(t.data_ptr(), 5, 400, cols, 5, None, 400, dev(y).data_ptr(), 13, 1, 1e-4, 1.0, 1, st.data_ptr(), ws.data_ptr(),
                            ws.numel(), None)
    assert rc == -1
    assert not st.any()
    # the largest shapes inside the limits run
    for C, D in ((13, 4), (5, 8), (7, 8)):
        Xc, yc = synthetic(3000, C, D, seed=C * D)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            lr = T.build_classifier(balanced=True, backend="device").fit(dev(Xc), dev(yc)).named_steps["logreg"]
        assert lr.converged_ and tuple(lr.coef_.shape) == (C, D)


@pytest.mark.parametrize("name", ["b1", "f2", "b3", "b4"])
def test_roc_on_the_fixture_scores(G, T, name):
    c = Case(G, T, name)
    s = H.fixture_scores(c)
    for wrap in (dev, lambda a: a):
        H.check_roc(T, c.truth, s, "device", wrap=wrap, fixture=c.g, label=name)
        H.check_roc(T, c.truth, np.round(s, 3), "device", wrap=wrap, label=name + " ties")
        H.check_roc(T, c.truth, np.full(len(s), 0.25), "device", wrap=wrap, label=name + " all equal")
        H.check_roc(T, c.truth, np.round(s - 0.5, 0), "device", wrap=wrap, label=name + " signed zeros")
    fpr, tpr, thr = T.roc_curve(dev(c.truth), dev(s), pos_label=1, drop_intermediate=False)
    assert fpr.is_cuda and len(fpr) == len(np.unique(s)) + 1 and abs(T.auc(fpr, tpr) - float(c.g["t_auc"])) <= len(fpr) * 2.0 ** -50


@pytest.mark.parametrize("n,decimals", [(1, 3), (2, 3), (255, 1), (256, 2), (256, 0), (257, 9), (65537, 2), (1000003, 3), (1000003, 12)])
def test_roc_against_the_host_backend(T, n, decimals):
    rng = np.random.default_rng(n + decimals)
    truth = (rng.random(n) < 0.3).astype(np.int64)
    truth[:2] = (0, 1)[:n]
    score = np.round(rng.normal(size=n) + 0.8 * truth, decimals)
    rh = T.roc_counts(truth, score, pos_label=1, backend="host")
    rd = T.roc_counts(dev(truth), dev(score), pos_label=1, backend="device")
    print("n=%d: %d distinct scores, %d points kept, U2 = %d" % (n, rh["n_distinct"], len(rh["fps"]), rh["U2"]))
    for k in ("n_pos", "n_neg", "n_distinct", "U2"):
        assert rd[k] == rh[k], k
    for k in ("fps", "tps", "thresholds", "fpr", "tpr"):
        assert host(rd[k]).tobytes() == np.ascontiguousarray(rh[k]).astype(host(rd[k]).dtype).tobytes(), k
    if n > 1:
        assert T.auc_score(dev(truth), dev(score), pos_label=1) == H.exact_auc(truth, score)[0]
        full = T.roc_counts(dev(truth), dev(score), pos_label=1, drop_intermediate=False)
        assert len(full["fps"]) == rh["n_distinct"] + 1


def test_evaluate_feature_groups_on_the_device(G, T):
    for name in ("b1", "b2", "f1", "f4"):
        c = Case(G, T, name)
        r = T.evaluate_feature_groups(dev(c.results), feature_groups=[",".join(str(k) for k in c.cols)], group_spec=c.spec,
                                      split=(c.idx_tr, c.idx_te), tol=1e-12)[0]
        bound = int(c.g["q"]) / (int(c.g["n_pos"]) * int(c.g["n_neg"]))
        wrong = int(np.abs(r["metrics"]["confusion_matrix"] - c.g["t_cm"]).sum())
        print("%s evaluate on the device: AUC %.6f vs %.6f (gate %.3e), confusion matrix differs by %d entries" % (name, r["auc"], c.g["t_auc"], bound, wrong))
        assert r["fpr"].is_cuda and r["p_fault"].is_cuda and torch.equal(r["kept_rows"], dev(c.kept))
        assert abs(r["auc"] - float(c.g["t_auc"])) <= bound and wrong <= 2 * round(float(c.g["close"]) * r["n_test"])
    res = T.evaluate_feature_groups(dev(Case(G, T, "b1").results))
    assert [round(r["n_test"] / (r["n_test"] + r["n_train"]), 2) for r in res] == [0.9] * 4 and all(0.5 < r["auc"] < 1.0 for r in res)
