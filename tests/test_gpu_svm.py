"""GPU: the device backend of pinn_amd.svm (csrc/pinn_svm.hip) against tests/golden/g_svm.npz and against the package's host
backend (float64 numpy, the same state machine).

Gates (from the problem's convexity and the number format, not from what the kernels give): gates 1-3 of
tests/test_svm_host.py on the fixture and on every drawn and named case; one row pass from a drawn interior state: every sum
within 1e-12 x the sum of its absolute terms; converged fits: |w_dev - w_host|_2 <= sqrt(2 gap_dev) + sqrt(2 gap_host) per pair
and equal predictions on every row further than eps from all pairwise boundaries.  The drawn cases are first held to the
margin condition on the host (at most 3 redraws).  Repeated fits, in-place and gathered reads, chunked diagnosis and tensor
inputs are compared bit for bit.  Every comparison prints its maxima before it asserts."""
import numpy as np
import pytest
import torch

from test_svm_host import (NAMED, OVERLAPPING, balanced, bounds_against, check_certificate, check_fixture, check_identical_classes,
                           check_named, check_predictions, decided_rows, drawn_case, host, model_wb, overlapping_case, own_decision,
                           settled_rows, svm_blobs)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(golden):
    g = golden("g_cluster.npz")
    g.update({"svm_" + k: v for k, v in golden("g_svm.npz").items()})
    return g


@pytest.fixture(scope="module")
def S():
    from pinn_amd import svm
    return svm


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_device_matches_reference_fixture(G, S):
    pipe = check_fixture(G, S, "device")
    m = pipe.named_steps["svc"]
    for a in (m.coef_, m.intercept_, m.alpha_, m.class_weight_, pipe.predict(G["X_te"])):
        assert isinstance(a, np.ndarray)
    tp = check_fixture(G, S, "device", dev)
    tm = tp.named_steps["svc"]
    for a in (tm.coef_, tm.intercept_, tm.alpha_, tm.class_weight_, tp.predict(dev(G["X_te"])), tp.decision_function(dev(G["X_te"]))):
        assert isinstance(a, torch.Tensor) and a.is_cuda
    for a, b in ((tm.coef_, m.coef_), (tm.intercept_, m.intercept_), (tm.alpha_, m.alpha_), (tp.predict(dev(G["X_te"])), pipe.predict(G["X_te"])),
                 (tp.decision_function(dev(G["X_te"]), shape="ovo"), pipe.decision_function(G["X_te"], shape="ovo"))):
        assert host(a).tobytes() == b.tobytes()                       # numpy in and tensor in: the same bytes
    # the "ovr" transform runs in torch for tensors and in numpy otherwise: a few roundings of values below 4
    assert np.abs(host(tp.decision_function(dev(G["X_te"]))) - pipe.decision_function(G["X_te"])).max() <= 1e-14
    again = S.build_svm_classifier("device").fit(G["X_tr"], G["y_tr"]).named_steps["svc"]
    assert again.alpha_.tobytes() == m.alpha_.tobytes() and again.coef_.tobytes() == m.coef_.tobytes()
    assert again.intercept_.tobytes() == m.intercept_.tobytes() and np.array_equal(again.n_iter_, m.n_iter_)
    assert np.array_equal(S.run_supervised_svm_rbf(G["X_tr"], G["y_tr"], G["X_te"], backend="device"), pipe.predict(G["X_te"]))


def test_in_place_reads_and_chunked_diagnosis(G, S):
    """Rows read in place from a 22-column array through a column list and a gather list, against the packed copy."""
    n_tr, n_te = len(G["y_tr"]), len(G["y_te"])
    rng = np.random.default_rng(5)
    res = rng.normal(size=(n_tr + n_te + 40, 22))
    where = rng.permutation(n_tr + n_te + 40)[:n_tr + n_te]
    res[where[:n_tr], 13:17], res[where[n_tr:], 13:17] = G["X_tr"], G["X_te"]
    res_d, cols = dev(res), [13, 14, 15, 16]
    packed = S.build_svm_classifier("device").fit(dev(G["X_tr"]), dev(G["y_tr"]))
    placed = S.build_svm_classifier("device").fit(res_d, dev(G["y_tr"]), columns=cols, row_index=dev(where[:n_tr]))
    a, b = packed.named_steps["svc"], placed.named_steps["svc"]
    for name in ("coef_", "intercept_", "alpha_"):
        assert host(getattr(a, name)).tobytes() == host(getattr(b, name)).tobytes(), name
    assert host(packed.named_steps["scaler"].mean_).tobytes() == host(placed.named_steps["scaler"].mean_).tobytes()
    one = packed.predict(dev(G["X_te"]))
    assert torch.equal(placed.predict(res_d, columns=cols, row_index=dev(where[n_tr:])), one)
    assert torch.equal(placed.decision_function(res_d, columns=cols, row_index=dev(where[n_tr:]), shape="ovo"),
                       packed.decision_function(dev(G["X_te"]), shape="ovo"))
    rows = dev(res[where[n_tr:]])
    d = S.SVMDiagnoser(placed)
    got = torch.cat([d.update(rows[i:i + 128]) for i in range(0, n_te, 128)])
    assert d.n_seen == n_te and torch.equal(got, one)
    h = S.SVMDiagnoser(S.build_svm_classifier("host").fit(G["X_tr"], G["y_tr"]))
    assert np.array_equal(h.update(res[where[n_tr:]]), host(one))


def test_compare_methods_on_the_device(G, S):
    from pinn_amd import comparison as P
    X, y = np.concatenate([G["X_tr"], G["X_te"]]), np.concatenate([G["y_tr"], G["y_te"]])
    n_tr = len(G["y_tr"])
    split = (np.arange(n_tr), n_tr + np.arange(len(G["y_te"])))
    with pytest.raises(NotImplementedError):
        P.compare_methods(dev(X), dev(y), methods=("Sup_SVM",), split=split, backend="device")
    r = P.compare_methods(dev(X), dev(y), methods=("Sup_LR", "Sup_SVM"), split=split, backend="device", extra=P.device_extras("device"))
    lo, hi = G["svm_acc_range"]
    e = max(abs(r["Sup_SVM"][k] - v) for k, v in zip(("accuracy", "macro_precision", "macro_recall", "macro_f1"), G["svm_svm_metrics"]))
    print("Sup_SVM on the device: accuracy %.4f (the reference's %.4f), metrics differ by %.3e (gate %.4f)"
          % (r["Sup_SVM"]["accuracy"], G["svm_svm_metrics"][0], e, hi - lo))
    assert list(r) == ["split", "Sup_LR", "Sup_SVM"] and e <= hi - lo


def against_host(S, X, y, h_pipe, cert, what, to=lambda a: a):
    """Gate 1 on the device fit and gate 4 against the host fit `h_pipe` (whose certificate is `cert`)."""
    Z, cw, c_row, w_h, b_h, gap_h, dec_h = cert
    C, hs = len(cw), h_pipe.named_steps["svc"]
    d_pipe = S.build_svm_classifier("device", C=hs.C, class_weight=hs.class_weight).fit(to(X), to(y))
    m, sc = d_pipe.named_steps["svc"], d_pipe.named_steps["scaler"]
    e_s = max(np.abs(host(sc.mean_) - h_pipe.named_steps["scaler"].mean_).max() / max(np.abs(h_pipe.named_steps["scaler"].mean_).max(), 1.0),
              np.abs(host(sc.scale_) / h_pipe.named_steps["scaler"].scale_ - 1.0).max())
    assert e_s <= 1e-12, e_s              # the worst case of sums in tile order, (128 + 1024) eps = 2.6e-13, with margin
    yi = np.searchsorted(np.unique(y), y)
    gap, _ = check_certificate(m, Z, yi, cw, m.C, what + ", device")
    w, b = model_wb(m)
    cb, ib = bounds_against(Z, yi, c_row, C, w, b, gap, w_h, b_h, h_pipe.named_steps["svc"].alpha_, gap_h, what + ", device against host")
    keep = decided_rows(Z, dec_h, cb, ib)
    check_predictions(host(d_pipe.predict(to(X))), h_pipe.predict(X), keep, what)
    return d_pipe


DRAWN = [(n, C, Dm) for n in (4, 127, 128, 129, 2049) for C in (2, 3, 4, 8) for Dm in (1, 4, 8) if n >= C]


@pytest.mark.parametrize("n,C,Dm", DRAWN)
def test_drawn_cases_against_the_host(S, n, C, Dm):
    X, y, h_pipe, cert = drawn_case(S, n, C, Dm)
    against_host(S, X, y, h_pipe, cert, "drawn %d x %d, %d classes" % (n, Dm, C))


def test_many_workgroups_against_the_host(S):
    """100003 rows: 782 workgroups' partials per sum."""
    X, y, h_pipe, cert = drawn_case(S, 100003, 3, 2)
    against_host(S, X, y, h_pipe, cert, "drawn 100003 x 2, 3 classes", dev)


# 140003 rows are 1094 tiles for 1024 workgroups: some take two tiles
@pytest.mark.parametrize("n,C,Dm", [(129, 2, 1), (2049, 4, 4), (300, 8, 8), (100003, 3, 2), (140003, 3, 2)])
def test_one_row_pass_against_the_host(S, n, C, Dm):
    """pinn_svm_pass from a drawn interior state: every sum within 1e-12 x the sum of its absolute terms."""
    X, y = svm_blobs(n, C, Dm, 31 * n + C)
    rng = np.random.default_rng(n + Dm)
    cw = balanced(y, C)
    al = rng.uniform(0.05, 0.95, (n, C - 1)) * (0.3 * cw[y])[:, None]
    s, z = rng.uniform(0.01, 3.0, (n, C - 1)), rng.uniform(0.01, 3.0, (n, C - 1))
    P = C * (C - 1) // 2
    coef, icpt = rng.normal(0.0, 1.0, (P, Dm)), rng.normal(0.0, 1.0, P)
    sc = S.DeviceStandardScaler("host").fit(X)
    mh, md = S.DeviceLinearSVC(C=0.3, class_weight="balanced", backend="host"), S.DeviceLinearSVC(C=0.3, class_weight="balanced", backend="device")
    want, scale = mh.pass_sums(X, y, al, s, z, coef, icpt, scaler=sc, want_abs=True)
    got = md.pass_sums(X, y, al, s, z, coef, icpt, scaler=sc)
    e = float(np.max(np.abs(got - want) / np.maximum(scale, 1e-300)))
    print("row pass %d x %d, %d classes: sums off by %.3e of their absolute terms (gate 1e-12)" % (n, Dm, C, e))
    assert got.shape == (P, S.n_pass_sums(Dm)) and e <= 1e-12
    res = np.zeros((n + 7, Dm + 3))
    where = rng.permutation(n + 7)[:n]
    res[where, 2:2 + Dm] = X
    placed = md.pass_sums(dev(res), y, al, s, z, coef, icpt, columns=list(range(2, 2 + Dm)), row_index=where, scaler=sc)
    assert host(placed).tobytes() == got.tobytes()


@pytest.mark.parametrize("name", NAMED)
def test_named_cases_on_the_device(S, name):
    X, y, args, h_pipe, (Z, yi, cw, c_row, w_h, b_h, gap_h) = check_named(S, name, "host")
    _, _, _, d_pipe, (_, _, _, _, w, b, gap) = check_named(S, name, "device")
    # duplicated rows and coincident classes leave alpha undetermined, and a pair without a free row its intercept: such a
    # pair has no eps, its vote counts as open on every row, and the rows that the other pairs settle are compared
    cb, ib = bounds_against(Z, yi, c_row, len(cw), w, b, gap, w_h, b_h, h_pipe.named_steps["svc"].alpha_, gap_h, name + ", device against host",
                            need_intercept=False)
    assert np.isfinite(ib).all() or name in ("duplicates", "coincident")
    dec_h, _ = own_decision(Z, w_h, b_h, len(cw))
    keep, near = settled_rows(Z, dec_h, cb, ib, len(cw))
    assert np.array_equal(keep, decided_rows(Z, dec_h, cb, ib)) or not np.isfinite(ib).all()
    check_predictions(host(d_pipe.predict(X)), h_pipe.predict(X), keep, name + ", device against host", near=near)
    check_predictions(host(d_pipe.predict(dev(X))), h_pipe.predict(X), keep, name + ", tensors in", near=near)
    assert np.isfinite(host(d_pipe.decision_function(X))).all()


@pytest.mark.parametrize("n,C", OVERLAPPING)
def test_one_feature_overlapping_against_the_host(S, n, C):
    """Bounded support vectors on one feature; the intercept has no bound there, so gate 1 and gate 2 on w."""
    Z, y, c_row, w_h, b_h, alpha_h, gap_h = overlapping_case(S, n, C, "host")
    _, _, _, w, b, _, gap = overlapping_case(S, n, C, "device")
    bounds_against(Z, y, c_row, C, w, b, gap, w_h, b_h, alpha_h, gap_h, "overlapping %d x 1, device against host" % n, need_intercept=False)


def test_identical_classes_on_the_device(S):
    check_identical_classes(S, "device")
    check_identical_classes(S, "device", dev)


def test_limits_and_bad_rows_on_the_device(G, S):
    from pinn_amd import _lib
    lib = _lib.load()
    assert lib.pinn_svm_state_bytes(100, 9, 4) == 0 and lib.pinn_svm_state_bytes(100, 4, 9) == 0 and lib.pinn_svm_workspace_bytes(100, 1, 4) == 0
    assert lib.pinn_svm_state_bytes(100, 8, 8) > 0 and lib.pinn_svm_workspace_bytes(100, 8, 8) > 0
    one = torch.zeros(64, dtype=torch.float64, device="cuda")
    cols = (_lib.c_int * 9)(*range(9))
    assert lib.pinn_svm_decision(one.data_ptr(), 9, 1, cols, 9, None, 1, 3, one.data_ptr(), None, None, None, None) == -1
    assert lib.pinn_svm_ipm(one.data_ptr(), 4, 1, cols, 4, None, 1, one.data_ptr(), 9, 1, 1, 1e-11, one.data_ptr(), one.data_ptr(), 1 << 30, None) == -1
    assert lib.pinn_svm_ipm(one.data_ptr(), 4, 1, cols, 4, None, 1, one.data_ptr(), 3, 1, 1, 1e-11, one.data_ptr(), one.data_ptr(), 8, None) == -3
    m = S.DeviceLinearSVC(backend="device")
    with pytest.raises(NotImplementedError):
        m.fit(dev(np.zeros((20, 9))), dev(np.arange(20) % 2))
    with pytest.raises(NotImplementedError):
        m.fit(dev(np.random.default_rng(0).normal(size=(90, 2))), dev(np.arange(90) % 9))
    X, y = G["X_tr"][:300].copy(), G["y_tr"][:300]
    with pytest.raises(ValueError):
        m.fit(dev(X), dev(np.zeros(300, dtype=np.int64)))
    where = np.arange(300)
    where[41] = 300                          # a gather index behind the array: the row is not read, and the fit says so
    with pytest.raises(ValueError, match="outside its range"):
        m.fit(dev(X), dev(y), row_index=dev(where))
    with pytest.raises(NotImplementedError):
        m.fit(dev(X), dev(y), trace=[])
    X[17, 2] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        m.fit(dev(X), dev(y))
