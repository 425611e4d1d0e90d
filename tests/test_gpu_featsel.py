"""GPU: the device backend of pinn_amd.featsel (the pinn_lr_batch_* entry points of csrc/pinn_lr.hip) against the single
device fit (bytes), against itself in other batches (bytes) and against the host backend.

Gates, none from what the kernels give: a candidate is the single device fit, so its parameters, scaler and p_fault are
compared byte for byte and its integers exactly; the validation log-loss is a sum of positive terms in a fixed order, held to
1e-12 x the sum of its absolute terms (the gate of a loss sum in test_gpu_detection.py); device against host at tol = 1e-10
within 1e-6 in the coefficients, the gate of test_full_fit_meets_its_tolerance and for its reason (both gradients are below
1e-10 sum sw and the curvature along any direction is above 1e-4 sum sw).  Every comparison prints its maxima before it
asserts."""
import warnings

import numpy as np
import pytest
import torch

import featsel_cases as K

pytestmark = pytest.mark.gpu

COLS8 = (11, 0, 3, 12, 8, 1, 2, 4)
PARTS = (("logreg", "coef_"), ("logreg", "intercept_"), ("scaler", "mean_"), ("scaler", "scale_"))


@pytest.fixture(scope="module")
def F():
    from pinn_amd import featsel
    return featsel


@pytest.fixture(scope="module")
def T():
    from pinn_amd import detection
    return detection


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def gather_split(n_rows, n_train, n_val, seed):
    """Positions with repeats: the first 13 train (and the next 13 validation) positions carry every label."""
    rng = np.random.default_rng(seed)
    tr = np.concatenate([np.arange(13), rng.integers(0, n_rows, n_train - 13)]).astype(np.int64)
    va = np.concatenate([np.arange(13, 26), rng.integers(0, n_rows, n_val - 13)]).astype(np.int64)
    return tr, va


def single_fit(T, A_dev, A, C, cols, idx_tr, **kw):
    y = K.class_of(A[:, K.LABEL], C)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return T.build_classifier(balanced=True, backend="device", **kw).fit(A_dev, dev(y[idx_tr]), columns=list(cols), row_index=dev(idx_tr))


def assert_same_model(m, one, what):
    for step, attr in PARTS:
        assert host(getattr(m.named_steps[step], attr)).tobytes() == host(getattr(one.named_steps[step], attr)).tobytes(), (what, attr)
    a, b = m.named_steps["logreg"], one.named_steps["logreg"]
    assert (a.n_iter_, a.n_passes_, a.loss_, a.grad_max_, a.converged_) == (b.n_iter_, b.n_passes_, b.loss_, b.grad_max_, b.converged_), what


def fingerprint(sw, i):
    m = sw.model(i)
    return tuple(host(getattr(m.named_steps[s], a)).tobytes() for s, a in PARTS) + (
        int(sw.n_iter[i]), int(sw.n_passes[i]), float(sw.loss[i]).hex(), float(sw.grad_max[i]).hex(), float(sw.val_logloss[i]).hex(),
        int(sw.val_hits[i]), int(sw.val_U2[i]), int(sw.n_pos[i]), int(sw.n_neg[i]), host(sw.val_p_fault[i]).tobytes())


@pytest.mark.parametrize("n,C,D", [(127, 2, 1), (129, 2, 8), (2049, 5, 8), (2049, 13, 4)])
def test_a_batch_of_one_is_the_single_device_fit(F, T, n, C, D):
    A = K.results_array(900, n + C + D)
    A_dev = dev(A)
    cols = COLS8[:D]
    idx_tr, idx_va = gather_split(900, n, 301, seed=n)
    sw = F.feature_sweep(A_dev, [cols], group_spec=K.SPECS[C], split=(idx_tr, idx_va), backend="device")
    one = single_fit(T, A_dev, A, C, cols, idx_tr)
    lr = one.named_steps["logreg"]
    print("n=%d C=%d D=%d: %d iterations, %d passes, F = %.6f, status %d" % (n, C, D, lr.n_iter_, lr.n_passes_, lr.loss_, sw.status[0]))
    assert sw.status[0] == 0 and sw.n_train == n
    m = sw.model(0)
    assert isinstance(m.named_steps["logreg"].coef_, torch.Tensor)
    assert_same_model(m, one, (n, C, D))
    assert (sw.n_iter[0], sw.n_passes[0], sw.loss[0], sw.grad_max[0]) == (lr.n_iter_, lr.n_passes_, lr.loss_, lr.grad_max_)
    assert np.array_equal(host(m.classes_), host(one.classes_))
    assert m.named_steps["scaler"].n_samples_seen_ == one.named_steps["scaler"].n_samples_seen_ == n


def test_a_candidate_does_not_depend_on_its_batch(F):
    A = K.results_array(700, 11)
    A_dev = dev(A)
    split = K.split_of(700, 1)
    subsets = F.feature_subsets(K.POOL5, 1, 3)
    kw = dict(group_spec=K.BINARY, split=split, backend="device", keep_p_fault=True)
    sw = F.feature_sweep(A_dev, subsets, **kw)
    iters = sorted(set(sw.n_iter.tolist()))
    print("25 candidates, sizes %s, iterations %s, passes %s" % (sorted(set(sw.n_features.tolist())), iters, sorted(set(sw.n_passes.tolist()))))
    assert (sw.status == 0).all() and sw.converged.all()
    assert len(iters) >= 2                                 # some candidates stop while the others go on
    whole = [fingerprint(sw, i) for i in range(25)]
    again = F.feature_sweep(A_dev, subsets, **kw)
    assert [fingerprint(again, i) for i in range(25)] == whole, "the same call twice"
    rev = F.feature_sweep(A_dev, subsets[::-1], **kw)
    assert [fingerprint(rev, 24 - i) for i in range(25)] == whole, "the batch in reversed order"
    for i, cols in enumerate(subsets):
        alone = F.feature_sweep(A_dev, [cols], **kw)
        assert fingerprint(alone, 0) == whole[i], ("alone", cols)
    hs = F.feature_sweep(A, subsets, group_spec=K.BINARY, split=split, backend="host")
    assert sw.n_iter.tolist() == hs.n_iter.tolist(), "the host backend shows the same iteration counts"


def test_more_than_1024_tiles(F, T):
    n = 131073 + 5
    A = K.results_array(3000, 4)
    A_dev = dev(A)
    idx_tr, idx_va = gather_split(3000, n, 300, seed=3)
    subsets = [(11,), (0, 3, 12), tuple(COLS8)]
    sw = F.feature_sweep(A_dev, subsets, group_spec=K.FIVE, split=(idx_tr, idx_va), backend="device")
    print("n = %d (%d tiles): iterations %s, passes %s" % (n, (n + 127) // 128, sw.n_iter.tolist(), sw.n_passes.tolist()))
    assert (sw.status == 0).all()
    for i, cols in enumerate(subsets):
        assert_same_model(sw.model(i), single_fit(T, A_dev, A, 5, cols, idx_tr), cols)


@pytest.mark.parametrize("C", [2, 5])
def test_scores_of_the_validation_rows(F, T, C):
    A = K.results_array(900, 21)
    A_dev = dev(A)
    idx_tr, idx_va = gather_split(900, 500, 333, seed=C)          # 333 validation rows: two tiles and a part of one
    subsets = [(K.TIED,), (0, 3), (11, 12, 8), (K.TIED, 11), tuple(COLS8)]
    sw = F.feature_sweep(A_dev, subsets, group_spec=K.SPECS[C], split=(idx_tr, idx_va), backend="device", keep_p_fault=True)
    y_va = K.class_of(A[idx_va, K.LABEL], C)
    truth = y_va != 0
    assert sw.val_p_fault.is_cuda and tuple(sw.val_p_fault.shape) == (5, 333) and sw.n_val == 333
    for i, cols in enumerate(subsets):
        m = sw.model(i)
        pf, pred = m.p_fault(A_dev, 0, columns=list(cols), row_index=dev(idx_va), with_pred=True)
        assert host(sw.val_p_fault[i]).tobytes() == host(pf).tobytes(), (cols, "p_fault bytes")
        hits = int((host(pred) == y_va).sum())
        r = T.roc_counts(truth, host(pf), pos_label=True, backend="host", curve=False)
        proba = host(m.predict_proba(A_dev, columns=list(cols), row_index=dev(idx_va)))
        terms = -np.log(proba[np.arange(333), y_va])
        err = abs(sw.val_logloss[i] * 333 - terms.sum())
        print("C=%d %s: hits %d, U2 %d (%d distinct scores), n_pos %d, log-loss sum off by %.3e (gate %.3e)" %
              (C, cols, hits, r["U2"], r["n_distinct"], r["n_pos"], err, 1e-12 * np.abs(terms).sum()))
        assert sw.val_hits[i] == hits and (sw.val_U2[i], sw.n_pos[i], sw.n_neg[i]) == (r["U2"], r["n_pos"], r["n_neg"])
        rd = T.roc_counts(dev(truth), pf, pos_label=True, backend="device", curve=False)
        assert (rd["U2"], rd["n_pos"], rd["n_neg"]) == (r["U2"], r["n_pos"], r["n_neg"])
        assert err <= 1e-12 * np.abs(terms).sum()
        assert sw.val_auc[i] == r["U2"] / (2 * r["n_pos"] * r["n_neg"])
        if cols == (K.TIED,):
            assert r["n_distinct"] == 2


def test_device_sweep_against_host_sweep(F):
    A = K.results_array(700, 11)
    split = K.split_of(700, 1)
    subsets = F.feature_subsets(K.POOL5, 1, 3)
    for C in (2, 5):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            d = F.feature_sweep(dev(A), subsets, group_spec=K.SPECS[C], split=split, backend="device", tol=1e-10)
            h = F.feature_sweep(A, subsets, group_spec=K.SPECS[C], split=split, backend="host", tol=1e-10)
        e = max(np.abs(host(d.model(i).named_steps["logreg"].coef_) - h.model(i).named_steps["logreg"].coef_).max() for i in range(25))
        ea = np.abs(d.val_auc - h.val_auc).max()
        print("C=%d: coef_ device - host %.3e (gate 1e-6), val_auc differs by at most %.3e, hits differ in %d candidates" %
              (C, e, ea, int((d.val_hits != h.val_hits).sum())))
        assert d.converged.all() and h.converged.all() and e <= 1e-6
    P = K.planted()
    ps = F.feature_subsets(K.PLANTED_POOL, 1, 2)
    d = F.feature_sweep(P, ps, test_size=K.PLANTED_TEST_SIZE, backend="device", tol=1e-10)
    h = F.feature_sweep(P, ps, test_size=K.PLANTED_TEST_SIZE, backend="host", tol=1e-10)
    print("planted: best by AUC %s / %s, by log-loss %s / %s" % (d.features[d.best("val_auc")], h.features[h.best("val_auc")],
                                                               d.features[d.best("val_logloss")], h.features[h.best("val_logloss")]))
    assert isinstance(d.model(0).named_steps["logreg"].coef_, np.ndarray)               # numpy in, numpy out
    for crit in ("val_auc", "val_logloss"):
        assert d.best(crit) == h.best(crit) and d.features[d.best(crit)] == K.PLANTED_PAIR
    clf, _ = F.select_features(dev(P), ps, test_size=K.PLANTED_TEST_SIZE, backend="device", tol=1e-10)
    assert host(clf.named_steps["logreg"].coef_).tobytes() == d.model(d.best()).named_steps["logreg"].coef_.tobytes()
    path = F.forward_select(dev(P), K.PLANTED_POOL, 2, test_size=K.PLANTED_TEST_SIZE, backend="device")
    assert set(path.selected) == set(K.PLANTED_PAIR) and len(path.sweeps) == 2


def test_a_split_sweep_gives_the_bytes_of_the_unsplit_one(F):
    from pinn_amd import _lib
    lib = _lib.load()
    A = K.results_array(700, 11)
    A_dev = dev(A)
    split = K.split_of(700, 1)
    subsets = F.feature_subsets(K.POOL5, 1, 3)
    kw = dict(group_spec=K.FIVE, split=split, backend="device", keep_p_fault=True)
    whole = F.feature_sweep(A_dev, subsets, **kw)
    per = lib.pinn_lr_batch_workspace_bytes(max(len(split[0]), len(split[1])), 1, 5, 3)
    budget = 4 * per + 100
    print("workspace of one candidate %d bytes, budget %d: batches of %d, scoring groups of %d" %
          (per, budget, budget // per, max(1, budget // (48 * len(split[1])))))
    assert budget // per == 4 and budget // (48 * len(split[1])) < 4
    parts = F.feature_sweep(A_dev, subsets, ws_budget=budget, **kw)
    assert [fingerprint(parts, i) for i in range(25)] == [fingerprint(whole, i) for i in range(25)]


def test_a_column_outside_the_array_in_the_device_copy_reads_nothing():
    """The host checks the host copy of the column lists; the kernels read the device copy.  A column outside [0, ld) there
    makes that candidate's rows read nothing (no row is counted), and leaves the other candidate's bytes alone."""
    import ctypes
    from pinn_amd import _lib
    lib = _lib.load()
    n, C, Dm, B = 300, 2, 2, 2
    A = K.results_array(n, 2)
    A_dev, y = dev(A), dev(K.class_of(A[:, K.LABEL], C))
    stride = lib.pinn_lr_batch_state_stride(C, Dm) // 8
    wb = lib.pinn_lr_batch_workspace_bytes(n, B, C, Dm)
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    n_feat, cols = (ctypes.c_int * 2)(2, 2), (ctypes.c_int * 4)(0, 3, 11, 12)
    d_n_feat = torch.tensor([2, 2], dtype=torch.int32, device="cuda")

    def scaler(device_cols):
        st = torch.zeros(B, stride, dtype=torch.float64, device="cuda")
        d_cols = torch.tensor(device_cols, dtype=torch.int32, device="cuda")
        rc = lib.pinn_lr_batch_scaler(A_dev.data_ptr(), 22, n, None, n, y.data_ptr(), C, B, n_feat, cols, Dm, d_n_feat.data_ptr(), d_cols.data_ptr(), 1,
                                      st.data_ptr(), ws.data_ptr(), wb, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        return st.cpu().numpy()
    good = scaler([0, 3, 11, 12])
    seen = [int(good[c, :16].view(np.int64)[_lib.LR_ST_NSEEN]) for c in range(B)]
    assert seen == [n, n]
    for bad_cols in ([0, 3, 11, 22], [0, 3, -1, 12], [0, 3, 11, 1 << 30]):
        bad = scaler(bad_cols)
        seen = [int(bad[c, :16].view(np.int64)[_lib.LR_ST_NSEEN]) for c in range(B)]
        print("device columns %s: rows seen %s" % (bad_cols, seen))
        assert seen == [n, 0] and bad[0].tobytes() == good[0].tobytes() and np.isfinite(bad[1]).all()
