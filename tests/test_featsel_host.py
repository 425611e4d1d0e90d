"""CPU: the host backend of pinn_amd.featsel (the loop of host fits, float64 numpy) and everything around the sweep that
does not need a device: the subsets, the shared row set, the counts behind the validation scores, `best`, and a planted
signal that the sweep and the greedy search must find.  Every comparison prints its maxima before it asserts."""
import warnings

import numpy as np
import pytest

import featsel_cases as K


@pytest.fixture(scope="module")
def F():
    from pinn_amd import featsel
    return featsel


@pytest.fixture(scope="module")
def T():
    from pinn_amd import detection
    return detection


def test_exported_from_the_package(F):
    import pinn_amd
    for name in ("feature_subsets", "feature_sweep", "select_features", "forward_select", "FeatureSweep"):
        assert getattr(pinn_amd, name) is getattr(F, name)


def test_feature_subsets_order_counts_and_limits(F):
    s = F.feature_subsets(K.POOL5, 1, 3)
    print("pool of 5, sizes 1..3: %d subsets" % len(s))
    assert len(s) == 25 and [len(t) for t in s] == [1] * 5 + [2] * 10 + [3] * 10
    assert s[:5] == [(0,), (3,), (11,), (12,), (8,)]                       # pool order, not column order
    assert s[5:9] == [(0, 3), (0, 11), (0, 12), (0, 8)] and s[14] == (12, 8) and s[15] == (0, 3, 11) and s[-1] == (11, 12, 8)
    assert F.feature_subsets("x0,x3,epi,res,y_true", 1, 3) == s             # names through detection.parse_features
    assert F.feature_subsets(["x0", 3, "epi", "res", 8], 1, 3) == s
    m = F.feature_subsets(K.POOL5, 1, 3, must_include=("epi",))
    assert m == [t for t in s if 11 in t] and len(m) == 1 + 4 + 6
    assert F.feature_subsets(K.POOL5, 2, 3, must_include=(11, "x0")) == [t for t in s if 11 in t and 0 in t]
    assert len(F.feature_subsets(range(17), 1, 3)) == 833 and len(F.feature_subsets(range(17), 1, 4)) == 3213
    assert len(F.feature_subsets(range(9), 8, 8)) == 9
    with pytest.raises(ValueError):
        F.feature_subsets(range(17), 1, 9)
    with pytest.raises(ValueError):
        F.feature_subsets(K.POOL5, 1, 2, must_include=("x7",))
    with pytest.raises(KeyError):
        F.feature_subsets(("x0", "nonsense"))


@pytest.mark.parametrize("C", [2, 5])
def test_a_host_candidate_is_the_single_host_fit(F, T, C):
    A = K.results_array(700, 11)
    split = K.split_of(700, 1)
    subsets = F.feature_subsets(K.POOL5, 1, 3)
    sw = F.feature_sweep(A, subsets, group_spec=K.SPECS[C], split=split, backend="host")
    y = K.class_of(A[:, K.LABEL], C)
    assert sw.features == subsets and sw.n_train == len(split[0]) and sw.n_val == len(split[1]) and len(sw) == 25
    for i, cols in enumerate(subsets):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            one = T.build_classifier(balanced=True, backend="host").fit(A, y[split[0]], columns=list(cols), row_index=split[0])
        m = sw.model(i)
        for step, attr in (("logreg", "coef_"), ("logreg", "intercept_"), ("scaler", "mean_"), ("scaler", "scale_")):
            assert getattr(m.named_steps[step], attr).tobytes() == getattr(one.named_steps[step], attr).tobytes(), (cols, attr)
        lr = one.named_steps["logreg"]
        assert (sw.n_iter[i], sw.n_passes[i], sw.loss[i], sw.grad_max[i], bool(sw.converged[i])) == \
               (lr.n_iter_, lr.n_passes_, lr.loss_, lr.grad_max_, lr.converged_)
    print("C=%d: 25 candidates equal their single fits; iterations %s" % (C, sorted(set(sw.n_iter.tolist()))))
    assert len(set(sw.n_iter.tolist())) >= 2          # the data of the device test "a candidate does not depend on its batch"


def test_all_candidates_share_one_row_set(F):
    A = K.results_array(400, 5)
    A[30, 12] = np.nan                   # res: named by one subset only
    A[31, 0] = np.inf
    A[32, 4] = np.nan                    # x4: named by no subset
    A[33, K.LABEL] = 40                  # a label outside the spec
    A[34, K.LABEL] = np.nan
    sw = F.feature_sweep(A, [(0,), (3, 11), (12,)], backend="host", test_size=0.5)
    kept = np.asarray(sw.kept_rows)
    print("kept %d of 400 rows" % len(kept))
    assert sorted(set(range(400)) - set(kept.tolist())) == [30, 31, 33, 34]
    assert sw.n_train + sw.n_val == 396 and sw.model(0).named_steps["scaler"].n_samples_seen_ == sw.n_train
    five = F.feature_sweep(A, [(0,), (3, 11)], group_spec="normal:0 | flooding:1,2,3", backend="host", test_size=0.5)
    lab = A[:, K.LABEL]
    want = np.flatnonzero(np.isin(lab, [0, 1, 2, 3]) & np.isfinite(A[:, [0, 3, 11]]).all(axis=1))
    assert np.array_equal(np.asarray(five.kept_rows), want) and five.class_names == ["normal", "flooding"]


@pytest.mark.parametrize("C", [2, 5])
def test_validation_counts_against_the_model_itself(F, T, C):
    A = K.results_array(700, 11)
    split = K.split_of(700, 2, frac=0.4)
    subsets = [(K.TIED,), (0, 3), (11, 12, 8), (K.TIED, 11)]
    sw = F.feature_sweep(A, subsets, group_spec=K.SPECS[C], split=split, backend="host")
    y_va = K.class_of(A[split[1], K.LABEL], C)
    for i, cols in enumerate(subsets):
        m = sw.model(i)
        pred = m.predict(A, columns=list(cols), row_index=split[1])
        pf = m.p_fault(A, 0, columns=list(cols), row_index=split[1])
        proba = m.predict_proba(A, columns=list(cols), row_index=split[1])
        r = T.roc_counts(y_va != 0, pf, pos_label=True, backend="host", curve=False)
        ll = -np.log(proba[np.arange(len(y_va)), y_va]).mean()
        print("C=%d %s: hits %d, U2 %d, %d distinct scores of %d, log-loss %.6f, AUC %.6f (by pairs %.6f)" %
              (C, cols, sw.val_hits[i], sw.val_U2[i], r["n_distinct"], len(pf), sw.val_logloss[i], sw.val_auc[i], K.auc_of(y_va != 0, pf)))
        assert sw.val_hits[i] == int((pred == y_va).sum()) and sw.val_accuracy[i] == sw.val_hits[i] / len(y_va)
        assert (sw.val_U2[i], sw.n_pos[i], sw.n_neg[i]) == (r["U2"], r["n_pos"], r["n_neg"])
        assert sw.n_pos[i] == int((y_va != 0).sum()) and sw.n_pos[i] + sw.n_neg[i] == len(y_va)
        assert sw.val_auc[i] == r["U2"] / (2 * r["n_pos"] * r["n_neg"]) and abs(sw.val_auc[i] - K.auc_of(y_va != 0, pf)) <= 1e-12
        assert abs(sw.val_logloss[i] - ll) <= 1e-12 * abs(ll)
        if cols == (K.TIED,):
            assert r["n_distinct"] == 2
    assert sw.val_hits.dtype == np.int64 and sw.val_U2.dtype == np.int64


def _sweep_with(F, **arrays):
    n = len(next(iter(arrays.values())))
    sw = F.FeatureSweep([(k,) for k in range(n)], "host")
    sw.n_val = 100
    sw.val_hits = np.zeros(n, np.int64)
    sw._finish()
    for k, v in arrays.items():
        setattr(sw, k, np.asarray(v))
    return sw


def test_best_direction_ties_and_failures(F):
    sw = _sweep_with(F, val_auc=[0.7, 0.9, 0.9, 0.8], val_accuracy=[0.5, 0.6, 0.7, 0.7], val_logloss=[0.4, 0.3, 0.2, 0.2],
                     loss=[5.0, 3.0, 4.0, 3.0], status=[0, 0, 0, 0])
    assert (sw.best("val_auc"), sw.best("val_accuracy"), sw.best("val_logloss"), sw.best("loss")) == (1, 2, 2, 1)
    assert sw.best() == 1
    # a failed candidate is left out, a stalled one takes part
    sw = _sweep_with(F, val_auc=[0.7, 0.99, 0.9, 0.95], val_logloss=[0.4, 0.01, 0.2, 0.1], val_accuracy=[0.1] * 4, loss=[1.0] * 4,
                     status=[0, F.SINGULAR, F.STALLED, F.NAN])
    assert sw.best("val_auc") == 2 and sw.best("val_logloss") == 2
    assert [r["index"] for r in sw.table(top=None, criterion="val_auc")] == [2, 0]
    sw = _sweep_with(F, val_auc=[np.nan, 0.6], val_accuracy=[0.1] * 2, val_logloss=[0.1] * 2, loss=[1.0] * 2, status=[0, 0])
    assert sw.best("val_auc") == 1
    with pytest.raises(ValueError):
        sw.best("bic")
    with pytest.raises(ValueError):
        _sweep_with(F, val_auc=[0.5], val_accuracy=[0.5], val_logloss=[0.5], loss=[0.5], status=[F.NAN]).best("val_auc")


def test_a_failed_candidate_is_reported_not_raised(F):
    """A column of 1e200 overflows the variance: the standardised values are not finite and the single fit raises."""
    A = K.results_array(300, 3)
    A[:, 6] = 1e200 * (1.0 + np.arange(300) % 7)
    sw = F.feature_sweep(A, [(0,), (6,), (0, 3)], backend="host", test_size=0.5)
    print("status %s" % sw.status.tolist())
    assert sw.status[1] in (F.SINGULAR, F.NAN) and sw.status[0] == 0 and sw.status[2] == 0
    assert np.isnan(sw.val_auc[1]) and np.isnan(sw.loss[1]) and np.isnan(sw.val_logloss[1]) and np.isnan(sw.val_accuracy[1])
    with pytest.raises(ValueError, match="logistic regression failed"):
        sw.model(1)
    assert sw.best("val_auc") in (0, 2)


def test_planted_signal_is_found(F):
    """600 rows, the labels drawn from a logistic model on (epi - x3); pool of 6, sizes <= 2 (21 candidates), half the
    rows validate.  Measured on the CPU with the host backend (seed 3, strength 6, a = 0.2): the planted pair has
    validation AUC 0.9729 against 0.5862 of the runner-up, 11.4 bootstrap standard errors of the paired difference, and
    its log-loss leads the runner-up's by 23.5 standard errors.  The gate is ten."""
    A = K.planted()
    subsets = F.feature_subsets(K.PLANTED_POOL, 1, 2)
    assert len(subsets) == 21
    sw = F.feature_sweep(A, subsets, test_size=K.PLANTED_TEST_SIZE, backend="host")
    assert sw.features[sw.best("val_logloss")] == K.PLANTED_PAIR and sw.features[sw.best("val_auc")] == K.PLANTED_PAIR
    best = sw.best("val_auc")
    rows = np.asarray(sw.kept_rows)[sw.idx_val]
    truth = A[rows, K.LABEL] > 0

    def post(i):
        m, cols = sw.model(i), list(sw.features[i])
        return m.p_fault(A, 0, columns=cols, row_index=rows), m.predict_proba(A, columns=cols, row_index=rows)
    ru_auc = [i for i in np.argsort(-sw.val_auc, kind="stable") if i != best][0]
    ru_ll = [i for i in np.argsort(sw.val_logloss, kind="stable") if i != best][0]
    (pa, qa), (pb, qb), (pc, qc) = post(best), post(ru_auc), post(ru_ll)
    m_auc = K.bootstrap_margin(truth, truth.astype(np.int64), pa, pb, qa, qb)[0]
    m_ll = K.bootstrap_margin(truth, truth.astype(np.int64), pa, pc, qa, qc)[1]
    print("planted pair: AUC %.4f vs %.4f of %s: %.1f standard errors; log-loss %.4f vs %.4f of %s: %.1f standard errors (gate 10)" %
          (sw.val_auc[best], sw.val_auc[ru_auc], sw.features[ru_auc], m_auc, sw.val_logloss[best], sw.val_logloss[ru_ll], sw.features[ru_ll], m_ll))
    assert m_auc >= 10.0 and m_ll >= 10.0
    clf, sw2 = F.select_features(A, subsets, criterion="val_logloss", test_size=K.PLANTED_TEST_SIZE, backend="host")
    assert clf.named_steps["logreg"].coef_.tobytes() == sw.model(best).named_steps["logreg"].coef_.tobytes()
    path = F.forward_select(A, K.PLANTED_POOL, 2, test_size=K.PLANTED_TEST_SIZE, backend="host")
    print("forward selection: %s, scores %s" % (path.sets, path.scores))
    assert len(path.sets) == 2 and len(path.sweeps) == 2 and set(path.selected) == set(K.PLANTED_PAIR)
    assert path.scores[1] == sw.val_auc[best] or abs(path.scores[1] - sw.val_auc[best]) < 0.01      # the same columns in the other order
    # with room for a third column the search stops by itself: noise adds nothing worth min_gain
    longer = F.forward_select(A, K.PLANTED_POOL, 4, min_gain=0.01, test_size=K.PLANTED_TEST_SIZE, backend="host")
    assert set(longer.selected) == set(K.PLANTED_PAIR) and len(longer.sweeps) == 3


def test_arguments(F):
    A = K.results_array(200, 1)
    with pytest.raises(ValueError):
        F.feature_sweep(A, [], backend="host")
    with pytest.raises(ValueError):
        F.feature_sweep(A, [tuple(range(9))], backend="host")
    with pytest.raises(ValueError):
        F.feature_sweep(A, [(0,)], backend="host", coef_init=np.zeros((2, 1)))
    with pytest.raises(ValueError):
        F.feature_sweep(A, [(0,)], backend="host", chunk=0)
    with pytest.raises(ValueError):
        F.forward_select(A, K.POOL5, 9, backend="host")
    sw = F.feature_sweep(A, ["x0,x3", (11,)], backend="host", test_size=0.5, tol=1e-8, C=0.5)
    assert sw.features == [(0, 3), (11,)] and sw.model(0).named_steps["logreg"].C == 0.5
    rows = sw.table(top=1)
    assert len(rows) == 1 and rows[0]["index"] == sw.best() and rows[0]["names"] == sw.names(sw.best())
