"""Generate tests/golden/g_svm.npz: scikit-learn's linear SVC as script 05 runs it, on the split of tests/golden/g_cluster.npz.

Build machine only: needs scikit-learn, and for the predictions at libsvm's default tolerance a checkout of the reference
(`--reference DIR`, as tools/make_golden_cluster.py: script 05's `run_supervised_svm_rbf` is called, its text is not read
into this file).  No test imports this file.  The fixture holds arrays only, and not the rows: the tests take `X_tr`, `y_tr`,
`X_te`, `y_te` from g_cluster.npz.  Per pair (scikit-learn's order) of `StandardScaler` + `SVC(kernel="linear", C=0.05,
class_weight="balanced", tol=1e-12)`: `coef`, `intercept`, `alpha` ([n_tr, 3]: |dual_coef_| scattered to the rows, slot j of a
row its j-th other class in increasing order, which is dual_coef_'s own layout), the one-vs-one decision values of the test
rows, `pred_tight` (tol=1e-12) and `pred_default` (script 05's call), the reference's own duality gap `ref_gap` =
primal(coef_, intercept_) - dual(alpha) and `ref_primal`, evaluated here in float64, the scaler's `mean` and `scale`, the class
weights, and the metrics of g_cluster.npz's `six_metrics` row of Sup_SVM with its `acc_range`.

Conditions asserted here: libsvm at tol=1e-10 and 1e-12 agree to 1e-8 in coef_; the tight and the default run predict the
same class on every test row; at most 1 % of the test rows have a pairwise decision value below 1e-3 in magnitude and none
below 1e-6.
"""
import argparse
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "g_svm.npz")
C_PEN = 0.05


def pair_objectives(Z, y, cw, a, b, w, beta, alpha):
    """(primal, dual) of the pair (a, b) in float64: alpha [n, C - 1] in the slot layout."""
    ia, ib = np.nonzero(y == a)[0], np.nonzero(y == b)[0]
    idx = np.concatenate([ia, ib])
    t = np.concatenate([np.ones(len(ia)), -np.ones(len(ib))])
    al = np.concatenate([alpha[ia, b - 1], alpha[ib, a]])
    c = C_PEN * cw[y[idx]]
    f = Z[idx] @ w + beta
    v = (al * t) @ Z[idx]
    return 0.5 * float(w @ w) + float(np.sum(c * np.maximum(0.0, 1.0 - t * f))), float(al.sum()) - 0.5 * float(v @ v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="folder holding the reference's scripts 03 and 05")
    args = ap.parse_args()
    warnings.filterwarnings("ignore")
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import SVC

    from make_golden_cluster import load_reference
    _, ref = load_reference(args.reference)
    G = np.load(os.path.join(ROOT, "tests", "golden", "g_cluster.npz"))
    X_tr, y_tr, X_te, y_te = G["X_tr"], G["y_tr"], G["X_te"], G["y_te"]
    sc = StandardScaler().fit(X_tr)
    Z, Zt = sc.transform(X_tr), sc.transform(X_te)
    fits = {tol: SVC(kernel="linear", C=C_PEN, class_weight="balanced", tol=tol).fit(Z, y_tr) for tol in (1e-10, 1e-12)}
    svc = fits[1e-12]
    agree = float(np.abs(fits[1e-10].coef_ - svc.coef_).max())
    assert agree <= 1e-8, agree
    n, C = len(y_tr), len(svc.classes_)
    alpha = np.zeros((n, C - 1))
    alpha[svc.support_] = np.abs(svc.dual_coef_.T)
    cw = n / (C * np.bincount(y_tr, minlength=C).astype(np.float64))
    assert np.allclose(cw, svc.class_weight_, rtol=1e-15)
    pairs = [(a, b) for a in range(C) for b in range(a + 1, C)]
    obj = np.array([pair_objectives(Z, y_tr, cw, a, b, svc.coef_[p], svc.intercept_[p], alpha) for p, (a, b) in enumerate(pairs)])
    svc.decision_function_shape = "ovo"
    dec = svc.decision_function(Zt)
    pred_tight = svc.predict(Zt).astype(np.int64)
    pred_default = np.asarray(ref.run_supervised_svm_rbf(X_tr, y_tr, X_te)).astype(np.int64)
    assert np.array_equal(pred_tight, pred_default)
    small = np.abs(dec).min(axis=1)
    assert (small < 1e-3).mean() <= 0.01 and not (small < 1e-6).any(), ((small < 1e-3).sum(), small.min())
    six = list(G["six_names"])
    out = {"coef": svc.coef_, "intercept": svc.intercept_, "alpha": alpha, "dec_te": dec, "pred_tight": pred_tight, "pred_default": pred_default,
           "ref_gap": obj[:, 0] - obj[:, 1], "ref_primal": obj[:, 0], "mean": sc.mean_, "scale": sc.scale_, "class_weight": cw,
           "C": np.array(C_PEN), "n_support": svc.n_support_.astype(np.int64), "metric_names": G["metric_names"],
           "svm_metrics": G["six_metrics"][six.index("Sup_SVM")], "acc_range": G["acc_range"], "tol_agreement": np.array(agree),
           "rows_below_1e-3": np.array(int((small < 1e-3).sum()), dtype=np.int64)}
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size <= 64 * 1024, size
    print("train %d, test %d, %d bytes; tol 1e-10 against 1e-12: %.3e in coef_" % (n, len(y_te), size, agree))
    print("reference gap per pair:", out["ref_gap"], "primal:", out["ref_primal"])
    print("test rows with a value below 1e-3: %d, smallest %.3e; accuracy %.4f" % (out["rows_below_1e-3"], small.min(), (pred_tight == y_te).mean()))
    m = ref.compute_macro_metrics(y_te, pred_default)
    assert max(abs(m[k] - v) for k, v in zip(G["metric_names"], out["svm_metrics"])) <= 1e-12


if __name__ == "__main__":
    sys.exit(main())
