"""Generate tests/golden/g_ksvm.npz: scikit-learn's RBF-kernel SVC, the machine script 05 names for Sup_SVM, on the split of
tests/golden/g_cluster.npz.

Build machine only: needs scikit-learn.  No test imports this file.  The fixture holds arrays only, and not the rows: the
tests take `X_tr`, `y_tr`, `X_te`, `y_te` from g_cluster.npz.  For `StandardScaler` + `SVC(kernel="rbf", gamma="scale",
class_weight="balanced", tol=1e-12)` at every C of `C` (0.05, script 05's, and 1.0), first axis = the C: `gamma`, `intercept`
[P], the support rows `support` (positions, ascending, padded with -1) with `dual_coef_sup` [n_sv, 3] (dual_coef_ transposed,
signs included; alpha is its magnitude, in the slot layout: slot j of a row is its j-th other class in increasing order;
every other alpha is 0), `dec_te` (one-vs-one) and `pred` of the test rows, the reference's own `ref_gap` = primal - dual
and `ref_primal` per pair, evaluated here in float64 numpy with the exact kernel, `n_support`, the agreement of the tol=1e-10 run with the tol=1e-12 run (`intercept_agreement`,
`dec_agreement`), the allowance for intercepts and the bound on decision values that tests/test_ksvm_host.py derives from
them (`intercept_allowance`, `pred_bound` per pair), `rows_below` (test rows with a pairwise |decision| below its pair's
bound), `pred_checked` (1 where at most 1 % of the test rows are, so that the predictions at this C are compared) and the
macro metrics of `pred` (`metric_names`, `metrics`).

Conditions asserted here: no duplicate training rows; every pair has a free support vector; the tol=1e-10 and the tol=1e-12
run predict alike; `pred_checked` holds for at least one C.  `--time` prints scikit-learn's wall time of fit and predict at
the fixture's size and at 1e4 rows of synthetic blobs; it stores nothing.
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g_ksvm.npz")
C_PENS = (0.05, 1.0)


def gram(A, B, gamma):
    d2 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=-1)
    return np.exp(-gamma * d2)


def pair_objectives(Z, y, c_row, a, b, alpha, beta, gamma):
    """(primal, dual) of the pair (a, b) in float64 with the exact kernel: alpha [n, C - 1] in the slot layout."""
    ia, ib = np.nonzero(y == a)[0], np.nonzero(y == b)[0]
    idx = np.concatenate([ia, ib])
    t = np.concatenate([np.ones(len(ia)), -np.ones(len(ib))])
    al = np.concatenate([alpha[ia, b - 1], alpha[ib, a]])
    Kv = gram(Z[idx], Z[idx], gamma) @ (al * t)
    quad = float((al * t) @ Kv)
    primal = 0.5 * quad + float(np.sum(c_row[idx] * np.maximum(0.0, 1.0 - t * (Kv + beta))))
    free = (al > 1e-6 * c_row[idx]) & (al < (1.0 - 1e-6) * c_row[idx])
    return primal, float(al.sum()) - 0.5 * quad, int(free.sum())


def blobs(n, C, D, seed):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 1.6, (C, D))
    centres[:, 0] += 2.5 * rng.permutation(C)
    y = rng.integers(0, C, n)
    return centres[y] + rng.normal(0.0, 1.0, (n, D)), y.astype(np.int64)


def timings(X_tr, y_tr, X_te):
    from sklearn.pipeline import make_pipeline
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import SVC
    Xb, yb = blobs(10000, 4, 4, 0)
    for name, (A, ya, B) in (("fixture (%d rows)" % len(y_tr), (X_tr, y_tr, X_te)), ("blobs (10000 rows)", (Xb, yb, Xb))):
        for C in C_PENS:
            for tol in (1e-3, 1e-10):
                pipe = make_pipeline(StandardScaler(), SVC(kernel="rbf", C=C, gamma="scale", class_weight="balanced", tol=tol))
                t0 = time.perf_counter()
                pipe.fit(A, ya)
                t1 = time.perf_counter()
                pipe.predict(B)
                t2 = time.perf_counter()
                print("%s, C = %g, tol = %g: fit %.3f s, predict of %d rows %.3f s (%d support rows)"
                      % (name, C, tol, t1 - t0, len(B), t2 - t1, pipe[-1].support_.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="print scikit-learn's wall times and store nothing")
    args = ap.parse_args()
    warnings.filterwarnings("ignore")
    from sklearn.metrics import accuracy_score, precision_recall_fscore_support
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import SVC

    G = np.load(os.path.join(ROOT, "tests", "golden", "g_cluster.npz"))
    X_tr, y_tr, X_te, y_te = G["X_tr"], G["y_tr"], G["X_te"], G["y_te"]
    if args.time:
        return timings(X_tr, y_tr, X_te)
    assert len(np.unique(X_tr, axis=0)) == len(X_tr), "duplicate training rows"
    sc = StandardScaler().fit(X_tr)
    Z, Zt = sc.transform(X_tr), sc.transform(X_te)
    n, C = len(y_tr), len(np.unique(y_tr))
    pairs = [(a, b) for a in range(C) for b in range(a + 1, C)]
    cw = n / (C * np.bincount(y_tr, minlength=C).astype(np.float64))
    gamma = 1.0 / (Z.shape[1] * Z.var())
    out = {k: [] for k in ("gamma", "intercept", "support", "dual_coef_sup", "dec_te", "pred", "ref_gap", "ref_primal", "n_support",
                           "intercept_agreement", "dec_agreement", "intercept_allowance", "pred_bound", "rows_below", "pred_checked", "metrics")}
    for C_pen in C_PENS:
        fits = {tol: SVC(kernel="rbf", C=C_pen, gamma="scale", class_weight="balanced", tol=tol, decision_function_shape="ovo").fit(Z, y_tr)
                for tol in (1e-10, 1e-12)}
        svc = fits[1e-12]
        assert abs(svc._gamma - gamma) <= 1e-15 * gamma and np.allclose(cw, svc.class_weight_, rtol=1e-15)
        order = np.argsort(svc.support_, kind="stable")                 # scikit-learn groups the support rows by class
        support, coef_sup = svc.support_[order].astype(np.int64), svc.dual_coef_.T[order]
        alpha = np.zeros((n, C - 1))
        alpha[support] = np.abs(coef_sup)
        obj = np.array([pair_objectives(Z, y_tr, C_pen * cw[y_tr], a, b, alpha, svc.intercept_[p], gamma) for p, (a, b) in enumerate(pairs)])
        assert (obj[:, 2] >= 1).all(), "a pair without a free support vector"
        dec, pred = svc.decision_function(Zt), svc.predict(Zt).astype(np.int64)
        assert np.array_equal(pred, fits[1e-10].predict(Zt))
        ref_gap = obj[:, 0] - obj[:, 1]
        i_agree = float(np.abs(fits[1e-10].intercept_ - svc.intercept_).max())
        d_agree = float(np.abs(fits[1e-10].decision_function(Zt) - dec).max())
        # tests 2 and 3 of tests/test_ksvm_host.py: values without intercept within sqrt(2 g) + sqrt(2 ref_gap), g <= ref_gap
        # expected of a float64 solver; intercepts within ten times the larger of libsvm's own agreement and sqrt(2 ref_gap) 1e-3
        allowance = 10.0 * np.maximum(i_agree, np.sqrt(2.0 * ref_gap) * 1e-3)
        bound = 2.0 * np.sqrt(2.0 * ref_gap) + allowance
        below = int((np.abs(dec) < bound[None, :]).any(axis=1).sum())
        prec, rec, f1, _ = precision_recall_fscore_support(y_te, pred, average="macro", zero_division=0)
        for k, v in (("gamma", gamma), ("intercept", svc.intercept_), ("support", support), ("dual_coef_sup", coef_sup), ("dec_te", dec), ("pred", pred),
                     ("ref_gap", ref_gap), ("ref_primal", obj[:, 0]), ("n_support", svc.n_support_.astype(np.int64)), ("intercept_agreement", i_agree),
                     ("dec_agreement", d_agree), ("intercept_allowance", allowance), ("pred_bound", bound), ("rows_below", below),
                     ("pred_checked", int(below <= 0.01 * len(y_te))), ("metrics", [accuracy_score(y_te, pred), prec, rec, f1])):
            out[k].append(v)
        small = np.abs(dec).min(axis=1)
        print("C = %g: %d support rows %s, libsvm iterations %s" % (C_pen, len(support), svc.n_support_, svc.n_iter_))
        print("  reference gap per pair %s, primal %s, free rows %s" % (ref_gap, obj[:, 0], obj[:, 2].astype(int)))
        print("  tol 1e-10 against 1e-12: intercept %.3e, decision values %.3e" % (i_agree, d_agree))
        print("  smallest |decision| %.3e, %d rows below 1e-3, %d below the bound %s; accuracy %.4f"
              % (small.min(), (small < 1e-3).sum(), below, bound, (pred == y_te).mean()))
    assert any(out["pred_checked"]), "no C at which at most 1 % of the test rows lie within the bound of a boundary"
    n_sv = max(len(s) for s in out["support"])
    out["support"] = [np.concatenate([s, -np.ones(n_sv - len(s), dtype=np.int64)]) for s in out["support"]]
    out["dual_coef_sup"] = [np.concatenate([a, np.zeros((n_sv - len(a), C - 1))]) for a in out["dual_coef_sup"]]
    out = {k: np.asarray(v) for k, v in out.items()}
    out["C"] = np.asarray(C_PENS)
    out["metric_names"] = np.asarray(["accuracy", "macro_precision", "macro_recall", "macro_f1"])
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size <= 64 * 1024, size
    print("train %d, test %d, %d bytes; predictions compared at C = %s" % (n, len(y_te), size, [c for c, k in zip(C_PENS, out["pred_checked"]) if k]))


if __name__ == "__main__":
    sys.exit(main())
