"""Script 05's question on the device: is the mixture with label-posterior mapping better than plain clustering?  A synthetic
results array with twelve fault segments (two residual columns drift per fault class), the fault rows split once, and GMM,
logistic regression, k-means and Ward clustering and, through `device_extras` and `spectral_extras`, the linear SVC of script
05's Sup_SVM and the spectral clustering of its Spectral: all six methods of the script, plus, through `kernel_extras`, the
RBF-kernel SVC that the script names for Sup_SVM (`Sup_SVM_RBF`), fitted on the training rows and judged
on the test rows by accuracy and macro precision / recall / F1.  A user's own method rides along as a callable.  Then the recording is replayed in chunks
through the online diagnoser of the k-means model.  Nothing leaves the GPU but the printed numbers; `--host` runs the
float64 numpy backend instead.

    python examples/method_comparison.py [--fault-rows 600] [--host]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from pinn_amd import comparison  # noqa: E402

SCALE = {13: 0.05, 14: 0.5, 15: 0.01, 16: 0.01}                       # sigma of pV, pT, pH, pO on normal rows
DRIFT_COLS = {0: (13, 16), 1: (16, 14), 2: (14, 15), 3: (15, 13)}     # two residual columns per fault class


def synthetic_results(n_normal, n_fault, seed=0):
    rng = np.random.default_rng(seed)
    n = n_normal + 12 * n_fault
    a = np.zeros((n, 22))
    for c, s in SCALE.items():
        a[:, c] = rng.normal(0.0, s, n)
    ramp = np.linspace(0.0, 1.0, n_fault)
    for k in range(1, 13):
        rows = slice(n_normal + (k - 1) * n_fault, n_normal + k * n_fault)
        a[rows, 17] = k
        for j, c in enumerate(DRIFT_COLS[(k - 1) // 3]):
            a[rows, c] += (1.0 if j == 0 else -1.0) * (6.0, 9.0, 12.0)[(k - 1) % 3] * SCALE[c] * (0.35 + 0.65 * ramp)
    return a


def nearest_class_mean(X_tr, y_tr, X_te):
    """A user's method: the class whose training mean is nearest (numpy or torch arrays alike)."""
    means = [X_tr[y_tr == c].mean(0) for c in range(comparison.N_CLASSES)]
    d2 = [((X_te - m) ** 2).sum(1) for m in means]
    return np.argmin(np.stack([np.asarray(d.cpu() if hasattr(d, "cpu") else d) for d in d2], axis=1), axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--normal-rows", type=int, default=2000)
    ap.add_argument("--fault-rows", type=int, default=600)
    ap.add_argument("--host", action="store_true", help="the float64 numpy backend (no GPU needed)")
    args = ap.parse_args()

    results = synthetic_results(args.normal_rows, args.fault_rows)
    backend = "host"
    if not args.host:
        import torch
        results, backend = torch.from_numpy(results).cuda(), "device"
    X, y, names = comparison.load_data_for_fault_4class(results, backend=backend)
    print("fault rows: %d x %d features, classes %s" % (X.shape[0], X.shape[1], names))
    methods = comparison.METHODS + ("Sup_SVM", "Sup_SVM_RBF", "Spectral", "NearestMean")
    # Sup_SVM: the package's linear SVC (svm.py), what script 05 runs; Sup_SVM_RBF: the RBF-kernel SVC it names (ksvm.py);
    # Spectral: its spectral clustering (spectral.py)
    extra = {**comparison.device_extras(backend), **comparison.kernel_extras(backend), **comparison.spectral_extras(backend),
             "NearestMean": nearest_class_mean}
    r = comparison.compare_methods(X, y, methods=methods, extra=extra, backend=backend)
    print("%-12s %9s %10s %9s %9s" % ("method", "accuracy", "precision", "recall", "F1"))
    for name in methods:
        m = r[name]
        print("%-12s %9.4f %10.4f %9.4f %9.4f" % (name, m["accuracy"], m["macro_precision"], m["macro_recall"], m["macro_f1"]))

    # the online form: k-means centres and their class distributions, one launch per chunk of the results array
    idx_tr = r["split"]["idx_train"]
    X_tr, y_tr = comparison._take(X, idx_tr), comparison._take(y, idx_tr)
    km = comparison.DeviceKMeans(5 * comparison.N_CLASSES, random_state=42, backend=backend).fit(X_tr)
    cmap = comparison.cluster_class_map(km.labels_, y_tr, km.n_clusters, comparison.N_CLASSES)
    diag = comparison.ClusterDiagnoser(km, cmap, backend=backend)
    print("\nk-means: %d iterations, inertia %.4f\n%8s %8s %s" % (km.n_iter_, km.inertia_, "rows", "label", "share of the chunk per predicted class"))
    for s in range(args.normal_rows, results.shape[0], 2 * args.fault_rows):
        chunk = results[s:s + 2 * args.fault_rows]
        _, pred = diag.update(chunk)
        pred = np.asarray(pred.cpu() if hasattr(pred, "cpu") else pred)
        print("%8d %8d %s" % (s + chunk.shape[0], int(chunk[-1, 17]), np.round(np.bincount(pred, minlength=4) / len(pred), 3)))


if __name__ == "__main__":
    main()
