"""Times of the linear SVC of pinn_amd.svm (csrc/pinn_svm.hip): `fit` (interior point, every pair to gap_tol) and one
`pinn_svm_decision` launch at 1349, 1e5 and 1e6 rows of 4 features in 4 classes, with the iterations taken and the
milliseconds per iteration; device events, the median of 7 windows after a warm-up, as tools/time_cluster.py.  Where
scikit-learn is importable, its SVC(kernel="linear") on the same rows at 1349 and 1e4 rows on the host (wall time).

    python tools/time_svm.py [--quick]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rows(n, seed=3):
    rng = np.random.default_rng(seed)
    y = np.arange(n) % 4
    centres = rng.normal(0.0, 1.6, (4, 4))
    return centres[y] + rng.normal(0.0, 1.0, (n, 4)), y.astype(np.int64)


def median_ms(fn, windows=7):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="skip the 1e6-row case")
    args = ap.parse_args()
    import torch

    from pinn_amd import svm
    print("%9s %10s %8s %12s %14s" % ("rows", "fit ms", "iters", "ms / iter", "decision ms"))
    for n in (1349, 100000) + (() if args.quick else (1000000,)):
        X, y = rows(n)
        Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
        pipe = svm.build_svm_classifier("device")
        t_fit = median_ms(lambda: pipe.fit(Xd, yd))
        iters = int(pipe.named_steps["svc"].n_iter_.max())
        t_dec = median_ms(lambda: pipe.predict(Xd))
        print("%9d %10.3f %8d %12.4f %14.4f" % (n, t_fit, iters, t_fit / max(iters, 1), t_dec))
    try:
        from sklearn.preprocessing import StandardScaler
        from sklearn.svm import SVC
    except ImportError:
        print("scikit-learn is not installed: no host times")
        return
    for n in (1349, 10000):
        X, y = rows(n)
        Z = StandardScaler().fit_transform(X)
        t0 = time.perf_counter()
        SVC(kernel="linear", C=0.05, class_weight="balanced").fit(Z, y)
        print("scikit-learn SVC on this CPU, %d rows: %.1f ms" % (n, 1e3 * (time.perf_counter() - t0)))


if __name__ == "__main__":
    sys.exit(main())
