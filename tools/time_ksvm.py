"""Times of the RBF-kernel SVC of pinn_amd.ksvm (csrc/pinn_ksvm.hip) at the fixture's size (1349 rows) and at 1e4 and 1e5
training rows of synthetic blobs, 4 features in 4 classes: microseconds per SMO iteration (both row passes, all six pairs
advancing together), `fit` to the default tol with the iterations it took, and the decision launch on as many rows as were
fitted (rows per second, with the number of support rows it walks).

An iteration is timed while every pair is still active: a window is 512 calls of 32 iterations from alpha = 0 (init = 1
each, so 65 launches per call, one of them the starting launch; 0.2 s and more per window), and the tool checks afterwards
that no pair has converged, since a converged pair's workgroups return at once.  32 is below the 51 iterations of the
fixture's quickest pair.  Device events, the median of 5 windows after a warm-up, as tools/time_svm.py.  The decision
figure is `predict` repeated until a window holds 0.1 s and more, per call.  A fit is timed by the host clock around fits
that each end in a device synchronise, after a warm-up fit: the mean of 20 fits at the fixture's size, of 3 above it.  Every
chunk of 64 iterations of a fit ends in the host's read of the pair blocks, so a fit's time holds that latency as well as
device work.  scikit-learn's times on the CPU come from `tools/make_golden_ksvm.py --time`.

    python tools/time_ksvm.py [--quick] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rows(n, seed=0):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 1.6, (4, 4))
    centres[:, 0] += 2.5 * rng.permutation(4)
    y = rng.integers(0, 4, n)
    return centres[y] + rng.normal(0.0, 1.0, (n, 4)), y.astype(np.int64)


def median_ms(fn, windows=5):
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
    ap.add_argument("--quick", action="store_true", help="skip the 1e5-row case")
    ap.add_argument("--out", help="also write the table to this file")
    args = ap.parse_args()
    import torch

    from pinn_amd import _lib, ksvm
    from pinn_amd._device import call
    G = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "g_cluster.npz"))
    lines = ["%9s %6s %12s %10s %9s %8s %12s %14s" % ("rows", "C", "us / iter", "fit s", "iters", "n_sv", "decision ms", "rows / s")]
    print(lines[0], flush=True)
    cases = [("fixture", G["X_tr"], G["y_tr"])] + [(str(n),) + rows(n) for n in ((10000,) if args.quick else (10000, 100000))]
    for name, X, y in cases:
        Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
        for C in (0.05, 1.0):
            pipe = ksvm.build_kernel_svm_classifier("device", C=C)
            m = pipe.named_steps["svc"]
            sc = pipe.named_steps["scaler"].fit(Xd)
            q = m.device_problem(Xd, yd, scaler=sc)
            n_it, n_calls, P = 32, 512, 6

            def calls():
                for _ in range(n_calls):
                    call("pinn_ksvm_smo", *q["head"], q["gamma"], 1, n_it, m.tol, q["state"], None, q["ws"], q["ws_bytes"])

            t_it = median_ms(calls)
            pairs = q["state"][_lib.KSVM_ST_HEADER:_lib.KSVM_ST_HEADER + P * _lib.KSVM_PAIR_WORDS].cpu().numpy().view(np.int64).reshape(P, -1)
            assert (pairs[:, _lib.KSVM_P_ITER] == n_it).all() and not pairs[:, _lib.KSVM_P_CONVERGED].any(), "a pair stopped inside the window"
            pipe.fit(Xd, yd)
            n_fits = 20 if len(y) <= 2000 else 3
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_fits):
                pipe.fit(Xd, yd)
            torch.cuda.synchronize()
            t_fit = (time.perf_counter() - t0) / n_fits
            n_dec = max(20, min(400, 2000000 // len(y)))

            def decisions():
                for _ in range(n_dec):
                    pipe.predict(Xd)

            t_dec = median_ms(decisions) / n_dec
            lines.append("%9s %6g %12.2f %10.4f %9d %8d %12.4f %14.4g" % (name, C, 1e3 * t_it / (n_it * n_calls), t_fit, int(m.n_iter_.max()), len(m.support_), t_dec,
                                                                     len(y) / (1e-3 * t_dec)))
            print(lines[-1], "" if m.converged_.all() else "(not converged)", flush=True)
            if args.out:                        # after every line: a case that is cut short keeps the lines before it
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
