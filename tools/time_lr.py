"""Time the fault detection of pinn_amd.detection on the GPU.

For 1e5 / 1e6 / 1e7 rows and (C, D) = (2, 2), (2, 4), (5, 4): one row pass (device events after warm-up, the median of
`--reps` repetitions), packed (8 D bytes per row) and read in place from a 22-column results array (176 B/row); a full fit
from zero at the default tol; predict_proba; roc_curve of 1 - P(class 0).  Beside them: the HBM floor of the pass at
`--hbm-gbs`, the same pass (loss, gradient, Hessian blocks) composed of torch float64 device ops, and this package's host
backend (numpy, this machine's CPU; skipped at 1e7 rows).  Prints one JSON line per case.  The scikit-learn figures of
DESIGN 3h come from `tools/make_golden_lr.py --time` on the build machine's CPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_amd import detection as T  # noqa: E402

COLS = {2: [11, 12], 4: [0, 3, 4, 5]}


def data(n, C, D, seed=0):
    rng = np.random.default_rng(seed)
    y = rng.integers(C, size=n)
    return rng.normal(size=(n, D)) + 0.5 * y[:, None] * rng.normal(size=D), y.astype(np.int64)


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def torch_pass(X, y, theta, cw):
    """The sums of one pass as torch float64 ops: softmax, gradient by matmul, Hessian blocks by weighted matmuls."""
    n, C = X.shape[0], theta.shape[0]
    U = torch.cat([X, torch.ones(n, 1, dtype=X.dtype, device=X.device)], dim=1)
    s = U @ theta.T
    lse = torch.logsumexp(s, dim=1)
    p = torch.exp(s - lse[:, None])
    sw = cw[y]
    loss = (sw * (lse - s.gather(1, y[:, None])[:, 0])).sum()
    R = p.clone()
    R.scatter_add_(1, y[:, None], -torch.ones(n, 1, dtype=X.dtype, device=X.device))
    g = (R * sw[:, None]).T @ U
    H = [(U * (sw * p[:, c] * ((1.0 if c == d else 0.0) - p[:, d]))[:, None]).T @ U for d in range(C) for c in range(d + 1)]
    return loss, g, H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--shapes", default="2x2,2x4,5x4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM bandwidth for the floor, GB/s (MI355X peak: 8000)")
    args = ap.parse_args()
    for n in [int(s) for s in args.sizes.split(",")]:
        for C, D in [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]:
            X, y = data(n, C, D)
            Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
            wide = torch.zeros(n, 22, dtype=torch.float64, device="cuda")
            wide[:, COLS[D]] = Xd
            theta = np.random.default_rng(1).normal(0.0, 0.3, (C, D + 1))
            lr = T.DeviceLogisticRegression(class_weight="balanced", backend="device")
            res = {"rows": n, "C": C, "D": D}
            # pass_sums = scaler launches + one pass + the allocation of the state: the pass alone is the difference to the scaler
            res["pass_packed_ms"] = event_ms(lambda: lr.pass_sums(Xd, yd, theta), args.reps)
            res["pass_in_place_ms"] = event_ms(lambda: lr.pass_sums(wide, yd, theta, columns=COLS[D]), args.reps)
            res["scaler_packed_ms"] = event_ms(lambda: T.DeviceStandardScaler(backend="device").fit(Xd), args.reps)
            res["hbm_floor_packed_ms"] = n * 8 * (D + 1) / (args.hbm_gbs * 1e9) * 1e3
            res["hbm_floor_in_place_ms"] = n * (176 + 8) / (args.hbm_gbs * 1e9) * 1e3
            t0 = time.perf_counter()
            clf = T.build_classifier(balanced=True, backend="device").fit(wide, yd, columns=COLS[D])
            torch.cuda.synchronize()
            f = clf.named_steps["logreg"]
            res["full_fit_in_place_ms"], res["newton_iterations"], res["passes"] = (time.perf_counter() - t0) * 1e3, f.n_iter_, f.n_passes_
            res["predict_proba_ms"] = event_ms(lambda: clf.predict_proba(wide, columns=COLS[D]), args.reps)
            pf = clf.p_fault(wide, 0, columns=COLS[D])
            truth = yd != 0
            res["roc_curve_ms"] = event_ms(lambda: T.roc_curve(truth, pf, pos_label=True), args.reps)
            res["auc_score_ms"] = event_ms(lambda: T.auc_score(truth, pf, pos_label=True), args.reps)
            try:
                th, cw = torch.from_numpy(theta).cuda(), torch.ones(C, dtype=torch.float64, device="cuda")
                res["torch_pass_ms"] = event_ms(lambda: torch_pass(Xd, yd, th, cw), max(3, args.reps // 2))
            except RuntimeError as e:
                res["torch_pass_ms"], res["torch_note"] = None, str(e).splitlines()[0][:80]
            if n <= 1000000:
                lh = T.DeviceLogisticRegression(class_weight="balanced", backend="host")
                t0 = time.perf_counter()
                lh.pass_sums(X, y, theta)
                res["host_pass_ms"] = (time.perf_counter() - t0) * 1e3
            print(json.dumps(res), flush=True)
            del Xd, wide
    return 0


if __name__ == "__main__":
    sys.exit(main())
