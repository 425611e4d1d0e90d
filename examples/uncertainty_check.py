"""Are the voltage network's standard deviations honest?  End to end on the device: train briefly on a synthetic recording
with twelve fault segments, assemble the results array on the device, score the predictive law y ~ N(y_pred, ale^2 + epi^2)
on the normal rows, calibrate a conformal half-width q on every other normal row, report the coverage of y_pred -+ q s on the
remaining normal rows and per fault class, and replay the recording through the online band.

    python examples/uncertainty_check.py [--rows 6000] [--fault-rows 600] [--epochs 3000] [--level 0.9]

Rows of one recording are correlated, so the coverage on the held-out half is a check of this recording, not the
exchangeable-rows guarantee; with real data calibrate on one recording and check on another.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pinn_amd  # noqa: E402
from pinn_amd import risk, synth, uncertainty  # noqa: E402


def coverage(results, lo, hi, rows):
    y = results[rows, 8]
    inside = (y >= lo[rows]) & (y <= hi[rows])
    return float(inside.double().mean()) if rows.numel() else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--fault-rows", type=int, default=600)
    ap.add_argument("--epochs", type=int, default=3000)
    ap.add_argument("--mc-times", type=int, default=32)
    ap.add_argument("--level", type=float, default=0.9)
    args = ap.parse_args()

    ds = synth.make_dataset(args.rows, (args.fault_rows,) * 12, seed=0)
    torch.manual_seed(0)
    model = pinn_amd.PhysicsInformedNN(ds[0], ds[1], [8, 256, 256, 256, 1], ds[4], ds[5], p=0.2, logvar=True, seed=1)
    model.verbose = False
    model.train_dnn(args.epochs)
    results = pinn_amd.create_comprehensive_results_array_v2(model, ds, mc_times=args.mc_times, dropout=0.2, device_output=True)

    groups = dict(normal=list(risk.NORMAL_LABELS), **{k: list(v) for k, v in risk.FAULT_RANGE_MAP.items()})
    report = uncertainty.score_uncertainty(results, groups=groups)
    print("%-22s %7s %9s %9s %8s %9s %9s   coverage at %s" % ("group", "rows", "rmse", "mean s", "scale", "nll", "crps", report["normal"].levels))
    for name, r in report.items():
        print("%-22s %7d %9.4g %9.4g %8.3f %9.4g %9.4g   %s" % (name, r.n, r.rmse, r.sharpness, r.scale, r.nll, r.crps, r.coverage.round(3).tolist()))
    r = report["normal"]
    print("normal rows: miscalibration area %.4f, PIT chi-square %.1f on %d bins; scale %.3f means s should be multiplied by it"
          % (r.miscalibration, r.pit_chi2, len(r.pit), r.scale))

    labels = results[:, 17].long()
    normal = torch.nonzero(torch.isin(labels, torch.tensor(groups["normal"], device=labels.device))).reshape(-1)
    cal, held = normal[0::2], normal[1::2]
    q = uncertainty.conformal_quantiles(results, levels=(args.level,), row_index=cal)
    print("\nconformal half-width at level %.2f from %d normal rows: q = %.4f (rank %d; a calibrated Gaussian would give %.4f)"
          % (args.level, int(q.n[0]), q.q[0, 0], int(q.rank[0, 0]), __import__("statistics").NormalDist().inv_cdf(0.5 + 0.5 * args.level)))
    lo, hi = uncertainty.conformal_band(results, q.q[0, 0])
    print("%-22s %7s %10s" % ("rows", "n", "coverage"))
    print("%-22s %7d %10.4f" % ("normal, held out", held.numel(), coverage(results, lo, hi, held)))
    for name, labs in groups.items():
        if name != "normal":
            rows = torch.nonzero(torch.isin(labels, torch.tensor(labs, device=labels.device))).reshape(-1)
            print("%-22s %7d %10.4f" % (name, rows.numel(), coverage(results, lo, hi, rows)))

    monitor = uncertainty.UncertaintyMonitor(level=args.level, window=1024, gamma=0.005, init=q)
    for s in range(0, results.shape[0], 1024):
        monitor.update(results[s:s + 1024])
    print("\nonline band over %d rows in chunks of 1024: %d valid, miss rate %.4f (target %.2f), final q = %.4f, alpha = %.4f"
          % (results.shape[0], monitor.n_valid, monitor.n_miss / max(monitor.n_valid, 1), 1.0 - args.level, monitor.q, monitor.alpha))


if __name__ == "__main__":
    main()
