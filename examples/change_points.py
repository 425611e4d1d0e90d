"""Change-point segmentation end to end on the device: build the results array of a synthetic recording with twelve fault
segments as examples/early_warning.py does, hide the label column, and find the regimes from the residual columns alone.
Prints every found boundary against the nearest true one, the table of found segments, then takes the first found segment
for the normal rows (`estimate_mu_sigma_normal`) and runs `rf_series` with the found `seg_starts`.

    python examples/change_points.py [--rows 6000] [--fault-rows 600] [--epochs 3000] [--kind mean] [--min-len 20] [--path]

The residual columns are no z-scores, and without labels there are no normal rows to take mu and sigma from.  For
kind="mean" the noise level of each column is therefore estimated from its first differences (a change of level moves one
difference per boundary, the noise moves them all): sigma = std(diff) / sqrt(2), mu = 0.  kind="meanvar" needs no scale.
With --path eight penalties around the default are run in one device call and the BIC and elbow choices are printed.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pinn_amd  # noqa: E402
from pinn_amd import changepoint, risk, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--fault-rows", type=int, default=600)
    ap.add_argument("--epochs", type=int, default=3000)
    ap.add_argument("--mc-times", type=int, default=32)
    ap.add_argument("--kind", default="mean", choices=("mean", "meanvar"))
    ap.add_argument("--min-len", type=int, default=20)
    ap.add_argument("--path", action="store_true", help="also run eight penalties in one call and print the BIC and elbow choices")
    args = ap.parse_args()

    ds = synth.make_dataset(args.rows, (args.fault_rows,) * 12, seed=0)
    torch.manual_seed(0)
    model = pinn_amd.PhysicsInformedNN(ds[0], ds[1], [8, 256, 256, 256, 1], ds[4], ds[5], p=0.2, logvar=True, seed=1)
    model.verbose = False
    model.train_dnn(args.epochs)
    results = pinn_amd.create_comprehensive_results_array_v2(model, ds, mc_times=args.mc_times, dropout=0.2, device_output=True)

    label = risk.INDEX["label"]
    truth = results[:, label].cpu().numpy()
    true_starts = np.flatnonzero(truth[1:] != truth[:-1]) + 1
    hidden = results.clone()
    hidden[:, label] = float("nan")                             # from here on nothing reads the labels

    features = changepoint.DEFAULT_FEATURES
    cols = pinn_amd.parse_features(features)
    scale = {}
    if args.kind == "mean":
        diff = hidden[1:, cols] - hidden[:-1, cols]
        scale = dict(mu=np.zeros(len(cols)), sigma=(diff.std(dim=0) / 2 ** 0.5).cpu().numpy())
        print("noise level from first differences:", dict(zip(features.split(","), scale["sigma"].round(6))))
    kw = dict(features=features, kind=args.kind, min_len=args.min_len, **scale)
    seg = changepoint.segment(hidden, **kw)
    found = seg.change_points[0]
    print("\n%d rows, penalty %.2f (BIC), %d change points found, %d true boundaries, %d cost evaluations"
          % (seg.n, seg.penalty, found.size, true_starts.size, int(seg.evaluations[0])))
    print("%10s %12s %8s" % ("found", "nearest true", "off by"))
    for p in found:
        near = true_starts[np.argmin(np.abs(true_starts - p))] if true_starts.size else -1
        print("%10d %12d %8d" % (p, near, p - near))
    missed = [int(t) for t in true_starts if found.size == 0 or np.min(np.abs(found - t)) > args.min_len]
    print("true boundaries with no found one within %d rows: %s" % (args.min_len, missed if missed else "none"))

    table = changepoint.segment_table(hidden, seg, features)
    print("\n%8s %8s  %s" % ("start", "length", "mean of " + features))
    for s, ln, m in zip(table["start"], table["length"], table["mean"]):
        print("%8d %8d  %s" % (s, ln, " ".join("%10.5f" % v for v in m)))

    if args.path:
        pens = seg.penalty * np.array([0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0])
        path = changepoint.penalty_path(hidden, pens, **kw)
        print("\n%10s %8s %14s" % ("penalty", "changes", "cost"))
        for p, k, c in zip(path.penalties, path.n_change_points, path.cost):
            print("%10.2f %8d %14.3f" % (p, k, c))
        print("BIC picks penalty %.2f, the elbow %.2f" % (pens[changepoint.select_penalty(path, "bic")], pens[changepoint.select_penalty(path, "elbow")]))

    # the first found segment stands in for the normal rows; the found starts restart the risk function
    first_end = int(seg.seg_starts[1]) if seg.seg_starts.size > 1 else seg.n
    labelled = hidden.clone()
    labelled[:, label] = 1.0
    labelled[:first_end, label] = 0.0
    mu, sigma = risk.estimate_mu_sigma_normal(labelled)
    series = risk.rf_series(results, mu, sigma, seg_starts=seg.seg_starts)
    rf = series["RF_smooth"].cpu().numpy()
    print("\nmu, sigma from the first found segment (%d rows); RF restarted at the %d found starts" % (first_end, seg.seg_starts.size))
    print("%8s %8s %10s" % ("start", "length", "peak RF"))
    for lo, hi in seg.bounds():
        print("%8d %8d %10.4f" % (lo, hi - lo, float(rf[lo:hi].max())))


if __name__ == "__main__":
    main()
