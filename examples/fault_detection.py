"""Fault detection on the device: a synthetic results array with twelve fault segments, script 02's four feature groups
(`epi,res` / `x0,x3,x4,x5` / `res` / `y_true`) each fitted with StandardScaler + logistic regression on a tenth of the rows
and judged by the ROC AUC of 1 - P(normal) on the rest; for the first group also the unsupervised AUC of an isolation forest
fitted on the normal training rows alone (no fault labels); then the recording replayed in chunks through the online detector
and the anomaly monitor of the first group.  Nothing leaves the GPU but the printed numbers.  With --inference, after the
AUCs: each AUC's DeLong interval, the paired DeLong tests between the groups (Holm-adjusted) and the bootstrap interval of
the difference between the first two groups, all on the same test rows (pinn_amd.rocstat).  With --select, first: the feature
group chosen from the data (pinn_amd.featsel): every subset of at most three of the 17 candidate columns is fitted on training
rows and scored on validation rows in one batch, and the winner is then reported beside script 02's four groups on held-out
rows that neither fit nor choice has seen.

    python examples/fault_detection.py [--normal-rows 20000] [--fault-rows 1500] [--five-class] [--inference [--n-boot 2000]] [--select]
"""
import argparse
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pinn_amd import anomaly, detection, featsel, rocstat  # noqa: E402


def synthetic_results(n_normal, n_fault, seed=0):
    """[n, 22] in the layout of the results array: noise on normal rows, and in every fault segment a ramp on res, epi,
    y_true and one of x3..x5 of about the size of the noise."""
    rng = np.random.default_rng(seed)
    n = n_normal + 12 * n_fault
    a = np.zeros((n, 22))
    a[:, 0] = rng.choice([108.0, 270.0, 405.0], n) + rng.normal(0.0, 2.0, n)
    for col, (mu, sd) in {3: (60.0, 1.5), 4: (2.0, 0.15), 5: (1.5, 0.1), 8: (3.0, 0.05), 12: (0.0, 0.03)}.items():
        a[:, col] = rng.normal(mu, sd, n)
    a[:, 11] = np.abs(rng.normal(0.02, 0.006, n))
    ramp = np.linspace(0.2, 1.0, n_fault)
    for k in range(1, 13):
        rows = slice(n_normal + (k - 1) * n_fault, n_normal + k * n_fault)
        cls, amp = (k - 1) // 3, (0.8, 1.3, 1.8)[(k - 1) % 3]
        a[rows, 17] = k
        a[rows, 12] += amp * 0.03 * ramp * (1.0 + 0.3 * cls)
        a[rows, 11] += amp * 0.005 * ramp * (1 + cls % 3)
        a[rows, 8] -= amp * 0.04 * ramp
        a[rows, 3 + cls % 3] += amp * (1.5, 0.15, 0.1)[cls % 3] * ramp
    return a


def print_inference(groups, n_boot):
    """What the list of AUCs leaves open: how sure each is, and which differences exceed the split's noise."""
    table = rocstat.compare_feature_groups(groups, level=0.95, n_boot=n_boot)
    names = list(table)
    print("\n%-14s %8s  %-19s %-19s" % ("features", "AUC", "95% DeLong", "95%% bootstrap (%d)" % n_boot))
    for name in names:
        row = table[name]
        print("%-14s %8.4f  [%.4f, %.4f]    [%.4f, %.4f]" % ((name, row["auc"]) + row["ci"] + row["boot_ci"]))
    print("paired DeLong tests, p-values after Holm's adjustment over the %d pairs (row minus column):" % (len(names) * (len(names) - 1) // 2))
    print("%-14s " % "" + " ".join("%17s" % n for n in names))
    for name in names:
        print("%-14s " % name + " ".join("%17s" % ("-" if o == name else "%+.4f p=%.1e" % (table[name]["diff"][o], table[name]["p_holm"][o]))
                                         for o in names))
    a, b = names[0], names[1]
    lo, hi = table[a]["boot_diff_ci"][b]
    print("AUC(%s) - AUC(%s) = %+.4f, 95%% bootstrap interval [%+.4f, %+.4f], DeLong z = %.2f\n"
          % (a, b, table[a]["diff"][b], lo, hi, table[a]["z"][b]))


def select_and_report(results, spec, max_size=3, random_state=detection.DEFAULT_RANDOM_STATE):
    """Choose the feature group on train / validation rows, judge it on rows outside both.  The rows are split twice: half
    are held out; the other half is split again into the rows the candidates are fitted on and the rows they are ranked on."""
    pool = list(range(17))
    label_map, _ = detection.build_label_mapper(detection.parse_group_spec(spec))
    _, y, _ = detection.extract_X_y(results, pool, label_map, return_index=True)
    y = y.cpu().numpy() if hasattr(y, "cpu") else np.asarray(y)
    inner, held_out = detection.stratified_split(y, 0.5, random_state)
    tr, va = detection.stratified_split(y[inner], 0.5, random_state + 1)
    subsets = featsel.feature_subsets(pool, 1, max_size)
    timings = {}
    sweep = featsel.feature_sweep(results, subsets, group_spec=spec, split=(inner[tr], inner[va]), timings=timings)
    print("feature sweep: %d subsets of at most %d of %d columns, %d training and %d validation rows%s"
          % (len(sweep), max_size, len(pool), sweep.n_train, sweep.n_val,
             "; device ms: " + ", ".join("%s %.1f" % kv for kv in timings.items()) if timings else ""))
    print("%-22s %6s %9s %9s %9s" % ("features", "iters", "val AUC", "val acc", "val loss"))
    for row in sweep.table(top=5, criterion="val_auc"):
        print("%-22s %6d %9.4f %9.4f %9.4f" % (",".join(row["names"]), row["n_iter"], row["val_auc"], row["val_accuracy"], row["val_logloss"]))
    best = sweep.best("val_auc")
    chosen = ",".join(sweep.names(best))
    # the validation AUC above chose the winner and is optimistic for it: the comparison runs on the held-out rows
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        groups = detection.evaluate_feature_groups(results, [chosen] + [g for g in detection.FEATURE_GROUPS if g != chosen], group_spec=spec,
                                                   split=(inner, held_out))
    table = rocstat.compare_feature_groups(groups)
    print("on %d held-out rows (validation AUC of the winner: %.4f):" % (groups[0]["n_test"], sweep.val_auc[best]))
    print("%-22s %8s  %-19s %s" % ("features", "AUC", "95% DeLong", "chosen minus this, Holm-adjusted p"))
    for name in table:
        row = table[name]
        diff = "-" if name == chosen else "%+.4f p=%.1e" % (table[chosen]["diff"][name], table[chosen]["p_holm"][name])
        print("%-22s %8.4f  [%.4f, %.4f]    %s" % ((name, row["auc"]) + row["ci"] + (diff,)))
    print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--normal-rows", type=int, default=20000)
    ap.add_argument("--fault-rows", type=int, default=1500)
    ap.add_argument("--five-class", action="store_true", help="normal and the four fault classes instead of normal / fault")
    ap.add_argument("--inference", action="store_true", help="intervals of the AUCs and paired tests between the feature groups")
    ap.add_argument("--n-boot", type=int, default=2000, help="resamples of the paired bootstrap of --inference")
    ap.add_argument("--select", action="store_true", help="choose the feature group from the data and judge it on held-out rows")
    args = ap.parse_args()

    results = torch.from_numpy(synthetic_results(args.normal_rows, args.fault_rows)).cuda()
    spec = detection.FIVE_CLASS_GROUP_SPEC if args.five_class else detection.DEFAULT_GROUP_SPEC
    if args.select:
        select_and_report(results, spec)
    groups = detection.evaluate_feature_groups(results, group_spec=spec, unsupervised=True)
    print("%-14s %8s %8s %6s %9s %9s %8s" % ("features", "train", "test", "iters", "accuracy", "macro F1", "AUC"))
    for g in groups:
        lr = g["clf"].named_steps["logreg"]
        print("%-14s %8d %8d %6d %9.4f %9.4f %8.4f" % (g["spec"], g["n_train"], g["n_test"], lr.n_iter_, g["accuracy"], g["metrics"]["macro_f1"],
                                                      g["auc"]))
    if args.inference:
        print_inference(groups, args.n_boot)
    forest = groups[0]["iforest"]
    print("unsupervised, %s: isolation forest of %d trees on %d rows each, AUC %.4f (supervised %.4f)"
          % (groups[0]["spec"], len(forest.trees_), forest.max_samples_, groups[0]["auc_unsup"], groups[0]["auc"]))
    for e in detection.explain_coefficients(groups[0]["clf"], groups[0]["features"], groups[0]["class_names"]):
        print("coefficients of %r in the standardised space: %s" % (e["class"], ", ".join("%s %+.3f" % p for p in e["positive"])))

    detector = detection.FaultDetector(groups[0]["clf"], features=detection.FEAT_GRP1, normal_class=0)
    monitor = anomaly.AnomalyMonitor(forest, features=detection.FEAT_GRP1)
    print("\n%8s %10s %12s %13s %12s %s" % ("rows", "label", "mean p_fault", "share flagged", "mean anomaly", "share outlying"))
    for s in range(0, results.shape[0], 4096):
        chunk = results[s:s + 4096]
        p_fault, pred = detector.update(chunk)
        score, outlying = monitor.update(chunk)
        print("%8d %10d %12.4f %13.3f %12.4f %.3f" % (s + chunk.shape[0], int(chunk[-1, 17]), float(p_fault.mean()), float((pred != 0).double().mean()),
                                                      float(score.mean()), float((outlying < 0).double().mean())))


if __name__ == "__main__":
    main()
