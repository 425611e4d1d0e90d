"""Fault diagnosis end to end on the device: train briefly on a synthetic recording with twelve fault segments, assemble the
results array on the device, fit the Gaussian mixture to the physics residual columns of a training subset, calibrate its
components against the labels, print the confusion matrix of the held-out rows, then replay the recording in chunks
through the risk monitor and the fault diagnoser side by side.

    python examples/fault_diagnosis.py [--rows 6000] [--fault-rows 600] [--epochs 3000] [--components 20] [--select]

With --select the number of components and the seed are not taken from the command line: `selection.select_gmm` fits the
grid K in {2, 4, 8, 12, 16, 20, 24, 32} x seeds 0-2 in one batch on the training rows, scores every candidate on the
held-out rows, prints the table and diagnoses with the candidate of the lowest BIC.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pinn_amd  # noqa: E402
from pinn_amd import diagnosis, risk, selection, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--fault-rows", type=int, default=600)
    ap.add_argument("--epochs", type=int, default=3000)
    ap.add_argument("--mc-times", type=int, default=32)
    ap.add_argument("--components", type=int, default=20)
    ap.add_argument("--select", action="store_true", help="choose the components and the seed by BIC over a grid")
    args = ap.parse_args()

    ds = synth.make_dataset(args.rows, (args.fault_rows,) * 12, seed=0)
    x_train, y_train, scaler_X, scaler_Y = ds[0], ds[1], ds[4], ds[5]
    torch.manual_seed(0)
    model = pinn_amd.PhysicsInformedNN(x_train, y_train, [8, 256, 256, 256, 1], scaler_X, scaler_Y, p=0.2, logvar=True, seed=1)
    model.verbose = False
    model.train_dnn(args.epochs)
    results = pinn_amd.create_comprehensive_results_array_v2(model, ds, mc_times=args.mc_times, dropout=0.2, device_output=True)

    features = diagnosis.parse_features(diagnosis.DEFAULT_FEATURES)
    label_map, class_names = diagnosis.build_label_mapper(diagnosis.parse_group_spec(diagnosis.DEFAULT_GROUP_SPEC))
    X, y, kept = diagnosis.extract_X_y(results, features, label_map, return_index=True)
    # every fourth kept row is held out (the reference draws a stratified random split with scikit-learn)
    pos = torch.arange(X.shape[0], device=X.device)
    test, train = pos[pos % 4 == 3], pos[pos % 4 != 3]
    if args.select:
        gmm, sweep = selection.select_gmm(X[train], X_val=X[test], criterion="bic")
        print(sweep.table())
        print("selected by BIC: %d components, seed %d" % (gmm.n_components, gmm.random_state))
        comp_fault_prob = gmm.label_map(X[train], y[train], len(class_names))
        y_prob, y_pred = gmm.diagnose(X[test], comp_fault_prob)
    else:
        y_prob, y_pred, gmm, comp_fault_prob = diagnosis.fit_gmm_and_get_probabilities(
            X[train], y[train], X[test], len(class_names), random_state=diagnosis.RANDOM_STATE, n_components=args.components)
    m = diagnosis.classification_metrics(y[test], y_pred, len(class_names))
    print("mixture: %d components, %d EM iterations, converged %s, lower bound %.4f" % (gmm.n_components, gmm.n_iter_, gmm.converged_,
                                                                                      gmm.lower_bound_))
    print("held-out rows: %d, accuracy %.4f, macro F1 %.4f" % (test.numel(), m["accuracy"], m["macro_f1"]))
    print("confusion matrix (rows = true class, columns = diagnosed):")
    for name, row in zip(class_names, m["confusion_matrix"]):
        print("  %-20s %s" % (name, " ".join("%6d" % v for v in row)))

    mu, sigma = risk.estimate_mu_sigma_normal(results)
    monitor = risk.RiskMonitor(mu, sigma)
    diagnoser = diagnosis.FaultDiagnoser(gmm, comp_fault_prob)
    print("\n%8s %10s %-22s %s" % ("rows", "RF_smooth", "diagnosis (last row)", "probabilities"))
    for s in range(0, results.shape[0], 1024):
        chunk = results[s:s + 1024]
        rf = monitor.update(chunk)
        prob, pred = diagnoser.update(chunk)
        print("%8d %10.4f %-22s %s" % (s + chunk.shape[0], float(rf[-1]), class_names[int(pred[-1])],
                                       " ".join("%.3f" % v for v in prob[-1].tolist())))
    print("first RF warning at row %s, first danger at row %s" % (monitor.first_warning, monitor.first_danger))


if __name__ == "__main__":
    main()
