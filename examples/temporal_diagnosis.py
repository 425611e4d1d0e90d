"""Temporal diagnosis end to end on the device: build the results array as examples/fault_diagnosis.py does, diagnose every
row with the Gaussian mixture, then put a hidden Markov chain over the classes with the per-row posteriors as emissions and
filter, smooth and decode the recording.  Prints the accuracy and the number of label switches of the four label series, then
replays the recording in chunks through `TemporalDiagnoser`.

    python examples/temporal_diagnosis.py [--rows 6000] [--fault-rows 600] [--epochs 3000] [--components 20] [--stay 0.99] [--fit]

With --fit the transition matrix is not `sticky_transitions(S, stay)`: Baum-Welch estimates it from the recording itself,
started from the sticky matrix.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pinn_amd  # noqa: E402
from pinn_amd import diagnosis, synth, temporal  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--fault-rows", type=int, default=600)
    ap.add_argument("--epochs", type=int, default=3000)
    ap.add_argument("--mc-times", type=int, default=32)
    ap.add_argument("--components", type=int, default=20)
    ap.add_argument("--stay", type=float, default=0.99)
    ap.add_argument("--fit", action="store_true", help="estimate the transitions by Baum-Welch instead of taking the sticky matrix")
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
    S = len(class_names)
    pos = torch.arange(X.shape[0], device=X.device)
    train = pos[pos % 4 != 3]
    _, _, gmm, comp_fault_prob = diagnosis.fit_gmm_and_get_probabilities(
        X[train], y[train], X[train], S, random_state=diagnosis.RANDOM_STATE, n_components=args.components)
    y_prob, y_pred = gmm.diagnose(X, comp_fault_prob)           # every kept row, in time order
    y_prob = y_prob.double()

    prior = torch.bincount(y[train].long(), minlength=S).double() / train.numel()
    hmm = temporal.DeviceHMM(temporal.sticky_transitions(S, args.stay), prior=prior.clamp_min(1e-6).cpu().numpy())
    if args.fit:
        hmm.fit_transitions(y_prob, n_iter=50, tol=1e-6)
        print("Baum-Welch: %d iterations, converged %s, log-likelihood %.3f -> %.3f" %
              (hmm.n_iter_, hmm.converged_, hmm.loglik_history_[0], hmm.loglik_history_[-1]))
        print("fitted transitions:\n%s" % "\n".join("  " + " ".join("%.4f" % v for v in row) for row in hmm.transitions_))
    alpha, loglik, _ = hmm.filter(y_prob)
    gamma, _ = hmm.smooth(y_prob)
    path, logprob = hmm.viterbi(y_prob)
    truth = y.long()
    print("rows %d, classes %d, log-likelihood %.3f, path log-probability %.3f" % (y_prob.shape[0], S, float(loglik[0]), float(logprob[0])))
    print("%-10s %9s %9s" % ("labels", "accuracy", "switches"))
    for name, labels in (("per row", y_pred.long()), ("filtered", alpha.argmax(1)), ("smoothed", gamma.argmax(1)), ("viterbi", path)):
        print("%-10s %9.4f %9d" % (name, float((labels == truth).double().mean()), int((labels[1:] != labels[:-1]).sum())))
    print("%-10s %9s %9d" % ("truth", "", int((truth[1:] != truth[:-1]).sum())))

    online = temporal.TemporalDiagnoser(hmm)
    print("\n%8s %-22s %s" % ("rows", "filtered (last row)", "probabilities"))
    for s in range(0, y_prob.shape[0], 1024):
        prob, pred = online.update(y_prob[s:s + 1024])
        print("%8d %-22s %s" % (online.n_seen, class_names[int(pred[-1])], " ".join("%.3f" % v for v in prob[-1].tolist())))
    print("label switches online: %d" % online.switches)


if __name__ == "__main__":
    main()
