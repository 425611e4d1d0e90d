"""Which residual made the diagnosis say so: train briefly on a synthetic recording with twelve fault segments, assemble the
results array on the device, fit and calibrate the Gaussian mixture as examples/fault_diagnosis.py does, then attribute the
fault probabilities of one fault segment to the four physics residuals with exact Shapley values (all 2^4 coalitions
against the normal rows as the background) and print the residuals that matter most per class.

    python examples/explain_diagnosis.py [--rows 6000] [--fault-rows 600] [--epochs 3000] [--segment 1] [--voltage]

The synthetic recording's fault segments differ little in their residuals (the printed accuracy says how little), so its
diagnoses sit near 1 / 4 and the attributions are small; the example shows the calls, a real recording shows the effect.

With --voltage the voltage network itself is explained too: its prediction and log-variance on the same segment are
attributed to the eight sensors (2^8 coalitions, 64 normal rows as the background).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pinn_amd  # noqa: E402
from pinn_amd import diagnosis, explain, synth  # noqa: E402
from pinn_amd.risk import INDEX  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--fault-rows", type=int, default=600)
    ap.add_argument("--epochs", type=int, default=3000)
    ap.add_argument("--mc-times", type=int, default=32)
    ap.add_argument("--components", type=int, default=20)
    ap.add_argument("--segment", type=int, default=1, help="the fault segment to explain, 1..12")
    ap.add_argument("--background", type=int, default=512, help="normal rows in the background")
    ap.add_argument("--voltage", action="store_true", help="also attribute the voltage network's outputs to the sensors")
    args = ap.parse_args()

    ds = synth.make_dataset(args.rows, (args.fault_rows,) * 12, seed=0)
    torch.manual_seed(0)
    model = pinn_amd.PhysicsInformedNN(ds[0], ds[1], [8, 256, 256, 256, 1], ds[4], ds[5], p=0.2, logvar=True, seed=1)
    model.verbose = False
    model.train_dnn(args.epochs)
    results = pinn_amd.create_comprehensive_results_array_v2(model, ds, mc_times=args.mc_times, dropout=0.2, device_output=True)

    features = diagnosis.parse_features(diagnosis.DEFAULT_FEATURES)
    names = [n for c in features for n, i in INDEX.items() if i == c]
    label_map, class_names = diagnosis.build_label_mapper(diagnosis.parse_group_spec(diagnosis.DEFAULT_GROUP_SPEC))
    X, y, kept = diagnosis.extract_X_y(results, features, label_map, return_index=True)
    _, _, gmm, comp_fault_prob = diagnosis.fit_gmm_and_get_probabilities(X, y, X[:1], len(class_names), random_state=diagnosis.RANDOM_STATE,
                                                                         n_components=args.components)

    m = diagnosis.classification_metrics(y, gmm.diagnose(X, comp_fault_prob)[1], len(class_names))
    print("mixture: %d components on %d fault rows, accuracy on them %.4f (how much the residuals of this recording tell)" % (
        gmm.n_components, X.shape[0], m["accuracy"]))

    # the segment to explain and the background: rows of the results array, read in place through gather lists
    label = results[:, INDEX["label"]]
    segment = torch.nonzero(label == args.segment).reshape(-1)
    normal = torch.nonzero(label == 0).reshape(-1)
    normal = normal[torch.linspace(0, normal.numel() - 1, min(args.background, normal.numel()), device=normal.device).long()]
    r = explain.shapley_diagnosis(gmm, comp_fault_prob, results, results, columns=features, row_index=segment, background_index=normal)
    gap = (r.phi.sum(dim=1) - (r.fx - r.base)).abs().max()
    print("segment %d: %d rows explained against %d normal rows; sum of attributions = f(x) - base within %.1e" % (
        args.segment, segment.numel(), normal.numel(), float(gap)))
    print("mean diagnosis of the segment: " + ", ".join("%s %.3f" % (c, v) for c, v in zip(class_names, r.fx.mean(dim=0).tolist())))
    print("mean diagnosis of the background: " + ", ".join("%s %.3f" % (c, v) for c, v in zip(class_names, r.base.tolist())))
    for t in explain.top_features(r.phi, names, class_names, topn=2):
        print("  %-20s moved most by %s; on average raised by %s(%+.3f), lowered by %s(%+.3f)" % (
            t["class"], ", ".join("%s(%.3f)" % p for p in t["importance"]), *t["positive"][0], *t["negative"][0]))

    # the online form: the same attributions chunk by chunk, next to the diagnoser
    ex = explain.DiagnosisExplainer(gmm, comp_fault_prob, results[normal])
    chunk = results[segment[0]:segment[0] + 256]
    phi, y_prob = ex.update(chunk)
    print("online: a chunk of %d rows -> phi %s, y_prob %s" % (chunk.shape[0], tuple(phi.shape), tuple(y_prob.shape)))

    if args.voltage:
        sensors = ["x%d" % i for i in range(8)]
        x_norm = torch.as_tensor(ds[2], dtype=torch.float32).cuda()      # the normalised sensors of every row, in the results' order
        lab_rows = label[:x_norm.shape[0]]
        seg = torch.nonzero(lab_rows == args.segment).reshape(-1)[:256]
        bg = torch.nonzero(lab_rows == 0).reshape(-1)[:64]
        if seg.numel() and bg.numel():
            v = explain.shapley_values(explain.voltage_predictor(model), x_norm, x_norm, row_index=seg, background_index=bg, dtype="float32")
            for t in explain.top_features(v.phi, sensors, ["voltage (normalised)", "log-variance"], topn=3):
                print("  %-22s moved most by %s" % (t["class"], ", ".join("%s(%.4f)" % p for p in t["importance"])))


if __name__ == "__main__":
    main()
