"""The t-SNE figure of script 03 without the figure: train briefly on a synthetic recording with twelve fault segments,
assemble the results array on the device, diagnose the held-out rows with the Gaussian mixture as examples/fault_diagnosis.py
does, and embed those rows in two dimensions with exact t-SNE on the device (script 03's settings).  Prints the KL
divergence, the iterations run, the trustworthiness of the embedding and the distances between the centroids of the
diagnosed classes in it.

    python examples/embedding.py [--rows 6000] [--fault-rows 600] [--epochs 3000] [--components 20]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pinn_amd  # noqa: E402
from pinn_amd import diagnosis, embedding, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--fault-rows", type=int, default=600)
    ap.add_argument("--epochs", type=int, default=3000)
    ap.add_argument("--mc-times", type=int, default=32)
    ap.add_argument("--components", type=int, default=20)
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
    pos = torch.arange(X.shape[0], device=X.device)
    test, train = pos[pos % 4 == 3], pos[pos % 4 != 3]
    _, y_pred, _, _ = diagnosis.fit_gmm_and_get_probabilities(X[train], y[train], X[test], len(class_names),
                                                              random_state=diagnosis.RANDOM_STATE, n_components=args.components)

    # the held-out rows are read in place from the results array: feature columns and a gather list
    tsne = embedding.DeviceTSNE(**embedding.TSNE_TEST_PARAMS)
    emb = tsne.fit_transform(results, columns=features, row_index=kept[test])
    print("t-SNE of %d held-out rows: KL %.4f after %d iterations (learning rate %.1f)" % (emb.shape[0], tsne.kl_divergence_, tsne.n_iter_ + 1,
                                                                                           tsne.learning_rate_))
    print("trustworthiness (10 neighbours): %.4f" % embedding.trustworthiness(X[test], emb, n_neighbors=10))
    seen = [c for c in range(len(class_names)) if bool((y_pred == c).any())]      # a class may have received no row
    cent = torch.stack([emb[y_pred == c].mean(dim=0) for c in seen])
    dist = torch.cdist(cent, cent)
    print("distances between the centroids of the diagnosed classes:")
    for c, row in zip(seen, dist.tolist()):
        print("  %-20s %s" % (class_names[c], " ".join("%8.2f" % v for v in row)))
    for c in range(len(class_names)):
        if c not in seen:
            print("  %-20s no row was diagnosed as this class" % class_names[c])


if __name__ == "__main__":
    main()
