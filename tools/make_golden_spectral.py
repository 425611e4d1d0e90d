"""Generate tests/golden/g_spectral.npz: what scikit-learn and the reference's script 05 make of the `Spectral` method on
the split of tests/golden/g_cluster.npz (X_tr, y_tr, X_te, y_te).

Build machine only: needs a checkout of the reference (`--reference DIR`, as tools/make_golden_cluster.py), scikit-learn,
scipy and matplotlib importable (MPLBACKEND=Agg, nothing is drawn).  No test imports this file.  The fixture holds arrays
only:
  knn_indices     scikit-learn's 10 nearest neighbours of every training row, the row itself first [n, 10]
  eigenvalues     the 17 largest eigenvalues of S = D^{-1/2} A D^{-1/2} from a dense numpy.linalg.eigh, descending
  sk_embedding    scikit-learn's spectral_embedding(A, n_components=16, drop_first=False) [n, 16]
  labels, y_pred, metrics   the reference's fit_spectral_posterior at random_state = 42 (16 clusters)
  acc_range       smallest and largest accuracy of the reference over random_state = 0..9
  ari_range       smallest and largest adjusted Rand index of those ten label vectors against the one at 42
  knn_gap, eigengap   the measured margins of the conditions below
`--time` also prints scikit-learn's wall time of SpectralClustering.fit on this CPU at the fixture's size and at 1e4 rows
(printed, not stored: the fixture regenerates byte for byte).

Conditions on the inputs (asserted here): no duplicate rows; the relative gap between consecutive neighbour distances up to
the 11th >= 1e-9 in every row (so the lists and their order are determined); lambda_16 - lambda_17 >= 1e-4; the package's
host graph equals scikit-learn's; the Spectral row of g_cluster.npz's six_metrics is reproduced.
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "g_spectral.npz")
K, C, NEIGHBORS, SEED = 16, 4, 10, 42
METRICS = ("accuracy", "macro_precision", "macro_recall", "macro_f1")


def capturing_spectral():
    """sklearn.cluster.SpectralClustering replaced by a subclass that keeps the last fitted model: the reference imports
    the class inside its function and returns y_pred only."""
    import sklearn.cluster

    class Capture(sklearn.cluster.SpectralClustering):
        last = None

        def fit(self, X, y=None):
            out = super().fit(X, y)
            Capture.last = self
            return out
    sklearn.cluster.SpectralClustering = Capture
    return Capture


def build(ref):
    from sklearn.manifold import spectral_embedding
    from sklearn.metrics import adjusted_rand_score
    from sklearn.neighbors import NearestNeighbors, kneighbors_graph

    from pinn_amd import spectral as S
    G = np.load(os.path.join(ROOT, "tests", "golden", "g_cluster.npz"))
    X_tr, y_tr, X_te, y_te = G["X_tr"], G["y_tr"], G["X_te"], G["y_te"]
    n = X_tr.shape[0]
    assert len(np.unique(X_tr, axis=0)) == n, "duplicate rows"

    dist, knn = NearestNeighbors(n_neighbors=NEIGHBORS + 1).fit(X_tr).kneighbors(X_tr)
    d2 = dist ** 2
    gap = float(np.min((d2[:, 2:] - d2[:, 1:-1]) / d2[:, 2:]))             # column 0 is the row itself at distance 0
    assert gap >= 1e-9, gap
    knn = knn[:, :NEIGHBORS].astype(np.int64)
    assert np.array_equal(knn[:, 0], np.arange(n))
    A = kneighbors_graph(X_tr, NEIGHBORS, include_self=True)
    A = 0.5 * (A + A.T)
    mine = S.knn_graph(X_tr, NEIGHBORS, backend="host")
    assert np.array_equal(mine["indices"], knn), "the package's host graph differs from scikit-learn's"
    csr = S.knn_affinity(X_tr, NEIGHBORS, backend="host")
    B = A.tolil()
    B.setdiag(0)
    B = B.tocsr()
    B.eliminate_zeros()
    B.sort_indices()
    assert np.array_equal(csr["indptr"], B.indptr) and np.array_equal(csr["indices"], B.indices) and np.array_equal(csr["data"], B.data)

    dd = np.sqrt(csr["degree"])
    Sd = B.toarray() / dd[:, None] / dd[None, :]
    lam = np.linalg.eigvalsh(0.5 * (Sd + Sd.T))[::-1][:K + 1].copy()
    assert lam[K - 1] - lam[K] >= 1e-4, lam[K - 1] - lam[K]
    emb = spectral_embedding(A, n_components=K, drop_first=False, random_state=SEED)

    Capture = capturing_spectral()
    runs = {}
    for rs in [SEED] + list(range(10)):
        y_pred = ref.fit_spectral_posterior(X_tr, y_tr, X_te, n_classes=C, random_state=rs, n_clusters=K)
        runs[rs] = (Capture.last.labels_.astype(np.int64), np.asarray(y_pred).astype(np.int64))
    labels, y_pred = runs[SEED]
    m = ref.compute_macro_metrics(y_te, y_pred)
    metrics = np.array([m[k] for k in METRICS])
    six = dict(zip([str(s) for s in G["six_names"]], G["six_metrics"]))
    assert np.allclose(metrics, six["Spectral"], rtol=0, atol=1e-15), (metrics, six["Spectral"])
    accs = [float((runs[rs][1] == y_te).mean()) for rs in range(10)]
    aris = [float(adjusted_rand_score(labels, runs[rs][0])) for rs in range(10)]
    return {"knn_indices": knn, "eigenvalues": lam, "sk_embedding": emb, "labels": labels, "y_pred": y_pred, "metrics": metrics,
            "metric_names": np.array(METRICS), "acc_range": np.array([min(accs), max(accs)]), "ari_range": np.array([min(aris), max(aris)]),
            "knn_gap": np.array(gap), "eigengap": np.array(lam[K - 1] - lam[K]), "n_clusters": np.array(K, dtype=np.int64),
            "n_neighbors": np.array(NEIGHBORS, dtype=np.int64), "random_state": np.array(SEED, dtype=np.int64)}


def time_sklearn():
    from sklearn.cluster import SpectralClustering
    G = np.load(os.path.join(ROOT, "tests", "golden", "g_cluster.npz"))
    rng = np.random.default_rng(3)
    centres = rng.normal(0.0, 4.0, (K, 4))
    big = centres[rng.integers(K, size=10000)] + rng.normal(0.0, 1.0, (10000, 4))
    out = []
    for name, X in (("the fixture's %d x 4" % len(G["X_tr"]), G["X_tr"]), ("10000 x 4 blobs", big)):
        t0 = time.perf_counter()
        SpectralClustering(n_clusters=K, affinity="nearest_neighbors", random_state=SEED, n_neighbors=NEIGHBORS, n_init=10).fit(X)
        out.append("SpectralClustering.fit on %s: %.3f s" % (name, time.perf_counter() - t0))
    return out


def main():
    from make_golden_cluster import load_reference
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="folder holding the reference's scripts 03 and 05")
    ap.add_argument("--time", action="store_true", help="also time scikit-learn on this CPU")
    args = ap.parse_args()
    warnings.filterwarnings("ignore")
    _, ref = load_reference(args.reference)
    out = build(ref)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size <= 256 * 1024, size
    print("%d rows, neighbour gap %.3e, eigengap %.3e, %d bytes" % (len(out["labels"]), out["knn_gap"], out["eigengap"], size))
    print("reference at random_state %d: %s" % (SEED, " ".join("%s=%.4f" % (k, v) for k, v in zip(METRICS, out["metrics"]))))
    print("accuracy over random_state 0..9 %s, adjusted Rand index against %d %s" % (out["acc_range"], SEED, out["ari_range"]))
    if args.time:
        for line in time_sklearn():
            print("scikit-learn on this CPU:", line)


if __name__ == "__main__":
    sys.exit(main())
