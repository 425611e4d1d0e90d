"""Time the stages of pinn_amd.spectral on the device and on the host backend: the neighbour search, the affinity, the eigen
stage (outer iterations and products of S with the block), ten k-means restarts on the embedding and the whole fit.  Rows
are script 05's kind (D = 4, 16 overlapping blobs), or the training rows of tests/golden/g_cluster.npz for --n 1349.
Wall times around a device synchronisation, the best of --repeat runs after one warm-up.

    python tools/time_spectral.py [--n 1349 10000] [--repeat 3] [--skip-host]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, NEIGHBORS = 16, 10


def rows_of(n):
    G = np.load(os.path.join(ROOT, "tests", "golden", "g_cluster.npz"))
    if n == len(G["X_tr"]):
        return G["X_tr"]
    rng = np.random.default_rng(3)
    centres = rng.normal(0.0, 4.0, (K, 4))
    return centres[rng.integers(K, size=n)] + rng.normal(0.0, 1.0, (n, 4))


def best(fn, repeat, sync):
    fn()
    sync()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        sync()
        times.append(time.perf_counter() - t0)
    return min(times) * 1e3, out


def stages(S, X, backend, repeat, sync):
    rng = np.random.default_rng(42)
    t_knn, g = best(lambda: S.knn_graph(X, NEIGHBORS, backend=backend), repeat, sync)
    t_aff, A = best(lambda: S.knn_affinity(knn=g["indices"], backend=backend), repeat, sync)
    t_eig, e = best(lambda: S.spectral_embedding(A, K, random_state=42, backend=backend), repeat, sync)
    t_km, _ = best(lambda: S._kmeans_restarts(e["embedding"], K, 10, np.random.default_rng(rng.integers(1 << 30)), backend), repeat, sync)
    t_fit, m = best(lambda: S.DeviceSpectralClustering(K, random_state=42, backend=backend).fit(X), repeat, sync)
    return ("knn %.1f ms, affinity %.1f ms, eigen stage %.1f ms (%d outer iterations, %d products, residual %.1e), 10 k-means restarts %.1f ms, "
            "fit %.1f ms (inertia %.5f)" % (t_knn, t_aff, t_eig, e["n_iter"], e["n_matvec"], float(np.max(np.asarray(e["residuals"].cpu() if hasattr(e["residuals"], "cpu") else e["residuals"]))),
                                            t_km, t_fit, m.inertia_))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1349, 10000])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    import torch

    from pinn_amd import spectral as S
    for n in args.n:
        X = rows_of(n)
        print("n = %d, device: %s" % (n, stages(S, torch.from_numpy(X).cuda(), "device", args.repeat, torch.cuda.synchronize)), flush=True)
        if not args.skip_host:
            print("n = %d, host:   %s" % (n, stages(S, X, "host", 1, lambda: None)), flush=True)


if __name__ == "__main__":
    sys.exit(main())
