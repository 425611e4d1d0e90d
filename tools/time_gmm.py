"""Time the Gaussian-mixture fault diagnosis of pinn_amd.diagnosis on the GPU.

For 1e5 / 1e6 / 1e7 rows, D = 4 features, K = 20 components: one EM iteration (device events after warm-up, the median of
`--reps` repetitions of a batch of iterations with the stopping rule disabled by tol = 0), a full fit from k-means-like
labels, and predict_proba; each on packed rows (32 B/row) and, for the iteration, read in place from a 22-column results
array (176 B/row, the bytes the hardware fetches when 4 of 22 columns are used: every 128-byte line of the row is touched).
Beside them: the HBM floor of the pass at `--hbm-gbs`, the same EM iteration composed of torch float64 device ops (the
honest competitor), and this package's host backend (numpy, this machine's CPU; skipped at 1e7 rows).  Prints one JSON line
per size.  The scikit-learn figure of DESIGN 3g comes from `tools/make_golden_gmm.py --time` on the build machine's CPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_amd import diagnosis as D  # noqa: E402

K, DM = 20, 4


def data(n, seed=0):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 4.0, (K, DM))
    z = rng.integers(K, size=n)
    return centres[z] + rng.normal(0.0, 1.0, (n, DM)), z


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


def torch_em_iteration(X, w, mu, U):
    """One EM iteration as torch float64 ops: batched (x - mu) @ U, logsumexp, moments by matmul, Cholesky."""
    n, d = X.shape
    y = torch.einsum("nki,kij->nkj", X[:, None, :] - mu[None], U)
    lp = -0.5 * (d * np.log(2 * np.pi) + (y * y).sum(-1)) + torch.log(torch.diagonal(U, dim1=1, dim2=2)).sum(-1) + torch.log(w)
    lpn = torch.logsumexp(lp, dim=1)
    r = torch.exp(lp - lpn[:, None])
    nk = r.sum(0) + D.EPS10
    mu2 = (r.T @ X) / nk[:, None]
    diff = X[:, None, :] - mu2[None]
    cov = torch.einsum("nk,nki,nkj->kij", r, diff, diff) / nk[:, None, None] + 1e-6 * torch.eye(d, dtype=X.dtype, device=X.device)
    L = torch.linalg.cholesky(cov)
    U2 = torch.linalg.solve_triangular(L, torch.eye(d, dtype=X.dtype, device=X.device).expand_as(L), upper=False).transpose(1, 2)
    return nk / nk.sum(), mu2, U2, lpn.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="EM iterations per timed batch")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM bandwidth for the floor, GB/s (MI355X peak: 8000)")
    args = ap.parse_args()
    for n in [int(s) for s in args.sizes.split(",")]:
        X, z = data(n)
        Xd = torch.from_numpy(X).cuda()
        wide = torch.zeros(n, 22, dtype=torch.float64, device="cuda")
        cols = [13, 14, 15, 16]
        wide[:, cols] = Xd
        lab = np.where(np.random.default_rng(1).uniform(size=n) < 0.2, (z + 1) % K, z)
        g = D.DeviceGMM(K, labels_init=lab, max_iter=0, tol=0.0, backend="device", em_chunk=args.iters).fit(Xd)
        res = {"rows": n, "K": K, "D": DM, "iters_per_batch": args.iters}
        res["em_iteration_packed_ms"] = event_ms(lambda: g.em_iterations(Xd, args.iters), args.reps) / args.iters
        gw = D.DeviceGMM(K, labels_init=lab, max_iter=0, tol=0.0, backend="device", em_chunk=args.iters).fit(wide, columns=cols)
        res["em_iteration_in_place_ms"] = event_ms(lambda: gw.em_iterations(wide, args.iters, columns=cols), args.reps) / args.iters
        res["hbm_floor_packed_ms"] = n * 32 / (args.hbm_gbs * 1e9) * 1e3
        res["hbm_floor_in_place_ms"] = n * 176 / (args.hbm_gbs * 1e9) * 1e3
        res["predict_proba_ms"] = event_ms(lambda: g.predict_proba(Xd), args.reps)
        t0 = time.perf_counter()
        f = D.DeviceGMM(K, labels_init=lab, backend="device").fit(Xd)
        torch.cuda.synchronize()
        res["full_fit_ms"], res["full_fit_iterations"] = (time.perf_counter() - t0) * 1e3, f.n_iter_
        try:
            w, mu, U = (torch.as_tensor(a).cuda() for a in (D._as_numpy(g.weights_), D._as_numpy(g.means_), D._as_numpy(g.precisions_cholesky_)))
            res["torch_em_iteration_ms"] = event_ms(lambda: torch_em_iteration(Xd, w, mu, U), max(3, args.reps // 2))
        except RuntimeError as e:                     # the [n, K, D] temporaries do not fit
            res["torch_em_iteration_ms"] = None
            res["torch_note"] = str(e).splitlines()[0][:80]
        if n <= 1000000:
            gh = D.DeviceGMM(K, labels_init=lab, max_iter=0, tol=0.0, backend="host").fit(X)
            t0 = time.perf_counter()
            gh.em_iterations(X, 1)
            res["host_em_iteration_ms"] = (time.perf_counter() - t0) * 1e3
        print(json.dumps(res), flush=True)
        del Xd, wide


if __name__ == "__main__":
    main()
