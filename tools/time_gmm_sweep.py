"""Time the batched model selection of pinn_amd.selection on the GPU against what it replaces ("Sweep and
selection").

The grid is the fixture's: K in {2, 4, 8, 12, 16, 20, 24, 32} x seeds 0-2, 24 candidates, D = 4, default tol / reg_covar.
Sizes: the 1349 training rows of tests/golden/g_gmm.npz, and 1.1e4 and 1e5 synthetic rows.  Per size, after one warm-up of
each side, alternating, `--reps` times: `gmm_sweep` end to end (device events around the call, which ends in a device
synchronise: it includes the Python wrapper, the uploads of the draws and the header reads) and the loop of 24
`DeviceGMM(backend="device").fit` calls, which is code this feature does not touch.  The median of each, their ratio, and the
sweep's phases (seeding, k-means, initial M-step, EM, scoring: device events between the entry points, from the median
run) go into one JSON line per size.  The loop does not score; the sweep's figure includes its scoring passes."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_amd import diagnosis as D, selection as S  # noqa: E402

GRID_K, SEEDS = (2, 4, 8, 12, 16, 20, 24, 32), (0, 1, 2)


def synthetic(n, seed=0):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 3.0, (8, 4))
    return centres[rng.integers(8, size=n)] + rng.normal(0.0, 1.0, (n, 4)) * rng.uniform(0.5, 1.5, 4)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1349,11000,100000")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_gmm_sweep.py measures on the GPU; none is present")
    fixture = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "g_gmm.npz")
    for n in [int(s) for s in args.sizes.split(",")]:
        X = np.load(fixture)["X_tr"] if n == 1349 else synthetic(n)
        Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()

        def sweep():
            t = {}
            return S.gmm_sweep(Xd, GRID_K, SEEDS, timings=t), t

        def loop():
            return [D.DeviceGMM(K, random_state=s, backend="device").fit(Xd) for K in GRID_K for s in SEEDS]
        sw, _ = sweep()
        fits = loop()
        torch.cuda.synchronize()
        res = {"rows": int(X.shape[0]), "candidates": len(sw), "n_iter_equal": [int(f.n_iter_) for f in fits] == [int(v) for v in sw.n_iter],
               "n_iter_max": int(sw.n_iter.max()), "selected_K_bic": int(sw.n_components[sw.best("bic")])}
        t_sweep, t_loop, phases = [], [], []
        for _ in range(args.reps):
            ms, (_, t) = timed(sweep)
            t_sweep.append(ms)
            phases.append(t)
            t_loop.append(timed(loop)[0])
        mid = int(np.argsort(t_sweep)[len(t_sweep) // 2])
        res.update(sweep_ms=float(np.median(t_sweep)), loop_ms=float(np.median(t_loop)), sweep_ms_all=[round(v, 2) for v in t_sweep],
                   loop_ms_all=[round(v, 2) for v in t_loop], phases_ms={k: round(v, 3) for k, v in phases[mid].items()})
        res["loop_over_sweep"] = res["loop_ms"] / res["sweep_ms"]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
