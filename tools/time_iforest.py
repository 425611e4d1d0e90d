"""Time the isolation-forest kernels of csrc/pinn_iforest.hip.

  fit          pinn_if_fit, 200 trees x 256 rows on 1e5 rows x D features: device time of the one launch from events, and the
               wall time of DeviceIsolationForest.fit (the launch, one read of the trees, packing the block on the host)
  score        pinn_if_score (depth sum, score and prediction out) with a forest of 200 trees fitted here, at 1e5 / 1e6 / 1e7
               rows, D = 2 and 4, packed [n, D] and in place (D columns of a [n, 22] array); variant 0 (trees staged through
               LDS) and variant 1 (nodes read from global memory, the forest resident in L2); against the HBM floor of the
               bytes it must read and write, and per (row, tree, level) step
  torch        the same descent composed of torch device ops (gathers and where, tree by tree, level by level), 1e5 and 1e6 rows
  scikit-learn IsolationForest.score_samples of an imported copy of the same forest on this machine's CPU, where installed
  host         the numpy backend
Device events around the timed window after warm-up; the median of the repeats.  One JSON line per case.

    python tools/time_iforest.py [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_TREES = 200
HBM_GBPS = 8000.0                        # MI355X peak; the floor below is bytes / this


def timed(fn, warm, reps):
    for _ in range(warm):
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
    return statistics.median(out)


def draw(n, D, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, D)) * np.linspace(1.0, 0.3, D)
    X[rng.random(n) < 0.02] *= 4.0
    return X


def torch_descent(forest, X32):
    """Depth sums by torch device ops: per tree one gather chain over the levels (float64 thresholds, as the host backend)."""
    total = torch.zeros(X32.shape[0], dtype=torch.float64, device=X32.device)
    rows = torch.arange(X32.shape[0], device=X32.device)
    for (feature, threshold, left, right, value, depth) in forest:
        node = torch.zeros(X32.shape[0], dtype=torch.int64, device=X32.device)
        for _ in range(depth):
            f = feature[node]
            inner = f >= 0
            x = X32[rows, f.clamp(min=0)].to(torch.float64)
            node = torch.where(inner, torch.where(x <= threshold[node], left[node], right[node]), node)
        total += value[node]
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="skip 1e7 rows and the torch composition at 1e6")
    args = ap.parse_args()
    from pinn_amd import _lib, anomaly as A
    from pinn_amd._device import _DevRows, _ptr
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream

    for D in (2, 4):
        X = draw(100000, D)
        t_X = torch.from_numpy(X).cuda()
        A.DeviceIsolationForest(T_TREES, random_state=1, backend="device").fit(t_X[:1000])          # warm-up: module load, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        forest = A.DeviceIsolationForest(T_TREES, random_state=1, backend="device").fit(t_X)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        rows, m = _DevRows(torch, t_X), forest.max_samples_
        M = 2 * m - 1
        i32 = dict(dtype=torch.int32, device="cuda")
        bufs = [torch.empty(T_TREES * M, **i32), torch.empty(T_TREES * M, dtype=torch.float64, device="cuda"), torch.empty(T_TREES * M, **i32),
                torch.empty(T_TREES * M, **i32), torch.empty(T_TREES * M, **i32), torch.empty(T_TREES, **i32),
                torch.empty(T_TREES * m, dtype=torch.int64, device="cuda"), torch.empty(T_TREES, **i32)]
        ms = timed(lambda: lib.pinn_if_fit(*rows.head(), T_TREES, m, A.max_depth_of(m), 1, *[_ptr(b) for b in bufs], stream), 3, 9)
        t0 = time.perf_counter()
        A.DeviceIsolationForest(T_TREES, random_state=1, backend="host").fit(X)
        host_s = time.perf_counter() - t0
        nodes = sum(len(t[0]) for t in forest.trees_)
        print(json.dumps({"case": "fit", "D": D, "rows": 100000, "trees": T_TREES, "max_samples": m, "nodes": nodes, "block_bytes": forest._block.nbytes,
                          "launch_ms": round(ms, 4), "fit_wall_s": round(wall, 4), "host_fit_wall_s": round(host_s, 3)}), flush=True)

        levels = float(np.mean([np.average(A.tree_depths(t[2], t[3])[t[0] < 0], weights=t[4][t[0] < 0]) for t in forest.trees_]))
        dev_forest = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (t[0], t[1], t[2], t[3], v)) + (int(A.tree_depths(t[2], t[3]).max()),)
                      for t, v in zip(forest.trees_, forest._values)]
        try:
            from sklearn.ensemble import IsolationForest
            sk = IsolationForest(n_estimators=T_TREES, random_state=1).fit(X[:20000])
        except ImportError:
            sk = None
        for n in (100000, 1000000) if args.quick else (100000, 1000000, 10000000):
            Xn = draw(n, D, seed=5)
            full = np.zeros((n, 22))
            cols = [11, 12, 3, 5][:D]
            full[:, cols] = Xn
            for layout, arr, cc in (("packed", torch.from_numpy(Xn).cuda(), None), ("in_place", torch.from_numpy(full).cuda(), cols)):
                r = _DevRows(torch, arr, cc)
                block = forest._device_block(torch, arr.device)
                out = [torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda"),
                       torch.empty(n, dtype=torch.int64, device="cuda")]
                line = 8 * D if cc is None else 64 * (1 if D <= 2 else 2)       # bytes of a row's columns, in 64-byte sectors when strided
                floor = n * (line + 24) / (HBM_GBPS * 1e9) * 1e3
                rec = {"case": "score", "D": D, "layout": layout, "rows": n, "hbm_floor_ms": round(floor, 4), "mean_levels": round(levels, 2)}
                for variant, name in ((0, "lds_ms"), (1, "l2_ms")):
                    ms = timed(lambda: lib.pinn_if_score(*r.head(), _ptr(block), -0.5, *[_ptr(o) for o in out], variant, stream), 3, 9)
                    rec[name] = round(ms, 4)
                    rec[name.replace("_ms", "_ps_per_step")] = round(ms * 1e9 / (n * T_TREES * levels), 2)
                print(json.dumps(rec), flush=True)
                del arr, r, out
            if n <= (100000 if args.quick else 1000000):
                X32 = torch.from_numpy(Xn.astype(np.float32)).cuda()
                ms = timed(lambda: torch_descent(dev_forest, X32), 1, 3)
                ok = bool(torch.equal(torch_descent(dev_forest, X32), forest.depth_sums(torch.from_numpy(Xn).cuda())))
                print(json.dumps({"case": "torch_ops", "D": D, "rows": n, "ms": round(ms, 3), "equal_to_kernel": ok}), flush=True)
                del X32
            if n <= 1000000:
                t0 = time.perf_counter()
                forest.backend = "host"
                forest.score_samples(Xn)
                forest.backend = "device"
                rec = {"case": "cpu", "D": D, "rows": n, "host_backend_s": round(time.perf_counter() - t0, 3)}
                if sk is not None:
                    t0 = time.perf_counter()
                    sk.score_samples(Xn)
                    rec["sklearn_score_samples_s"] = round(time.perf_counter() - t0, 3)
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
