"""Time the clustering kernels of csrc/pinn_cluster.hip.

  Ward         DeviceWard.fit at 1e3 / 1e4 / 1e5 rows x 4 features: wall time of the whole fit (queueing, header reads, the
               host's sort and cut included), the chain steps it took, and the device time per chain step from events
               around a queue of steps on a fresh state
  Lloyd        one iteration (pinn_km_lloyd, 20 clusters x 4 features) at 1e5 / 1e6 / 1e7 rows, packed [n, 4] and in place
               (4 columns of a [n, 22] array), against the HBM floor of the bytes it must read and write
  assign       pinn_cluster_assign with a map (cluster, y_prob, y_pred out) at the same sizes
  host         the float64 numpy backend on this machine's CPU, at the sizes it finishes in reasonable time
Device events around the timed window after warm-up; the median of the repeats.  One JSON line per case.  scikit-learn's
wall times come from `tools/make_golden_cluster.py --time` on a machine that has it.

    python tools/time_cluster.py [--quick]
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

K, D, C = 20, 4, 4
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


def draw(n, seed=3):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 4.0, (K, D))
    return centres[rng.integers(K, size=n)] + rng.normal(0.0, 1.0, (n, D)), centres


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="skip the largest size of every group")
    args = ap.parse_args()
    from pinn_amd import _lib, comparison as P
    from pinn_amd._device import _DevRows, _ptr
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream

    for n in (1000, 10000) if args.quick else (1000, 10000, 100000):
        X, _ = draw(n)
        t_X = torch.from_numpy(X).cuda()
        P.DeviceWard(16, backend="device").fit(t_X[:256])                     # warm-up: module load, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w = P.DeviceWard(16, backend="device").fit(t_X)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        rows = _DevRows(torch, t_X)
        st = torch.zeros(lib.pinn_ward_state_bytes(n, D) // 8, dtype=torch.float64, device="cuda")
        wb = lib.pinn_ward_workspace_bytes(n, D)
        ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
        lib.pinn_ward_tree(*rows.head(), 1, 64, _ptr(st), _ptr(ws), wb, stream)      # fresh state: the next 512 steps all run
        steps = min(512, n - 200)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        lib.pinn_ward_tree(*rows.head(), 0, steps, _ptr(st), _ptr(ws), wb, stream)
        b.record()
        b.synchronize()
        rec = {"case": "ward", "rows": n, "fit_wall_s": round(wall, 4), "chain_steps": w.n_steps_, "bound": 3 * (n - 1),
               "us_per_step_device": round(1e3 * a.elapsed_time(b) / steps, 2), "state_MB": round(st.numel() * 8 / 1e6, 2)}
        if n <= 10000:
            t0 = time.perf_counter()
            P.DeviceWard(16, backend="host").fit(X)
            rec["host_fit_wall_s"] = round(time.perf_counter() - t0, 3)
        print(json.dumps(rec), flush=True)

    for n in (100000, 1000000) if args.quick else (100000, 1000000, 10000000):
        X, centres = draw(n)
        full = np.zeros((n, 22))
        full[:, 13:17] = X
        cmap = np.random.default_rng(0).dirichlet(np.ones(C), K)
        for layout, arr, cols in (("packed", torch.from_numpy(X).cuda(), None), ("in_place", torch.from_numpy(full).cuda(), [13, 14, 15, 16])):
            rows = _DevRows(torch, arr, cols)
            st, ws, wb = P._narrow(torch, lib, rows).state(K, centres)
            lib.pinn_km_lloyd(*rows.head(), K, 1, 0, 1e-4, 0, _ptr(st), _ptr(ws), wb, stream)

            def one():
                st[1:3] = 0.0                                             # clear CONVERGED and STATUS: the iteration always runs
                lib.pinn_km_lloyd(*rows.head(), K, 0, 1, 0.0, 0, _ptr(st), _ptr(ws), wb, stream)
            ms = timed(one, 3, 9)
            line = 32 if cols is None else 64                             # bytes of a row's columns, in 64-byte sectors when strided
            floor = n * (line + 16) / (HBM_GBPS * 1e9) * 1e3              # + label read and written
            print(json.dumps({"case": "lloyd_iteration", "layout": layout, "rows": n, "ms": round(ms, 4), "hbm_floor_ms": round(floor, 4)}), flush=True)
            ms = timed(lambda: P.assign_clusters(arr, centres, cmap, cols, None, "device", want=("cluster", "y_prob", "y_pred")), 3, 9)
            floor = n * (line + 8 + 8 * C + 8) / (HBM_GBPS * 1e9) * 1e3
            print(json.dumps({"case": "assign", "layout": layout, "rows": n, "ms": round(ms, 4), "hbm_floor_ms": round(floor, 4)}), flush=True)
            del arr, rows, st, ws
        if n <= 1000000:
            t0 = time.perf_counter()
            P.lloyd_iteration(X, centres, backend="host")
            t1 = time.perf_counter()
            P.assign_clusters(X, centres, cmap, backend="host", want=("cluster", "y_prob", "y_pred"))
            print(json.dumps({"case": "host", "rows": n, "lloyd_iteration_s": round(t1 - t0, 3), "assign_s": round(time.perf_counter() - t1, 3)}), flush=True)


if __name__ == "__main__":
    main()
