"""Time the change-point segmentation of pinn_amd.changepoint on the GPU: `segment`, `penalty_path` with 8
penalties in one call against the loop of 8 single-penalty calls, pruning on against off (time and cost evaluations), the
numpy backend at the sizes it finishes in reasonable time (`--host-sizes`), the per-step composition of the same recursion
from batched torch operations on the device (`--torch-sizes`: one step is a handful of launches over all candidates), and
`ChangeMonitor.update` at 2048-row chunks with a 4096-row window.

Shapes: 1.1e4 rows with D = 4 (the reference's size) with few (7) and with many (a change every 50 rows) true changes, 1e5
rows, 1e6 rows with max_len set.  Per call: one warm-up, then `--reps` calls timed with device events around the Python call
(it includes the wrapper, its allocations and the copy of the outputs to the host; the closing event synchronises the
stream).  The median goes into one JSON line.  The data is made on the device from a seed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_amd import changepoint as cp  # noqa: E402


def recording(n, D, every, seed=0):
    """z-scores with a change of mean every `every` rows, made on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, D, generator=g, device="cuda", dtype=torch.float64)
    level = torch.randn((n + every - 1) // every, D, generator=g, device="cuda", dtype=torch.float64) * 2.0
    return x + level[torch.arange(n, device="cuda") // every]


def timed(fn, reps):
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [round(v, 3) for v in ms], out


def torch_per_step(x, beta, min_len):
    """Optimal partitioning (kind "mean", no pruning) one step at a time from batched torch operations: prefix sums once, then
    per step the costs of all candidates, the minimum and two scalar writes.  Returns (F(n), change points)."""
    n, D = x.shape
    c = x - x[0]
    P = torch.cat([torch.zeros(1, 2 * D, dtype=x.dtype, device=x.device), torch.cumsum(torch.cat([c, c * c], dim=1), dim=0)])
    F = torch.full((n + 1,), float("inf"), dtype=x.dtype, device=x.device)
    F[0] = -beta
    last = torch.zeros(n + 1, dtype=torch.int64, device=x.device)
    lens = torch.arange(n, 0, -1, dtype=x.dtype, device=x.device)            # t - s for s = t - n .. t - 1: sliced per step
    for t in range(min_len, n + 1):
        hi = t - min_len + 1                                                # candidates s = 0 .. t - min_len
        d = P[t] - P[:hi]
        ln = lens[n - t:n - t + hi]
        ss = torch.clamp_min(d[:, D:] - d[:, :D] * d[:, :D] / ln[:, None], 0.0).sum(dim=1)
        v, i = torch.min(F[:hi] + ss + beta, dim=0)
        F[t], last[t] = v, i
    last = last.cpu().numpy()
    cps, u = [], n
    while last[u] > 0:
        u = int(last[u])
        cps.append(u)
    return float(F[n]), cps[::-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="11000:1500,11000:50,100000:2000,1000000:2000", help="rows:rows between true changes, comma separated")
    ap.add_argument("--features", type=int, default=4)
    ap.add_argument("--max-len-from", type=int, default=1000000, help="from this many rows on max_len is set (to --max-len)")
    ap.add_argument("--max-len", type=int, default=8192)
    ap.add_argument("--unpruned-sizes", default="11000,100000")
    ap.add_argument("--host-sizes", default="11000")
    ap.add_argument("--torch-sizes", default="11000")
    ap.add_argument("--min-len", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-monitor", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_changepoint.py measures on the GPU; none is present")
    ints = lambda s: {int(v) for v in s.split(",") if v}                      # noqa: E731
    unpruned, host_sizes, torch_sizes = ints(args.unpruned_sizes), ints(args.host_sizes), ints(args.torch_sizes)
    D = args.features
    for shape in args.shapes.split(","):
        n, every = [int(v) for v in shape.split(":")]
        x = recording(n, D, every)
        beta = cp.default_penalty(n, D, "mean")
        max_len = args.max_len if n >= args.max_len_from else None
        kw = dict(features=list(range(D)), min_len=args.min_len, max_len=max_len, backend="device")
        pens = [beta * f for f in (0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 4.0, 8.0)]
        base = {"rows": n, "D": D, "true_changes": (n - 1) // every, "max_len": max_len, "penalty": round(beta, 3)}

        ms, all_ms, seg = timed(lambda: cp.segment(x, penalty=beta, **kw), args.reps)
        res = dict(base, call="segment", device_ms=round(ms, 3), device_ms_all=all_ms, change_points=seg.n_change_points,
                   evaluations=int(seg.evaluations[0]), evals_per_us=round(int(seg.evaluations[0]) / ms / 1e3, 1))
        if n in unpruned:
            ms_off, all_off, off = timed(lambda: cp.segment(x, penalty=beta, prune=False, **kw), max(args.reps // 2, 1))
            assert np.array_equal(off.change_points[0], seg.change_points[0]) and off.F[0] == seg.F[0]
            res.update(unpruned_ms=round(ms_off, 3), unpruned_ms_all=all_off, unpruned_evaluations=int(off.evaluations[0]),
                       pruning_saves_evaluations=round(int(off.evaluations[0]) / int(seg.evaluations[0]), 2), pruning_saves_time=round(ms_off / ms, 2))
        if n in host_sizes:
            xh = x.cpu().numpy()
            t = time.perf_counter()
            h = cp.segment(xh, penalty=beta, **dict(kw, backend="numpy"))
            res["numpy_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            res["numpy_over_device"] = round(res["numpy_ms"] / ms, 1)
            assert np.array_equal(h.change_points[0], seg.change_points[0]) and h.F[0] == seg.F[0] and h.evaluations[0] == seg.evaluations[0]
        if n in torch_sizes and max_len is None:
            t = time.perf_counter()
            Ft, cps = torch_per_step(x, beta, args.min_len)
            torch.cuda.synchronize()
            res["torch_per_step_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            res["torch_per_step_over_device_unpruned"] = round(res["torch_per_step_ms"] / res.get("unpruned_ms", ms), 1)
            res["torch_per_step_same_change_points"] = cps == [int(v) for v in seg.change_points[0]]
        print(json.dumps(res), flush=True)

        ms8, all8, path = timed(lambda: cp.penalty_path(x, pens, **kw), args.reps)
        ms_loop, all_loop, _ = timed(lambda: [cp.segment(x, penalty=p, **kw) for p in pens], args.reps)
        print(json.dumps(dict(base, call="penalty_path", penalties=8, one_call_ms=round(ms8, 3), one_call_ms_all=all8,
                              loop_of_calls_ms=round(ms_loop, 3), loop_ms_all=all_loop, loop_over_one_call=round(ms_loop / ms8, 2),
                              change_points=[int(k) for k in path.n_change_points], evaluations=int(path.evaluations.sum()))), flush=True)

    if not args.no_monitor:
        x = recording(64 * 2048, D, 1500, seed=1)
        for backend in ("device", "numpy"):
            mon = cp.ChangeMonitor(4096, features=list(range(D)), min_len=args.min_len, backend=backend)
            data = x if backend == "device" else x.cpu().numpy()
            mon.update(data[:4096])
            ms = []
            for k in range(2, 2 + (args.reps if backend == "device" else 2) * 4):
                t = time.perf_counter()
                found, _ = mon.update(data[k * 2048:(k + 1) * 2048])
                if backend == "device":
                    torch.cuda.synchronize()
                ms.append((time.perf_counter() - t) * 1e3)
            print(json.dumps({"call": "ChangeMonitor.update", "backend": backend, "window": 4096, "chunk": 2048, "D": D,
                              "ms": round(float(np.median(ms)), 3), "ms_all": [round(v, 3) for v in ms], "evaluations": mon.evaluations,
                              "change_points_in_window": int(found.size)}), flush=True)


if __name__ == "__main__":
    main()
