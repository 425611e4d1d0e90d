"""Time pinn_amd.uncertainty on the GPU: `score_uncertainty` (1 and 5 groups), `conformal_quantiles` (1 and 8
levels, 1 and 5 groups) and `UncertaintyMonitor.update` (chunks of 2048 rows) at 1.1e4, 1e6 and 1e7 rows of a 22-column
float64 results array, against the same results composed from torch operations on the device (masks per group, `torch.sort` /
`torch.kthvalue`) and against the host backend at the sizes it finishes in reasonable time (`--host-sizes`).

Per (rows, call): one warm-up, then `--reps` calls timed with device events around the Python call (it includes the wrapper,
its allocations and the copy of the few result words to the host; the stream is synchronised by the closing event).  The
median goes into one JSON line, with the HBM floor: a pass over a 22-column float64 array moves 176 B per row whichever
columns it reads (a row is shorter than two cache lines), the select makes at most 8 passes (fewer once it gathers the
surviving keys, so its `floor_over_measured` can exceed 1; `one_pass_floors` is the measured time in floors of one pass),
and a plain copy reaches 6.29 TB/s of the 8 TB/s peak on an MI355X.  The data is made on the device from a seed."""
import argparse
import json
import os
import sys
import time
from statistics import NormalDist

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_amd import uncertainty as U  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
ROW_BYTES = 22 * 8
GROUPS5 = {"normal": [0], "flooding": [1, 2, 3], "oxygen_starvation": [4, 5, 6], "membrane_drying": [7, 8, 9], "hydrogen_starvation": [10, 11, 12]}


def results(n, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(n, 22, generator=g, device="cuda", dtype=torch.float64)
    A[:, 10] = 0.8 + 1.2 * torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    A[:, 11] = 0.8 + 1.2 * torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    A[:, 8] = A[:, 9] + torch.sqrt(A[:, 10] ** 2 + A[:, 11] ** 2) * torch.randn(n, generator=g, device="cuda", dtype=torch.float64)
    A[:, 17] = (torch.arange(n, device="cuda") * 13 // max(n, 1)).double()
    return A


def torch_masks(A, groups):
    lab = A[:, 17].long()
    return [torch.ones_like(lab, dtype=torch.bool)] if groups is None else [torch.isin(lab, torch.tensor(v, device="cuda")) for v in groups.values()]


def torch_z(A):
    v = A[:, 10] * A[:, 10] + A[:, 11] * A[:, 11]
    s = torch.sqrt(v)
    return (A[:, 8] - A[:, 9]) / s, s, v


def torch_score(A, groups, levels=U.LEVELS, bins=20):
    """The report's numbers from torch operations: the same sums, hits and PIT histogram per group."""
    nd = NormalDist()
    z, s, v = torch_z(A)
    r = A[:, 8] - A[:, 9]
    phi = 0.5 * torch.erfc(-z * U.INV_SQRT2)
    nll = 0.5 * (U.LOG_2PI + torch.log(v) + z * z)
    crps = s * (z * (2.0 * phi - 1.0) + 2.0 * torch.exp(-0.5 * z * z) * U.INV_SQRT2PI - U.INV_SQRTPI)
    edges = torch.tensor([nd.inv_cdf(i / bins) for i in range(1, bins)], device="cuda", dtype=torch.float64)
    zl = [nd.inv_cdf(0.5 + 0.5 * lv) for lv in levels]
    out = []
    for m in torch_masks(A, groups):
        sums = torch.stack([t[m].sum() for t in (r, r * r, s, v, z, z * z, nll, crps)])
        hits = torch.stack([(z[m].abs() <= t).sum() for t in zl])
        pit = torch.bincount(torch.bucketize(z[m], edges, right=True), minlength=bins)
        out.append((sums.cpu(), hits.cpu(), pit.cpu()))
    return out


def torch_quantiles(A, groups, levels, how):
    z, _, _ = torch_z(A)
    az = z.abs()
    out = []
    for m in torch_masks(A, groups):
        sc = az[m]
        n = sc.numel()
        ks = [min(max(int(np.ceil((n + 1) * lv)), 1), n) for lv in levels]
        if how == "sort":
            srt = torch.sort(sc).values
            out.append(torch.stack([srt[k - 1] for k in ks]).cpu())
        else:
            out.append(torch.stack([torch.kthvalue(sc, k).values for k in ks]).cpu())
    return out


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [round(v, 3) for v in ms]


def host_timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="11000,1000000,10000000")
    ap.add_argument("--host-sizes", default="11000,1000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--monitor-rows", type=int, default=204800, help="rows replayed through the monitor (chunks of 2048)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_uncertainty.py measures on the GPU; none is present")
    host_sizes = {int(s) for s in args.host_sizes.split(",") if s}
    lv8 = (0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99, 0.999)
    for n in [int(s) for s in args.sizes.split(",")]:
        A = results(n)
        calls = []
        for gname, groups in (("1", None), ("5", GROUPS5)):
            calls.append(("score/groups=%s" % gname, 1, lambda b, X, g=groups: U.score_uncertainty(X, groups=g, backend=b),
                          [("torch", lambda g=groups: torch_score(A, g))]))
            for lname, lv in (("1", (0.9,)), ("8", lv8)):
                calls.append(("quantiles/levels=%s/groups=%s" % (lname, gname), 8,
                              lambda b, X, g=groups, l=lv: U.conformal_quantiles(X, levels=l, groups=g, backend=b),
                              [("torch_sort", lambda g=groups, l=lv: torch_quantiles(A, g, l, "sort")),
                               ("torch_kthvalue", lambda g=groups, l=lv: torch_quantiles(A, g, l, "kth"))]))
        for name, passes, fn, others in calls:
            ms, all_ms = timed(lambda: fn("device", A), args.reps)
            floor_ms = passes * n * ROW_BYTES / HBM_BYTES_PER_S * 1e3
            res = {"call": name, "rows": n, "device_ms": round(ms, 4), "device_ms_all": all_ms, "ns_per_row": round(ms * 1e6 / n, 3),
                   "passes": passes, "hbm_floor_ms": round(floor_ms, 5), "floor_over_measured": round(floor_ms / ms, 5),
                   "one_pass_floors": round(ms * passes / floor_ms, 2)}
            for oname, ofn in others:
                oms, _ = timed(ofn, args.reps)
                res[oname + "_ms"] = round(oms, 4)
                res[oname + "_over_device"] = round(oms / ms, 2)
            if n in host_sizes:
                Ah = A.cpu().numpy()
                res["host_ms"] = round(host_timed(lambda: fn("host", Ah)), 2)
                res["host_over_device"] = round(res["host_ms"] / ms, 1)
            print(json.dumps(res), flush=True)
    # the monitor: launches per second matter, not bytes
    n = args.monitor_rows
    A = results(n)
    chunks = [A[i:i + U.MAX_CHUNK] for i in range(0, n, U.MAX_CHUNK)]

    def replay(backend, parts):
        mon = U.UncertaintyMonitor(level=0.9, window=4096, gamma=0.005, backend=backend)
        for c in parts:
            mon.update(c)
        return mon.q

    ms, all_ms = timed(lambda: replay("device", chunks), args.reps)
    res = {"call": "monitor/window=4096", "rows": n, "chunks": len(chunks), "device_ms": round(ms, 3), "device_ms_all": all_ms,
           "us_per_chunk": round(ms * 1e3 / len(chunks), 2)}
    hchunks = [c.cpu().numpy() for c in chunks]
    res["host_ms"] = round(host_timed(lambda: replay("host", hchunks)), 2)
    res["host_over_device"] = round(res["host_ms"] / ms, 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
