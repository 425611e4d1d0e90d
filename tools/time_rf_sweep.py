"""Time the RF parameter sweep against what it replaces.  python tools/time_rf_sweep.py [--reps 15]

Layout of examples/early_warning.py: 6000 normal rows, then twelve fault segments of 600 rows (labels 1..12), one condition
per segment: 13 segments and 13 200 rows per candidate.  In one process, after warm-up, medians with the spread:
  - rf_sweep on the device at P = 256 and P = 4096: the whole call (selection of the rows, table upload, the two launches
    and the voltage alarms) by a host clock around a synchronise, and the two launches of pinn_rf_sweep alone by device events;
  - a loop of P = 256 calls of rf_advance_for_conditions on the device, which is what a user had before the sweep
    (it yields the condition indices only: a second call per candidate would be needed for the quiet rows);
  - the host backend at P = 16;
  - the launches at P = 4096 without the quiet rows and with them cut into one-tile ranges: the cost of the one long segment.
Each figure is printed as median [min .. max] over the repetitions.  A machine without a GPU fails: nothing falls back."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pinn_amd import risk  # noqa: E402
from pinn_amd._device import call  # noqa: E402

N_NORMAL, N_FAULT, FAULT_ROWS = 6000, 12, 600


def recording(seed=3):
    rng = np.random.default_rng(seed)
    n = N_NORMAL + N_FAULT * FAULT_ROWS
    a = np.zeros((n, 22))
    a[:, 12:17] = rng.normal(size=(n, 5))
    a[:, 8] = 3.4 + rng.normal(0, 0.005, n)
    ramp = np.linspace(0.0, 1.0, FAULT_ROWS)
    for k in range(1, N_FAULT + 1):
        rows = slice(N_NORMAL + (k - 1) * FAULT_ROWS, N_NORMAL + k * FAULT_ROWS)
        a[rows, 17] = k
        a[rows, 12 + (k % 5)] += (6.0 + k) * ramp ** 1.5
        a[rows, 8] -= 0.25 * ramp
    return a


def candidates(P, seed=0):
    rng = np.random.default_rng(seed)
    return {"z_safe": rng.uniform(1.5, 3.0, P), "lambda_decay": rng.uniform(0.99, 1.0, P), "alpha_smooth": rng.uniform(0.1, 1.0, P),
            "p_layer": rng.choice([2.0, 3.0], P), "k_logistic": rng.uniform(5e-4, 2e-3, P), "C0_logistic": rng.uniform(200.0, 500.0, P),
            "warn_threshold": rng.uniform(0.2, 0.4, P)}


def stats(ts):
    ts = np.sort(np.asarray(ts))
    return float(np.median(ts)), float(ts[0]), float(ts[-1])


def wall(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return stats(out)


def events(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3)
    return stats(out)


def launches_only(arr, mu, sigma, sweep):
    """The pinn_rf_sweep call alone on buffers allocated once: what the two launches cost."""
    _, _lib, lib = risk._torch_lib()
    cfg0 = risk._Config()
    prm = cfg0.c_struct()
    P, S, n = sweep.n_candidates, int(sweep.seg_starts.numel()), int(sweep.row_index.numel())
    d = arr.device
    cand = torch.from_numpy(sweep.table).to(d)
    i64 = [torch.empty(P, S, dtype=torch.int64, device=d) for _ in range(3)]
    peak, carry = torch.empty(P, S, dtype=torch.float64, device=d), torch.empty(P, S, 2, dtype=torch.float64, device=d)
    bad = torch.empty(P, dtype=torch.int32, device=d)
    wb = lib.pinn_rf_sweep_workspace_bytes(n, prm.n_cols)
    ws = torch.empty(wb, dtype=torch.uint8, device=d)
    return lambda: call("pinn_rf_sweep", arr, arr.stride(0), arr.shape[0], ctypes.byref(prm), mu, sigma, sweep.row_index, n, sweep.seg_starts,
                        S, cand, P, i64[0], i64[1], i64[2], peak, carry, bad, ws, wb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_rf_sweep.py measures on a GPU"
    a = recording()
    arr = torch.from_numpy(a).cuda()
    conditions = [(0.0, [k], None) for k in range(1, N_FAULT + 1)]
    mu, sigma = risk.estimate_mu_sigma_normal(arr)
    kw = dict(conditions=conditions, current_tol=float("inf"))
    rows = N_NORMAL + N_FAULT * FAULT_ROWS
    fmt = "%-58s %10.3f ms  [%.3f .. %.3f]"

    res = {}
    for P in (256, 4096):
        cand = candidates(P)
        sw = risk.rf_sweep(arr, mu, sigma, cand, **kw)
        assert int(sw.row_index.numel()) == rows and int(sw.seg_starts.numel()) == N_FAULT + 1
        res["call", P] = wall(lambda: risk.rf_sweep(arr, mu, sigma, cand, **kw), args.reps)
        res["launch", P] = events(launches_only(arr, mu, sigma, sw), args.reps)
        for what in ("call", "launch"):
            m, lo, hi = res[what, P]
            print(fmt % ("rf_sweep P=%d, %s" % (P, "whole call (host clock)" if what == "call" else "pinn_rf_sweep alone (events)"), m * 1e3, lo * 1e3, hi * 1e3), flush=True)
        m = res["launch", P][0]
        print("    %.3e candidate-rows/s in the launches, %.3e in the whole call; fired %d of %d"
              % (P * rows / m, P * rows / res["call", P][0], int(sw.fired.sum()), sw.fired.size), flush=True)

    # what the sequential walk of the one long segment costs: the same candidates without the quiet rows (12 x 600 rows),
    # and with the quiet rows cut into ranges of one tile (workgroups then walk one tile each, a false-alarm count is a sum)
    cand = candidates(4096)
    for name, quiet in (("no quiet rows", None), ("quiet rows as 3 ranges of <= 2048", [(0, 2048), (2048, 4096), (4096, N_NORMAL)])):
        sq = risk.rf_sweep(arr, mu, sigma, cand, quiet=quiet, **kw)
        m, lo, hi = events(launches_only(arr, mu, sigma, sq), args.reps)
        print(fmt % ("pinn_rf_sweep alone P=4096, %s" % name, m * 1e3, lo * 1e3, hi * 1e3), flush=True)

    cand = candidates(256)
    sw = risk.rf_sweep(arr, mu, sigma, cand, **kw)
    params = [sw.candidate(i) for i in range(256)]

    def loop():
        for p in params:
            risk.rf_advance_for_conditions(arr, mu, sigma, **kw, **p)
    res["loop"] = wall(loop, max(3, args.reps // 3), warm=1)
    m, lo, hi = res["loop"]
    print(fmt % ("loop of 256 rf_advance_for_conditions calls (host clock)", m * 1e3, lo * 1e3, hi * 1e3), flush=True)
    c = res["call", 256]
    print("    one sweep against the loop at P=256: %.1f x by the medians, %.1f x slowest sweep against fastest loop" % (m / c[0], lo / c[2]), flush=True)
    table = risk.rf_advance_for_conditions(arr, mu, sigma, **kw, **params[7])
    assert [(-1 if r["idx_rf_warn"] is None else r["idx_rf_warn"]) for r in table] == list(sw.idx_rf_warn[7]), "the loop and the sweep disagree"

    cand16 = {k: v[:16] for k, v in cand.items()}
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        hs = risk.rf_sweep(a, mu.cpu().numpy(), sigma.cpu().numpy(), cand16, backend="host", **kw)
        ts.append(time.perf_counter() - t0)
    m, lo, hi = stats(ts)
    print(fmt % ("host backend, P=16", m * 1e3, lo * 1e3, hi * 1e3), flush=True)
    print("    %.3e candidate-rows/s on the host" % (16 * rows / m), flush=True)
    assert np.array_equal(hs.idx_v_alarm, sw.idx_v_alarm)


if __name__ == "__main__":
    main()
