"""Which supply parameter moved: track the air excess-ratio law of a recording over time, with bands.

The recording is synthetic and its excess ratio follows the law itself (`synth.synth_rows` draws excess ratios without one):
currents on 10 A setpoints between 20 and 300 A, act = l1 + l2 min(It, l3) / 100 plus noise of 0.05.  Three segments of equal
length: normal rows; rows over which the base value l1 ramps down by 40 % (oxygen starvation); rows over which the
threshold l3 moves from 150 A to 95 A with l1 back at its normal value.  A baseline is fitted on the first segment, then the
recording is replayed in chunks through `SupplyTracker`, which refits the trailing window at every chunk, and per segment
the parameter it blames (largest |z| against the baseline) is printed with its band.

    python examples/supply_tracking.py [--rows 6000] [--window 512] [--chunk 64] [--backend auto|host|device]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import pinn_amd  # noqa: E402,F401
from pinn_amd import supply  # noqa: E402

NORMAL = (1.5, 0.8, 150.0)
L1_RAMP, L3_END, NOISE = 0.40, 95.0, 0.05
LABELS = ("normal", "l1 ramps down by %.0f %%" % (100 * L1_RAMP), "l3 moves to %.0f A" % L3_END)
MOVED = (None, "l1", "l3")


def synthetic_recording(n=6000, seed=0):
    """{"table" [n, 2] (It, act), "segments" (starts), "theta" [n, 3] the true parameters per row}."""
    n3 = n // 3
    rng = np.random.default_rng(seed)
    x = np.round(rng.uniform(20.0, 300.0, n) / 10.0) * 10.0
    th = np.tile(np.array(NORMAL), (n, 1))
    th[n3:2 * n3, 0] *= 1.0 - L1_RAMP * np.linspace(0.0, 1.0, n3)
    th[2 * n3:, 2] = np.linspace(NORMAL[2], L3_END, n - 2 * n3)
    act = th[:, 0] + th[:, 1] * (np.minimum(x, th[:, 2]) / 100.0) + rng.normal(0.0, NOISE, n)
    return {"table": np.column_stack([x, act]), "segments": np.array([0, n3, 2 * n3]), "theta": th}


def track(rec, window=512, chunk=64, backend="host", table=None):
    """Replay the recording: the baseline on the first segment, then one update per chunk; a list of (end row, update)."""
    table = rec["table"] if table is None else table
    n, n3 = len(rec["table"]), int(rec["segments"][1])
    base = supply.fit_breakpoint_baseline(table[:min(n3, supply.MAX_WINDOW)], backend=backend)
    tracker = supply.SupplyTracker(base, window, backend=backend)
    out = []
    for a in range(0, n, chunk):
        out.append((min(a + chunk, n), tracker.update(table[a:a + chunk])))
    return base, out


def last_windows(rec, updates, window):
    """Per segment the last update whose window lies inside it: [(end row, update) or None]."""
    bounds = list(rec["segments"]) + [len(rec["table"])]
    out = []
    for s in range(3):
        inside = [(end, u) for end, u in updates if end - window >= bounds[s] and end <= bounds[s + 1] and u["status"] == 0]
        out.append(inside[-1] if inside else None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--backend", default="auto")
    args = ap.parse_args()

    rec = synthetic_recording(args.rows)
    table, backend = rec["table"], args.backend
    if backend in ("auto", "device"):
        import torch
        if torch.cuda.is_available():
            table, backend = torch.from_numpy(table).cuda(), "device"
        elif backend == "auto":
            backend = "host"
    base, updates = track(rec, args.window, args.chunk, backend, table)
    print("baseline on rows 0..%d (%s backend, %s): " % (min(rec["segments"][1], supply.MAX_WINDOW), backend, supply.KIND[int(base.kind[0])])
          + ", ".join("%s = %.6g +- %.2g" % (k, v[0][0], v[1][0]) for k, v in base.params("oxygen").items())
          + "; lambda_O3 within [%.0f, %.0f] A, plateau F = %.0f" % (base.c_interval[0, 0], base.c_interval[0, 1], base.plateau_F[0]))
    for s, (label, last) in enumerate(zip(LABELS, last_windows(rec, updates, args.window))):
        if last is None:
            print("segment %d (%s): no window of %d rows inside" % (s, label, args.window))
            continue
        end, u = last
        k = supply.THETA_NAMES.index(u["blamed"])
        verdict = "blames %s" % u["blamed"] if abs(u["z"][k]) >= 4.0 else "blames nothing (max |z| %.2f < 4)" % float(np.nanmax(np.abs(u["z"])))
        print("segment %d (%s): last window ends at row %d, %s: %s went from %.4g to %.4g +- %.2g (z = %+.1f, %s), p = %.2g"
              % (s, label, end, verdict, u["blamed"], base.theta[0][k], u["theta"][k], 1.96 * u["se"][k], u["z"][k],
                 supply.KIND[u["kind"]], u["p"]))


if __name__ == "__main__":
    main()
