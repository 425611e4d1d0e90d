"""Which parameter moved: track the polarisation parameters of a recording over time, with bands.

The recording is synthetic and its voltage is the model's own: physical rows as `synth.synth_rows` draws them, the per-cell
voltage V(theta) of pinn_amd.identify plus 2 mV of noise.  Three segments of equal length: normal rows; rows over which the
ohmic resistance r = lambda_1 ramps up by 40 % (membrane drying); rows over which c = 1 / lambda_3 ramps up by 50 % (the
limiting current density falls: flooding) with r back at its normal value.  A baseline is fitted on the first segment, then
the recording is replayed in chunks through `ParameterTracker`, which refits the trailing window at every chunk, and per
segment the parameter it blames (largest |z| against the baseline) is printed with its band.

    python examples/parameter_tracking.py [--rows 6000] [--window 1024] [--chunk 64] [--backend auto|host|device]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import pinn_amd  # noqa: E402,F401
from pinn_amd import identify, synth  # noqa: E402

R_RAMP, C_RAMP, NOISE = 0.40, 0.50, 0.002


def synthetic_recording(n=6000, seed=0):
    """{"table" [n, 4] (i, b, E, v), "segments" (starts), "theta" [n, 3] the true parameters per row}."""
    n3 = n // 3
    rng = np.random.default_rng(seed)
    X, _ = synth.synth_rows(n, seed + 1)
    X[:, 5] = rng.uniform(57.0, 80.0, n)
    i, b, e = identify.voltage_columns(X)
    th = np.tile(identify.theta_from_lambdas(identify.LAMBDA_START["voltage"]), (n, 1))
    th[n3:2 * n3, 0] *= 1.0 + R_RAMP * np.linspace(0.0, 1.0, n3)
    th[2 * n3:, 2] *= 1.0 + C_RAMP * np.linspace(0.0, 1.0, n - 2 * n3)
    v = e - b * (np.log(i) - th[:, 1]) - i * th[:, 0] + 0.5 * b * np.log1p(-i * th[:, 2]) + rng.normal(0.0, NOISE, n)
    return {"table": np.column_stack([i, b, e, v]), "segments": np.array([0, n3, 2 * n3]), "theta": th}


def track(rec, window=1024, chunk=64, backend="host", table=None):
    """Replay the recording: the baseline on the first segment, then one update per chunk; a list of (end row, update)."""
    table = rec["table"] if table is None else table
    n, n3 = len(rec["table"]), int(rec["segments"][1])
    base = identify.fit_baseline(table[:n3], backend=backend)
    tracker = identify.ParameterTracker(base, window, backend=backend)
    out = []
    for a in range(0, n, chunk):
        out.append((min(a + chunk, n), tracker.update(table[a:a + chunk])))
    return base, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--window", type=int, default=1024)
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
    p = base.params
    print("baseline on rows 0..%d (%s backend, %d passes): " % (rec["segments"][1], backend, base.passes[0])
          + ", ".join("%s = %.6g +- %.2g" % (k, v[0][0], v[1][0]) for k, v in p.items()))
    names = identify.THETA_NAMES["voltage"]
    bounds = list(rec["segments"]) + [args.rows]
    for s, label in enumerate(("normal", "r ramps by %.0f %%" % (100 * R_RAMP), "c ramps by %.0f %%" % (100 * C_RAMP))):
        # the windows that lie inside the segment, and the last of them
        inside = [(end, u) for end, u in updates if end - args.window >= bounds[s] and end <= bounds[s + 1] and u["status"] == 0]
        if not inside:
            print("segment %d (%s): no window of %d rows inside" % (s, label, args.window))
            continue
        zmax = max(float(np.max(np.abs(u["z"]))) for _, u in inside)
        end, u = inside[-1]
        k = names.index(u["blamed"])
        rel = u["theta"][k] / base.theta[0][k] - 1.0
        band = 1.96 * u["se"][k] / abs(base.theta[0][k])
        verdict = "blames %s" % u["blamed"] if abs(u["z"][k]) >= 4.0 else "blames nothing (max |z| %.2f < 4)" % zmax
        print("segment %d (%s): last window ends at row %d, %s: %s moved by %+.1f %% +- %.1f %% (z = %+.1f), p = %.2g"
              % (s, label, end, verdict, u["blamed"], 100 * rel, 100 * band, u["z"][k], u["p"]))


if __name__ == "__main__":
    main()
