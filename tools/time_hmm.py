"""Time the temporal diagnosis of pinn_amd.temporal on the GPU: `filter`, `smooth`, `viterbi` and one EM iteration
(`em_iterations(n=1)`: the E-step's launches, the M-step launch and the one host read of the model) at 1.1e4, 1e6 and 1e7
rows for S = 4 and S = 8, against the host backend at the sizes it finishes in reasonable time (`--host-sizes`).

Per (rows, S, call): one warm-up, then `--reps` calls timed with device events around the Python call (it includes the
wrapper and its allocations; the stream is synchronised by the closing event).  The median goes into one JSON line, with
the bytes the call has to move per row (emissions read once, each per-row output written once: the floor, not what the three
launches of a scan actually move) and that floor's time at the HBM rate a plain copy reaches on an MI355X (6.29 TB/s of the
8 TB/s peak) as a fraction of the measured time.  The data is a sampled sticky chain with noisy posteriors, generated on the device from a seed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_amd import temporal  # noqa: E402

HBM_BYTES_PER_S = 6.29e12


def posteriors(n, S, seed=0):
    """Noisy posteriors of a chain that switches state every few hundred rows, made on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    state = (torch.arange(n, device="cuda") // 400 * 7 + 3) % S
    z = torch.randn(n, S, generator=g, device="cuda", dtype=torch.float64)
    z[torch.arange(n, device="cuda"), state] += 1.5
    return torch.softmax(z, dim=1)


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
    ap.add_argument("--states", default="4,8")
    ap.add_argument("--host-sizes", default="11000,100000")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_hmm.py measures on the GPU; none is present")
    host_sizes = {int(s) for s in args.host_sizes.split(",") if s}
    for S in [int(s) for s in args.states.split(",")]:
        for n in [int(s) for s in args.sizes.split(",")]:
            y = posteriors(n, S)
            A = temporal.sticky_transitions(S, 0.99)
            dev = temporal.DeviceHMM(A, backend="device")
            calls = {"filter": (lambda h, v: h.filter(v), 2 * 8 * S), "smooth": (lambda h, v: h.smooth(v), 2 * 8 * S),
                     "viterbi": (lambda h, v: h.viterbi(v), 8 * S + 8),
                     "em_iteration": (lambda h, v: temporal.DeviceHMM(A, backend=h.backend).em_iterations(v, 1), 8 * S)}
            for name, (fn, bytes_per_row) in calls.items():
                ms, all_ms = timed(lambda: fn(dev, y), args.reps)
                floor_ms = n * bytes_per_row / HBM_BYTES_PER_S * 1e3
                res = {"call": name, "rows": n, "S": S, "device_ms": round(ms, 4), "device_ms_all": all_ms, "ns_per_row": round(ms * 1e6 / n, 3),
                       "floor_bytes_per_row": bytes_per_row, "hbm_floor_ms": round(floor_ms, 5), "floor_over_measured": round(floor_ms / ms, 5)}
                if n in host_sizes:
                    yh = y.cpu().numpy()
                    host = temporal.DeviceHMM(A, backend="host")
                    res["host_ms"] = round(host_timed(lambda: fn(host, yh)), 2)
                    res["host_over_device"] = round(res["host_ms"] / ms, 1)
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
