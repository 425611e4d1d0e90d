"""Time the parameter identification of pinn_amd.identify on the GPU: `fit_windows` on four cases of the voltage
model, against the host backend and against the same Levenberg-Marquardt composed from batched torch float64 operations on
the device (`torch.linalg.cholesky_ex` on [W, 3, 3], one host read per iteration to see whether every window has stopped).

  stride 64 at 1.1e4 rows, window 512      stride 64 at 1.1e4 rows, window 4096
  stride 256 at 1e6 rows, window 2048      one baseline of 65536 rows

Per case: one warm-up, then `--reps` calls timed with device events around the Python call (wrapper and allocations included;
the closing event synchronises the stream); the median goes into one JSON line with the row passes per second (rows of every
window times its passes, over the time) and the time of reading the table once at the HBM rate a plain copy reaches on an
MI355X (6.29 TB/s) as a fraction of the measured time.  The table is the model's own voltage plus 2 mV of noise, from a seed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_amd import identify, synth  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
CASES = (("n1.1e4_w512_s64", 11000, 512, 64), ("n1.1e4_w4096_s64", 11000, 4096, 64), ("n1e6_w2048_s256", 1000000, 2048, 256),
         ("baseline_65536", 65536, 65536, 65536))


def make_table(n, seed=0):
    rng = np.random.default_rng(seed)
    X, _ = synth.synth_rows(n, seed + 1)
    X[:, 5] = rng.uniform(57.0, 80.0, n)
    i, b, e = identify.voltage_columns(X)
    th = identify.theta_from_lambdas(identify.LAMBDA_START["voltage"]) + np.array([0.03, -0.2, 0.05])
    return np.column_stack([i, b, e, identify.voltage_model(i, b, e, th) + rng.normal(0.0, 0.002, n)])


def torch_lm(table, start, length, theta0, tol=identify.TOL, xtol=identify.XTOL, mu0=identify.MU0, max_passes=identify.MAX_PASSES):
    """The same solver over windows of one length, every step a batched torch operation; returns (theta [W, 3], passes)."""
    idx = start[:, None] + torch.arange(length, device=table.device)[None, :]
    X = table[idx]                                                     # [W, L, 4]
    i, b, e, v = X.unbind(-1)
    log_i = torch.log(i)
    W = X.shape[0]

    def sums(th):
        r, q, c = th[:, 0:1], th[:, 1:2], th[:, 2:3]
        ic = i * c
        res = e - b * (log_i - q) - i * r + 0.5 * b * torch.log1p(-ic) - v
        J = torch.stack([-i, b, -(0.5 * b * i) / (1.0 - ic)], dim=-1)
        return J.transpose(1, 2) @ J, (J * res[..., None]).sum(1), (res * res).sum(1)

    imax = i.max(dim=1).values
    th = theta0.expand(W, 3).clone()
    mu = torch.full((W,), mu0, dtype=torch.float64, device=table.device)
    A, g, sse = sums(th)
    eye = torch.eye(3, dtype=torch.float64, device=table.device)
    passes = 1
    done = torch.zeros(W, dtype=torch.bool, device=table.device)
    while passes < max_passes:
        sc = torch.rsqrt(torch.diagonal(A, dim1=1, dim2=2))
        C = A * sc[:, :, None] * sc[:, None, :]
        gs = (g * sc)[..., None]
        L, _ = torch.linalg.cholesky_ex(C)
        y = torch.linalg.solve_triangular(L, gs, upper=False)[..., 0]
        m = torch.sqrt((y * y).sum(1) / (sse / (length - 3.0)))
        Lm, _ = torch.linalg.cholesky_ex(C + mu[:, None, None] * eye)
        d = -sc * torch.cholesky_solve(gs, Lm)[..., 0]
        done = done | (m <= tol) | (d.abs() <= xtol * (th.abs() + xtol)).all(1) | (mu > 1e15)
        active = ~done
        if not bool(active.any()):                                     # the one host read of an iteration
            break
        tht = th + d
        At, gt, sset = sums(tht)
        passes += 1
        acc = active & (sset < sse) & (tht[:, 2] * imax < 1.0)
        th = torch.where(acc[:, None], tht, th)
        A, g, sse = torch.where(acc[:, None, None], At, A), torch.where(acc[:, None], gt, g), torch.where(acc, sset, sse)
        mu = torch.where(acc, (mu / 10.0).clamp_min(1e-15), torch.where(active, mu * 10.0, mu))
    return th, passes


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_identify.py measures on the GPU; none is present")
    for name, n, length, stride in CASES:
        if name not in args.cases.split(","):
            continue
        table = make_table(n)
        start, lens = identify.sliding_windows(n, length, stride)
        td = torch.from_numpy(table).cuda()
        sd, ld = torch.from_numpy(start).cuda(), torch.from_numpy(lens).cuda()
        fit = identify.fit_windows(td, sd, ld)
        ms, all_ms = timed(lambda: identify.fit_windows(td, sd, ld), args.reps)
        row_passes = float(np.sum(fit.passes * lens))
        floor_ms = n * 32 / HBM_BYTES_PER_S * 1e3
        res = {"case": name, "rows": n, "windows": len(start), "window": length, "statuses": np.bincount(fit.status, minlength=1).tolist(),
               "passes_max": int(fit.passes.max()), "passes_mean": round(float(fit.passes.mean()), 2), "device_ms": round(ms, 4),
               "device_ms_all": all_ms, "row_passes_per_s": round(row_passes / (ms * 1e-3), 1), "table_read_once_ms": round(floor_ms, 6),
               "read_once_over_measured": round(floor_ms / ms, 6)}
        th0 = torch.from_numpy(identify.theta_from_lambdas(identify.LAMBDA_START["voltage"])).cuda()
        tth, tpasses = torch_lm(td, sd, length, th0)
        tms, tall = timed(lambda: torch_lm(td, sd, length, th0), max(3, args.reps // 2))
        res.update({"torch_ms": round(tms, 3), "torch_ms_all": tall, "torch_passes": tpasses, "torch_over_device": round(tms / ms, 1),
                    "torch_max_dtheta_in_se": float(np.nanmax(np.abs(tth.cpu().numpy() - fit.theta) / fit.se))})
        if not args.no_host:
            t = time.perf_counter()
            h = identify.fit_windows(table, start, lens, backend="host")
            res["host_ms"] = round((time.perf_counter() - t) * 1e3, 2)
            res["host_over_device"] = round(res["host_ms"] / ms, 1)
            res["host_max_dtheta_in_se"] = float(np.nanmax(np.abs(h.theta - fit.theta) / fit.se))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
