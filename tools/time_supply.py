"""Time the supply-law fit of pinn_amd.supply on the GPU: `fit_breakpoints` on three shapes, beside the host
backend and beside the same enumeration composed from batched torch float64 operations on the device (`unfold`, `sort`,
`cumsum`, `argmin`: the candidates' SSEs and the winner per window, without the pass at the winner and the covariance).

  164 windows of 512 rows (stride 64 at 1.1e4 rows)      108 windows of 4096 rows (stride 64 at 1.1e4 rows)
  3899 windows of 2048 rows (stride 256 at 1e6 rows)

Per shape: one warm-up, then `--reps` calls timed with device events around the Python call (wrapper and allocations included;
the closing event synchronises the stream); the median goes into one JSON line.  The table follows the law at (1.5, 0.8, 150 A)
with noise of 0.05, currents on 10 A setpoints, from a seed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_amd import identify, supply  # noqa: E402

CASES = (("n1.1e4_w512_s64", 11000, 512, 64), ("n1.1e4_w4096_s64", 11000, 4096, 64), ("n1e6_w2048_s256", 1000000, 2048, 256))


def make_table(n, seed=0):
    rng = np.random.default_rng(seed)
    x = np.round(rng.uniform(20.0, 300.0, n) / 10.0) * 10.0
    return np.column_stack([x, 1.5 + 0.8 * (np.minimum(x, 150.0) / 100.0) + rng.normal(0.0, 0.05, n)])


def torch_enumeration(table, length, stride):
    """The enumeration over windows of one length, every step a batched torch operation: (smallest SSE [W], k [W], free [W])."""
    inf = float("inf")
    win = table.unfold(0, length, stride)                             # [W, 2, L]
    x, order = torch.sort(win[:, 0, :], dim=1, stable=True)
    y = torch.gather(win[:, 1, :], 1, order)
    m = float(length)
    z = x / 100.0
    z = z - z.mean(1, keepdim=True)
    y = y - y.mean(1, keepdim=True)
    P = torch.cumsum(torch.stack([torch.ones_like(z), z, y, z * z, z * y, y * y], dim=-1), dim=1)
    T = P[:, -1:, :]
    n, Pz, Py, Pzz, Pzy, Pyy = P.unbind(-1)
    Ty, Tyy = T[..., 2], T[..., 5]
    valid = torch.cat([x[:, :-1] < x[:, 1:], torch.ones_like(x[:, :1], dtype=torch.bool)], dim=1)
    two = x > x[:, :1]
    rem = m - n
    Su, Suu, Suy = Pz + rem * z, Pzz + rem * (z * z), Pzy + z * (Ty - Py)
    Duu, Duy, Dyy = Suu - Su * Su / m, Suy - Su * Ty / m, Tyy - Ty * Ty / m
    lin = two & (Duu > 0)
    s_knot = torch.where(lin, Dyy - Duy * Duy / Duu, Dyy.expand_as(Duu))
    s_knot = torch.where(valid, s_knot, torch.full_like(s_knot, inf))
    nr = (m - n).clamp_min(1.0)
    Lzz, Lzy, Lyy = Pzz - Pz * Pz / n, Pzy - Pz * Py / n, Pyy - Py * Py / n
    bl = Lzy / Lzz
    al = (Py - bl * Pz) / n
    ry = Ty - Py
    s_free = (Lyy - Lzy * Lzy / Lzz) + ((Tyy - Pyy) - ry * ry / nr)
    c = (ry / nr - al) / bl                                           # centred z units, as z
    zn = torch.cat([z[:, 1:], torch.full_like(z[:, :1], inf)], dim=1)
    adm = valid & two & (n >= 2) & (n <= m - 1) & (Lzz > 0) & (bl != 0) & (c >= z) & (c <= zn)
    s_free = torch.where(adm, s_free, torch.full_like(s_free, inf)).nan_to_num(nan=inf)
    bk, kk = s_knot.nan_to_num(nan=inf).min(dim=1)
    bf, kf = s_free.min(dim=1)
    free = bf < bk
    return torch.where(free, bf, bk), torch.where(free, kf, kk) + 1, free


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
        sys.exit("time_supply.py measures on the GPU; none is present")
    for name, n, length, stride in CASES:
        if name not in args.cases.split(","):
            continue
        table = make_table(n)
        start, lens = identify.sliding_windows(n, length, stride)
        td = torch.from_numpy(table).cuda()
        fit = supply.fit_breakpoints(td, start, lens)
        ms, all_ms = timed(lambda: supply.fit_breakpoints(td, start, lens), args.reps)
        res = {"case": name, "rows": n, "windows": len(start), "window": length, "statuses": np.bincount(fit.status, minlength=1).tolist(),
               "kinds": np.bincount(fit.kind, minlength=4).tolist(), "device_ms": round(ms, 4), "device_ms_all": all_ms,
               "rows_per_s": round(float(np.sum(lens)) / (ms * 1e-3), 1)}
        tsse, tk, tfree = torch_enumeration(td, length, stride)
        tms, tall = timed(lambda: torch_enumeration(td, length, stride), max(3, args.reps // 2))
        same = (tk.cpu().numpy() == fit.k) & (tfree.cpu().numpy() == (fit.kind == 0))
        res.update({"torch_ms": round(tms, 3), "torch_ms_all": tall, "torch_over_device": round(tms / ms, 2),
                    "torch_same_winner": round(float(same.mean()), 4)})
        if not args.no_host:
            t = time.perf_counter()
            h = supply.fit_breakpoints(table, start, lens, backend="host")
            res["host_ms"] = round((time.perf_counter() - t) * 1e3, 2)
            res["host_over_device"] = round(res["host_ms"] / ms, 1)
            res["host_same_winner"] = round(float(np.mean((h.k == fit.k) & (h.kind == fit.kind))), 4)
            with np.errstate(invalid="ignore"):
                res["host_max_dtheta_rel"] = float(np.nanmax(np.abs(h.theta[:, :2] - fit.theta[:, :2]) / np.abs(fit.theta[:, :2])))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
