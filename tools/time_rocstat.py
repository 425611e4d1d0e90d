"""Time the ROC inference against what stood before it.  python tools/time_rocstat.py [--reps 9] [--n-boot 2000]

N = 12 000 and N = 1 000 000 test rows, a quarter of them positive, K = 4 continuous score vectors (as many tied groups as
rows: the bootstrap's histogram is in LDS at the small size and in the workspace at the large one).  In one process, after
warm-up, medians with the spread:
  - delong_covariance on the device at K = 4 and K = 1, the whole call by a host clock around a synchronise, and beside it
    detection.roc_counts(curve=False) on one score vector, which is what gave the AUC alone before;
  - where delong_covariance spends it: torch.sort of the K vectors, the five launches of pinn_auc_components and the launches
    of pinn_auc_cross_sums for both classes, each by device events on buffers allocated once;
  - bootstrap_auc(n_boot) on the device, the whole call and the launches of pinn_auc_bootstrap alone; and the host backend,
    with all n_boot resamples at the small size and --host-boot of them at the large one (its cost is linear in them).
Each figure is printed as median [min .. max] over the repetitions.  A machine without a GPU fails: nothing falls back."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pinn_amd import detection, rocstat  # noqa: E402
from pinn_amd._device import call  # noqa: E402

K = 4
FMT = "%-74s %10.3f ms  [%.3f .. %.3f]"


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


def data(N, seed=0):
    rng = np.random.default_rng(seed)
    y = (rng.random(N) < 0.25).astype(np.int64)
    s = rng.normal(size=(K, N)) + np.array([1.5, 1.2, 0.8, 0.3])[:, None] * y
    return y, s


def show(name, t):
    print(FMT % (name, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3), flush=True)
    return t[0]


def parts(ty, ts):
    """The launches of delong_covariance on buffers allocated once."""
    _, _lib, lib = rocstat._torch_lib()
    k, N = ts.shape
    pos = ty == 1
    s_sorted, order = torch.sort(ts, dim=1, stable=True)
    pos_sorted = pos.to(torch.int64)[order].contiguous()
    counts = torch.empty(k * 8, dtype=torch.int64, device=ts.device)
    comp, group = torch.empty((k, N), dtype=torch.int64, device=ts.device), torch.empty((k, N), dtype=torch.int32, device=ts.device)
    wb = lib.pinn_auc_components_workspace_bytes(N, k)
    ws = torch.empty(wb, dtype=torch.uint8, device=ts.device)
    a, b = comp[:, torch.nonzero(pos).reshape(-1)].contiguous(), comp[:, torch.nonzero(~pos).reshape(-1)].contiguous()
    out = torch.empty(k * (k + 1), dtype=torch.int64, device=ts.device)
    wa, wbb = lib.pinn_auc_cross_sums_workspace_bytes(a.shape[1], k), lib.pinn_auc_cross_sums_workspace_bytes(b.shape[1], k)
    wsa, wsb = torch.empty(wa, dtype=torch.uint8, device=ts.device), torch.empty(wbb, dtype=torch.uint8, device=ts.device)

    def cross():
        call("pinn_auc_cross_sums", a, a.stride(0), a.shape[1], k, out, wsa, wa)
        call("pinn_auc_cross_sums", b, b.stride(0), b.shape[1], k, out, wsb, wbb)
    return (lambda: torch.sort(ts, dim=1, stable=True),
            lambda: call("pinn_auc_components", s_sorted, pos_sorted, order, N, k, counts, comp, group, ws, wb), cross)


def boot_launch(ty, ts, n_boot):
    """pinn_auc_bootstrap alone: the first chunk bootstrap_auc would launch, and how many resamples it holds."""
    _, _lib, lib = rocstat._torch_lib()
    c = rocstat.auc_components(ty, ts)
    gpos, gneg = c["group"][:, c["pos_rows"]].contiguous(), c["group"][:, c["neg_rows"]].contiguous()
    g = (ctypes.c_longlong * K)(*[int(v) for v in c["n_groups"]])
    per = lib.pinn_auc_bootstrap_workspace_bytes(1, K, g)
    chunk = n_boot if per == 0 else max(1, min(n_boot, rocstat.DEFAULT_WORKSPACE_CAP // per))
    ws = torch.empty(per * chunk, dtype=torch.uint8, device=ts.device) if per else None
    out = torch.empty((chunk, K), dtype=torch.int64, device=ts.device)
    return (lambda: call("pinn_auc_bootstrap", gpos, gneg, c["n_pos"], c["n_neg"], K, g, 0, 0, chunk, out, ws, per * chunk)), chunk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--n-boot", type=int, default=2000)
    ap.add_argument("--host-boot", type=int, default=4, help="resamples of the host backend at the large size")
    ap.add_argument("--sizes", type=int, nargs="+", default=[12000, 1000000])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_rocstat.py measures on a GPU"
    for N in args.sizes:
        y, s = data(N)
        ty, ts = torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda()
        print("N = %d rows, %d positive, K = %d" % (N, int(y.sum()), K), flush=True)
        d4 = show("delong_covariance K=4, whole call (host clock)", wall(lambda: rocstat.delong_covariance(ty, ts), args.reps))
        d1 = show("delong_covariance K=1, whole call (host clock)", wall(lambda: rocstat.delong_covariance(ty, ts[0]), args.reps))
        r1 = show("roc_counts(curve=False), one score vector, whole call (host clock)",
                  wall(lambda: detection.roc_counts(ty, ts[0], pos_label=1, curve=False), args.reps))
        print("    delong_covariance / roc_counts: K=1 %.2f x, K=4 %.2f x of one vector's count" % (d1 / r1, d4 / r1), flush=True)
        for k in (4, 1):
            sort, comp, cross = parts(ty, ts[:k].contiguous())
            show("  K=%d torch.sort (events)" % k, events(sort, args.reps))
            show("  K=%d pinn_auc_components, five launches (events)" % k, events(comp, args.reps))
            show("  K=%d pinn_auc_cross_sums, both classes (events)" % k, events(cross, args.reps))
        b = show("bootstrap_auc n_boot=%d K=4, whole call (host clock)" % args.n_boot,
                 wall(lambda: rocstat.bootstrap_auc(ty, ts, n_boot=args.n_boot), max(3, args.reps // 3), warm=1))
        launch, chunk = boot_launch(ty, ts, args.n_boot)
        bl = show("  pinn_auc_bootstrap alone, %d resamples in one launch (events)" % chunk, events(launch, max(3, args.reps // 3), warm=1))
        print("    %.3e row visits/s in the launch, %.3e in the whole call" % (chunk * K * N / bl, args.n_boot * K * N / b), flush=True)
        hb = args.n_boot if N <= 20000 else args.host_boot
        t0 = time.perf_counter()
        h = rocstat.bootstrap_auc(y, s, n_boot=hb, backend="host")
        th = time.perf_counter() - t0
        print(FMT % ("host backend, %d resamples (one run)" % hb, th * 1e3, th * 1e3, th * 1e3), flush=True)
        print("    %.3e row visits/s on the host; the device call is %.0f x faster per resample" % (hb * K * N / th, (th / hb) / (b / args.n_boot)),
              flush=True)
        dv = rocstat.bootstrap_auc(ty, ts, n_boot=hb)
        assert np.array_equal(dv["U2_boot"].cpu().numpy(), h["U2_boot"]), "the backends disagree"
        assert rocstat.delong_covariance(ty, ts)["cov"].tobytes() == rocstat.delong_covariance(y, s, backend="host")["cov"].tobytes()


if __name__ == "__main__":
    main()
