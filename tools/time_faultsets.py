"""Time pinn_amd.faultsets on the GPU: `prediction_sets` and `evaluate_sets` at 1.1e4 / 1e6 / 1e7 rows of y_prob
with C = 4 classes and 1349 / 1e5 / 1e6 calibration rows, in every table regime that fits, against the same result composed
from `torch.searchsorted` and comparisons; `GMMSetDiagnoser.predict` against `DeviceGMM.diagnose` plus that composition;
`GMMSetDiagnoser.update` per chunk of 2048 rows against the host backend; the build of the calibration state; and the two
questions the regimes leave to measurement: from how many rows on staging pays (`--crossover`: every regime at small row
counts) and whether the largest staged table still beats the other regimes.

Per (shape, call): `--warmup` calls, then `--reps` calls timed with device events around the Python call (it includes the
wrapper and its allocations; the closing event synchronises the stream).  The median goes into one JSON line with the HBM
floor: a row has to cross HBM with n (8 C + 4 C + 2 L) bytes (y_prob in, counts and masks out; sizes, novel flags and the
missing flag add n (2 L + 1)), and a plain copy reaches 6.29 TB/s on an MI355X.  The data is made on the device from a seed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_amd import faultsets as F  # noqa: E402
from pinn_amd.diagnosis import DeviceGMM  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
LEVELS = (0.9, 0.95)
C = 4


def posteriors(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    P = torch.softmax(2.0 * torch.randn(n, C, generator=g, device="cuda", dtype=torch.float64), dim=1)
    y = torch.multinomial(P.float(), 1, generator=g).reshape(-1).long() if n <= 2 ** 24 else P.argmax(1)
    return P, y


def timed(fn, warmup, reps):
    for _ in range(warmup):
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
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def torch_sets(tables, kmin, P, y=None):
    """The lac sets from torch operations: counts by searchsorted per class, masks and sizes by comparisons; with y the tallies."""
    S = 1.0 - P
    count = torch.stack([t.numel() - torch.searchsorted(t, S[:, c].contiguous()) for c, t in enumerate(tables)], dim=1).int()
    inc = count[:, :, None] >= kmin[None]
    mask = (inc.long() << torch.arange(C, device="cuda")[None, :, None]).sum(1).short()
    size = inc.sum(1).to(torch.uint8)
    if y is None:
        return count, mask, size, size == 0
    n_c = torch.bincount(y, minlength=C)
    own = inc[torch.arange(P.shape[0], device="cuda"), y]
    covered = torch.stack([torch.bincount(y, weights=own[:, l].double(), minlength=C) for l in range(inc.shape[2])], 1)
    hist = torch.stack([torch.bincount(size[:, l].long(), minlength=C + 1) for l in range(inc.shape[2])])
    single = ((size == 1) & own).sum(0)
    return n_c, covered, hist, single


def line(**kw):
    print(json.dumps(kw), flush=True)


def floor_ms(n, L):
    return 1e3 * n * (8 * C + 4 * C + 2 * L) / HBM_BYTES_PER_S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="11000:1349,1000000:100000,10000000:1000000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--crossover", default="256,1024,4096,16384,65536,262144")
    ap.add_argument("--skip-gmm", action="store_true")
    ap.add_argument("--skip-sets", action="store_true", help="only the fused path under a mixture")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on a GPU"
    L = len(LEVELS)
    t = lambda fn: timed(fn, args.warmup, args.reps)

    for shape in ([] if args.skip_sets else args.shapes.split(",")):
        n, n_cal = (int(v) for v in shape.split(":"))
        Pc, yc = posteriors(n_cal, 1)
        P, y = posteriors(n, 2)
        t0 = time.perf_counter()
        cal = F.calibrate(Pc, yc, "lac")
        torch.cuda.synchronize()
        first_build = 1e3 * (time.perf_counter() - t0)
        line(call="calibrate", n_cal=n_cal, ms=t(lambda: F.calibrate(Pc, yc, "lac"))[0], first_ms=first_build,
             torch_sort_ms=t(lambda: [torch.sort((1.0 - Pc)[yc == c, c]) for c in range(C)])[0])
        tables = [torch.from_numpy(cal.table(c)).cuda() for c in range(C)]
        kmin = torch.from_numpy(F.kmin_table(cal.n_cal, LEVELS)).cuda()
        ref = torch_sets(tables, kmin, P)
        got = F.prediction_sets(cal, P, LEVELS)
        assert torch.equal(ref[0], got.count) and torch.equal(ref[1], got.mask) and torch.equal(ref[2], got.size)
        padded = sum(F._pad(int(v)) for v in cal.n_cal)
        sampled = sum((int(v) + F.LINE - 1) // F.LINE for v in cal.n_cal)
        for regime in ("auto", "lds", "sampled", "global"):
            if (regime == "lds" and padded > F.LDS_ENTRIES) or (regime == "sampled" and sampled > F.LDS_ENTRIES):
                continue
            ms = t(lambda: F.prediction_sets(cal, P, LEVELS, force_regime=regime))
            ev = t(lambda: F.evaluate_sets(cal, P, y, LEVELS, force_regime=regime))
            line(call="prediction_sets", rows=n, n_cal=n_cal, regime=regime, ms=ms[0], min_ms=ms[1], max_ms=ms[2], floor_ms=floor_ms(n, L),
                 floor_over_measured=floor_ms(n, L) / ms[0], evaluate_ms=ev[0], evaluate_floor_ms=1e3 * n * (8 * C + 8) / HBM_BYTES_PER_S)
        ms = t(lambda: torch_sets(tables, kmin, P))
        ev = t(lambda: torch_sets(tables, kmin, P, y))
        line(call="torch_composition", rows=n, n_cal=n_cal, ms=ms[0], min_ms=ms[1], max_ms=ms[2], evaluate_ms=ev[0])
        del P, y, ref, got

    # from how many rows on staging pays, at the smallest and at the largest staged tables
    for n_cal in (() if args.skip_sets else (1349, 4 * (F.LDS_ENTRIES // 4 - F.LINE))):
        Pc, yc = posteriors(n_cal, 3)
        cal = F.calibrate(Pc, yc, "lac")
        padded = sum(F._pad(int(v)) for v in cal.n_cal)
        for n in (int(v) for v in args.crossover.split(",")):
            P, _ = posteriors(n, 4)
            out = {}
            for regime in ("lds", "sampled", "global"):
                if regime == "lds" and padded > F.LDS_ENTRIES:
                    continue
                out[regime + "_ms"] = t(lambda: F.prediction_sets(cal, P, LEVELS, force_regime=regime))[0]
            line(call="crossover", rows=n, n_cal=n_cal, padded_entries=padded, **out)

    if args.skip_gmm:
        return
    # the fused path: rows of a results array under a mixture of 8 components
    rng = np.random.default_rng(0)
    centres = rng.normal(size=(C, 4)) * 5.0
    for n, n_cal in ((11000, 1349), (1000000, 100000)):
        yk = torch.randint(0, C, (n + n_cal + 4000,), device="cuda")
        A = torch.randn(n + n_cal + 4000, 22, device="cuda", dtype=torch.float64)
        A[:, 13:17] += torch.from_numpy(centres).cuda()[yk]
        cols = [13, 14, 15, 16]
        fit, calr, te = torch.arange(4000, device="cuda"), torch.arange(4000, 4000 + n_cal, device="cuda"), torch.arange(4000 + n_cal, A.shape[0], device="cuda")
        gmm = DeviceGMM(8, random_state=0, backend="device").fit(A, columns=cols, row_index=fit)
        cfp = gmm.label_map(A, yk[fit], C, columns=cols, row_index=fit)
        for kind in ("lac", "density"):
            cal = F.calibrate_gmm(gmm, cfp, A, yk[calr], kind, columns=cols, row_index=calr)
            d = F.GMMSetDiagnoser(gmm, cfp, cal, LEVELS)
            ms = t(lambda: d.predict(A, columns=cols, row_index=te))
            forced = {}
            for regime in ("lds", "sampled", "global"):
                d.force_regime = regime
                try:
                    forced[regime + "_ms"] = t(lambda: d.predict(A, columns=cols, row_index=te))[0]
                except Exception:
                    forced[regime + "_ms"] = None       # the tables do not fit this regime's budget
            d.force_regime = "auto"
            out = dict(forced, call="gmm_predict", kind=kind, rows=n, n_cal=n_cal, ms=ms[0], min_ms=ms[1], max_ms=ms[2],
                       diagnose_ms=t(lambda: gmm.diagnose(A, cfp, columns=cols, row_index=te))[0])
            if kind == "lac":
                tables = [torch.from_numpy(cal.table(c)).cuda() for c in range(C)]
                kmin = torch.from_numpy(F.kmin_table(cal.n_cal, LEVELS)).cuda()
                out["diagnose_plus_torch_ms"] = t(lambda: torch_sets(tables, kmin, gmm.diagnose(A, cfp, columns=cols, row_index=te)[0]))[0]
            line(**out)
            if n == 11000:
                rows = A[4000 + n_cal:4000 + n_cal + 2048].contiguous()
                dev_ms = t(lambda: d.update(rows))[0]
                host_gmm = DeviceGMM(8, backend="host")
                host_gmm._set_attrs({k: getattr(gmm, k + "_").cpu().numpy() for k in ("weights", "means", "covariances", "precisions_cholesky")}, gmm.n_iter_, True, gmm.lower_bound_)
                hc = F.calibrate_gmm(host_gmm, cfp.cpu().numpy(), A[calr].cpu().numpy(), yk[calr].cpu().numpy(), kind, columns=cols, backend="host")
                hd = F.GMMSetDiagnoser(host_gmm, cfp.cpu().numpy(), hc, LEVELS, backend="host")
                rows_h = rows.cpu().numpy()
                t0 = time.perf_counter()
                for _ in range(5):
                    hd.update(rows_h)
                line(call="update_chunk_2048", kind=kind, device_ms=dev_ms, host_ms=1e3 * (time.perf_counter() - t0) / 5)


if __name__ == "__main__":
    main()
