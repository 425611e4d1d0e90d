"""Generate tests/golden/g_rf.npz by running the reference's script 04 on a synthetic results array.

Build machine only: needs a checkout of the reference (`--reference PATH/04_risk_function_early_warning_index.py.py`) and
matplotlib importable (the script imports it; MPLBACKEND=Agg, nothing is drawn).  Neither the package nor any test imports
this file.  The fixture holds numeric arrays only: the eight input columns that are read (0, 8, 12-17) and what the
reference computed from them.  `--time` also prints the wall time of the reference's compute_rf_time_series at 1e6 rows
(the CPU comparison figure of DESIGN 3f); it is printed, not stored, so that the fixture regenerates byte for byte.

Alarm-margin condition (asserted here): at every recorded alarm index the series is at least 1e-6 past its threshold and
at every earlier index at least 1e-6 short of it, so that rounding differences of 1e-11 cannot move an index.
"""
import argparse
import contextlib
import importlib.util
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g_rf.npz")
KEPT = [0, 8, 12, 13, 14, 15, 16, 17]
N_NORMAL, N_SEG, SEG = 800, 12, 180
PLATEAUS = (108.0, 270.0, 405.0)
SCALE = {12: 0.02, 13: 0.05, 14: 0.5, 15: 0.01, 16: 0.01}            # sigma of res, pV, pT, pH, pO on normal rows
DRIFT_COLS = {0: (13, 16), 1: (16, 12), 2: (14, 12), 3: (15, 13)}     # two residual columns per fault class
AMPLITUDE = (10.0, 16.0, 22.0)                                        # ramp height in sigma, by plateau
SAG = (0.0, 0.125, 0.3)                                               # volts over the segment
MARGIN = 1e-6


def load_reference(path):
    os.environ.setdefault("MPLBACKEND", "Agg")
    spec = importlib.util.spec_from_file_location("ref04", path)
    ref = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(ref)
    return ref


def synthetic_results(seed):
    rng = np.random.default_rng(seed)
    n = N_NORMAL + N_SEG * SEG
    a = np.zeros((n, 22))
    for c, s in SCALE.items():
        a[:, c] = rng.normal(0.0, s, n)
    a[:, 8] = 3.4 + rng.normal(0.0, 0.005, n)
    a[:N_NORMAL, 0] = PLATEAUS[0] + rng.uniform(-0.4, 0.4, N_NORMAL)
    ramp = np.linspace(0.0, 1.0, SEG)
    for k in range(1, N_SEG + 1):
        rows = slice(N_NORMAL + (k - 1) * SEG, N_NORMAL + k * SEG)
        a[rows, 17] = k
        a[rows, 0] = PLATEAUS[(k - 1) % 3] + rng.uniform(-0.4, 0.4, SEG)
        for j, c in enumerate(DRIFT_COLS[(k - 1) // 3]):
            a[rows, c] += (1.0 if j == 0 else -1.0) * AMPLITUDE[(k - 1) % 3] * SCALE[c] * ramp ** 1.5
        a[rows, 8] -= SAG[(k + (k - 1) // 3) % 3] * ramp
    base = N_NORMAL + 5 * SEG                     # two NaN rows in segment 6, in different residual columns
    a[base + 40, 14] = np.nan
    a[base + 41, 15] = np.nan
    return a


def check_margin(series, thr, mode, idx):
    s = np.asarray(series, dtype=float)
    past = (s - thr) if mode == "above" else (thr - s)
    before = past if idx is None else past[:idx]
    before = before[~np.isnan(before)]
    ok = bool(np.all(before <= -MARGIN))
    if idx is not None:
        ok = ok and bool(past[idx] >= MARGIN)
    return ok


def build(ref, seed):
    a = synthetic_results(seed)
    sink = io.StringIO()
    mu, sigma = ref.estimate_mu_sigma_normal(a)
    rf_inst, rf_smooth, extra = ref.compute_rf_time_series(a, mu, sigma)
    out = {"cols": a[:, KEPT], "col_index": np.array(KEPT, dtype=np.int64), "mu": mu, "sigma": sigma, "S_tot": extra["S_tot"],
           "C": extra["C"], "RF_inst": rf_inst, "RF_smooth": rf_smooth, "seed": np.array(seed, dtype=np.int64)}
    full = []
    for thr in (ref.RF_WARN_THRESHOLD, ref.RF_DANGER_THRESHOLD):
        idx = ref.find_first_alarm_index(rf_smooth, thr, mode="above")
        if not check_margin(rf_smooth, thr, "above", idx):
            return None
        full.append(-1 if idx is None else idx)
    out["full_alarm"] = np.array(full, dtype=np.int64)

    labels = a[:, 17].astype(int)
    cond = []
    for current, fault, index_range in ref.RF_CONDITIONS:
        with contextlib.redirect_stdout(sink):
            delta = ref.compute_rf_advance_for_condition(a, mu, sigma, fault, current, plot=False, index_range=index_range)
        # the sub-series again, to record n and the two indices (the function returns their difference only)
        idx = np.flatnonzero(np.isin(labels, list(ref.FAULT_RANGE_MAP[fault])) & (np.abs(a[:, 0] - current) <= ref.CURRENT_TOL))
        if index_range is not None:
            idx = idx[max(index_range[0], 0):min(index_range[1], len(idx))]
        sub = a[idx]
        _, rs, _ = ref.compute_rf_time_series(sub, mu, sigma)
        v = sub[:, 8]
        v_thr = float(v[0]) - 0.1
        iv = ref.find_first_alarm_index(v, v_thr, mode="below")
        ir = ref.find_first_alarm_index(rs, ref.RF_WARN_THRESHOLD, mode="above")
        assert delta == (iv - ir if iv is not None and ir is not None else None)
        if not (check_margin(v, v_thr, "below", iv) and check_margin(rs, ref.RF_WARN_THRESHOLD, "above", ir)):
            return None
        none = -(1 << 40)                                            # "no value" for the signed delta
        cond.append([current, len(idx), -1 if iv is None else iv, -1 if ir is None else ir, none if delta is None else delta])
    out["conditions"] = np.array(cond, dtype=np.float64)             # current, n, idx_v_alarm, idx_rf_warn, delta_idx
    out["condition_class"] = np.array([list(ref.FAULT_RANGE_MAP).index(f) for _, f, _ in ref.RF_CONDITIONS], dtype=np.int64)

    alt = dict(p_layer=3.0, feature_weights=np.array([1.0, 0.5, 2.0, 1.5, 0.75]), layer_weights={"voltage": 1.0, "gas": 0.5, "temp": 2.0},
               z_safe=3.0, lambda_decay=0.999)
    _, rs2, extra2 = ref.compute_rf_time_series(a, mu, sigma, **alt)
    out["alt_feature_weights"] = alt["feature_weights"]
    out["alt_layer_weights"] = np.array([1.0, 0.5, 2.0])             # voltage, gas, temp
    out["alt_scalars"] = np.array([3.0, 3.0, 0.999])                 # p_layer, z_safe, lambda_decay
    out["alt_C"] = extra2["C"]
    out["alt_RF_smooth"] = rs2
    return out


def time_reference(ref, n=1000000):
    rng = np.random.default_rng(1)
    a = np.zeros((n, 22))
    a[:, 12:17] = rng.normal(0.0, 1.0, (n, 5)) * 3.0
    mu, sigma = np.zeros(5), np.ones(5)
    t0 = time.perf_counter()
    ref.compute_rf_time_series(a, mu, sigma)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="path of the reference's script 04")
    ap.add_argument("--time", action="store_true", help="also time the reference at 1e6 rows")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    for seed in range(20240, 20260):              # the first seed that meets the alarm-margin condition
        out = build(ref, seed)
        if out is not None:
            break
    else:
        raise SystemExit("no seed met the alarm-margin condition")
    assert out["cols"].shape[0] <= 3000
    np.savez_compressed(OUT, **out)
    c = out["conditions"]
    print("seed %d, %d rows, %d bytes" % (seed, out["cols"].shape[0], os.path.getsize(OUT)))
    print("RF warnings: %d of 12, voltage alarms: %d of 12, full-series alarms %s" % ((c[:, 3] >= 0).sum(), (c[:, 2] >= 0).sum(), out["full_alarm"]))
    print("delta_idx:", [None if d < -1e9 else int(d) for d in c[:, 4]])
    if args.time:
        print("reference compute_rf_time_series at 1e6 rows: %.2f s" % time_reference(ref))


if __name__ == "__main__":
    sys.exit(main())
