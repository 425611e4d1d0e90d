"""Generate tests/golden/g_rf_sweep.npz: the reference's script 04 run once per candidate of a fixed parameter grid.

Build machine only, as tools/make_golden_rf.py (same `--reference` argument, matplotlib importable, nothing drawn); neither the
package nor any test imports this file.  The input is make_golden_rf.py's synthetic results array at the seed stored in
tests/golden/g_rf.npz, so both fixtures describe the same rows.  For every candidate of

    z_safe {1.5, 2, 3} x lambda_decay {0.99, 0.9971, 1.0} x alpha_smooth {0.1, 0.2, 1.0} x p_layer {2, 3}
    x k_logistic {5e-4, 2e-3} x C0_logistic {200, 500}                                       (216 candidates, last axis fastest)

and both warning thresholds (0.3 and 0.25; the reference reads RF_WARN_THRESHOLD from its module, so it is set on the imported
module object) the reference's compute_rf_advance_for_condition gives the lead of each of its twelve conditions; the
sub-series is then formed again, as make_golden_rf.py does, to record the two indices.  The thirteenth segment is the run
of normal rows, where the reference's compute_rf_time_series gives the number of rows at or past the threshold and the peak.

Stored, numbers only: `grid` [216, 6] (the axes in the order above), `thresholds` [2], `idx_v_alarm` [12], and per threshold
and candidate `idx_rf_warn` [2, 216, 12], `delta` [2, 216, 12] (NONE where an alarm does not fire), `quiet_alarm_rows`
[2, 216], `peak` [216, 13], and `clear` [2, 216, 13]: 1 where the reference's own RF_smooth keeps every row of that segment
at least 1e-6 away from the threshold, so that rounding differences of 1e-11 cannot move an index or a count there.
"""
import argparse
import contextlib
import io
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_rf import N_NORMAL, ROOT, load_reference, synthetic_results  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g_rf_sweep.npz")
AXES = (("z_safe", (1.5, 2.0, 3.0)), ("lambda_decay", (0.99, 0.9971, 1.0)), ("alpha_smooth", (0.1, 0.2, 1.0)),
        ("p_layer", (2.0, 3.0)), ("k_logistic", (5e-4, 2e-3)), ("C0_logistic", (200.0, 500.0)))
THRESHOLDS = (0.3, 0.25)
MARGIN = 1e-6
NONE = -(1 << 40)


def is_clear(series, thr):
    s = np.asarray(series, dtype=float)
    s = s[~np.isnan(s)]
    return bool(np.all(np.abs(s - thr) >= MARGIN))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="path of the reference's script 04")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    seed = int(np.load(os.path.join(ROOT, "tests", "golden", "g_rf.npz"))["seed"])
    a = synthetic_results(seed)
    mu, sigma = ref.estimate_mu_sigma_normal(a)
    labels = a[:, 17].astype(int)
    subs = []
    for current, fault, index_range in ref.RF_CONDITIONS:
        idx = np.flatnonzero(np.isin(labels, list(ref.FAULT_RANGE_MAP[fault])) & (np.abs(a[:, 0] - current) <= ref.CURRENT_TOL))
        if index_range is not None:
            idx = idx[max(index_range[0], 0):min(index_range[1], len(idx))]
        subs.append(a[idx])
    normal = a[:N_NORMAL]
    assert np.all(labels[:N_NORMAL] == 0) and labels[N_NORMAL] != 0
    idx_v = []
    for sub in subs:
        iv = ref.find_first_alarm_index(sub[:, 8], float(sub[0, 8]) - 0.1, mode="below")
        idx_v.append(-1 if iv is None else iv)

    grid = np.array(list(itertools.product(*[v for _, v in AXES])), dtype=np.float64)
    P, n_cond, T = grid.shape[0], len(subs), len(THRESHOLDS)
    idx_rf = np.full((T, P, n_cond), -1, dtype=np.int64)
    delta = np.full((T, P, n_cond), NONE, dtype=np.int64)
    quiet_rows = np.zeros((T, P), dtype=np.int64)
    peak = np.full((P, n_cond + 1), np.nan)
    clear = np.zeros((T, P, n_cond + 1), dtype=np.int8)
    sink = io.StringIO()
    for i, row in enumerate(grid):
        kw = {name: float(v) for (name, _), v in zip(AXES, row)}
        series = [ref.compute_rf_time_series(sub, mu, sigma, **kw)[1] for sub in subs + [normal]]
        for s, rs in enumerate(series):
            if not np.isnan(rs).all():
                peak[i, s] = np.nanmax(rs)
        for t, thr in enumerate(THRESHOLDS):
            ref.RF_WARN_THRESHOLD = thr
            for c, (current, fault, index_range) in enumerate(ref.RF_CONDITIONS):
                with contextlib.redirect_stdout(sink):
                    d = ref.compute_rf_advance_for_condition(a, mu, sigma, fault, current, plot=False, index_range=index_range, **kw)
                ir = ref.find_first_alarm_index(series[c], thr, mode="above")
                assert d == (idx_v[c] - ir if idx_v[c] >= 0 and ir is not None else None)
                idx_rf[t, i, c] = -1 if ir is None else ir
                delta[t, i, c] = NONE if d is None else d
            quiet_rows[t, i] = int(np.sum(series[-1] >= thr))
            clear[t, i] = [is_clear(rs, thr) for rs in series]
        sink.seek(0)
        sink.truncate()
    np.savez_compressed(OUT, grid=grid, thresholds=np.array(THRESHOLDS), idx_v_alarm=np.array(idx_v, dtype=np.int64), idx_rf_warn=idx_rf,
                        delta=delta, quiet_alarm_rows=quiet_rows, peak=peak, clear=clear, seed=np.array(seed, dtype=np.int64))
    print("seed %d, %d candidates, %d bytes" % (seed, P, os.path.getsize(OUT)))
    print("triples not clear of their threshold: %d of %d" % (int((clear == 0).sum()), clear.size))
    print("RF warnings that fire: %d of %d; quiet alarm rows: max %d" % (int((idx_rf >= 0).sum()), idx_rf.size, int(quiet_rows.max())))


if __name__ == "__main__":
    sys.exit(main())
