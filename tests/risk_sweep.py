"""What test_risk_sweep_host.py and test_gpu_risk_sweep.py share: the fixture's grid, the referee series of a sweep, and the
comparison of a sweep against its referee under the margin condition.

Margin condition (a condition on the inputs, not a tolerance): a triple (candidate, segment, threshold) is compared
exactly on its first index and its count only if the REFEREE's RF_smooth stays at least 1e-6 away from the threshold at
every row of the segment; a 1e-11 difference cannot move an index or a count there.  The other triples are still held:
their index may differ only across rows whose referee value lies within 1e-6 of the threshold, their count by no more than
the number of such rows.  The share of such triples may not exceed 2 %: `compare_sweeps` prints the count and fails past it.
Gates on values: peak and carry RF atol 1e-11, carry C rtol 1e-11.
"""
import numpy as np

from test_risk_host import check_series

MARGIN = 1e-6
MAX_EXCLUDED = 0.02
NONE_DELTA = -(1 << 40)
GRID_AXES = dict(z_safe=[1.5, 2.0, 3.0], lambda_decay=[0.99, 0.9971, 1.0], alpha_smooth=[0.1, 0.2, 1.0], p_layer=[2.0, 3.0],
                 k_logistic=[5e-4, 2e-3], C0_logistic=[200.0, 500.0])
THRESHOLDS = [0.3, 0.25]


def fixture_grid(risk, gs):
    """The fixture's 216 candidates at both warning thresholds: candidate 2 i + t is grid row i at threshold t."""
    grid = risk.rf_grid(**GRID_AXES, warn_threshold=THRESHOLDS)      # the last axis is the fastest
    assert np.array_equal(np.stack([grid[k] for k in GRID_AXES], axis=1)[0::2], gs["grid"])
    assert np.array_equal(grid["warn_threshold"][:2], gs["thresholds"])
    return grid


def to_numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def referee_series(risk, a, mu, sigma, sweep):
    """RF_smooth of every candidate of `sweep` over its rows, by the float64 host backend: [P, n] (NaN rows for a bad one)."""
    ridx, starts = to_numpy(sweep.row_index), to_numpy(sweep.seg_starts)
    out = np.full((sweep.n_candidates, len(ridx)), np.nan)
    bad = risk._table_bad(sweep.table)
    for i in range(sweep.n_candidates):
        if bad[i]:
            continue
        prm = sweep.candidate(i)
        prm.pop("warn_threshold"), prm.pop("danger_threshold")
        with np.errstate(all="ignore"):
            out[i] = risk.rf_series(a, mu, sigma, row_index=ridx, seg_starts=starts, backend="host", **prm)["RF_smooth"]
    return out


def _held(seg, thr, near, first, count, want_count):
    """A triple that is not clear of its threshold: the index may move only across near rows, the count by their number."""
    stop = len(seg) if first < 0 else first
    before = seg[:stop]
    ok = bool(np.all((before < thr) | np.isnan(before) | near[:stop]))
    if first >= 0:
        ok = ok and bool(seg[first] >= thr or near[first])
    return ok and (count is None or abs(int(count) - int(want_count)) <= int(near.sum()))


def compare_sweeps(tag, got, want, series):
    """`got` (the sweep under test) against `want` (the host sweep) with `series` = referee_series of it."""
    g = {k: to_numpy(v) for k, v in got.raw.items()}
    w = {k: to_numpy(v) for k, v in want.raw.items()}
    assert np.array_equal(g["bad"].astype(bool), w["bad"].astype(bool)), tag + ": bad flags differ"
    for k in ("first_warn", "first_danger", "n_warn", "peak"):
        assert g[k].shape == w[k].shape, (tag, k)
    check_series(tag + " peak", g["peak"], w["peak"], atol=1e-11)
    check_series(tag + " carry C", g["carry"][..., 0], w["carry"][..., 0], rtol=1e-11)
    check_series(tag + " carry RF", g["carry"][..., 1], w["carry"][..., 1], atol=1e-11)
    starts = to_numpy(want.seg_starts)
    bounds = list(starts) + [series.shape[1]]
    P, S = w["first_warn"].shape
    table = want.table
    excluded = total = fired = 0
    for i in range(P):
        if w["bad"][i]:
            for k, v in (("first_warn", -1), ("first_danger", -1), ("n_warn", 0)):
                assert np.all(g[k][i] == v), (tag, "bad candidate", i, k)
            continue
        for s in range(S):
            seg = series[i, bounds[s]:bounds[s + 1]]
            for thr, key, cnt in ((table[i, 19], "first_warn", "n_warn"), (table[i, 20], "first_danger", None)):
                total += 1
                fired += int(w[key][i, s] >= 0)
                near = np.abs(seg - thr) < MARGIN
                if not near.any():
                    assert g[key][i, s] == w[key][i, s], (tag, key, i, s, g[key][i, s], w[key][i, s])
                    if cnt:
                        assert g[cnt][i, s] == w[cnt][i, s], (tag, cnt, i, s, g[cnt][i, s], w[cnt][i, s])
                else:
                    excluded += 1
                    assert _held(seg, thr, near, int(g[key][i, s]), g[cnt][i, s] if cnt else None, w[cnt][i, s] if cnt else 0), (tag, key, i, s)
    print("%s: %d of %d triples within %.0e of their threshold (held, not exact); %d fire" % (tag, excluded, total, MARGIN, fired))
    assert excluded <= MAX_EXCLUDED * max(total, 1), "%s: inputs: %d of %d triples lie within the margin" % (tag, excluded, total)
    return excluded, total, fired


def compare_with_fixture(tag, sweep, gs):
    """A sweep of fixture_grid's candidates against the reference's recorded values, on the triples the fixture marks clear."""
    iw, qa, pk = sweep.idx_rf_warn, sweep.quiet_alarm_rows, to_numpy(sweep.raw["peak"])
    assert np.array_equal(sweep.idx_v_alarm, gs["idx_v_alarm"])
    delta, fired = sweep.delta_idx, sweep.fired
    skipped = 0
    for t in range(2):
        clear = gs["clear"][t].astype(bool)                      # [216, 13]
        rows = slice(t, None, 2)
        assert np.array_equal(np.where(clear[:, :12], iw[rows], 0), np.where(clear[:, :12], gs["idx_rf_warn"][t], 0)), tag
        want_fired = gs["delta"][t] != NONE_DELTA
        assert np.array_equal(fired[rows] & clear[:, :12], want_fired & clear[:, :12]), tag
        both = want_fired & clear[:, :12]
        assert np.array_equal(delta[rows][both], gs["delta"][t][both]), tag
        assert np.array_equal(qa[rows][clear[:, 12]], gs["quiet_alarm_rows"][t][clear[:, 12]]), tag
        check_series("%s peak, threshold %d" % (tag, t), pk[rows], gs["peak"], atol=1e-11)
        skipped += int((~clear).sum())
    print("%s: %d of %d fixture triples not clear of their threshold" % (tag, skipped, gs["clear"].size))
    assert skipped <= MAX_EXCLUDED * gs["clear"].size
