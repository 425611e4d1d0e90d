"""GPU: pinn_rf_sweep (csrc/pinn_risk.hip) behind pinn_amd.risk.rf_sweep / calibrate_rf, against the float64 host backend at
the gates of DESIGN 3f: peak and carry RF atol 1e-11, carry C rtol 1e-11, indices and counts exact under the margin
condition that risk_sweep.py states (with its 2 % cap on the triples that lie within 1e-6 of their threshold), and against
tests/golden/g_rf_sweep.npz, the reference's own values.  Every comparison prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from risk_sweep import GRID_AXES, MARGIN, compare_sweeps, compare_with_fixture, fixture_grid, referee_series, to_numpy
from test_gpu_risk import MU5, SIGMA5, dev, synthetic
from test_risk_host import results_from_golden

pytestmark = pytest.mark.gpu

SEG_ROWS = (1, 7, 2047, 2048, 2049, 4100, 6000)                 # below, on and above one tile; two and three tiles
EDGE_AXES = dict(C0_logistic=[10.0, 400.0], lambda_decay=[0.99, 0.9971, 1.0], alpha_smooth=[0.2, 1.0], p_layer=[2.0, 3.0])
EDGE_FIXED = dict(k_logistic=1e-2)      # a steep logistic: first alarms from row 14 to row 2432, counts from 6 rows to nearly all


@pytest.fixture(scope="module")
def g(golden):
    return golden("g_rf.npz")


@pytest.fixture(scope="module")
def gs(golden):
    return golden("g_rf_sweep.npz")


@pytest.fixture(scope="module")
def fixture_sweeps(g, gs):
    """The fixture's grid at both thresholds (432 candidates x 13 segments): device sweep, host sweep and the referee series, once."""
    from pinn_amd import risk
    a = results_from_golden(g)
    grid = fixture_grid(risk, gs)
    want = risk.rf_sweep(a, g["mu"], g["sigma"], grid, backend="host")
    got = risk.rf_sweep(dev(a), g["mu"], g["sigma"], grid)
    return a, grid, got, want, referee_series(risk, a, g["mu"], g["sigma"], want)


@pytest.fixture(scope="module")
def edge_sweeps():
    """Seven segments of 1 to 6000 rows cut from one synthetic series, 24 candidates including alpha = 1, lambda = 1, p = 3."""
    from pinn_amd import risk
    a = synthetic(40000, 7) * 1.5
    ends = np.cumsum(SEG_ROWS)
    ranges = list(zip([0] + list(ends[:-1]), ends))
    grid = risk.rf_grid(**EDGE_AXES)
    want = risk.rf_sweep(a, MU5, SIGMA5, grid, conditions=[], quiet=ranges, backend="host", **EDGE_FIXED)
    got = risk.rf_sweep(dev(a), MU5, SIGMA5, grid, conditions=[], quiet=ranges, **EDGE_FIXED)
    return a, got, want, referee_series(risk, a, MU5, SIGMA5, want)


def test_fixture_grid_against_host_and_reference(gs, fixture_sweeps):
    a, grid, got, want, series = fixture_sweeps
    assert got.backend == "device" and got.raw["first_warn"].is_cuda and got.raw["first_warn"].shape == (432, 13)
    assert np.array_equal(got.idx_v_alarm, want.idx_v_alarm) and np.array_equal(got.n_rows, want.n_rows)
    assert np.array_equal(to_numpy(got.row_index), want.row_index) and np.array_equal(to_numpy(got.seg_starts), want.seg_starts)
    excluded, total, fired = compare_sweeps("fixture grid", got, want, series)
    assert total == 432 * 13 * 2 and fired > 4000
    compare_with_fixture("device", got, gs)


def test_tile_edges_and_carry_between_tiles(edge_sweeps):
    a, got, want, series = edge_sweeps
    assert got.raw["peak"].shape == (24, 7) and not np.isnan(to_numpy(want.raw["carry"])).any()
    excluded, total, fired = compare_sweeps("tile edges", got, want, series)
    assert total == 336 and fired >= 150                         # the series do cross their thresholds (a 7-row segment cannot)
    w = to_numpy(want.raw["first_warn"])
    assert (w[:, 4:] >= 2048).any(), "no first warning lies past the first tile"
    assert len(np.unique(to_numpy(want.raw["n_warn"])[:, 5:])) > 30      # counts run over all tiles of a segment


def test_each_candidate_equals_series_kernel_and_first_alarm(edge_sweeps):
    """The sweep against what the shipped kernels give one candidate at a time: pinn_rf_series on the same gather list and
    segments, then pinn_rf_first_alarm per threshold.  The margin condition is taken on the device series here."""
    from pinn_amd import risk
    a, got, want, _ = edge_sweeps
    ad = dev(a)
    raw = {k: to_numpy(v) for k, v in got.raw.items()}
    starts = to_numpy(got.seg_starts)
    bounds = list(starts) + [int(got.row_index.numel())]
    excluded = total = 0
    worst_peak = worst_c = worst_rf = 0.0
    for i in range(got.n_candidates):
        kw = got.candidate(i)
        thr = (kw.pop("warn_threshold"), kw.pop("danger_threshold"))
        r = risk.rf_series(ad, MU5, SIGMA5, row_index=got.row_index, seg_starts=got.seg_starts, **kw)
        firsts = [risk._device_first(r["RF_smooth"], t, "above", seg_starts=got.seg_starts).cpu().numpy() for t in thr]
        rs, carry = r["RF_smooth"].cpu().numpy(), r["carry_out"].cpu().numpy()
        if i == 0:                                               # the public search, on one candidate's segments
            for s in range(len(starts)):
                f = risk.find_first_alarm_index(r["RF_smooth"][bounds[s]:bounds[s + 1]], thr[0])
                assert firsts[0][s] == (-1 if f is None else f)
        for s in range(len(starts)):
            seg = rs[bounds[s]:bounds[s + 1]]
            worst_peak = max(worst_peak, abs(raw["peak"][i, s] - seg.max()))
            worst_rf = max(worst_rf, abs(raw["carry"][i, s, 1] - carry[s, 1]))
            worst_c = max(worst_c, abs(raw["carry"][i, s, 0] - carry[s, 0]) / max(abs(carry[s, 0]), 1e-300))
            for t, key in enumerate(("first_warn", "first_danger")):
                total += 1
                if (np.abs(seg - thr[t]) < MARGIN).any():
                    excluded += 1
                    continue
                assert raw[key][i, s] == firsts[t][s], (key, i, s, raw[key][i, s], firsts[t][s])
                if t == 0:
                    assert raw["n_warn"][i, s] == int((seg >= thr[0]).sum()), (i, s)
    print("against pinn_rf_series: peak err %.3e, carry RF err %.3e, carry C rel err %.3e; %d of %d triples within the margin"
          % (worst_peak, worst_rf, worst_c, excluded, total))
    assert worst_peak <= 1e-11 and worst_rf <= 1e-11 and worst_c <= 1e-11
    assert excluded <= 0.02 * total


def _direct(risk, a, table, ridx, starts, mu=MU5, sigma=SIGMA5):
    """pinn_rf_sweep and its host twin on a gather list given as it stands (rf_sweep builds ascending lists only).  The host
    side reads a row of NaN where the list points outside the array, which is what 'reads nothing' means."""
    cfg0 = risk._Config()
    ridx, starts = np.asarray(ridx, dtype=np.int64), np.asarray(starts, dtype=np.int64)
    outside = (ridx < 0) | (ridx >= a.shape[0])
    a_ext = np.vstack([a, np.full((1, a.shape[1]), np.nan)])
    ridx_h = np.where(outside, a.shape[0], ridx)
    raw_h = risk._host_sweep(a_ext, mu, sigma, cfg0, {}, table, ridx_h, starts)
    raw_d = risk._device_sweep(dev(a), mu, sigma, cfg0, table, dev(ridx), dev(starts))
    mk = lambda raw, be, r: risk.RFSweep(raw, [], [], [], table, cfg0, {}, [], be, r, starts)        # noqa: E731
    want, got = mk(raw_h, "host", ridx_h), mk(raw_d, "device", ridx)
    return got, want, referee_series(risk, a_ext, mu, sigma, want)


def _table(risk, rows):
    """Candidate words from keyword dicts over the defaults."""
    cand = {k: [r.get(k, risk._SWEEP_DEFAULTS[k]) for r in rows] for k in risk._SWEEP_SCALARS}
    return risk._candidate_table(cand, {})[3]


def test_nan_rows_gathers_and_special_candidates():
    from pinn_amd import risk
    a = synthetic(9000, 23) * 1.5
    a[1203, 14] = np.nan                                         # two NaN rows, in different columns, inside segment 1
    a[1250, 16] = np.nan
    rng = np.random.default_rng(5)
    ridx = np.concatenate([np.arange(0, 1000), np.arange(1000, 4000), rng.permutation(9000)[:2500], np.arange(8999, 6999, -1)])
    ridx[700] = 9000                                             # one past the array
    ridx[4100] = -3
    starts = [0, 1000, 4000, 6500]
    rows = [dict(), dict(k_logistic=0.0), dict(z_safe=float("nan")), dict(alpha_smooth=1.0, lambda_decay=1.0, p_layer=3.0), dict(p_layer=0.0),
            dict(warn_threshold=0.2, danger_threshold=0.5), dict(C_max=float("inf")), dict(z_safe=1.0, C0_logistic=200.0, k_logistic=2e-3)]
    table = _table(risk, rows)
    got, want, series = _direct(risk, a, table, ridx, starts)
    excluded, total, fired = compare_sweeps("special", got, want, series)
    raw = {k: to_numpy(v) for k, v in got.raw.items()}
    assert list(raw["bad"]) == [False, False, True, False, True, False, True, False]
    for i in (2, 4, 6):                                          # flagged, and nothing but the empty result
        assert np.all(raw["first_warn"][i] == -1) and np.all(raw["n_warn"][i] == 0) and np.isnan(raw["peak"][i]).all() and np.isnan(raw["carry"][i]).all()
    assert np.all(raw["peak"][1] == 0.0) and np.all(raw["first_warn"][1] == -1)          # k = 0: denom -> 1e-6, RF stays 0
    # a NaN stays in its segment, and the rows before it still count
    assert np.isnan(raw["carry"][0, 0]).all() and np.isnan(raw["carry"][0, 1]).all() and np.isnan(raw["carry"][0, 2]).all()
    assert not np.isnan(raw["carry"][0, 3]).any() and not np.isnan(raw["peak"][0]).any()
    assert fired > 10 and raw["first_warn"][0, 3] >= 0
    # the neighbours of a bad candidate equal the same candidates swept alone
    alone, _, _ = _direct(risk, a, table[[0, 3, 5, 7]], ridx, starts)
    for k in ("first_warn", "first_danger", "n_warn", "peak", "carry"):
        assert np.array_equal(to_numpy(alone.raw[k]), raw[k][[0, 3, 5, 7]], equal_nan=True), k


def test_one_candidate_one_segment_and_a_grid_past_the_resident_workgroups(g):
    from pinn_amd import risk
    a = results_from_golden(g)
    ad = dev(a)
    one = dict(conditions=[(405.0, "flooding")], quiet=None)
    grid = {"z_safe": [2.0]}
    got, want = risk.rf_sweep(ad, g["mu"], g["sigma"], grid, **one), risk.rf_sweep(a, g["mu"], g["sigma"], grid, backend="host", **one)
    assert got.raw["first_warn"].shape == (1, 1) and int(got.seg_starts.numel()) == 1
    compare_sweeps("P = 1", got, want, referee_series(risk, a, g["mu"], g["sigma"], want))
    grid = {"z_safe": np.linspace(1.0, 3.5, 1025), "lambda_decay": np.where(np.arange(1025) % 2 == 0, 0.9971, 1.0)}
    got, want = risk.rf_sweep(ad, g["mu"], g["sigma"], grid, **one), risk.rf_sweep(a, g["mu"], g["sigma"], grid, backend="host", **one)
    assert got.raw["first_warn"].shape == (1025, 1) and got.n_rows.tolist() == [180]
    excluded, total, fired = compare_sweeps("P = 1025", got, want, referee_series(risk, a, g["mu"], g["sigma"], want))
    assert total == 2050 and fired > 500 and len(np.unique(want.idx_rf_warn)) > 10


def _same_bytes(x, y):
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t          # noqa: E731  (NaN == NaN as bytes)
    return x.shape == y.shape and torch.equal(bits(x), bits(y))


def test_two_calls_give_identical_bytes(g, fixture_sweeps, edge_sweeps):
    from pinn_amd import risk
    a, grid, got, _, _ = fixture_sweeps
    again = risk.rf_sweep(dev(a), g["mu"], g["sigma"], grid)
    for k, v in got.raw.items():
        assert _same_bytes(v, again.raw[k]), k
    e, first = edge_sweeps[0], edge_sweeps[1]
    ends = np.cumsum(SEG_ROWS)
    again = risk.rf_sweep(dev(e), MU5, SIGMA5, risk.rf_grid(**EDGE_AXES), conditions=[], quiet=list(zip([0] + list(ends[:-1]), ends)), **EDGE_FIXED)
    for k, v in first.raw.items():
        assert _same_bytes(v, again.raw[k]), k


def test_calibrate_on_the_device_and_replay_through_the_monitor(g, fixture_sweeps):
    from pinn_amd import risk
    a = fixture_sweeps[0]
    ad = dev(a)
    grid = risk.rf_grid(**GRID_AXES)
    with pytest.raises(ValueError, match="216 silent on a condition"):                   # the fixture's NaN rows silence one condition
        risk.calibrate_rf(ad, g["mu"], g["sigma"], grid)
    host = risk.calibrate_rf(a, g["mu"], g["sigma"], grid, backend="host", require_all=False)
    cal = risk.calibrate_rf(ad, g["mu"], g["sigma"], grid, require_all=False)
    print("chosen on the device %d, on the host %d: %s" % (cal.index, host.index, {k: cal.params[k] for k in GRID_AXES}))
    assert cal.index == host.index and cal.sweep.backend == "device"
    assert np.array_equal(cal.sweep.quiet_alarm_rows, host.sweep.quiet_alarm_rows)
    assert [{k: r[k] for k in ("n", "idx_v_alarm", "idx_rf_warn", "delta_idx")} for r in cal.table] == \
           [{k: r[k] for k in ("n", "idx_v_alarm", "idx_rf_warn", "delta_idx")} for r in host.table]
    labels, current = a[:, 17].astype(int), a[:, 0]
    replayed = 0
    for (cur, name, index_range), r in zip(risk.RF_CONDITIONS, cal.table):
        rows = np.flatnonzero(np.isin(labels, list(risk.FAULT_RANGE_MAP[name])) & (np.abs(current - cur) <= risk.CURRENT_TOL))
        if index_range is not None:
            rows = rows[index_range[0]:index_range[1]]
        mon = risk.RiskMonitor(g["mu"], g["sigma"], **cal.params)
        for s in range(0, len(rows), 64):
            mon.update(ad[torch.from_numpy(rows[s:s + 64]).cuda()])
        assert mon.first_warning == r["idx_rf_warn"], (name, cur)
        replayed += r["idx_rf_warn"] is not None
    assert replayed >= 8
