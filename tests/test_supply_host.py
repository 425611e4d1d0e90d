"""CPU: the host backend of pinn_amd.supply (float64 numpy, the solver statement of include/pinn_hip.h, section pinn_bp_fit)
against the brute force of supply_cases.py.

Gates, from the issue and the arithmetic, not from what the code gives:
  G            SSE(theta returned) <= SSE_brute (1 + 1e-9) + 1e-12 sum (y - mean y)^2 (supply_cases states the two terms).
  calibration  the standard deviation of z = (estimate - truth) / se lies in [0.85, 1.15] per parameter over 400 windows
               with status 0 and kind 0 or 1 (the prototype: 0.98 .. 1.05); under 2 % of the windows are left out.
  interval     c_lo <= c <= c_hi for kinds 0 and 1, and the true c inside in at least 90 % of 400 windows (nominal 95 %, the
               margin is for the discretisation to knots).
Every comparison prints its worst figure before it asserts."""
import os
import sys

import numpy as np
import pytest

import supply_cases as C
from pinn_amd import identify as I
from pinn_amd import supply as S

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def host_fit(table, start, length, **kw):
    return S.fit_breakpoints(table, start, length, backend="numpy", **kw)


def test_gate_G_on_the_prototype_windows():
    windows = C.prototype_windows()
    table, start, length = C.stack(windows)
    f = host_fit(table, start, length)
    worst, kinds = -np.inf, np.bincount(f.kind, minlength=4)
    for w, rows in enumerate(windows):
        assert f.status[w] in (0, 5), (w, f.status[w])
        sse, bound = C.gate_G(rows, f.theta[w], C.brute_sse(rows))
        worst = max(worst, (sse - bound) / C.syy(rows))
        assert sse <= bound, (w, sse, bound, f.kind[w], f.k[w])
        # the returned sse is the direct one
        assert abs(f.sse[w] - sse) <= 1e-9 * sse + 1e-12 * C.syy(rows)
    print("gate G over %d windows: worst (sse - bound) / syy = %.3g (gate 0); kinds free/knot/line/constant %s" % (len(windows), worst, kinds))
    assert len(windows) == 300 and kinds[0] > 0 and kinds[1] > 0 and kinds[2] > 0


def test_kinds_and_statuses():
    C.check_kinds_and_statuses(host_fit)


CALIBRATION = {"continuous_400": (400, False, 0.05), "quantised_400": (400, True, 0.05), "continuous_64": (64, False, 0.02)}
_calibration = {}


def calibration_fit(name):
    if name not in _calibration:
        m, quantised, noise = CALIBRATION[name]
        rng = np.random.default_rng(4000 + m + int(quantised))
        table, start, length = C.stack([C.draw(rng, m, quantised, noise) for _ in range(400)])
        _calibration[name] = host_fit(table, start, length)
    return _calibration[name]


@pytest.mark.parametrize("name", list(CALIBRATION))
def test_standard_errors_are_calibrated(name):
    f = calibration_fit(name)
    keep = (f.status == 0) & np.isin(f.kind, (0, 1))
    left_out = 1.0 - keep.mean()
    z = (f.theta[keep] - np.array(C.TRUTH)) / f.se[keep]
    sd = z.std(axis=0)
    print("%s: sd of z %s (gate 0.85 .. 1.15), mean %s, left out %.2f %% (gate < 2 %%)" % (name, np.round(sd, 3), np.round(z.mean(axis=0), 3), 100 * left_out))
    assert left_out < 0.02
    assert np.all(sd >= 0.85) and np.all(sd <= 1.15)


def test_profile_interval():
    f = calibration_fit("continuous_400")
    for name in CALIBRATION:
        g = calibration_fit(name)
        k = np.isin(g.kind, (0, 1))
        assert np.all(g.c_interval[k, 0] <= g.theta[k, 2]) and np.all(g.theta[k, 2] <= g.c_interval[k, 1]), name
    cover = np.mean((f.c_interval[:, 0] <= C.TRUTH[2]) & (C.TRUTH[2] <= f.c_interval[:, 1]))
    print("profile interval: the true c inside in %.1f %% of 400 windows (gate 90 %%, nominal 95 %%)" % (100 * cover))
    assert cover >= 0.90


def test_drift_takes_breakpoint_fits():
    rng = np.random.default_rng(31)
    base = S.fit_breakpoint_baseline(C.draw(rng, 1000, True, 0.05), backend="numpy")
    same = C.draw(rng, 400, True, 0.05)
    lowered = C.draw(rng, 400, True, 0.05, (0.7 * C.TRUTH[0], C.TRUTH[1], C.TRUTH[2]))      # the base value lowered by 30 %
    table, start, length = C.stack([same, lowered])
    f = host_fit(table, start, length)
    d = I.drift(f, base)
    print("drift z: unchanged %s, l1 lowered %s; wald %s p %s" % (np.round(d["z"][0], 2), np.round(d["z"][1], 2), d["wald"], d["p"]))
    assert f.names == ("l1", "l2", "l3") and d["z"].shape == (2, 3) and np.all(np.isfinite(d["wald"]))
    assert f.names[int(np.argmax(np.abs(d["z"][1])))] == "l1" and abs(d["z"][1, 0]) >= 4.0 and d["p"][1] < 1e-6
    assert np.max(np.abs(d["z"][0])) < 4.0


def test_result_views():
    rng = np.random.default_rng(32)
    table, start, length = C.stack([C.draw(rng, 300, True, 0.02), C.status_cases()[0][350:550]])       # the second: every row below c
    f = host_fit(table, start, length)
    assert f.kind[1] == 2 and f.theta[1, 2] == np.inf
    p = f.params("oxygen")
    assert list(p) == ["lambda_O1", "lambda_O2", "lambda_O3"] and p["lambda_O3"][0][1] == np.inf and list(f.params("hydrogen"))[0] == "lambda_H1"
    assert np.isfinite(p["lambda_O3"][1][0]) and np.isnan(p["lambda_O3"][1][1])
    x = np.linspace(f.x_range[0, 0], f.x_range[0, 1], 1001)
    law = S.supply_law(x, f.theta[0])
    assert np.allclose(f.target_range[0], [law.min(), law.max()], rtol=1e-12)
    assert f.inside_oxygen_clamp[0] and f.plateau_F[0] > 100.0 and abs(f.plateau_F[1]) < 1e-6      # the line against itself
    low = host_fit(np.column_stack([table[:300, 0], table[:300, 1] - 1.0]), [0], [300])        # the law dips below 1.05
    assert not low.inside_oxygen_clamp[0]
    with pytest.raises(ValueError):
        f.params("nitrogen")
    with pytest.raises(ValueError):
        host_fit(table, [0], [10], q=0.0)


def test_flow_tables_from_physical_rows():
    from pinn_amd import synth
    X, _ = synth.synth_rows(500, 3)
    X = np.asarray(X, dtype=np.float64)
    It = (X[:, 0] / 270.0 + 1e-5) * 270.0
    # the reference's expressions (01:660-667 and 01:564-566), float64
    q_h2 = np.maximum(It / (2 * 96485.0) * 5 * 22.4 * 60.0, 1e-8)
    q_o2 = np.maximum(It * 5 / (4 * 96485.0) * 22.4 * 60.0, 1e-8)
    h, o = S.flow_table(None, X, "hydrogen"), S.flow_table(None, X, "oxygen")
    assert h.dtype == np.float64 and h.shape == (500, 2) and o.shape == (500, 2)
    assert np.array_equal(h[:, 0], It) and np.array_equal(o[:, 0], It)
    assert np.allclose(h[:, 1], (X[:, 6] + 1e-6) / q_h2, rtol=4e-16, atol=0)
    assert np.allclose(o[:, 1], (X[:, 7] + 1e-6) * 0.21 / q_o2, rtol=4e-16, atol=0)
    with pytest.raises(ValueError):
        S.flow_table(None, X, "air")


def test_tracker_equals_fit_breakpoints_on_the_host():
    C.check_tracker("host", lambda a: a)


def test_example_segments_on_the_host():
    C.check_example("host", lambda a: a)


def test_exports():
    import pinn_amd
    for name in ("flow_table", "fit_breakpoints", "fit_breakpoint_baseline", "BreakpointFit", "SupplyTracker", "supply_law"):
        assert getattr(pinn_amd, name) is getattr(S, name)
    for name in ("fit_windows", "fit_baseline", "drift", "sliding_windows", "WindowFit", "ParameterTracker"):
        assert getattr(pinn_amd, name) is getattr(I, name)
    assert S.sliding_windows is I.sliding_windows
