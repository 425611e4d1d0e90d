"""CPU: the sweep and calibration of pinn_amd.risk on the host backend: against tests/golden/g_rf_sweep.npz (the reference's
script 04 run per candidate, tools/make_golden_rf_sweep.py), against a loop of rf_advance_for_conditions, rf_grid's product,
the calibration rule on a hand-made integer table, and the argument checks of pinn_rf_sweep through ctypes (no GPU needed:
they return before any launch).  Indices and counts are exact on the triples the fixture marks clear of their threshold
(risk_sweep.py states the margin condition and its 2 % cap)."""
import ctypes

import numpy as np
import pytest

from risk_sweep import GRID_AXES, THRESHOLDS, compare_sweeps, compare_with_fixture, fixture_grid, referee_series
from test_risk_host import results_from_golden


@pytest.fixture(scope="module")
def g(golden):
    return golden("g_rf.npz")


@pytest.fixture(scope="module")
def gs(golden):
    return golden("g_rf_sweep.npz")


@pytest.fixture(scope="module")
def host_sweep(g, gs):
    from pinn_amd import risk
    a = results_from_golden(g)
    assert int(gs["seed"]) == int(g["seed"])
    return a, risk.rf_sweep(a, g["mu"], g["sigma"], fixture_grid(risk, gs), backend="host")


def test_host_sweep_matches_reference_fixture(g, gs, host_sweep):
    from pinn_amd import risk
    a, sw = host_sweep
    assert sw.n_candidates == 432 and sw.n_conditions == 12 and sw.quiet_ranges == [(0, 800)] and sw.backend == "host"
    assert sw.idx_rf_warn.shape == (432, 12) and sw.idx_rf_danger.shape == (432, 12) and sw.fired.dtype == bool
    assert np.array_equal(sw.n_rows, np.full(12, 180)) and not sw.bad.any()
    assert sw.raw["first_warn"].shape == (432, 13) and sw.raw["carry"].shape == (432, 13, 2)
    compare_with_fixture("host", sw, gs)
    assert (gs["idx_rf_warn"] >= 0).sum() > 4000 and (gs["quiet_alarm_rows"] > 0).any()          # the grid does fire, on quiet rows too
    # the sweep against its own series: every triple, under the margin condition
    compare_sweeps("host against its series", sw, sw, referee_series(risk, a, g["mu"], g["sigma"], sw))
    # a candidate's keyword arguments name what was swept
    kw = sw.candidate(5)
    assert kw["warn_threshold"] == THRESHOLDS[1] and kw["C0_logistic"] == 200.0 and kw["k_logistic"] == 2e-3 and kw["danger_threshold"] == 0.6
    assert np.array_equal(kw["feature_weights"], np.ones(5)) and kw["layer_weights"] == {"voltage": 1.0, "gas": 1.0, "temp": 1.0}


def test_host_sweep_equals_loop_of_condition_calls(g, host_sweep, capsys):
    from pinn_amd import risk
    a, sw = host_sweep
    iw, delta, fired = sw.idx_rf_warn, sw.delta_idx, sw.fired
    for i in range(sw.n_candidates):
        table = risk.rf_advance_for_conditions(a, g["mu"], g["sigma"], backend="host", **sw.candidate(i))
        for c, r in enumerate(table):
            assert r["n"] == sw.n_rows[c]
            assert (-1 if r["idx_v_alarm"] is None else r["idx_v_alarm"]) == sw.idx_v_alarm[c]
            assert (-1 if r["idx_rf_warn"] is None else r["idx_rf_warn"]) == iw[i, c], (i, c)
            assert (r["delta_idx"] is not None) == bool(fired[i, c])
            if r["delta_idx"] is not None:
                assert r["delta_idx"] == delta[i, c]
    # the warning threshold reaches the one-condition form and its report
    kw = sw.candidate(1)
    assert kw.pop("danger_threshold") == 0.6 and kw["warn_threshold"] == 0.25
    d = risk.compute_rf_advance_for_condition(a, g["mu"], g["sigma"], "flooding", 108.0, index_range=(0, 1050), backend="host", **kw)
    assert "RF warning threshold = 0.25" in capsys.readouterr().out
    assert d == delta[1, 0] and d >= delta[0, 0] and fired[0, 0]


def test_sweep_segments_bad_candidates_and_fixed_arguments(g):
    from pinn_amd import risk
    a = results_from_golden(g)
    mu, sigma = g["mu"], g["sigma"]
    cand = {"z_safe": np.array([2.0, np.nan, 2.0, 2.0]), "p_layer": np.array([2.0, 2.0, 0.0, 3.0])}
    sw = risk.rf_sweep(a, mu, sigma, cand, conditions=[(108.0, "flooding"), (999.0, "flooding"), (270.0, "membrane_drying", (10, 100))],
                       quiet=[(0, 300), (300, 301)], backend="host", lambda_decay=0.999, feature_weights=[1.0, 0.5, 2.0, 1.5, 0.75])
    assert list(sw.bad) == [False, True, True, False] and list(sw.n_rows) == [180, 0, 90]
    assert sw.raw["first_warn"].shape == (4, 4)                                          # two conditions with rows, two quiet ranges
    assert list(sw.idx_rf_warn[1]) == [-1, -1, -1] and sw.quiet_alarm_rows[1] == 0 and np.isnan(sw.quiet_peak[1])
    assert sw.idx_v_alarm[1] == -1 and not sw.fired[:, 1].any() and np.isnan(sw.peak[0, 1])
    for i in (0, 3):
        kw = sw.candidate(i)
        assert kw["lambda_decay"] == 0.999 and list(kw["feature_weights"]) == [1.0, 0.5, 2.0, 1.5, 0.75]
        table = risk.rf_advance_for_conditions(a, mu, sigma, [(108.0, "flooding"), (999.0, "flooding"), (270.0, "membrane_drying", (10, 100))],
                                               backend="host", **kw)
        assert [(-1 if r["idx_rf_warn"] is None else r["idx_rf_warn"]) for r in table] == list(sw.idx_rf_warn[i])
        kw.pop("warn_threshold"), kw.pop("danger_threshold")
        rs = risk.rf_series(a[:300], mu, sigma, backend="host", **kw)
        assert sw.raw["peak"][i, 2] == rs["RF_smooth"].max() and np.array_equal(sw.raw["carry"][i, 2], rs["carry_out"][0])
    none = risk.rf_sweep(a, mu, sigma, {"z_safe": [2.0]}, conditions=[(108.0, "flooding")], quiet=None, backend="host")
    assert none.raw["first_warn"].shape == (1, 1) and none.quiet_alarm_rows[0] == 0 and np.isnan(none.quiet_peak[0])
    with pytest.raises(ValueError, match="same length"):
        risk.rf_sweep(a, mu, sigma, {"z_safe": [2.0, 3.0], "p_layer": [2.0]}, backend="host")
    with pytest.raises(ValueError, match="both"):
        risk.rf_sweep(a, mu, sigma, {"z_safe": [2.0]}, backend="host", z_safe=3.0)
    with pytest.raises(ValueError, match="structure"):
        risk.rf_sweep(a, mu, sigma, {"res_keys": [("res",)]}, backend="host")
    with pytest.raises(TypeError, match="unknown"):
        risk.rf_sweep(a, mu, sigma, {"z_safe": [2.0]}, backend="host", zsafe=1.0)
    with pytest.raises(ValueError, match="quiet"):
        risk.rf_sweep(a, mu, sigma, {"z_safe": [2.0]}, quiet=[(0, 99999)], backend="host")
    with pytest.raises(ValueError, match="nothing to sweep"):
        risk.rf_sweep(a, mu, sigma, {"z_safe": [2.0]}, conditions=[(999.0, "flooding")], quiet=None, backend="host")


def test_rf_grid_product_and_order():
    import pinn_amd
    from pinn_amd import risk
    assert pinn_amd.rf_grid is risk.rf_grid and pinn_amd.rf_sweep is risk.rf_sweep and pinn_amd.calibrate_rf is risk.calibrate_rf
    grid = risk.rf_grid(z_safe=[1.5, 2, 3], warn_threshold=[0.3, 0.25])
    assert list(grid) == ["z_safe", "warn_threshold"]
    assert grid["z_safe"].tolist() == [1.5, 1.5, 2.0, 2.0, 3.0, 3.0] and grid["warn_threshold"].tolist() == [0.3, 0.25] * 3
    full = risk.rf_grid(**GRID_AXES)
    assert all(v.shape == (216,) for v in full.values())
    assert full["C0_logistic"][:3].tolist() == [200.0, 500.0, 200.0] and full["z_safe"][71] == 1.5 and full["z_safe"][72] == 2.0
    mixed = risk.rf_grid(feature_weights=[[1, 1, 1, 1, 1], [1, 2, 1, 2, 1]], layer_weights=[{"voltage": 1.0}, {"voltage": 2.0, "gas": 0.5}],
                         danger_threshold=[0.5])
    assert mixed["feature_weights"].shape == (4, 5) and mixed["feature_weights"][2].tolist() == [1, 2, 1, 2, 1]
    assert mixed["layer_weights"].shape == (4,) and mixed["layer_weights"][1] == {"voltage": 2.0, "gas": 0.5} and mixed["danger_threshold"].tolist() == [0.5] * 4
    for name in ("res_keys", "layer_config", "columns"):
        with pytest.raises(ValueError, match="structure"):
            risk.rf_grid(**{name: [1, 2]})
    with pytest.raises(TypeError, match="unknown"):
        risk.rf_grid(zsafe=[1.0])
    with pytest.raises(ValueError, match="empty"):
        risk.rf_grid(z_safe=[])


def test_calibration_rule_on_a_hand_made_table():
    from pinn_amd import risk
    choose = risk._calibration_choice
    iv = np.array([50, -1, 40])                                  # the voltage alarm fires on conditions 0 and 2
    ir = np.array([[30, 5, 30],                                  # 0: leads 20, 10 -> min 10, sum 30
                   [35, -1, 25],                                 # 1: leads 15, 15 -> min 15, sum 30: the largest minimum
                   [10, -1, 10],                                 # 2: leads 40, 30, but 3 alarm rows on the quiet segments
                   [35, 7, 25],                                  # 3: as 1: the lower index wins
                   [30, -1, 25],                                 # 4: leads 20, 15 -> min 15, sum 35: beats 1 on the sum
                   [5, -1, -1],                                  # 5: silent on condition 2
                   [0, -1, 0]])                                  # 6: bad
    quiet = np.array([0, 0, 3, 0, 0, 0, 0])
    bad = np.array([0, 0, 0, 0, 0, 0, 1], dtype=bool)
    assert choose(iv, ir, quiet, bad) == 4
    assert choose(iv, ir[:4], quiet[:4], bad[:4]) == 1                                    # tie on (min, sum): the lowest index
    assert choose(iv, ir[:1], quiet[:1], bad[:1]) == 0
    assert choose(iv, ir, quiet, bad, max_quiet_alarm_rows=3) == 2                        # the noisy one becomes feasible and leads
    assert choose(iv, ir[5:6], quiet[5:6], bad[5:6], require_all=False) == 0              # silent on one condition is allowed then
    assert choose(iv, ir[[5, 0]], quiet[[5, 0]], bad[[5, 0]], require_all=False) == 0     # min over the fired ones: 45 beats 10
    # a warning after the voltage alarm is a negative lead, not a failure
    assert choose(np.array([10]), np.array([[30], [20]]), np.zeros(2, int), np.zeros(2, bool)) == 1
    with pytest.raises(ValueError) as e:
        choose(iv, ir[[2, 5, 6]], quiet[[2, 5, 6]], bad[[2, 5, 6]])
    assert str(e.value) == ("no feasible candidate among 3: 1 bad, 1 with more than 0 alarm rows on the quiet segments, "
                            "1 silent on a condition whose voltage alarm fires")
    with pytest.raises(ValueError, match="no condition's voltage alarm fires"):
        choose(np.array([-1, -1]), ir[:, :2], quiet, bad)


def test_calibrate_rf_host(g, gs):
    from pinn_amd import risk
    a = results_from_golden(g)
    grid = risk.rf_grid(**GRID_AXES)
    with pytest.raises(ValueError, match="216 silent on a condition"):                   # the fixture's NaN rows silence one condition
        risk.calibrate_rf(a, g["mu"], g["sigma"], grid, backend="host")
    cal = risk.calibrate_rf(a, g["mu"], g["sigma"], grid, backend="host", require_all=False)
    sw = cal.sweep
    assert cal.index == risk._calibration_choice(sw.idx_v_alarm, sw.idx_rf_warn, sw.quiet_alarm_rows, sw.bad, 0, False)
    assert sw.quiet_alarm_rows[cal.index] == 0 and set(cal.params) == set(risk._SWEEP_NAMES)
    assert all(cal.params[k] == sw.candidate(cal.index)[k] for k in GRID_AXES)
    assert [(-1 if r["idx_rf_warn"] is None else r["idx_rf_warn"]) for r in cal.table] == list(sw.idx_rf_warn[cal.index])
    lead = [r["delta_idx"] for r in cal.table if r["delta_idx"] is not None]
    default = [r["delta_idx"] for r in risk.rf_advance_for_conditions(a, g["mu"], g["sigma"], backend="host") if r["delta_idx"] is not None]
    print("chosen", cal.index, {k: v for k, v in cal.params.items() if k in GRID_AXES}, "leads", lead, "default leads", default)
    assert min(lead) >= min(default)                                                      # the defaults are one candidate of the grid


def test_sweep_entry_point_checks_arguments_on_the_host():
    """NULL, misaligned, empty, overflowing and short-workspace calls return PINN_E_ARG (-1) / PINN_E_WORKSPACE (-3) before a launch."""
    import __graft_entry__ as gentry
    gentry.build()
    from pinn_amd import _lib, risk
    lib = _lib.load(build_if_missing=False)
    one, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    E_ARG, E_WS = -1, -3
    prm = risk._Config().c_struct()
    n = 5000
    need = lib.pinn_rf_sweep_workspace_bytes(n, 5)
    assert need >= 5 * 8 * n and need % 256 == 0 and lib.pinn_rf_sweep_workspace_bytes(0, 5) == 0
    assert _lib.RF_SWEEP_WORDS == risk.SWEEP_WORDS == 24

    def sweep(arr=one, p=ctypes.byref(prm), mu=one, sigma=one, ridx=None, n_rows=n, seg=one, n_seg=3, cand=one, n_cand=4, fw=one, fd=one,
              nw=one, peak=one, carry=None, bad=one, ws=one, ws_bytes=need, n_arr=n):
        return lib.pinn_rf_sweep(arr, 22, n_arr, p, mu, sigma, ridx, n_rows, seg, n_seg, cand, n_cand, fw, fd, nw, peak, carry, bad,
                                 ws, ws_bytes, None)
    for name in ("arr", "p", "mu", "sigma", "seg", "cand", "fw", "fd", "nw", "peak", "bad", "ws"):
        assert sweep(**{name: None}) == E_ARG, name
    for name in ("arr", "mu", "sigma", "ridx", "seg", "cand", "fw", "fd", "nw", "peak", "carry", "ws"):
        assert sweep(**{name: odd}) == E_ARG, name
    assert sweep(bad=ctypes.c_void_p(0x1002)) == E_ARG
    assert sweep(n_cand=0) == E_ARG and sweep(n_cand=-1) == E_ARG
    assert sweep(n_cand=(1 << 31) // 3 + 1) == E_ARG                  # n_cand * n_segments past 2^31 - 1
    assert sweep(n_cand=1 << 31, seg=None, n_seg=0) == E_ARG
    assert sweep(ws_bytes=need - 1) == E_WS and sweep(ws_bytes=0) == E_WS
    assert sweep(n_arr=n - 1) == E_ARG                                 # more positions than rows and no gather list
    assert sweep(n_rows=-1) == E_ARG and sweep(n_seg=-1) == E_ARG
    shape = risk._Config().c_struct()
    shape.col[2] = 22
    assert sweep(p=ctypes.byref(shape)) == E_ARG
    shape = risk._Config().c_struct()
    shape.n_cols = 9
    assert sweep(p=ctypes.byref(shape)) == E_ARG
    shape = risk._Config().c_struct()
    shape.lambda_decay = float("nan")                                  # the scalars of `shape` are ignored: the workspace check is reached
    assert sweep(p=ctypes.byref(shape), ws_bytes=8) == E_WS
