"""CPU: the host backend of pinn_amd.risk against tests/golden/g_rf.npz (the reference's script 04 on a synthetic results
array, tools/make_golden_rf.py), the label aliases and error cases, and the argument checks of the three C entry points.

Tolerances: S_tot rtol 1e-13, C rtol 1e-11, RF_inst / RF_smooth atol 1e-11, mu atol 1e-13 sigma, sigma rtol 1e-12.
Alarm indices, deltas and NaN positions are exact: the fixture's generator asserts a 1e-6 margin around every alarm."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE_DELTA = -(1 << 40)


def results_from_golden(g):
    a = np.zeros((g["cols"].shape[0], 22))
    a[:, g["col_index"]] = g["cols"]
    return a


def alt_params(g):
    fw, lw, sc = g["alt_feature_weights"], g["alt_layer_weights"], g["alt_scalars"]
    return dict(feature_weights=fw, layer_weights={"voltage": lw[0], "gas": lw[1], "temp": lw[2]}, p_layer=float(sc[0]),
                z_safe=float(sc[1]), lambda_decay=float(sc[2]))


def check_series(name, got, want, rtol=0.0, atol=0.0):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, name
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN positions differ" % name
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    bound = atol + rtol * np.abs(want[ok])
    worst = float((err - bound).max()) if err.size else 0.0
    rel = float((err / np.maximum(np.abs(want[ok]), 1e-300)).max()) if err.size else 0.0
    print("%s: max abs err %.3e, max rel err %.3e" % (name, float(err.max()) if err.size else 0.0, rel))
    assert worst <= 0.0, "%s misses its gate by %.3e" % (name, worst)


def check_stats(mu, sigma, g):
    print("mu err / sigma:", np.abs(mu - g["mu"]) / g["sigma"], "sigma rel err:", np.abs(sigma - g["sigma"]) / g["sigma"])
    assert np.all(np.abs(np.asarray(mu) - g["mu"]) <= 1e-13 * g["sigma"])
    assert np.all(np.abs(np.asarray(sigma) - g["sigma"]) <= 1e-12 * g["sigma"])


def golden_conditions(g):
    out = []
    for row in g["conditions"]:
        iv, ir, d = int(row[2]), int(row[3]), int(row[4])
        out.append({"n": int(row[1]), "idx_v_alarm": None if iv < 0 else iv, "idx_rf_warn": None if ir < 0 else ir,
                    "delta_idx": None if d == NONE_DELTA else d})
    return out


@pytest.fixture(scope="module")
def g(golden):
    return golden("g_rf.npz")


def test_host_series_matches_reference(g):
    from pinn_amd import risk
    a = results_from_golden(g)
    mu, sigma = risk.estimate_mu_sigma_normal(a, backend="host")
    check_stats(mu, sigma, g)
    rf_inst, rf_smooth, extra = risk.compute_rf_time_series(a, g["mu"], g["sigma"], backend="host")
    assert set(extra) == {"S_layers", "S_tot", "C"} and set(extra["S_layers"]) == {"voltage", "gas", "temp"}
    check_series("S_tot", extra["S_tot"], g["S_tot"], rtol=1e-13)
    check_series("C", extra["C"], g["C"], rtol=1e-11)
    check_series("RF_inst", rf_inst, g["RF_inst"], atol=1e-11)
    check_series("RF_smooth", rf_smooth, g["RF_smooth"], atol=1e-11)
    assert np.isnan(g["RF_smooth"]).any() and not np.isnan(g["RF_smooth"][:1700]).any()      # the fixture does hold the NaN rows
    _, rs2, extra2 = risk.compute_rf_time_series(a, g["mu"], g["sigma"], backend="host", **alt_params(g))
    check_series("alt C", extra2["C"], g["alt_C"], rtol=1e-11)
    check_series("alt RF_smooth", rs2, g["alt_RF_smooth"], atol=1e-11)
    for thr, want in zip((risk.RF_WARN_THRESHOLD, risk.RF_DANGER_THRESHOLD), g["full_alarm"]):
        assert risk.find_first_alarm_index(rf_smooth, thr, backend="host") == (None if want < 0 else int(want))


def test_host_conditions_match_reference(g, capsys):
    from pinn_amd import risk
    a = results_from_golden(g)
    want = golden_conditions(g)
    assert sum(w["delta_idx"] is not None for w in want) >= 4 and any(w["idx_rf_warn"] is None for w in want)
    got = risk.rf_advance_for_conditions(a, g["mu"], g["sigma"], backend="host")
    assert len(got) == 12
    for r, w in zip(got, want):
        assert {k: r[k] for k in w} == w
    # one condition at a time, by class name, by the reference's key and by explicit labels
    keys = list(risk.FAULT_ALIASES)
    for (current, name, index_range), w, cls in zip(risk.RF_CONDITIONS, want, g["condition_class"]):
        assert list(risk.FAULT_RANGE_MAP)[cls] == name
        for fault in (name, keys[cls], list(risk.FAULT_RANGE_MAP[name])):
            d = risk.compute_rf_advance_for_condition(a, g["mu"], g["sigma"], fault, current, index_range=index_range, backend="host")
            assert d == w["delta_idx"]
    text = capsys.readouterr().out
    assert "first RF warning (sub-series index): None" in text and "precedes the voltage alarm by" in text
    assert risk.compute_rf_advance_for_condition(a, g["mu"], g["sigma"], "flooding", 999.0, backend="host") is None
    assert risk.compute_rf_advance_for_condition(a, g["mu"], g["sigma"], "flooding", 108.0, index_range=(500, 600), backend="host") is None


def test_find_first_alarm_index_host():
    from pinn_amd import risk
    s = np.array([0.0, np.nan, 0.2, 0.5, 0.1, 0.9])
    assert risk.find_first_alarm_index(s, 0.5) == 3
    assert risk.find_first_alarm_index(s, 0.05, mode="below") == 0
    assert risk.find_first_alarm_index(s, 2.0) is None
    assert risk.find_first_alarm_index(s[1:2], 0.0) is None and risk.find_first_alarm_index(s[1:2], 0.0, mode="below") is None
    with pytest.raises(ValueError):
        risk.find_first_alarm_index(s, 0.5, mode="sideways")


def test_segments_and_carry_host(g):
    """Restarting at segment starts equals separate calls, and a series cut in two and continued from the carried state equals
    the uncut series bit for bit (the host loops are sequential)."""
    from pinn_amd import risk
    a = results_from_golden(g)[:1500]
    whole = risk.rf_series(a, g["mu"], g["sigma"], backend="host")
    first = risk.rf_series(a[:700], g["mu"], g["sigma"], backend="host")
    second = risk.rf_series(a[700:], g["mu"], g["sigma"], carry_in=first["carry_out"], backend="host")
    for k in ("C", "RF_smooth"):
        assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k])
    assert np.array_equal(second["carry_out"], whole["carry_out"])
    seg = risk.rf_series(a, g["mu"], g["sigma"], seg_starts=[0, 700, 701], backend="host")
    parts = [risk.rf_series(a[s:e], g["mu"], g["sigma"], backend="host") for s, e in ((0, 700), (700, 701), (701, 1500))]
    for k in ("C", "RF_smooth"):
        assert np.array_equal(seg[k], np.concatenate([p[k] for p in parts]))
    idx = np.arange(1499, -1, -3)
    assert np.array_equal(risk.rf_series(a, g["mu"], g["sigma"], row_index=idx, backend="host")["C"],
                          risk.rf_series(a[idx], g["mu"], g["sigma"], backend="host")["C"])


def test_error_cases(g):
    import pinn_amd
    from pinn_amd import risk
    a = results_from_golden(g)
    with pytest.raises(ValueError, match="normal"):
        risk.estimate_mu_sigma_normal(a, normal_labels=(99,), backend="host")
    with pytest.raises(ValueError, match="feature_weights"):
        risk.compute_rf_time_series(a, g["mu"], g["sigma"], feature_weights=np.ones(4), backend="host")
    with pytest.raises(ValueError, match="unknown fault"):
        risk.compute_rf_advance_for_condition(a, g["mu"], g["sigma"], "short_circuit", 108.0, backend="host")
    with pytest.raises(NotImplementedError, match="matplotlib"):
        risk.compute_rf_advance_for_condition(a, g["mu"], g["sigma"], "flooding", 108.0, plot=True, backend="host")
    with pytest.raises(ValueError, match="seg_starts"):
        risk.rf_series(a, g["mu"], g["sigma"], seg_starts=[0, 50, 50], backend="host")
    with pytest.raises(ValueError, match="seg_starts"):
        risk.rf_series(a, g["mu"], g["sigma"], seg_starts=[5, 50], backend="host")
    with pytest.raises(ValueError, match="backend"):
        risk.compute_rf_time_series(a, g["mu"], g["sigma"], backend="fpga")
    # the reference's names and defaults, exported from the package
    assert pinn_amd.compute_rf_time_series is risk.compute_rf_time_series and pinn_amd.RiskMonitor is risk.RiskMonitor
    assert risk.INDEX["res"] == 12 and risk.INDEX["label"] == 17 and risk.RF_RES_KEYS == ("res", "pV", "pT", "pH", "pO")
    assert (risk.RF_LAMBDA_DECAY, risk.RF_K_LOGISTIC, risk.RF_C0_LOGISTIC, risk.RF_C_MAX, risk.RF_ALPHA_SMOOTH, risk.RF_Z_SAFE,
            risk.RF_P_LAYER, risk.RF_WARN_THRESHOLD, risk.RF_DANGER_THRESHOLD, risk.CURRENT_TOL) == (
        0.9971, 5e-4, 500.0, 1000.0, 0.2, 2.0, 2.0, 0.3, 0.6, 0.5)
    assert [list(r) for r in risk.FAULT_RANGE_MAP.values()] == [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]]
    # the device backend sums a layer in column order and needs disjoint layers: said, not silently different
    with pytest.raises(ValueError, match="more than one layer"):
        risk._Config(layer_config={"a": ["res"], "b": ["res", "pV"]}).c_struct()


def test_import_needs_numpy_only():
    """pinn_amd.risk and its host backend load neither torch nor the HIP library (a fresh interpreter: this process has both)."""
    import subprocess
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import pinn_amd; from pinn_amd import risk; "
            "a = np.zeros((50, 22)); a[:, 12:17] = np.arange(250).reshape(50, 5) %% 7; "
            "mu, sg = risk.estimate_mu_sigma_normal(a); risk.compute_rf_time_series(a, mu, sg); "
            "assert 'torch' not in sys.modules and 'pinn_amd._lib' not in sys.modules") % ROOT
    subprocess.run([sys.executable, "-c", code], check=True)


def test_entry_points_check_arguments_on_the_host():
    """NULL and too-small workspace arguments fail on the host with PINN_E_ARG (-1) / PINN_E_WORKSPACE (-3): no GPU needed."""
    import __graft_entry__ as gentry
    gentry.build()
    from pinn_amd import _lib
    lib = _lib.load(build_if_missing=False)
    one = ctypes.c_void_p(0x1000)
    E_ARG, E_WS = -1, -3
    cols = (ctypes.c_int * 5)(12, 13, 14, 15, 16)
    normal = (ctypes.c_longlong * 1)(0)
    big = lib.pinn_rf_stats_workspace_bytes()
    assert big > 0
    assert lib.pinn_rf_stats(one, 22, 100, cols, 5, 17, normal, 1, one, one, None, None, big, None) == E_ARG
    assert lib.pinn_rf_stats(one, 22, 100, cols, 5, 17, normal, 1, one, one, None, one, 16, None) == E_WS
    assert lib.pinn_rf_stats(None, 22, 100, cols, 5, 17, normal, 1, one, one, None, one, big, None) == E_ARG
    assert lib.pinn_rf_stats(one, 22, 100, cols, 5, 17, normal, 1, None, one, None, one, big, None) == E_ARG
    assert lib.pinn_rf_stats(one, 16, 100, cols, 5, 15, normal, 1, one, one, None, one, big, None) == E_ARG        # column 16 of 16
    assert lib.pinn_rf_stats(one, 22, 100, cols, 9, 17, normal, 1, one, one, None, one, big, None) == E_ARG
    assert lib.pinn_rf_stats(ctypes.c_void_p(0x1004), 22, 100, cols, 5, 17, normal, 1, one, one, None, one, big, None) == E_ARG

    from pinn_amd import risk
    prm = risk._Config().c_struct()
    n = 100000
    need = lib.pinn_rf_workspace_bytes(n, 1)
    assert need >= 2 * 8 * n and lib.pinn_rf_workspace_bytes(_lib.RF_TILE, 1) == 0 and lib.pinn_rf_workspace_bytes(_lib.RF_TILE + 1, 1) > 0

    def series(arr=one, n_rows=n, p=ctypes.byref(prm), mu=one, sigma=one, ws=one, ws_bytes=need, seg=None, n_seg=0, ridx=None, n_arr=n):
        return lib.pinn_rf_series(arr, 22, n_arr, p, mu, sigma, ridx, n_rows, seg, n_seg, None, None, None, one, None, one, None,
                                  ws, ws_bytes, None)
    assert series(ws=None) == E_ARG
    assert series(ws_bytes=need - 1) == E_WS
    assert series(arr=None) == E_ARG and series(mu=None) == E_ARG and series(sigma=None) == E_ARG and series(p=None) == E_ARG
    assert series(n_seg=3) == E_ARG                                    # segments announced without their starts
    assert series(n_arr=n - 1) == E_ARG                                # more positions than rows and no gather list
    assert series(ws=ctypes.c_void_p(0x1004)) == E_ARG
    bad = risk._Config().c_struct()
    bad.col[2] = 22
    assert series(p=ctypes.byref(bad)) == E_ARG
    bad = risk._Config().c_struct()
    bad.lambda_decay = float("nan")
    assert series(p=ctypes.byref(bad)) == E_ARG

    assert lib.pinn_rf_first_alarm(one, 1, 100, None, 100, None, 0, _lib.RF_ABOVE, 0, 0.3, None, None) == E_ARG
    assert lib.pinn_rf_first_alarm(None, 1, 100, None, 100, None, 0, _lib.RF_ABOVE, 0, 0.3, one, None) == E_ARG
    assert lib.pinn_rf_first_alarm(one, 1, 100, None, 100, None, 2, _lib.RF_ABOVE, 0, 0.3, one, None) == E_ARG
    assert lib.pinn_rf_first_alarm(one, 1, 100, None, 100, None, 0, 7, 0, 0.3, one, None) == E_ARG
    assert lib.pinn_rf_first_alarm(one, 1, 50, None, 100, None, 0, _lib.RF_BELOW, 0, 0.3, one, None) == E_ARG
    assert lib.pinn_abi_version() == 2
    assert ctypes.sizeof(_lib.RFParams) == 4 * 2 + 4 * 8 * 2 + 8 * 8 + 8 * 4 + 8 * 7


def test_risk_module_never_imports_the_oracle_or_the_reference():
    pkg = os.path.join(ROOT, "physics-informed-neural-network-for-explainable-fault-diagnosis-in-fuel-cells_amd")
    for rel in ("risk.py", os.path.join("csrc", "pinn_risk.hip")):
        txt = open(os.path.join(pkg, rel), encoding="utf-8").read()
        for word in ("pinn_oracle", "import oracle", "/reference", "04_risk_function", "matplotlib.pyplot", "make_golden"):
            assert word not in txt, (rel, word)
