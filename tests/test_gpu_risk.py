"""GPU: the device backend of pinn_amd.risk (csrc/pinn_risk.hip) against tests/golden/g_rf.npz and against the package's
host backend (float64 numpy, sequential loops).

Gates (derived from the arithmetic, not from what the kernels give): S_tot rtol 1e-13, C rtol 1e-11, RF_inst and
RF_smooth atol 1e-11, mu atol 1e-13 sigma, sigma rtol 1e-12; alarm indices and NaN positions exact.  Every comparison
prints its maxima before it asserts.  Where a test draws its own series it first checks the 1e-6 alarm margin on the host
series: a condition on the inputs, under which a 1e-11 difference cannot move an index."""
import numpy as np
import pytest
import torch

from test_risk_host import alt_params, check_series, check_stats, golden_conditions, results_from_golden

pytestmark = pytest.mark.gpu

TILE = 2048
MU5, SIGMA5 = np.zeros(5), np.ones(5)


@pytest.fixture(scope="module")
def g(golden):
    return golden("g_rf.npz")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def synthetic(n, seed):
    """Residual columns with a slowly breathing amplitude: C swings between a few tens and well past C_max."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 22))
    amp = 1.0 + 2.2 * np.sin(2 * np.pi * np.arange(n) / 90000.0) ** 2
    a[:, 12:17] = rng.normal(size=(n, 5)) * amp[:, None]
    a[:, 8] = 3.4 + rng.normal(0, 0.005, n)
    return a


def margin_ok(series, thr, idx, mode="above"):
    past = (series - thr) if mode == "above" else (thr - series)
    before = past if idx is None else past[:idx]
    before = before[~np.isnan(before)]
    return bool(np.all(before <= -1e-6)) and (idx is None or bool(past[idx] >= 1e-6))


def compare_all(tag, got, want):
    check_series(tag + " S_tot", got["S_tot"], want["S_tot"], rtol=1e-13)
    check_series(tag + " C", got["C"], want["C"], rtol=1e-11)
    check_series(tag + " RF_inst", got["RF_inst"], want["RF_inst"], atol=1e-11)
    check_series(tag + " RF_smooth", got["RF_smooth"], want["RF_smooth"], atol=1e-11)
    co, wo = np.asarray(got["carry_out"]), np.asarray(want["carry_out"])
    check_series(tag + " carry C", co[:, 0], wo[:, 0], rtol=1e-11)
    check_series(tag + " carry RF", co[:, 1], wo[:, 1], atol=1e-11)


def test_device_matches_reference_fixture(g):
    from pinn_amd import risk
    a = results_from_golden(g)
    mu, sigma = risk.estimate_mu_sigma_normal(a, backend="device")
    assert isinstance(mu, np.ndarray)
    check_stats(mu, sigma, g)
    mu_d, sigma_d = risk.estimate_mu_sigma_normal(dev(a))
    assert mu_d.is_cuda and np.array_equal(mu_d.cpu().numpy(), mu) and np.array_equal(sigma_d.cpu().numpy(), sigma)
    rf_inst, rf_smooth, extra = risk.compute_rf_time_series(dev(a), g["mu"], g["sigma"])
    assert rf_smooth.is_cuda and extra["C"].is_cuda and set(extra["S_layers"]) == {"voltage", "gas", "temp"}
    check_series("S_tot", extra["S_tot"].cpu().numpy(), g["S_tot"], rtol=1e-13)
    check_series("C", extra["C"].cpu().numpy(), g["C"], rtol=1e-11)
    check_series("RF_inst", rf_inst.cpu().numpy(), g["RF_inst"], atol=1e-11)
    check_series("RF_smooth", rf_smooth.cpu().numpy(), g["RF_smooth"], atol=1e-11)
    layers = sum(v.cpu().numpy() for v in extra["S_layers"].values())
    check_series("sum of S_layers", layers, g["S_tot"], rtol=1e-13)
    # numpy in, numpy out
    _, rs2, extra2 = risk.compute_rf_time_series(a, g["mu"], g["sigma"], backend="device", **alt_params(g))
    assert isinstance(rs2, np.ndarray)
    check_series("alt C", extra2["C"], g["alt_C"], rtol=1e-11)
    check_series("alt RF_smooth", rs2, g["alt_RF_smooth"], atol=1e-11)
    for thr, want in zip((risk.RF_WARN_THRESHOLD, risk.RF_DANGER_THRESHOLD), g["full_alarm"]):
        assert risk.find_first_alarm_index(rf_smooth, thr) == (None if want < 0 else int(want))
    v = dev(a[:, 8])
    assert risk.find_first_alarm_index(v, float(a[0, 8]) - 0.1, mode="below") == risk.find_first_alarm_index(
        a[:, 8], float(a[0, 8]) - 0.1, mode="below", backend="host")
    nan = dev(np.full(300, np.nan))
    assert risk.find_first_alarm_index(nan, 0.0) is None and risk.find_first_alarm_index(nan, 0.0, mode="below") is None


def test_batched_conditions_equal_single_calls_and_reference(g, capsys):
    from pinn_amd import risk
    a = results_from_golden(g)
    ad = dev(a)
    want = golden_conditions(g)
    got = risk.rf_advance_for_conditions(ad, g["mu"], g["sigma"])
    for r, w in zip(got, want):
        assert {k: r[k] for k in w} == w
    singles = [risk.compute_rf_advance_for_condition(ad, g["mu"], g["sigma"], name, current, index_range=rng)
               for current, name, rng in risk.RF_CONDITIONS]
    capsys.readouterr()
    assert singles == [w["delta_idx"] for w in want]
    # the concatenated series itself: one call with twelve segments against twelve calls
    labels, current = a[:, 17].astype(int), a[:, 0]
    lists = [np.flatnonzero(np.isin(labels, list(risk.FAULT_RANGE_MAP[name])) & (np.abs(current - cur) <= risk.CURRENT_TOL))
             for cur, name, _ in risk.RF_CONDITIONS]
    starts = np.concatenate([[0], np.cumsum([len(l) for l in lists])[:-1]])
    batched = risk.rf_series(ad, g["mu"], g["sigma"], row_index=np.concatenate(lists), seg_starts=starts)
    one = [risk.rf_series(ad, g["mu"], g["sigma"], row_index=l) for l in lists]
    for k, (rtol, atol) in {"S_tot": (1e-13, 0), "C": (1e-11, 0), "RF_inst": (0, 1e-11), "RF_smooth": (0, 1e-11)}.items():
        check_series("batched " + k, batched[k].cpu().numpy(), np.concatenate([o[k].cpu().numpy() for o in one]), rtol=rtol, atol=atol)
    check_series("batched carry", batched["carry_out"].cpu().numpy()[:, 0], np.array([o["carry_out"].cpu().numpy()[0, 0] for o in one]), rtol=1e-11)


@pytest.mark.parametrize("source,chunk", [("golden", 1), ("golden", 7), ("synthetic", 4096), ("synthetic", 100003)])
def test_monitor_chunking_invariance(g, source, chunk):
    from pinn_amd import risk
    if source == "golden":
        a, mu, sigma = results_from_golden(g)[:1700], g["mu"], g["sigma"]          # up to the fixture's NaN rows
    else:
        a, mu, sigma = synthetic(250000, 6), MU5, SIGMA5
    whole = risk.rf_series(a, mu, sigma, backend="host")
    firsts = [risk.find_first_alarm_index(whole["RF_smooth"], thr, backend="host") for thr in (0.3, 0.6)]
    assert firsts[0] is not None and firsts[1] is not None
    assert all(margin_ok(whole["RF_smooth"], thr, i) for thr, i in zip((0.3, 0.6), firsts)), "inputs: alarm margin below 1e-6"
    ad = dev(a)
    mon = risk.RiskMonitor(mu, sigma)
    rs, cs = [], []
    for s in range(0, a.shape[0], chunk):
        r, c = mon.update(ad[s:s + chunk], return_C=True)
        rs.append(r)
        cs.append(c)
    rs, cs = torch.cat(rs).cpu().numpy(), torch.cat(cs).cpu().numpy()
    check_series("chunk %d C" % chunk, cs, whole["C"], rtol=1e-11)
    check_series("chunk %d RF_smooth" % chunk, rs, whole["RF_smooth"], atol=1e-11)
    assert [mon.first_warning, mon.first_danger] == firsts and mon.n_seen == a.shape[0]
    dwhole = risk.rf_series(ad, mu, sigma)
    assert [risk.find_first_alarm_index(dwhole["RF_smooth"], thr) for thr in (0.3, 0.6)] == firsts
    check_series("state C", np.array(mon.state[:1]), whole["C"][-1:], rtol=1e-11)
    mon.reset()
    assert mon.state is None and mon.first_warning is None and mon.n_seen == 0


def _windows_against_host(n, full_host):
    from pinn_amd import risk
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n % 1000 + 3)
    ad = torch.zeros(n, 22, dtype=torch.float64, device="cuda")
    amp = 1.0 + 2.2 * torch.sin(2 * np.pi * torch.arange(n, device="cuda", dtype=torch.float64) / 90000.0) ** 2
    ad[:, 12:17] = torch.randn(n, 5, dtype=torch.float64, device="cuda", generator=gen) * amp[:, None]
    del amp
    d = risk.rf_series(ad, MU5, SIGMA5)
    W = 65536
    for start in (0, (n // 2) - W // 2, n - W):
        rows = ad[start:start + W].cpu().numpy()
        carry = None if start == 0 else np.array([[d["C"][start - 1].item(), d["RF_smooth"][start - 1].item()]])
        h = risk.rf_series(rows, MU5, SIGMA5, carry_in=carry, backend="host")
        got = {k: d[k][start:start + W].cpu().numpy() for k in ("S_tot", "C", "RF_inst", "RF_smooth")}
        got["carry_out"] = np.array([[got["C"][-1], got["RF_smooth"][-1]]])
        compare_all("n=%d window@%d" % (n, start), got, h)
    last = d["carry_out"].cpu().numpy()
    assert last[0, 0] == d["C"][-1].item() and last[0, 1] == d["RF_smooth"][-1].item()
    if full_host:
        h = risk.rf_series(ad.cpu().numpy(), MU5, SIGMA5, backend="host")
        compare_all("n=%d full" % n, {k: (v.cpu().numpy() if k != "S_layers" else v) for k, v in d.items()}, h)
    mu, sigma = risk.estimate_mu_sigma_normal(ad)
    print("n=%d mu, sigma:" % n, mu.cpu().numpy(), sigma.cpu().numpy())
    if full_host:
        mh, sh = risk.estimate_mu_sigma_normal(ad.cpu().numpy(), backend="host")
        err_mu = np.abs(mu.cpu().numpy() - mh) / sh
        err_sg = np.abs(sigma.cpu().numpy() - sh) / sh
        print("n=%d stats: mu err / sigma %.3e, sigma rel err %.3e" % (n, err_mu.max(), err_sg.max()))
        assert err_mu.max() <= 1e-13 and err_sg.max() <= 1e-12


def test_full_size_windows_1e6():
    _windows_against_host(1_000_000, full_host=True)


def test_full_size_windows_1e7():
    """1e7 rows when the card has the memory for the 1.76 GB array, the outputs and the workspace; else 4e6."""
    free, _ = torch.cuda.mem_get_info()
    _windows_against_host(10_000_000 if free > 6 * (1 << 30) else 4_000_000, full_host=False)


@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE, 3 * TILE + 1])
def test_ragged_sizes(n):
    from pinn_amd import risk
    a = synthetic(n, 11) * 2.0
    got = risk.rf_series(a, MU5, SIGMA5, backend="device")
    compare_all("n=%d" % n, got, risk.rf_series(a, MU5, SIGMA5, backend="host"))
    carry = np.array([[321.5, 0.25]])
    got = risk.rf_series(a, MU5, SIGMA5, carry_in=carry, backend="device")
    compare_all("n=%d carried" % n, got, risk.rf_series(a, MU5, SIGMA5, carry_in=carry, backend="host"))


@pytest.mark.parametrize("n,starts", [
    (5000, [0, 1, 2, 3, 2047, 2048, 2049, 4096, 4999]),          # segments of length 1; starts on, before and after tile boundaries
    (TILE, [0, 1000, 1001, TILE - 1]),                           # single-launch path with segments
    (3 * TILE, [0, TILE, 2 * TILE]),                             # every tile its own segment
    (20000, [0, 9000]),
])
def test_segments_and_carry_in(n, starts):
    from pinn_amd import risk
    a = synthetic(n, 13) * 2.0
    a[n // 3 + 5, 14] = np.nan                                   # a NaN stays inside its segment
    got = risk.rf_series(a, MU5, SIGMA5, seg_starts=starts, backend="device")
    want = risk.rf_series(a, MU5, SIGMA5, seg_starts=starts, backend="host")
    assert np.isnan(want["C"]).any() and not np.isnan(want["C"][-1])
    compare_all("segments", got, want)
    carry = np.stack([np.linspace(10.0, 900.0, len(starts)), np.linspace(0.0, 1.0, len(starts))], axis=1)
    got = risk.rf_series(a, MU5, SIGMA5, seg_starts=starts, carry_in=carry, backend="device")
    compare_all("segments carried", got, risk.rf_series(a, MU5, SIGMA5, seg_starts=starts, carry_in=carry, backend="host"))
    # per-segment first alarm against the host search in every segment
    rs = torch.from_numpy(want["RF_smooth"]).cuda()
    first = risk._device_first(rs, 0.3, "above", seg_starts=starts).cpu().numpy()
    bounds = list(starts) + [n]
    for s, (b, e) in enumerate(zip(bounds[:-1], bounds[1:])):
        w = risk.find_first_alarm_index(want["RF_smooth"][b:e], 0.3, backend="host")
        assert first[s] == (-1 if w is None else w)


def test_gather_list_not_ascending():
    from pinn_amd import risk
    a = synthetic(30000, 17) * 2.0
    rng = np.random.default_rng(0)
    idx = rng.permutation(30000)[:7001]
    compare_all("gather", risk.rf_series(a, MU5, SIGMA5, row_index=idx, backend="device"),
                risk.rf_series(a, MU5, SIGMA5, row_index=idx, backend="host"))
    idx = np.arange(29999, -1, -1)
    d = risk.rf_series(dev(a), MU5, SIGMA5, row_index=idx, seg_starts=[0, 12345])
    h = risk.rf_series(a, MU5, SIGMA5, row_index=idx, seg_starts=[0, 12345], backend="host")
    compare_all("reversed", {k: (v.cpu().numpy() if k != "S_layers" else v) for k, v in d.items()}, h)
    # the voltage alarm on gathered rows, threshold read on the device from each segment's first row
    ad = dev(a)
    starts = torch.tensor([0, 12345], device="cuda")
    got = risk._device_first(ad[:, 8], -0.004, "below", stride=ad.stride(0), n_src=ad.shape[0], row_index=torch.from_numpy(idx.copy()).cuda(),
                             seg_starts=starts, relative=True).cpu().numpy()
    v = a[idx, 8]
    for s, (b, e) in enumerate(((0, 12345), (12345, 30000))):
        w = risk.find_first_alarm_index(v[b:e], v[b] - 0.004, mode="below", backend="host")
        assert got[s] == (-1 if w is None else w) and w is not None


def test_run_to_run_bit_identity():
    from pinn_amd import risk
    a = synthetic(300000, 19)
    a[:, 17] = (np.arange(300000) // 1000) % 3
    a[::977, 13] = np.nan
    ad = dev(a)
    m1, s1 = risk.estimate_mu_sigma_normal(ad)
    m2, s2 = risk.estimate_mu_sigma_normal(ad)
    assert torch.equal(m1, m2) and torch.equal(s1, s2)
    mh, sh = risk.estimate_mu_sigma_normal(a, backend="host")
    assert np.all(np.abs(m1.cpu().numpy() - mh) <= 1e-13 * sh) and np.all(np.abs(s1.cpu().numpy() - sh) <= 1e-12 * sh)
    a[::977, 13] = 0.0
    ad = dev(a)
    r1 = risk.rf_series(ad, MU5, SIGMA5, seg_starts=[0, 150001])
    r2 = risk.rf_series(ad, MU5, SIGMA5, seg_starts=[0, 150001])
    for k in ("S_tot", "C", "RF_inst", "RF_smooth", "carry_out"):
        assert torch.equal(r1[k], r2[k]), k
    with pytest.raises(ValueError, match="normal"):
        risk.estimate_mu_sigma_normal(ad, normal_labels=(7,))


def test_monitor_update_rows_online():
    """The online form on normalised rows, in chunks, against the host backend on five columns this test builds itself in
    float64 numpy from the model's eval-mode net_u output and _residuals columns with results.py's de-normalisation."""
    import pinn_amd
    from pinn_amd import _lib, risk, synth
    ds = synth.make_dataset(3000, (900, 900, 900), seed=4)
    x_train, y_train, x_test, y_test, sx, sy, info = ds
    torch.manual_seed(0)
    m = pinn_amd.PhysicsInformedNN(x_train, y_train, [8, 256, 256, 256, 1], sx, sy, p=0.2, logvar=True, seed=3)
    m.verbose = False
    m.dnn.eval()
    xd = m._dev_rows(x_test)
    u, _ = m.net_u(xd)
    cols = m._residuals(xd, sx, _lib.RES_ALL, u=u.reshape(-1)).cpu().numpy()
    u = u.detach().reshape(-1).cpu().numpy()
    y32 = y_test.detach().cpu().numpy().astype(np.float32).reshape(-1)
    t = (y32.astype(np.float64) - float(np.asarray(sy.min_).reshape(-1)[0])).astype(np.float32)
    y_true = (t.astype(np.float64) / float(np.asarray(sy.scale_).reshape(-1)[0])).astype(np.float32).astype(np.float64)
    scale_y = 2.0 / (float(np.asarray(sy.data_max_).reshape(-1)[0]) - float(np.asarray(sy.data_min_).reshape(-1)[0]) + 1e-12)
    min_y = -1.0 - float(np.asarray(sy.data_min_).reshape(-1)[0]) * scale_y
    y_pred = (u.astype(np.float64) - min_y) / (scale_y + 1e-12)
    five = np.stack([y_true - y_pred] + [cols[_lib.C[c]].astype(np.float64) for c in ("FV", "FT", "FH", "FO")], axis=1)
    n = five.shape[0]
    mu, sigma = np.nanmean(five[:3000], axis=0), np.nanstd(five[:3000], axis=0, ddof=1)
    want = risk.rf_series(five, mu, sigma, columns=range(5), backend="host")
    # an untrained net's residuals drive C less far than a real fault does: the monitor's two thresholds sit at 30 % and
    # 60 % of the peak of the host series, so that both alarms fire inside the run
    peak = float(np.nanmax(want["RF_smooth"]))
    thrs = (0.3 * peak, 0.6 * peak)
    firsts = [risk.find_first_alarm_index(want["RF_smooth"], thr, backend="host") for thr in thrs]
    print("host alarms:", firsts, "max C %.1f, peak RF_smooth %.4f" % (np.nanmax(want["C"]), peak))
    assert peak > 1e-3 and None not in firsts
    assert all(margin_ok(want["RF_smooth"], thr, i) for thr, i in zip(thrs, firsts)), "inputs: alarm margin below 1e-6"
    mon = risk.RiskMonitor(mu, sigma, warn_threshold=thrs[0], danger_threshold=thrs[1])
    rs, cs, res = [], [], []
    for s in range(0, n, 777):
        r, c = mon.update_rows(m, x_test[s:s + 777], y_test[s:s + 777], sx, sy, return_C=True)
        rs.append(r)
        cs.append(c)
        res.append(mon.last_columns[:, 0])
    res = torch.cat(res).cpu().numpy()
    print("res: max abs err %.3e" % np.abs(res - five[:, 0]).max())
    assert np.abs(res - five[:, 0]).max() <= 1e-12
    check_series("online C", torch.cat(cs).cpu().numpy(), want["C"], rtol=1e-11)
    check_series("online RF_smooth", torch.cat(rs).cpu().numpy(), want["RF_smooth"], atol=1e-11)
    assert [mon.first_warning, mon.first_danger] == firsts
    # and the results array's device form feeds the RF stage without a host copy
    arr = pinn_amd.create_comprehensive_results_array_v2(m, ds, mc_times=4, dropout=0.2, device_output=True)
    assert arr.is_cuda and arr.shape == (n, 22) and arr.dtype == torch.float64
    mu_d, sigma_d = risk.estimate_mu_sigma_normal(arr)
    out = risk.rf_advance_for_conditions(arr, mu_d, sigma_d, [(float(arr[3000, 0].item()), [1], None)], current_tol=1e9)
    assert out[0]["n"] == 900
