"""CPU: the host backend of pinn_amd.identify (float64 numpy, the solver statement of include/pinn_hip.h) against two referees:
scipy's MINPACK Levenberg-Marquardt for the optimum, numpy.longdouble for the normal equations.

Gates, from the issue and the arithmetic, not from what the code gives:
  optimum     |theta_k - theta_ref,k| <= 4 max(m, tol) se_k: m se_k is the first-order bound of the certificate, the 4 covers
              second-order terms and the referee's own error.  Measured worst ratio at tol = 1e-8: 1.0 (voltage), 0.98 (thermal).
  noise-free  the true theta to 1e-10 |theta|.
  normal eq.  32 * 2^-53 * sum of magnitudes (identify_cases.longdouble_normal states the count).  Measured worst ratio: 0.046.
  statistics  z-scores of 200 windows: |mean| <= 0.25, standard deviation in [0.8, 1.2], checked on the referee's answers first.
Every comparison prints its worst figure before it asserts."""
import math
import os
import sys

import numpy as np
import pytest

import identify_cases as C
from pinn_amd import identify as I

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

TOL = 1e-8
MODELS = ("voltage", "thermal")


def host_fit(table, start, length, model, **kw):
    return I.fit_windows(table, start, length, model=model, backend="numpy", **kw)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", C.SIZES)
def test_optimum_against_scipy(model, n):
    table, start, length, truths, ref = C.noisy_case(model, n)
    f = host_fit(table, start, length, model, tol=TOL)
    print("passes", f.passes.tolist())
    assert np.all(f.status == 0), f.status
    ratio = C.gate_ratio(f.theta, ref, f.m, f.se, TOL)
    print("%s n=%d: worst |dtheta| / (max(m, tol) se) = %.3g (gate 4), most passes %d" % (model, n, ratio.max(), f.passes.max()))
    assert ratio.max() <= 4.0
    if model == "thermal":
        assert np.all(f.in_reference_box)
    else:
        assert not np.any(f.no_limit)


@pytest.mark.parametrize("model", MODELS)
def test_noise_free_windows_recover_the_truth(model):
    table, start, length, truths = C.windows(1024, 8, model, 77, noise=0.0)
    f = host_fit(table, start, length, model)
    rel = np.abs(f.theta - truths) / np.abs(truths)
    print("%s noise-free: worst relative error %.3g (gate 1e-10), status %s" % (model, rel.max(), f.status.tolist()))
    assert np.all(f.status == 0) and rel.max() <= 1e-10


@pytest.mark.parametrize("model", MODELS)
def test_normal_equations_against_longdouble(model):
    worst = 0.0
    for n in (4, 257, 4096, 65536):
        rng = np.random.default_rng(n)
        table, _ = C.window(n, model, rng)
        th = C.start_theta(model) if model == "voltage" else C.CENTRE[model]
        f = host_fit(table, [0], [n], model, theta0=th, max_passes=0)
        assert f.passes[0] == 1 and f.status[0] in (0, 1)
        worst = max(worst, C.normal_ratio(f.normal[0], table, th, model))
    print("%s normal equations: worst error / bound = %.3g (gate 1)" % (model, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("model", MODELS)
def test_z_scores_are_standard(model):
    table, start, length, truths = C.windows(1024, 200, model, 4242)
    f = host_fit(table, start, length, model)
    assert np.all(f.status == 0)
    ref = np.stack([C.scipy_optimum(table[s:s + l], t, model) for s, l, t in zip(start[:200], length, f.theta)])
    for name, est in (("referee", ref), ("host", f.theta)):
        z = (est - truths) / f.se
        print("%s %s: z mean %s, std %s" % (model, name, np.round(z.mean(axis=0), 3), np.round(z.std(axis=0, ddof=1), 3)))
        assert np.all(np.abs(z.mean(axis=0)) <= 0.25) and np.all((z.std(axis=0, ddof=1) >= 0.8) & (z.std(axis=0, ddof=1) <= 1.2)), name


def check_statuses(fit_fn, model):
    """Every status reached on purpose; shared with the GPU file (fit_fn(table, start, length, **kw) -> WindowFit)."""
    table, cases, missing = C.status_cases(model)
    names = list(cases)
    start, length = [cases[k][0] for k in names], [cases[k][1] for k in names]
    f = fit_fn(table, start, length)
    got = dict(zip(names, f.status.tolist()))
    print(model, got, "n_used", f.n_used.tolist())
    assert got == {k: cases[k][2] for k in names}
    assert f.n_used[names.index("missing_rows")] == 300 - missing and f.n_used[names.index("three_rows")] == 3
    k3, k5 = names.index("three_rows"), names.index("constant_current")
    assert np.all(np.isnan(f.raw[k3, :12])) and np.all(np.isfinite(f.theta[k5])) and np.all(np.isnan(f.cov[k5])) and np.isnan(f.m[k5])
    # an out-of-range gather index is one more missing row; the identity gather list changes nothing
    ident = np.arange(len(table))
    g = fit_fn(table, start, length, row_index=ident)
    assert np.array_equal(g.raw, f.raw, equal_nan=True) and np.array_equal(g.normal, f.normal, equal_nan=True)
    holes = ident.copy()
    holes[[10, 500]] = (-1, len(table))
    h = fit_fn(table, [0], [1000], row_index=holes)
    assert h.status[0] == 0 and h.n_used[0] == 998
    # max_passes = 2 on a noisy window
    one = fit_fn(table, [0], [1000], max_passes=2)
    assert one.status[0] == 1 and one.passes[0] == 2 and np.all(np.isfinite(one.cov[0]))
    # a window's result does not depend on the other windows of the call
    alone = fit_fn(table, [cases["converged"][0]], [cases["converged"][1]])
    assert np.array_equal(alone.raw[0], f.raw[names.index("converged")]) and np.array_equal(alone.normal[0], f.normal[names.index("converged")])
    # bad windows
    bad = fit_fn(table, [-1, 0, len(table) - 10, 0], [10, -1, 11, I.MAX_WINDOW + 1])
    assert bad.status.tolist() == [6, 6, 6, 6] and np.all(np.isnan(bad.raw[:, :12]))
    if model == "voltage":
        imax = table[:1000, 0].max()
        th = C.start_theta(model)
        th[2] = 1.0 / imax
        out = fit_fn(table, [0], [1000], theta0=th)
        assert out.status[0] == 4 and np.all(np.isnan(out.raw[0, :12])) and out.n_used[0] == 1000
        th[2] = np.nextafter(1.0 / imax, 0.0) * (1 - 1e-12)
        assert fit_fn(table, [0], [1000], theta0=th).status[0] != 4
    nanstart = fit_fn(table, [0], [1000], theta0=[np.nan, 0.0, 0.1])
    assert nanstart.status[0] == 4
    # theta0 per window
    per = fit_fn(table, [0, 0], [1000, 1000], theta0=np.stack([C.start_theta(model), f.theta[names.index("converged")]]))
    assert per.status.tolist() == [0, 0] and per.passes[1] < per.passes[0]
    assert np.array_equal(per.raw[0], f.raw[names.index("converged")])


@pytest.mark.parametrize("model", MODELS)
def test_every_status_is_reached(model):
    check_statuses(lambda t, s, l, **kw: host_fit(t, s, l, model, **kw), model)


def test_drift_on_hand_computed_cases():
    def wf(theta, cov):
        raw = np.zeros((1, 16))
        raw[0, 0:3] = theta
        for k, (p, q) in enumerate(I._TRI):
            raw[0, 3 + k] = cov[p][q]
        return I.WindowFit(raw, np.zeros((1, 12)), "voltage", "host")
    # diagonal covariances: the Wald statistic is the sum of the squared z
    a, b = wf([1.0, 2.0, 3.0], np.diag([0.09, 0.16, 1.0])), wf([0.0, 0.0, 0.0], np.diag([0.16, 0.09, 3.0]))
    d = I.drift(a, b)
    assert np.allclose(d["z"][0], [1.0 / 0.5, 2.0 / 0.5, 3.0 / 2.0], rtol=1e-15)
    assert math.isclose(d["wald"][0], 4.0 + 16.0 + 2.25, rel_tol=1e-14)
    # a correlated pair: S = [[2, 1, 0], [1, 2, 0], [0, 0, 1]], delta = (1, 1, 2): S^-1 delta = (1/3, 1/3, 2), Wald = 2/3 + 4
    a = wf([1.0, 1.0, 2.0], [[1.0, 0.5, 0.0], [0.5, 1.0, 0.0], [0.0, 0.0, 0.5]])
    b = wf([0.0, 0.0, 0.0], [[1.0, 0.5, 0.0], [0.5, 1.0, 0.0], [0.0, 0.0, 0.5]])
    d = I.drift(a, b)
    assert math.isclose(d["wald"][0], 2.0 / 3.0 + 4.0, rel_tol=1e-14)
    assert math.isclose(d["p"][0], I.chi2_sf3(2.0 / 3.0 + 4.0), rel_tol=0)


def test_chi2_tail_against_scipy():
    from scipy.stats import chi2
    xs = np.concatenate([[0.0, 1e-12, 1e-6], np.logspace(-3, 2.8, 200)])
    rel = max(abs(I.chi2_sf3(x) - chi2.sf(x, 3)) / chi2.sf(x, 3) for x in xs)
    print("chi-square(3) tail: worst relative error %.3g (gate 1e-13)" % rel)
    assert rel <= 1e-13


def test_params_and_box():
    raw = np.zeros((3, 16))
    raw[:, 0:3] = [[0.2, math.log(2.4e-6), 0.4], [0.2, math.log(2.4e-6), -0.1], [2.0, math.log(2.4e-6), 0.0]]
    raw[:, 3], raw[:, 5], raw[:, 8] = 1e-4, 4e-4, 9e-4
    f = I.WindowFit(raw, np.zeros((3, 12)), "voltage", "host")
    p = f.params
    assert math.isclose(p["lambda_2"][0][0], 2.4e-6, rel_tol=1e-14) and math.isclose(p["lambda_2"][1][0], 2.4e-6 * 0.02, rel_tol=1e-12)
    assert math.isclose(p["lambda_3"][0][0], 2.5) and math.isclose(p["lambda_3"][1][0], 0.03 / 0.16, rel_tol=1e-12)
    assert f.no_limit.tolist() == [False, True, True] and np.isinf(p["lambda_3"][0][1]) and np.isinf(p["lambda_3"][0][2])
    assert f.in_reference_box.tolist() == [[True, True, True], [True, True, False], [False, True, False]]


def test_sliding_windows_respect_segments():
    s, l = I.sliding_windows(100, 30, 20)
    assert s.tolist() == [0, 20, 40, 60] and l.tolist() == [30] * 4
    s, l = I.sliding_windows(100, 30, 20, segments=[0, 45, 70])
    assert s.tolist() == [0, 70] and np.all(s + l <= 100)
    assert len(I.sliding_windows(10, 30, 5)[0]) == 0
    with pytest.raises(ValueError):
        I.sliding_windows(100, 30, 20, segments=[5, 50])


def check_tracker(backend, to_backend=lambda a: a):
    """ParameterTracker with chunks of 1, 7 and `length` rows equals fit_windows on the trailing window started where the tracker
    started; shared with the GPU file."""
    rng = np.random.default_rng(3)
    table, _ = C.window(400, "voltage", rng)
    base = I.fit_baseline(to_backend(table[:200]), backend=backend)
    L = 64
    for chunk in (1, 7, L):
        tr = I.ParameterTracker(base, L, backend=backend)
        for a in range(0, 200 if chunk > 1 else 90, chunk):
            u = tr.update(to_backend(table[a:a + chunk]))
            end = min(a + chunk, len(table))
            lo = max(0, end - L)
            want = I.fit_windows(to_backend(table), [lo], [end - lo], theta0=tr.theta_start, backend=backend)
            assert u["status"] == want.status[0] and u["n_used"] == end - lo
            assert np.array_equal(tr.last.raw, want.raw, equal_nan=True), (chunk, a)
            if u["status"] == 0:
                assert u["blamed"] in I.THETA_NAMES["voltage"]


def test_tracker_equals_fit_windows_on_the_trailing_window():
    check_tracker("numpy")


def recording_outcomes(backend, to_backend=lambda a: a):
    """The three outcomes of the example's recording of 6000 rows; shared with the GPU file."""
    import parameter_tracking as P
    rec = P.synthetic_recording(6000)
    base, ups = P.track(rec, 1024, 100, backend, to_backend(rec["table"]))
    by_end = dict(ups)
    normal = [u for end, u in ups if 1024 <= end <= 2000]
    zmax = max(float(np.max(np.abs(u["z"]))) for u in normal)
    print("normal rows: max |z| %.2f; r segment: %s z %s; c segment: %s z %s" % (
        zmax, by_end[4000]["blamed"], np.round(by_end[4000]["z"], 2), by_end[6000]["blamed"], np.round(by_end[6000]["z"], 2)))
    assert zmax < 4.0
    assert by_end[4000]["blamed"] == "r" and abs(by_end[4000]["z"][0]) >= 4.0
    assert by_end[6000]["blamed"] == "c" and abs(by_end[6000]["z"][2]) >= 4.0
    return rec, base


def test_recording_outcomes_on_the_host_and_by_the_referee_alone():
    rec, base = recording_outcomes("numpy")
    T = rec["table"]
    ref0 = C.scipy_optimum(T[:2000], base.theta[0], "voltage")
    for end, k in ((2000, None), (4000, 0), (6000, 2)):
        x = C.scipy_optimum(T[end - 1024:end], base.theta[0], "voltage")
        f = host_fit(T, [end - 1024], [1024], "voltage")
        z = (x - ref0) / np.sqrt(f.se[0] ** 2 + base.se[0] ** 2)
        print("referee, window ending at %d: z %s" % (end, np.round(z, 2)))
        assert (np.max(np.abs(z)) < 4.0) if k is None else (int(np.argmax(np.abs(z))) == k and abs(z[k]) >= 4.0)


def test_physical_row_tables():
    rng = np.random.default_rng(9)
    X = C.physical_rows(50, rng)
    t = I.voltage_table(None, X, y=np.full(50, 3.5))
    assert t.shape == (50, 4) and np.all(t[:, 3] == 0.7) and np.all(t[:, 0] == X[:, 0] / 270.0 + 1e-5)
    assert np.allclose(t[:, 1], 8.314 * (X[:, 5] + 273.15) / 96485.0, rtol=1e-15)
    th = I.thermal_table(None, X)
    assert np.array_equal(th[:, 2], X[:, 2]) and np.array_equal(th[:, 3], X[:, 5])
    with pytest.raises(ValueError):
        I.voltage_table(None, X)


def test_no_scipy_or_sklearn_in_the_package():
    src = open(I.__file__).read()
    assert "import scipy" not in src and "from scipy" not in src and "sklearn" not in src
