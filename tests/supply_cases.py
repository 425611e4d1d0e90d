"""Case builders and referees shared by the tests of pinn_amd.supply (host, ABI and GPU files).

Windows are drawn like the prototype's of the issue: currents x ~ U(20, 300) A, continuous or quantised to 10 A (about 28
distinct values: ties are the normal case), y = a + b min(x, c) / 100 plus Gaussian noise.

Referee: a brute force in numpy that is independent of the package: every distinct current as c (numpy.linalg.lstsq of y on
[1, min(x, c) / 100]) and the free split of every gap (lstsq of y on [1_left, x_left / 100, 1_right], admissible when b != 0
and the implied c lies inside the gap), O(m^2).  For a returned theta the tests compute the direct SSE themselves.

Gate G, on the objective: SSE(theta returned) <= SSE_brute (1 + 1e-9) + 1e-12 sum (y - mean y)^2.  The second term is the
worst-case cancellation of m <= 4096 centred float64 terms (m eps = 4.5e-13, doubled); the first term's margin sits over the
2.7e-12 the moment form measured in the prototype.  Near-ties between candidates cannot make it flaky.
"""
import numpy as np

TRUTH = (1.5, 0.8, 150.0)
G_REL, G_ABS = 1e-9, 1e-12


def draw(rng, m, quantised, noise, theta=TRUTH, lo=20.0, hi=300.0):
    """One window [m, 2] = (x, y) of the law at theta."""
    x = rng.uniform(lo, hi, m)
    if quantised:
        x = np.round(x / 10.0) * 10.0
    y = theta[0] + theta[1] * (np.minimum(x, theta[2]) / 100.0) + rng.normal(0.0, noise, m)
    return np.column_stack([x, y])


def direct_sse(rows, theta):
    """Sum of squared residuals of the used rows at theta = (a, b, c), c = inf the line, c = NaN with b = 0 the constant."""
    r = rows[np.isfinite(rows).all(axis=1)]
    u = r[:, 0] if np.isnan(theta[2]) else np.minimum(r[:, 0], theta[2])
    return float(np.sum((r[:, 1] - (theta[0] + theta[1] * (u / 100.0))) ** 2))


def brute_candidates(rows):
    """The SSE of every candidate of the brute force, ascending."""
    r = rows[np.isfinite(rows).all(axis=1)]
    x, y = r[:, 0], r[:, 1]
    vals = np.unique(x)
    one = np.ones(len(x))
    out = []
    for c in vals:
        A = np.column_stack([one, np.minimum(x, c) / 100.0])
        coef = np.linalg.lstsq(A, y, rcond=None)[0]
        out.append(float(np.sum((y - A @ coef) ** 2)))
    for j in range(1, len(vals) - 1):                            # the gap (vals[j], vals[j + 1]): at least two currents on the left
        left = x <= vals[j]
        A = np.column_stack([left.astype(float), np.where(left, x / 100.0, 0.0), (~left).astype(float)])
        a, b, d = np.linalg.lstsq(A, y, rcond=None)[0]
        if b != 0.0 and vals[j] <= 100.0 * (d - a) / b <= vals[j + 1]:
            out.append(float(np.sum((y - A @ np.array([a, b, d])) ** 2)))
    return np.sort(np.array(out))


def brute_sse(rows):
    return float(brute_candidates(rows)[0])


def syy(rows):
    r = rows[np.isfinite(rows).all(axis=1)]
    return float(np.sum((r[:, 1] - np.mean(r[:, 1])) ** 2))


def gate_G(rows, theta, sse_ref):
    """(direct SSE at theta, the bound of gate G against the referee's SSE)."""
    return direct_sse(rows, theta), sse_ref * (1.0 + G_REL) + G_ABS * syy(rows)


def grid_sse(rows, n_grid=64):
    """The smallest SSE over n_grid values of c across the window's currents (lstsq per value): the referee of long windows."""
    r = rows[np.isfinite(rows).all(axis=1)]
    x, y = r[:, 0], r[:, 1]
    one, best = np.ones(len(x)), np.inf
    for c in np.linspace(x.min(), x.max(), n_grid):
        A = np.column_stack([one, np.minimum(x, c) / 100.0])
        coef = np.linalg.lstsq(A, y, rcond=None)[0]
        best = min(best, float(np.sum((y - A @ coef) ** 2)))
    return best


def prototype_windows(count=300, seed=2024):
    """The windows of gate G: m in 5..200, continuous and quantised currents, noise 1e-3 / 0.05 / 0.3, c drawn from 0..350 A
    so that line-only and plateau-only windows occur."""
    rng = np.random.default_rng(seed)
    out = []
    for w in range(count):
        m = int(rng.integers(5, 201))
        theta = (rng.uniform(1.0, 2.5), rng.uniform(0.2, 1.5), rng.uniform(0.0, 350.0))
        out.append(draw(rng, m, w % 2 == 1, (1e-3, 0.05, 0.3)[(w // 2) % 3], theta))
    return out


_separated = {}


def separated(m, quantised):
    """A well-separated window of m rows, built once: noise 0.02, b = 0.8, the breakpoint inside the middle half of the
    currents and the runner-up split's SSE at least 1e-6 relative above the best (the brute force checks it here; the next
    seed is drawn until it holds).  Returns (rows, theta true, brute SSE)."""
    key = (m, quantised)
    if key not in _separated:
        for attempt in range(20):
            rng = np.random.default_rng(1000 * m + 10 * attempt + int(quantised))
            c = float(rng.uniform(90.0, 230.0))                  # the middle half of U(20, 300)
            rows = draw(rng, m, quantised, 0.02, (1.5, 0.8, c))
            cand = brute_candidates(rows)
            if len(cand) > 1 and cand[1] >= cand[0] * (1.0 + 1e-6) and cand[0] > 0.0:
                _separated[key] = (rows, (1.5, 0.8, c), float(cand[0]))
                break
        else:
            raise AssertionError("no well-separated window of %d rows in 20 draws" % m)
    return _separated[key]


def stack(windows):
    """Windows of any lengths stacked into one table: (table, start, length)."""
    length = np.array([len(w) for w in windows], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.int64)
    return np.vstack(windows), start, length


def status_cases(seed=5):
    """A table and windows that reach a kind or status each on purpose: (table, {name: (start, length)})."""
    rng = np.random.default_rng(seed)
    normal = draw(rng, 300, True, 0.02)                          # rows 0..299
    one_current = draw(rng, 50, True, 0.02)                      # 300..349: all x equal
    one_current[:, 0] = 120.0
    # 350..549: every row below the threshold of 150 A.  Noise alone lets a late knot beat the line in most draws (one more
    # parameter), so the rows bend upwards a little: every hinge with b > 0 is concave and then fits worse than the line
    below = draw(rng, 200, False, 0.02, hi=140.0)
    below[:, 1] += 0.2 * (below[:, 0] / 100.0) ** 2
    plateau = draw(rng, 100, True, 0.0, (1.5, 0.8, 0.0))         # 550..649: the threshold below every current, no noise: y = 1.5 exactly
    missing = draw(rng, 300, True, 0.02)                         # 650..949: rows with missing entries
    missing[5, 0] = np.nan; missing[17, 1] = np.inf; missing[40, 0] = -np.inf; missing[41, 1] = np.nan
    table = np.vstack([normal, one_current, below, plateau, missing])
    cases = {"normal": (0, 300), "one_current": (300, 50), "below": (350, 200), "plateau_only": (550, 100), "missing": (650, 300),
             "three_rows": (0, 3), "negative_start": (-1, 10), "negative_length": (0, -1), "beyond_the_end": (900, 51),
             "too_long": (0, 4097)}
    return table, cases


def check_kinds_and_statuses(fit):
    """Host test 2 of the issue, for either backend: fit(table, start, length, **kw) -> BreakpointFit."""
    table, cases = status_cases()
    names = list(cases)
    f = fit(table, [cases[n][0] for n in names], [cases[n][1] for n in names])
    at = {n: i for i, n in enumerate(names)}
    i = at["normal"]
    assert f.status[i] == 0 and f.kind[i] in (0, 1) and f.n_used[i] == 300 and np.all(np.isfinite(f.cov[i]))
    i = at["one_current"]
    assert f.status[i] == 7 and f.n_used[i] == 50 and f.distinct[i] == 1 and f.theta[i, 1] == 0.0 and np.isnan(f.theta[i, 2])
    assert abs(f.theta[i, 0] - table[300:350, 1].mean()) <= 1e-12 and np.all(np.isnan(f.cov[i]))
    i = at["below"]
    rows = table[350:550]
    assert f.status[i] == 0 and f.kind[i] == 2 and f.theta[i, 2] == np.inf and f.k[i] == 200
    A = np.column_stack([np.ones(200), rows[:, 0] / 100.0])
    coef, res = np.linalg.lstsq(A, rows[:, 1], rcond=None)[:2]
    ols = (float(res[0]) / 198.0) * np.linalg.inv(A.T @ A)
    assert np.allclose(f.theta[i, :2], coef, rtol=1e-9, atol=0) and np.allclose(f.cov[i, :2, :2], ols, rtol=1e-7, atol=0)
    assert np.all(np.isnan(f.cov[i, 2])) and np.all(np.isnan(f.cov[i, :, 2]))
    i = at["plateau_only"]                                       # the constant model wins: one distinct current on the left of its knot
    assert f.status[i] == 5 and f.kind[i] == 3 and np.all(np.isnan(f.cov[i]))
    assert f.theta[i, 0] == 1.5 and f.theta[i, 1] == 0.0 and f.theta[i, 2] == table[550:650, 0].min() and f.sse[i] == 0.0
    i = at["missing"]
    assert f.status[i] == 0 and f.n_used[i] == 296
    sse, bound = gate_G(table[650:950], f.theta[i], brute_sse(table[650:950]))
    assert sse <= bound
    assert f.status[at["three_rows"]] == 3 and f.n_used[at["three_rows"]] == 3 and np.all(np.isnan(f.theta[at["three_rows"]]))
    for n in ("negative_start", "negative_length", "beyond_the_end", "too_long"):
        assert f.status[at[n]] == 6 and np.all(np.isnan(f.theta[at[n]])), n
    # gather indices outside the table read nothing: the same rows through a list with strays are the same fit
    ridx = np.concatenate([np.arange(0, 150), [-1, len(table), 10 ** 12], np.arange(150, 300)])
    g = fit(table, [0], [303], row_index=ridx)
    assert g.n_used[0] == 300 and g.raw[0].tobytes() == f.raw[at["normal"]].tobytes()
    # a window of more than 4096 positions that do exist is answered by status 6 all the same
    long = fit(table, [0, 0], [4097, 4096], row_index=np.arange(5000) % 300)
    assert long.status[0] == 6 and long.status[1] == 0 and long.n_used[1] == 4096
    return table, names, f


def check_tracker(backend, to_backend):
    """SupplyTracker.update equals fit_breakpoints on the same trailing rows, bit for bit: 20 chunks of 64 rows, a ring of 512."""
    from pinn_amd import supply as S
    rng = np.random.default_rng(9)
    table = draw(rng, 20 * 64, True, 0.05)
    base = S.fit_breakpoint_baseline(to_backend(table[:512]), backend=backend)
    tracker = S.SupplyTracker(base, 512, backend=backend)
    for c in range(20):
        end = 64 * (c + 1)
        u = tracker.update(to_backend(table[end - 64:end]))
        lo = max(0, end - 512)
        f = S.fit_breakpoints(to_backend(table[lo:end]), [0], [end - lo], backend=backend)
        assert tracker.last.raw[0].tobytes() == f.raw[0].tobytes(), c
        assert u["status"] == f.status[0] and u["n_used"] == end - lo and np.array_equal(u["theta"], f.theta[0])


def check_example(backend, to_backend):
    """The example's three segments: nothing is blamed on the normal one, the moved parameter with |z| >= 4 on the others."""
    import supply_tracking as E
    rec = E.synthetic_recording(6000)
    base, updates = E.track(rec, 512, 64, backend, to_backend(rec["table"]))
    last = E.last_windows(rec, updates, 512)
    assert all(l is not None for l in last)
    print("baseline theta %s se %s" % (base.theta[0], base.se[0]))
    for s, (end, u) in enumerate(last):
        print("segment %d: blamed %s, z %s, kind %d" % (s, u["blamed"], np.round(u["z"], 2), u["kind"]))
    assert np.nanmax(np.abs(last[0][1]["z"])) < 4.0
    for s in (1, 2):
        u = last[s][1]
        assert u["blamed"] == E.MOVED[s] and abs(u["z"][("l1", "l2", "l3").index(E.MOVED[s])]) >= 4.0, (s, u)
