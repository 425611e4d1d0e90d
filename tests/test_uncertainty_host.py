"""CPU: the float64 numpy backend of pinn_amd.uncertainty (the referee of the device tests) is held to brute force: counts by
explicit loops, quantiles as sorted(scores)[k - 1] with the stated k, crps against scipy.integrate.quad of the integral
of (F - 1{y <= x})^2, the monitor against a sequential restatement; and to the statistics it claims, with fixed seeds."""
import math
from statistics import NormalDist

import numpy as np
import pytest

import uncertainty_cases as C
from pinn_amd import risk, uncertainty as U

GROUPS = dict(normal=[0], **{k: list(v) for k, v in risk.FAULT_RANGE_MAP.items()})


def brute_rows(A, var_model=(1.0, 1.0, 0.0), groups=None, row_index=None):
    """(group, r, s, v, z) per valid position, None otherwise: a row at a time, in Python floats."""
    a, b, c = var_model
    label_group = {}
    if groups is not None:
        for g, labs in enumerate(groups.values()):
            for lab in labs:
                label_group[int(lab)] = g
    n_labels = max(label_group) + 1 if label_group else 0
    out = []
    for j in (range(A.shape[0]) if row_index is None else row_index):
        if not 0 <= j < A.shape[0]:
            out.append(None)
            continue
        row = A[j]
        g = 0
        if groups is not None:
            lab = float(row[C.LABEL])
            if not (lab >= 0.0 and lab < n_labels):
                out.append(None)
                continue
            g = label_group.get(int(lab), -1)
        yt, yp, ale, epi = (float(row[k]) for k in (C.Y_TRUE, C.Y_PRED, C.ALE, C.EPI))
        v = (a * ale) * ale + (b * epi) * epi + c
        if g < 0 or not (math.isfinite(yt) and math.isfinite(yp) and math.isfinite(v) and v > 0.0):
            out.append(None)
            continue
        s = math.sqrt(v)
        r = yt - yp
        out.append((g, r, s, v, r / s))
    return out


@pytest.mark.parametrize("grouped", [False, True], ids=["one-group", "fault-groups"])
def test_counts_and_sums_against_explicit_loops(grouped):
    A = C.spoil(C.results_array(700, 1), 2)
    groups = GROUPS if grouped else None
    ridx = None if not grouped else np.array([5, 5, -1, 700, 699] + list(range(0, 700, 3)))
    levels, bins = (0.5, 0.9, 0.99), 7
    rep, per = U.score_uncertainty(A, levels=levels, bins=bins, groups=groups, row_index=ridx, backend="host", per_row=True)
    rows = brute_rows(A, groups=groups, row_index=None if ridx is None else ridx.tolist())
    nd = NormalDist()
    zl = [nd.inv_cdf(0.5 + 0.5 * v) for v in levels]
    ze = [nd.inv_cdf(i / bins) for i in range(1, bins)]
    names = list(groups) if grouped else ["all"]
    assert list(rep) == names
    assert rep[names[0]].n_skipped == sum(1 for r in rows if r is None) > 0
    for g, name in enumerate(names):
        mine = [r for r in rows if r is not None and r[0] == g]
        R = rep[name]
        assert R.n == len(mine) > 0
        hits = [sum(1 for r in mine if abs(r[4]) <= z) for z in zl]
        pit = [0] * bins
        for r in mine:
            pit[sum(1 for e in ze if e <= r[4])] += 1
        assert R.hits.tolist() == hits and R.pit.tolist() == pit and sum(pit) == R.n
        assert R.sums["1"] == R.n
        for key, k, f in (("r", 1, lambda x: x), ("s", 2, lambda x: x), ("s2", 3, lambda x: x), ("z", 4, lambda x: x),
                          ("z2", 4, lambda x: x * x), ("r2", 1, lambda x: x * x)):
            assert R.sums[key] == math.fsum(f(r[k]) for r in mine), key
        assert R.coverage.tolist() == [h / R.n for h in hits]
        assert R.scale == math.sqrt(R.sums["z2"] / R.n) and R.rmse == math.sqrt(R.sums["r2"] / R.n)
        assert R.miscalibration == pytest.approx(np.mean([abs(h / R.n - lv) for h, lv in zip(hits, levels)]), rel=1e-14)
        assert R.pit_chi2 == pytest.approx(sum((p - R.n / bins) ** 2 for p in pit) / (R.n / bins), rel=1e-13)
    # per-row z: the same bits as the row-at-a-time floats; NaN exactly on the rows that are not valid
    z = np.array([np.nan if r is None else r[4] for r in rows])
    assert per["z"].tobytes() == z.tobytes()
    assert np.array_equal(np.isnan(per["nll"]), np.isnan(z)) and np.array_equal(np.isnan(per["crps"]), np.isnan(z))


def test_nll_and_crps_terms_against_quadrature_and_mpmath():
    from scipy import integrate, stats
    A = C.results_array(40, 3)
    A[:6, C.Y_TRUE] = A[:6, C.Y_PRED] + np.array([0.0, 1e-9, -7.0, 7.0, 0.3, -0.3]) * np.sqrt(A[:6, C.ALE] ** 2 + A[:6, C.EPI] ** 2)
    rep, per = U.score_uncertainty(A, backend="host", per_row=True)
    rows = brute_rows(A)
    for j in range(0, 40, 3):
        _, r, s, v, z = rows[j]
        y, mu = A[j, C.Y_TRUE], A[j, C.Y_PRED]
        F = lambda x: stats.norm.cdf(x, mu, s)
        left = integrate.quad(lambda x: F(x) ** 2, mu - 40 * s, y, epsabs=1e-13, epsrel=1e-13, limit=200)[0]
        right = integrate.quad(lambda x: (F(x) - 1.0) ** 2, y, mu + 40 * s, epsabs=1e-13, epsrel=1e-13, limit=200)[0]
        assert per["crps"][j] == pytest.approx(left + right, rel=1e-9, abs=1e-11), j
        assert per["nll"][j] == pytest.approx(-stats.norm.logpdf(y, mu, s), rel=1e-13), j
        assert per["pit"][j] == pytest.approx(stats.norm.cdf(z), rel=1e-13), j
    z, v, s = per["z"], np.array([r[3] for r in rows]), np.array([r[2] for r in rows])
    phi, nll, crps = C.mp_terms(z, v, s)
    # Phi: the argument -z / sqrt 2 carries up to 2 roundings (the constant, the product), erfc's condition number at t > 0 is
    # at most 2 t^2 + 1 = z^2 + 1, and libm's erfc and the halving add at most 2 more; nll and crps are sums of a few well
    # conditioned terms of their own size on these rows (v >= 1.28)
    assert (C.mp_ulp_distance(per["pit"], phi) <= 2.0 * (z * z + 1.0) + 2.0).all()
    assert C.mp_ulp_distance(per["nll"], nll).max() <= 4 and C.mp_ulp_distance(per["crps"], crps).max() <= 8
    assert rep["all"].sums["nll"] == math.fsum(per["nll"].tolist()) and rep["all"].sums["crps"] == math.fsum(per["crps"].tolist())


@pytest.mark.parametrize("kind", ["abs_z", "z", "column"])
@pytest.mark.parametrize("conformal", [True, False])
def test_quantiles_are_sorted_scores_at_the_stated_rank(kind, conformal):
    A = C.spoil(C.results_array(500, 4), 5)
    A[100:140, C.Y_TRUE] = A[100:140, C.Y_PRED]                   # a run of ties at z = 0
    A[140:150, C.Y_TRUE] = -0.0
    A[140:150, C.Y_PRED] = 0.0                                     # z = -0: the same key as +0
    A[30, 3], A[31, 3], A[32, 3] = np.inf, -np.inf, np.nan          # not valid as a column score
    groups = dict(GROUPS, nobody=[13], spoiled=[14])
    A[:5, C.LABEL] = 14
    A[:5, C.ALE] = np.nan                                          # a group whose rows are all invalid
    levels = (0.001, 0.2, 0.5, 0.9, 0.999, 1.0)
    column = 3 if kind == "column" else None
    Q = U.conformal_quantiles(A, levels=levels, kind=kind, conformal=conformal, groups=groups, column=column, backend="host")
    rows = brute_rows(A, groups=groups)
    skipped = 0
    scores = [[] for _ in groups]
    for j, r in enumerate(rows):
        if kind == "column":
            lab = A[j, C.LABEL]
            g = -1
            if lab >= 0 and lab < 15:
                g = [i for i, labs in enumerate(groups.values()) if int(lab) in labs][0]
            if g >= 0 and math.isfinite(A[j, 3]):
                scores[g].append(float(A[j, 3]))
            else:
                skipped += 1
        elif r is None:
            skipped += 1
        else:
            scores[r[0]].append(abs(r[4]) if kind == "abs_z" else r[4] + 0.0)
    assert Q.n_skipped == skipped and Q.n.tolist() == [len(s) for s in scores]
    assert Q.n[list(groups).index("nobody")] == 0 and (kind == "column" or Q.n[list(groups).index("spoiled")] == 0)
    for g in range(len(groups)):
        for i, lv in enumerate(levels):
            q, k = C.brute_quantile(scores[g], lv, conformal)
            assert Q.rank[g, i] == k
            assert np.array([Q.q[g, i]]).tobytes() == np.array([q]).tobytes(), (g, lv)
    if conformal:
        assert np.isinf(Q.q[0, -1]) and Q.rank[0, -1] == Q.n[0] + 1     # level 1: beyond the last score
    assert np.isnan(Q["nobody"]).all() and (Q.rank[list(groups).index("nobody")] == 0).all()


def test_key_map_round_trip_orders_like_floats():
    rng = np.random.default_rng(6)
    xs = np.concatenate([rng.normal(size=200), [0.0, -0.0, 5e-324, -5e-324, np.inf, -np.inf, 1e308, -1e308], C.bit_split_values(20, 50, rng)])
    keys = [C.double_to_key(x) for x in xs]
    order = np.argsort(xs, kind="stable")
    assert all(keys[a] <= keys[b] for a, b in zip(order, order[1:]))
    assert C.double_to_key(0.0) == C.double_to_key(-0.0)
    for x in xs:
        assert C.key_to_double(C.double_to_key(x)) == x
    for bit in (0, 13, 51, 52, 62, 63):
        v = C.bit_split_values(bit, 40, rng)
        k = [C.double_to_key(x) for x in v]
        assert len({x >> (bit + 1) for x in k}) == 1 and len({(x >> bit) & 1 for x in k}) == 2


def test_coverage_of_a_true_law_lies_inside_three_binomial_sd():
    A = C.results_array(20000, 0)
    R = U.score_uncertainty(A, backend="host")["all"]
    for lv, cov in zip(R.levels, R.coverage):
        assert abs(cov - lv) <= 3.0 * math.sqrt(lv * (1.0 - lv) / R.n), (lv, cov)
    assert abs(R.scale - 1.0) < 0.02 and abs(R.z_mean) < 0.03 and R.miscalibration < 0.01
    assert R.pit_chi2 < 43.8                                      # chi-square, 19 degrees of freedom, 0.999 point


@pytest.mark.parametrize("understate", [1.0, 2.0])
def test_split_conformal_covers_fresh_rows(understate):
    level = 0.9
    cal, fresh = C.results_array(2000, 0, understate=understate), C.results_array(20000, 1, understate=understate)
    Q = U.conformal_quantiles(cal, levels=(level,), backend="host")
    lo, hi = U.conformal_band(fresh, Q.q[0, 0], backend="host")
    cov = float(np.mean((fresh[:, C.Y_TRUE] >= lo) & (fresh[:, C.Y_TRUE] <= hi)))
    assert cov >= level - 3.0 * math.sqrt(level * (1.0 - level) / 20000), cov
    R = U.score_uncertainty(cal, backend="host")["all"]
    assert abs(R.scale - understate) < 0.06 * understate
    if understate == 2.0:                                          # the raw band is far too narrow, and the report says so
        assert R.coverage[2] < 0.65 and Q.q[0, 0] > 2.9


def sequential_monitor(chunks, W, level, gamma, amin, amax, q0=math.inf, learn=None):
    """The monitor's four steps, a score at a time, with a list as the ring."""
    ring, pos, alpha, q = [], 0, 1.0 - level, q0
    out = []
    for ci, A in enumerate(chunks):
        for c0 in range(0, len(A), 2048):
            rows = brute_rows(A[c0:c0 + 2048])
            nv = nm = 0
            los, flags, new = [], [], []
            for j, r in enumerate(rows):
                if r is None:
                    los.append((math.nan, math.nan))
                    flags.append(-1)
                    continue
                yp = float(A[c0 + j, C.Y_PRED])
                los.append((yp - q * r[2], yp + q * r[2]))
                miss = 0 if abs(r[4]) <= q else 1
                flags.append(miss)
                nv += 1
                nm += miss
                new.append(abs(r[4]))
            if learn is None or learn[ci]:
                for sc in new:
                    if len(ring) < W:
                        ring.append(sc)
                    else:
                        ring[pos] = sc
                    pos = (pos + 1) % W
                if nv:
                    alpha = min(max(alpha + gamma * ((1.0 - level) - nm / nv), amin), amax)
                m = len(ring)
                k = max(1, math.ceil((m + 1) * (1.0 - alpha)))
                q = math.inf if k > m else sorted(ring)[k - 1]
            out.append((los, flags, q, alpha, list(ring), pos))
    return out


@pytest.mark.parametrize("gamma", [0.0, 0.5])
def test_monitor_against_a_sequential_restatement(gamma):
    A = C.spoil(C.results_array(300, 7, understate=1.5), 8, share=0.1)
    A[100:130, C.Y_TRUE] += 1000.0                                  # a chunk in which every row misses: alpha falls to its lower clip
    A[200:300, C.ALE] *= 10.0 ** (1 + np.arange(100) // 10)         # every chunk's scores below the ring's: no misses, alpha climbs to its upper clip
    A[40:44] = A[39]                                                # ties in the ring
    A[60:67, C.Y_TRUE] = np.nan                                     # a chunk with no valid row
    cuts = [0, 1, 8, 60, 67, 100, 130, 150] + list(range(200, 301, 10))
    chunks = [A[a:b] for a, b in zip(cuts, cuts[1:])]
    learn = [True, True, True, True, False] + [True] * (len(chunks) - 5)
    W, level, amin, amax = 16, 0.9, 0.02, 0.3
    mon = U.UncertaintyMonitor(level=level, window=W, gamma=gamma, alpha_min=amin, alpha_max=amax, backend="host")
    ref = sequential_monitor(chunks, W, level, gamma, amin, amax, learn=learn)
    alphas = []
    for ch, lr, (los, flags, q, alpha, ring, pos) in zip(chunks, learn, ref):
        before = mon.state_words()
        up = mon.update(ch, learn=lr)
        assert up.lo.tobytes() == np.array([l for l, _ in los]).tobytes() and up.hi.tobytes() == np.array([h for _, h in los]).tobytes()
        assert up.miss.tolist() == flags
        assert mon.q == q and mon.alpha == alpha
        st = mon.state_words()
        if not lr:
            assert st.tobytes() == before.tobytes()
        assert st.view(np.int64)[U.ST_FILL] == len(ring)
        assert st.view(np.float64)[U.STATE_HEADER:U.STATE_HEADER + len(ring)].tolist() == ring
        alphas.append(alpha)
    if gamma > 0:
        assert amin in alphas and amax in alphas                   # both clips were reached
    else:
        assert alphas == [1.0 - level] * len(alphas)
    assert mon.n_valid == sum(1 for ch, lr in zip(chunks, learn) if lr for r in brute_rows(ch) if r is not None)


def test_monitor_tracks_a_drifting_scale():
    """Plain rolling split-conformal on rows whose s is understated by 2: after the window has filled the band covers."""
    A = C.results_array(6000, 9, understate=2.0)
    mon = U.UncertaintyMonitor(level=0.9, window=500, backend="host")
    miss = np.concatenate([mon.update(A[i:i + 100]).miss for i in range(0, 6000, 100)])
    assert (miss[:100] == 0).all()                                  # q_0 = +inf: nothing can miss before the first chunk has been learnt
    rate = float(np.mean(miss[1000:] == 1))
    assert abs(rate - 0.1) <= 3.0 * math.sqrt(0.09 / 5000) + 0.01, rate


def test_arguments():
    A = C.results_array(10, 0)
    with pytest.raises(ValueError):
        U.score_uncertainty(A, var_model=(1.0, -1.0, 0.0), backend="host")
    with pytest.raises(ValueError):
        U.score_uncertainty(A, groups={"a": [0], "b": [0]}, backend="host")
    with pytest.raises(ValueError):
        U.score_uncertainty(A, groups={"a": [64]}, backend="host")
    with pytest.raises(ValueError):
        U.conformal_quantiles(A, levels=(0.0,), backend="host")
    with pytest.raises(ValueError):
        U.conformal_quantiles(A, levels=[0.5] * 9, backend="host")
    with pytest.raises(ValueError):
        U.conformal_quantiles(A, kind="column", backend="host")
    with pytest.raises(ValueError):
        U.UncertaintyMonitor(window=4097)
    empty = U.score_uncertainty(A[:0], backend="host")["all"]
    assert empty.n == 0 and math.isnan(empty.scale)
    assert np.isnan(U.conformal_quantiles(A[:0], backend="host").q).all()
