"""CPU: the statistics of pinn_amd.faultsets on its host backend, held to something simpler than themselves: double loops,
exact rationals, the exact finite-sample law of split-conformal p-values."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import faultsets_cases as FC
from pinn_amd import faultsets as F

HOST = dict(backend="host")


# ---------------------------------------------------------------------------------------------- brute force
@pytest.mark.parametrize("C", [1, 2, 5, 16])
@pytest.mark.parametrize("kind", FC.KINDS)
def test_counts_and_p_values_equal_a_double_loop(kind, C):
    Pc, yc = FC.posteriors(90, C, 10 + C)
    Pt, _ = FC.posteriors(70, C, 20 + C)
    Pt, spoiled = FC.spoil(Pt, 3)
    for randomized in ((False, True) if kind == "aps" else (False,)):
        cal = F.calibrate(Pc, yc, kind, randomized=randomized, seed=77, **HOST)
        u_cal = F.uniforms(77, F.DRAW_CAL, 0, 90) if randomized else None
        u_te = F.uniforms(77, F.DRAW_TEST, 0, 70) if randomized else None
        Sc, St = FC.brute_scores(Pc, kind, u_cal), FC.brute_scores(Pt, kind, u_te)
        assert np.array_equal(F.scores(Pt, kind, randomized, 77, **HOST), St, equal_nan=True)
        tables = FC.brute_tables(Sc, yc, C)
        for c in range(C):
            assert np.array_equal(cal.table(c), tables[c]) and cal.n_cal[c] == tables[c].size
        pv = F.p_values(cal, Pt, **HOST)
        want = FC.brute_counts(tables, St)
        assert pv.count.dtype == np.int32 and np.array_equal(pv.count, want)
        assert (pv.count[spoiled] == -1).all() and np.isnan(pv.p[spoiled]).all()
        ok = want[:, 0] >= 0
        assert np.array_equal(pv.p[ok], (want[ok] + 1) / (cal.n_cal + 1.0))
        fs = F.prediction_sets(cal, Pt, levels=(0.8, 0.9), **HOST)
        assert fs.mask.dtype == np.uint16 and fs.size.dtype == np.uint8 and fs.novel.dtype == bool and fs.missing.dtype == bool
        assert np.array_equal(np.flatnonzero(fs.missing), spoiled) and not fs.mask[spoiled].any() and not fs.novel[spoiled].any()
        for l, lv in enumerate((0.8, 0.9)):
            alpha = 1 - Fraction(lv)
            for i in np.flatnonzero(ok):
                members = [c for c in range(C) if Fraction(int(want[i, c]) + 1, int(cal.n_cal[c]) + 1) > alpha]
                assert fs.members(i, lv) == members and fs.size[i, l] == len(members) and fs.novel[i, l] == (not members)


# ---------------------------------------------------------------------------------------------- ties and exact levels
def test_ties_exact_integer_levels_and_inexact_floats():
    C = 3
    sizes = (3, 7, 9)
    Pc, yc = FC.with_class_sizes(sizes, C, 5, quantise=8)
    Pt, _ = FC.posteriors(60, C, 6, quantise=8)
    Pt = np.concatenate([Pt, Pc])                           # test rows that are calibration rows
    levels = (0.5, 0.75, 0.9)                               # alpha (n_c + 1): 2 exactly for n_c = 3, 2 exactly for n_c = 7, 0.9 is no decimal
    for kind in FC.KINDS:
        cal = F.calibrate(Pc, yc, kind, **HOST)
        assert cal.n_cal.tolist() == list(sizes)
        km = F.kmin_table(cal.n_cal, levels)
        for c, n_c in enumerate(sizes):
            for l, lv in enumerate(levels):
                assert km[c, l] == FC.kmin_exact(n_c, lv) == math.floor((1 - Fraction(lv)) * (n_c + 1))
        assert km[0, 0] == 2 and km[1, 1] == 2               # 0.5 * 4 and 0.25 * 8, exactly
        assert km[2, 2] == 0 and Fraction(0.9) > Fraction(9, 10)      # 0.9 the float is above 9/10: floor(alpha 10) is 0, not 1
        St = FC.brute_scores(Pt, kind)
        tables = FC.brute_tables(FC.brute_scores(Pc, kind), yc, C)
        want = FC.brute_counts(tables, St)
        fs = F.prediction_sets(cal, Pt, levels=levels, **HOST)
        assert np.array_equal(fs.count, want)
        ties = sum(int((tables[c][None, :] == St[:, c][:, None]).any(axis=1).sum()) for c in range(C))
        assert ties > St.shape[0]                            # the quantised scores do tie with the tables
        for l in range(len(levels)):
            inc = want >= km[:, l][None, :]
            assert np.array_equal(fs.mask[:, l], (inc << np.arange(C)).sum(axis=1).astype(np.uint16))
        assert np.array_equal(fs.can_reject, km > 0) and not fs.can_reject[2, 2]
        own = np.arange(60, Pt.shape[0])                     # a calibration row counts itself
        assert (fs.count[own, yc] >= 1).all()


# ---------------------------------------------------------------------------------------------- the finite-sample property
@pytest.fixture(scope="module")
def mixture():
    return FC.MixtureCase(seed=3)


def _leave_one_out_p(kind, rows, c, mixture=None):
    """The p-value of every row of class c's rows under a calibration on the others, as exact fractions."""
    out = []
    n = len(rows)
    for i in range(n):
        rest = np.delete(np.arange(n), i)
        if kind == "density":
            cal = F.calibrate_gmm(mixture.gmm, mixture.cfp, rows[rest], np.full(n - 1, c), "density", **HOST)
            d = F.GMMSetDiagnoser(mixture.gmm, mixture.cfp, cal, features=list(range(mixture.D)), **HOST)
            count = d.predict(rows[i:i + 1])[2].count[0, c]
        else:
            # aps with u = 1: the property is one of n + 1 fixed scores, and a randomized row would score differently in its two roles
            cal = F.calibrate(rows[rest], np.full(n - 1, c), kind, n_classes=rows.shape[1], **HOST)
            count = F.p_values(cal, rows[i:i + 1], **HOST).count[0, c]
        assert cal.n_cal[c] == n - 1
        out.append(Fraction(int(count) + 1, n))
    return out


@pytest.mark.parametrize("kind", FC.KINDS + ("density",))
def test_leave_one_out_p_values_obey_the_exact_bound(kind, mixture):
    n1 = 81                                                 # n_c + 1: at alpha = 0.013 one row may be rejected (floor(1.053) = 1)
    for c in range(4):
        if kind == "density":
            rows = np.concatenate([mixture.X_cal[mixture.y_cal == c], mixture.X_te[mixture.y_te == c]])[:n1]
        else:
            P, y = FC.posteriors(700, 4, 50 + c)
            rows = P[y == c][:n1]
        assert rows.shape[0] == n1
        p = _leave_one_out_p(kind, rows, c, mixture)
        for alpha in (0.1, 0.05, 0.013):
            a = Fraction(alpha)
            assert sum(1 for v in p if v <= a) <= math.floor(a * n1), (kind, c, alpha)

# ---------------------------------------------------------------------------------------------- the density score's referee
def test_density_scores_counts_and_p_against_a_referee_from_the_covariances(mixture):
    """s_c and s_any against an mpmath evaluation from weights_, means_ and covariances_ under a soft label map with zeros,
    then counts and p against a double loop.  The gate: the host reads precisions_cholesky_, which carries the covariance's
    rounding times its condition number kappa, forms the quadratic form in D (D + 1) / 2 products and the logsumexp in K
    terms; 8 (D (D + 1) / 2 + K + 4) kappa spacings at max(|s|, 1) bound that with room, and a score with log m dropped,
    the component subset ignored or s_any in place of s_c misses it by many orders of magnitude."""
    m = mixture
    g = m.gmm
    cfp = np.asarray(m.cfp, np.float64).copy() + 0.05        # soft: every component speaks for every class ...
    cfp[0, 1] = cfp[3, 0] = cfp[5, 2] = cfp[5, 3] = 0.0      # ... but for these
    cfp[6] = (0.0, 0.0, 1.0, 0.0)
    cfp /= cfp.sum(axis=1, keepdims=True)
    assert ((cfp > 0) & (cfp < 1)).sum() > m.K * 2 and (cfp == 0).sum() >= 7
    X = np.concatenate([m.X_te[:40], m.X_far[:8]])
    mix = F._Mixture(g, cfp)
    _, _, S, s_any, miss = mix.host(X, None, None, F.KINDS["density"], False, 0, 0, F.DRAW_TEST)
    want_S, want_any = FC.mp_density_scores(X, np.asarray(g.weights_), np.asarray(g.means_), np.asarray(g.covariances_), cfp)
    kappa = max(np.linalg.cond(np.asarray(g.covariances_)[k]) for k in range(m.K))
    gate = 8.0 * (m.D * (m.D + 1) / 2 + m.K + 4) * kappa
    assert not miss.any() and np.isfinite(want_S).all()
    dS, dA = FC.float_distance(S, want_S), FC.float_distance(s_any, want_any)
    print("density score against the referee: %.2f and %.2f spacings, gate %.0f (kappa %.2f)" % (dS.max(), dA.max(), gate, kappa))
    assert dS.max() <= gate and dA.max() <= gate
    # what the gate tells apart: the classes' scores differ from one another and from s_any by far more than the gate
    assert (FC.float_distance(want_S, want_any[:, None]) > 1e6 * gate).all()
    assert (FC.float_distance(want_S[:, 0], want_S[:, 1]) > 1e6 * gate).all()
    # counts and p by a double loop over the calibration rows
    cal = F.calibrate_gmm(g, cfp, m.X_cal, m.y_cal, "density", **HOST)
    _, _, Sc, ac, _ = mix.host(m.X_cal, None, None, F.KINDS["density"], False, 0, 0, F.DRAW_CAL)
    tables = FC.brute_tables(Sc, m.y_cal, m.C)
    assert all(np.array_equal(cal.table(c), tables[c]) for c in range(m.C)) and np.array_equal(cal.table("any"), np.sort(ac + 0.0))
    _, _, fs = F.GMMSetDiagnoser(g, cfp, cal, (0.9,), features=list(range(m.D)), **HOST).predict(X)
    want = FC.brute_counts(tables, S)
    assert np.array_equal(fs.count, want) and 0 < want[:40].max() and (want[40:] == 0).all()
    assert np.array_equal(F.PValues(fs.count, cal.n_cal).p, (want + 1) / (cal.n_cal + 1.0))
    assert np.array_equal(fs.count_any, [sum(1 for t in cal.table("any").tolist() if t >= a) for a in s_any.tolist()])
    assert np.array_equal(fs.p_any, (fs.count_any + 1) / (cal.n_any + 1.0))


# ---------------------------------------------------------------------------------------------- seeded coverage
@pytest.mark.parametrize("kind", FC.KINDS + ("density",))
def test_coverage_of_fresh_rows_lies_in_the_exact_beta_binomial_region(kind, mixture):
    levels = (0.8, 0.9, 0.95)
    if kind == "density":
        cal = F.calibrate_gmm(mixture.gmm, mixture.cfp, mixture.X_cal, mixture.y_cal, "density", **HOST)
        d = F.GMMSetDiagnoser(mixture.gmm, mixture.cfp, cal, levels=levels, features=list(range(mixture.D)), **HOST)
        rep = d.evaluate(mixture.X_te, mixture.y_te)
    else:
        P, y = FC.posteriors(2400, 4, 91)
        cal = F.calibrate(P[:600], y[:600], kind, randomized=(kind == "aps"), seed=4, **HOST)
        rep = F.evaluate_sets(cal, P[600:], y[600:], levels=levels, **HOST)
    km = F.kmin_table(cal.n_cal, levels)
    for c in range(4):
        for l in range(len(levels)):
            assert km[c, l] >= 1
            lo, hi = FC.hits_region(int(rep.n[c]), int(cal.n_cal[c]), int(km[c, l]))
            assert lo <= rep.covered[c, l] <= hi, (kind, c, levels[l], lo, int(rep.covered[c, l]), hi)


# ---------------------------------------------------------------------------------------------- the unknown fault
def test_a_far_cluster_is_rejected_by_density_scores_and_not_by_lac():
    from pinn_amd.diagnosis import DeviceGMM
    m = FC.MixtureCase(seed=5)
    C = m.C
    # one component per class and a one-hot label map: a far row's posterior is then the largest a row can have
    gmm = DeviceGMM(C, labels_init=m.y_fit, max_iter=0, backend="host").fit(m.X_fit)
    cfp = np.eye(C)
    feats = list(range(m.D))
    cal = F.calibrate_gmm(gmm, cfp, m.X_cal, m.y_cal, "density", **HOST)
    levels = tuple(1.0 - 1.0 / (int(n) + 1) for n in cal.n_cal) + (0.5,)          # alpha = 1 / (n_c + 1) and above
    d = F.GMMSetDiagnoser(gmm, cfp, cal, levels=levels[:8], features=feats, **HOST)
    _, _, fs = d.predict(m.X_far)
    worst = max(cal.table(c)[-1] for c in range(C))
    assert not fs.missing.any() and (fs.count == 0).all() and fs.count_any is not None and (fs.count_any == 0).all()
    pv = F.PValues(fs.count, cal.n_cal)
    assert np.array_equal(pv.p, np.broadcast_to(1.0 / (cal.n_cal + 1.0), pv.p.shape))
    assert np.array_equal(fs.p_any, np.full(m.X_far.shape[0], 1.0 / (cal.n_any + 1)))
    km = F.kmin_table(cal.n_cal, levels[:8])
    for l, lv in enumerate(levels[:8]):
        for c in range(C):
            if 1 - Fraction(lv) >= Fraction(1, int(cal.n_cal[c]) + 1):
                assert km[c, l] >= 1 and not ((fs.mask[:, l] >> c) & 1).any()
    assert fs.novel[:, -1].all() and (fs.size[:, -1] == 0).all()                  # at 0.5 every class can be rejected
    assert np.isfinite(worst)
    cal_lac = F.calibrate_gmm(gmm, cfp, m.X_cal, m.y_cal, "lac", **HOST)
    _, y_pred, fs_lac = F.GMMSetDiagnoser(gmm, cfp, cal_lac, levels=(0.5, 0.9), features=feats, **HOST).predict(m.X_far)
    top = fs_lac.count[np.arange(m.X_far.shape[0]), y_pred]
    assert np.array_equal(top, cal_lac.n_cal[y_pred])                             # the smallest score a row can have: p = 1
    assert (fs_lac.size >= 1).all() and not fs_lac.novel.any()


# ---------------------------------------------------------------------------------------------- edges
def test_missing_rows_enter_nothing():
    P, y = FC.posteriors(200, 4, 1)
    Ps, spoiled = FC.spoil(P, 2)
    cal = F.calibrate(Ps, y, "lac", **HOST)
    clean = np.setdiff1d(np.arange(200), spoiled)
    ref = F.calibrate(P[clean], y[clean], "lac", **HOST)
    assert cal.n_skipped == spoiled.size and all(np.array_equal(cal.table(c), ref.table(c)) for c in range(4))
    y_bad = y.copy()
    y_bad[:5] = (-1, 4, 99, -7, 4)
    assert F.calibrate(P, y_bad, "lac", **HOST).n_skipped == 5
    rep = F.evaluate_sets(ref, Ps, y, **HOST)
    assert rep.n.sum() == clean.size and rep.outside_n == 0 and rep.size_hist.sum() == clean.size


def test_an_empty_class_is_in_every_set_and_says_so():
    P, y = FC.posteriors(300, 4, 8)
    keep = y != 2
    for kind in FC.KINDS:
        cal = F.calibrate(P[keep], y[keep], kind, n_classes=4, **HOST)
        assert cal.n_cal[2] == 0 and cal.table(2).size == 0
        fs = F.prediction_sets(cal, P, levels=(0.5, 0.99), **HOST)
        assert (fs.count[:, 2] == 0).all() and (F.p_values(cal, P, **HOST).p[:, 2] == 1.0).all()
        assert ((fs.mask >> 2) & 1).all() and not fs.can_reject[2].any() and not fs.novel.any()


def test_a_class_no_component_stands_for_scores_plus_infinity(mixture):
    cfp = np.asarray(mixture.cfp).copy()
    cfp[:, 1] = 0.0                                         # pi_1 = 0
    keep = mixture.y_cal != 1
    cal = F.calibrate_gmm(mixture.gmm, cfp, mixture.X_cal[keep], mixture.y_cal[keep], "density", **HOST)
    d = F.GMMSetDiagnoser(mixture.gmm, cfp, cal, features=list(range(mixture.D)), **HOST)
    assert cal.n_cal[1] == 0 and d.mix.logpi[1] == -np.inf
    _, _, fs = d.predict(mixture.X_te)
    assert (fs.count[:, 1] == 0).all() and not fs.missing.any()
    cal2 = F.calibrate_gmm(mixture.gmm, cfp, mixture.X_cal, mixture.y_cal, "density", **HOST)       # class 1's rows: +inf in the table
    assert np.isinf(cal2.table(1)).all() and cal2.n_cal[1] == (mixture.y_cal == 1).sum()
    fs2 = F.GMMSetDiagnoser(mixture.gmm, cfp, cal2, features=list(range(mixture.D)), **HOST).predict(mixture.X_te)[2]
    assert (fs2.count[:, 1] == cal2.n_cal[1]).all()         # inf >= inf


def test_one_class():
    P = np.random.default_rng(0).uniform(0.1, 1.0, size=(50, 1))
    for kind in FC.KINDS:
        cal = F.calibrate(P[:30], np.zeros(30, np.int64), kind, **HOST)
        fs = F.prediction_sets(cal, P[30:], levels=(0.9,), **HOST)
        assert np.array_equal(fs.count, FC.brute_counts([cal.table(0)], FC.brute_scores(P[30:], kind)))
    assert np.array_equal(F.scores(P, "margin", **HOST), -P)


def test_aps_draws_follow_the_row_number_and_the_kind_of_row():
    P, y = FC.posteriors(300, 5, 12)
    whole = F.scores(P, "aps", randomized=True, seed=2 ** 40 + 5, first=7, **HOST)
    for cuts in ((100, 200), (1, 299), (256,)):
        parts = np.split(np.arange(300), cuts)
        got = np.concatenate([F.scores(P[p], "aps", randomized=True, seed=2 ** 40 + 5, first=7 + int(p[0]), **HOST) for p in parts])
        assert got.tobytes() == whole.tobytes()
    cal = F.calibrate(P, y, "aps", randomized=True, seed=3, **HOST)
    sets_whole = F.prediction_sets(cal, P, **HOST)
    sets_parts = [F.prediction_sets(cal, P[a:b], first=a, **HOST) for a, b in ((0, 130), (130, 300))]
    assert np.array_equal(np.concatenate([s.count for s in sets_parts]), sets_whole.count)
    u_cal, u_te = F.uniforms(3, F.DRAW_CAL, 0, 300), F.uniforms(3, F.DRAW_TEST, 0, 300)
    assert F.DRAW_CAL != F.DRAW_TEST and not np.array_equal(u_cal, u_te) and ((0 <= u_te) & (u_te < 1)).all()
    assert np.array_equal(F.scores(P, "aps", randomized=True, seed=3, **HOST), FC.brute_scores(P, "aps", u_te))
    assert np.array_equal(F.scores(P, "aps", **HOST), FC.brute_scores(P, "aps", np.ones(300)))         # u = 1


def test_evaluate_sets_equals_tallies_counted_from_the_sets():
    P, y = FC.posteriors(900, 5, 30)
    P, spoiled = FC.spoil(P, 31)
    y[::13] = 13                                            # a held-back condition
    y[5::29] = -1
    levels = (0.5, 0.9, 0.99)
    for kind in FC.KINDS:
        cal = F.calibrate(P[:300], y[:300], kind, **HOST)
        Pt, yt = P[300:], y[300:]
        rep, fs = F.evaluate_sets(cal, Pt, yt, levels, **HOST), F.prediction_sets(cal, Pt, levels, **HOST)
        ok = ~fs.missing
        inside = ok & (yt >= 0) & (yt < 5)
        assert rep.n.dtype == np.int64 and np.array_equal(rep.n, np.bincount(yt[inside], minlength=5))
        for l in range(3):
            bit = (fs.mask[:, l] >> np.where(inside, yt, 0)) & 1
            assert np.array_equal(rep.covered[:, l], [int(bit[inside & (yt == c)].sum()) for c in range(5)])
            assert np.array_equal(rep.size_hist[l], np.bincount(fs.size[inside, l], minlength=6))
            assert rep.singleton_correct[l] == int(((fs.size[:, l] == 1) & (bit == 1) & inside).sum())
            assert rep.outside_novel[l] == int((fs.novel[:, l] & ok & ~inside).sum())
        assert rep.outside_n == int((ok & ~inside).sum()) and rep.outside_n > 0
        assert np.allclose(rep.coverage, rep.covered / rep.n[:, None]) and rep.mean_size.shape == (3,)


def test_calibrate_gmm_equals_calibrate_on_the_diagnosis(mixture):
    saved, mixture.gmm.backend = mixture.gmm.backend, "host"
    y_prob, y_pred = mixture.gmm.diagnose(mixture.X_cal, mixture.cfp)
    y_te, pred_te = mixture.gmm.diagnose(mixture.X_te, mixture.cfp)
    mixture.gmm.backend = saved
    wide = np.full((mixture.X_cal.shape[0], 9), np.nan)     # rows read in place: columns and a gather list
    cols = [7, 2, 4, 0]
    wide[:, cols] = mixture.X_cal
    pick = np.arange(0, wide.shape[0], 2)
    for kind in FC.KINDS:
        a = F.calibrate_gmm(mixture.gmm, mixture.cfp, mixture.X_cal, mixture.y_cal, kind, randomized=True, seed=6, **HOST)
        b = F.calibrate(y_prob, mixture.y_cal, kind, randomized=True, seed=6, **HOST)
        assert all(a.table(c).tobytes() == b.table(c).tobytes() for c in range(mixture.C)) and a.n_skipped == b.n_skipped == 0
        d = F.GMMSetDiagnoser(mixture.gmm, mixture.cfp, a, levels=(0.9, 0.95), features=list(range(mixture.D)), **HOST)
        yp, pred, fs = d.predict(mixture.X_te)
        ref = F.prediction_sets(b, y_te, levels=(0.9, 0.95), **HOST)
        assert yp.tobytes() == y_te.tobytes() and np.array_equal(pred, pred_te)
        assert np.array_equal(fs.count, ref.count) and np.array_equal(fs.mask, ref.mask)
        c = F.calibrate_gmm(mixture.gmm, mixture.cfp, wide, mixture.y_cal[pick], kind, columns=cols, row_index=pick, randomized=True, seed=6, **HOST)
        e = F.calibrate(y_prob[pick], mixture.y_cal[pick], kind, randomized=True, seed=6, **HOST)
        assert all(c.table(k).tobytes() == e.table(k).tobytes() for k in range(mixture.C))
    # the online form: chunks against the whole
    cal = F.calibrate_gmm(mixture.gmm, mixture.cfp, mixture.X_cal, mixture.y_cal, "aps", randomized=True, seed=6, **HOST)
    res = np.zeros((mixture.X_te.shape[0], 22))
    res[:, 13:17] = mixture.X_te
    d = F.GMMSetDiagnoser(mixture.gmm, mixture.cfp, cal, **HOST)
    whole = d.predict(res, columns=d.columns)
    parts = [d.update(res[a:b]) for a, b in ((0, 1), (1, 100), (100, res.shape[0]))]
    assert d.n_seen == res.shape[0]
    assert np.array_equal(np.concatenate([p[2].count for p in parts]), whole[2].count)
    # y_prob has diagnose's bytes chunk by chunk (the host's matrix product may round a row differently in another batch)
    mixture.gmm.backend = "host"
    for (a, b), part in zip(((0, 1), (1, 100), (100, res.shape[0])), parts):
        assert part[0].tobytes() == mixture.gmm.diagnose(res[a:b], mixture.cfp, columns=d.columns)[0].tobytes()
    mixture.gmm.backend = saved


def test_arguments_are_checked():
    P, y = FC.posteriors(20, 3, 0)
    cal = F.calibrate(P, y, **HOST)
    for bad in (dict(levels=()), dict(levels=(0.0,)), dict(levels=(1.0,)), dict(levels=tuple([0.5] * 9))):
        with pytest.raises(ValueError):
            F.prediction_sets(cal, P, **bad, **HOST)
    with pytest.raises(ValueError):
        F.calibrate(P, y, "density", **HOST)
    with pytest.raises(ValueError):
        F.calibrate(P, y, "nothing", **HOST)
    with pytest.raises(ValueError):
        F.prediction_sets(cal, P[:, :2], **HOST)
    with pytest.raises(ValueError):
        F.calibrate(np.ones((3, 17)), np.zeros(3), **HOST)
    with pytest.raises(ValueError):
        F.calibrate(P, y[:5], **HOST)
    import pinn_amd
    assert pinn_amd.faultsets is F and pinn_amd.prediction_sets is F.prediction_sets and pinn_amd.GMMSetDiagnoser is F.GMMSetDiagnoser


def test_the_example_runs_on_the_host_backend(capsys):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "examples"))
    try:
        import open_set_diagnosis as ex
    finally:
        sys.path.pop(0)
    held_novel, n_held = ex.main(["--backend", "host", "--rows", "450", "--chunk", "700"])
    out = capsys.readouterr().out
    assert "density" in out and "lac" in out and "held back, novel" in out and "coverage@0.95" in out
    assert n_held == 450 and held_novel == n_held            # every held-back row, 25 sigma away, has an empty density set
