"""GPU: csrc/pinn_faultsets.hip against the host backend of pinn_amd.faultsets.  Integers (counts, masks, sizes, tallies),
scores of the posterior kinds and tables are compared byte for byte; the density kind's counts outside close pairs."""
import numpy as np
import pytest

import faultsets_cases as FC

pytestmark = pytest.mark.gpu

# The allowance for log / exp in the density score, in float64 spacings at max(|s|, 1): twice the largest device-to-host
# distance of s_c and s_any over this file's cases as test_the_measured_allowance_still_holds prints it (2.000 on an MI355X).
MEASURED_SPACINGS = 2.0
U_SPACINGS = 2.0 * MEASURED_SPACINGS
DEV, HOST = dict(backend="device"), dict(backend="host")


@pytest.fixture(scope="module")
def F():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    from pinn_amd import faultsets
    return faultsets


def same_sets(a, b):
    for name in ("count", "mask", "size", "novel", "missing"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name
    assert np.array_equal(a.can_reject, b.can_reject)


def same_reports(a, b):
    for name in ("n", "covered", "size_hist", "singleton_correct", "outside_novel"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.outside_n == b.outside_n


def same_tables(a, b, C):
    assert np.array_equal(a.n_cal, b.n_cal) and a.n_skipped == b.n_skipped and a.n_any == b.n_any
    for c in range(C):
        assert a.table(c).tobytes() == b.table(c).tobytes(), c


LEVELS8 = (0.5, 0.75, 0.8, 0.9, 0.95, 0.975, 0.99, 0.999)


# ---------------------------------------------------------------------------------------------- the posterior kinds
@pytest.mark.parametrize("C", [1, 2, 5, 16])
@pytest.mark.parametrize("kind", FC.KINDS)
def test_posterior_kinds_equal_the_host_backend(F, kind, C):
    Pc, yc = FC.posteriors(700, C, 100 + C)
    Pc, _ = FC.spoil(Pc, 1, share=0.02)
    yc[::37] = C + 3                                         # classes outside the range are skipped
    rnd = kind == "aps"
    host = F.calibrate(Pc, yc, kind, randomized=rnd, seed=2 ** 33 + 9, **HOST)
    dev = F.calibrate(Pc, yc, kind, randomized=rnd, seed=2 ** 33 + 9, **DEV)
    assert dev.backend == "device" and host.backend == "host"
    same_tables(dev, host, C)
    Pt, yt = FC.posteriors(257, C, 200 + C)
    Pt, _ = FC.spoil(Pt, 2, share=0.03)
    yt[::11] = -1
    for levels in ((0.9,), LEVELS8):
        for n in (1, 255, 256, 257):
            h = F.prediction_sets(host, Pt[:n], levels, first=5, **HOST)
            for regime in ("auto", "lds", "sampled", "global"):
                same_sets(F.prediction_sets(dev, Pt[:n], levels, first=5, force_regime=regime, **DEV), h)
            same_sets(F.prediction_sets(host, Pt[:n], levels, first=5, **DEV), h)       # a host calibration packed for the device
            same_reports(F.evaluate_sets(dev, Pt[:n], yt[:n], levels, **DEV), F.evaluate_sets(host, Pt[:n], yt[:n], levels, **HOST))
        sd, sh = F.scores(Pt, kind, rnd, 2 ** 33 + 9, first=5, **DEV), F.scores(Pt, kind, rnd, 2 ** 33 + 9, first=5, **HOST)
        assert sd.tobytes() == sh.tobytes()
    # two calls give the same bytes; chunks through first= against the whole
    a, b = F.prediction_sets(dev, Pt, LEVELS8, **DEV), F.prediction_sets(dev, Pt, LEVELS8, **DEV)
    same_sets(a, b)
    parts = [F.prediction_sets(dev, Pt[lo:hi], LEVELS8, first=lo, **DEV) for lo, hi in ((0, 100), (100, 257))]
    assert np.concatenate([p.count for p in parts]).tobytes() == a.count.tobytes()
    assert np.concatenate([p.mask for p in parts]).tobytes() == a.mask.tobytes()
    pv = F.p_values(dev, Pt, **DEV)
    assert pv.count.tobytes() == a.count.tobytes() and np.array_equal(pv.p, F.PValues(a.count, host.n_cal).p, equal_nan=True)


def test_table_sizes_around_a_line_and_a_block_in_every_regime(F):
    sizes = [0, 1, 2, 15, 16, 17, 4095, 4096, 4097]
    C = len(sizes)
    Pc, yc = FC.with_class_sizes(sizes, C, 7)
    Pt, yt = FC.posteriors(4100, C, 8)
    for kind in FC.KINDS:
        host = F.calibrate(Pc, yc, kind, **HOST)
        dev = F.calibrate(Pc, yc, kind, **DEV)
        assert host.n_cal.tolist() == sizes
        same_tables(dev, host, C)
        h = F.prediction_sets(host, Pt, (0.9, 0.99), **HOST)
        for regime in ("auto", "sampled", "global"):         # 12 336 padded entries: beyond the on-chip budget of "lds"
            same_sets(F.prediction_sets(dev, Pt, (0.9, 0.99), force_regime=regime, **DEV), h)
        from pinn_amd._lib import PinnError
        with pytest.raises(PinnError):
            F.prediction_sets(dev, Pt, (0.9,), force_regime="lds", **DEV)
        same_reports(F.evaluate_sets(dev, Pt, yt, (0.9, 0.99), **DEV), F.evaluate_sets(host, Pt, yt, (0.9, 0.99), **HOST))


def test_the_largest_tables_of_the_on_chip_regime_and_one_row_more(F):
    Pt, _ = FC.posteriors(4096, 2, 3)
    for sizes, fits in (((F.LDS_ENTRIES - 16, 16), True), ((F.LDS_ENTRIES - 16, 17), False)):
        Pc, yc = FC.with_class_sizes(sizes, 2, 4)
        host = F.calibrate(Pc, yc, "margin", **HOST)
        dev = F.calibrate(Pc, yc, "margin", **DEV)
        same_tables(dev, host, 2)
        h = F.prediction_sets(host, Pt, (0.9,), **HOST)
        for regime in ("auto", "sampled", "global") + (("lds",) if fits else ()):
            same_sets(F.prediction_sets(dev, Pt, (0.9,), force_regime=regime, **DEV), h)


def test_auto_stages_small_tables_under_many_rows(F):
    """Around both thresholds of the "auto" rule: STAGE_MIN_ROWS - 1 and STAGE_MIN_ROWS rows, tables of AUTO_LDS_ENTRIES padded
    entries and one row more."""
    Pt, yt = FC.posteriors(F.STAGE_MIN_ROWS, 2, 21)
    for sizes in ((F.AUTO_LDS_ENTRIES - 16, 16), (F.AUTO_LDS_ENTRIES - 16, 17)):
        Pc, yc = FC.with_class_sizes(sizes, 2, 22)
        host, dev = F.calibrate(Pc, yc, "lac", **HOST), F.calibrate(Pc, yc, "lac", **DEV)
        h = F.prediction_sets(host, Pt, (0.9,), **HOST)
        same_sets(F.prediction_sets(dev, Pt, (0.9,), **DEV), h)
        for name in ("count", "mask", "size", "novel", "missing"):
            assert getattr(F.prediction_sets(dev, Pt[:-1], (0.9,), **DEV), name).tobytes() == getattr(h, name)[:-1].tobytes()
        same_reports(F.evaluate_sets(dev, Pt, yt, (0.9,), **DEV), F.evaluate_sets(host, Pt, yt, (0.9,), **HOST))


def test_more_tiles_than_workgroups(F):
    n = F.TILE * F.MAX_BLOCKS + 1
    Pc, yc = FC.posteriors(500, 2, 1)
    Pt, yt = FC.posteriors(n, 2, 2)
    Pt[-1] = (0.25, 0.75)
    host, dev = F.calibrate(Pc, yc, "aps", randomized=True, seed=3, **HOST), F.calibrate(Pc, yc, "aps", randomized=True, seed=3, **DEV)
    same_sets(F.prediction_sets(dev, Pt, (0.9, 0.95), **DEV), F.prediction_sets(host, Pt, (0.9, 0.95), **HOST))
    same_reports(F.evaluate_sets(dev, Pt, yt, (0.9, 0.95), **DEV), F.evaluate_sets(host, Pt, yt, (0.9, 0.95), **HOST))


def test_ties_and_exact_integer_levels(F):
    C, sizes, levels = 3, (3, 7, 9), (0.5, 0.75, 0.9)
    Pc, yc = FC.with_class_sizes(sizes, C, 5, quantise=8)
    Pt, yt = FC.posteriors(300, C, 6, quantise=8)
    Pt, yt = np.concatenate([Pt, Pc]), np.concatenate([yt, yc])
    for kind in FC.KINDS:
        host, dev = F.calibrate(Pc, yc, kind, **HOST), F.calibrate(Pc, yc, kind, **DEV)
        same_tables(dev, host, C)
        h = F.prediction_sets(host, Pt, levels, **HOST)
        for regime in ("lds", "sampled", "global"):
            d = F.prediction_sets(dev, Pt, levels, force_regime=regime, **DEV)
            same_sets(d, h)
        assert (d.count[300:][np.arange(len(yc)), yc] >= 1).all()
        same_reports(F.evaluate_sets(dev, Pt, yt, levels, **DEV), F.evaluate_sets(host, Pt, yt, levels, **HOST))


# ---------------------------------------------------------------------------------------------- the sort
def test_build_equals_numpy_sort_per_class(F):
    import torch
    sizes = [0, 1, 2, 4096, 4097, 2 ** 17 + 3]
    C = len(sizes)
    rng = np.random.default_rng(11)
    y = rng.permutation(np.repeat(np.arange(C), sizes))
    n = y.size
    S = rng.normal(size=(n, C))
    S[rng.random((n, C)) < 0.2] = 0.5                        # equal keys
    S[rng.random((n, C)) < 0.05] = 0.0
    S[rng.random((n, C)) < 0.05] = -0.0
    S[rng.random((n, C)) < 0.02] = np.inf
    S[rng.random((n, C)) < 0.02] = -np.inf
    skip = rng.random(n) < 0.01
    S[skip, y[skip]] = np.nan                                # skipped and counted
    any_score = rng.normal(size=n).round(1)
    st, n_cal, n_any, skipped = F._device_build(torch, torch.from_numpy(S).cuda(), y, C, 0, 0, False, torch.from_numpy(any_score).cuda())
    cal = F.SetCalibration("density", C, n_cal, n_any, skipped, 0, False, state=st)
    assert skipped == int(skip.sum()) and n_any == n - skipped
    for c in range(C):
        want = np.sort(S[(y == c) & ~skip, c] + 0.0)
        assert n_cal[c] == want.size and cal.table(c).tobytes() == want.tobytes(), c
    assert cal.table("any").tobytes() == np.sort(any_score[~skip] + 0.0).tobytes()
    st2 = F._device_build(torch, torch.from_numpy(S).cuda(), y, C, 0, 0, False, torch.from_numpy(any_score).cuda())[0]
    assert torch.equal(st.view(torch.int64), st2.view(torch.int64))                     # whatever order the places were handed out in


# ---------------------------------------------------------------------------------------------- the density kind, fused
@pytest.fixture(scope="module")
def mixture():
    return FC.MixtureCase(seed=3, n_per=600)


def density_pair(F, m, levels=(0.9, 0.95)):
    feats = list(range(m.D))
    ch = F.calibrate_gmm(m.gmm, m.cfp, m.X_cal, m.y_cal, "density", **HOST)
    cd = F.calibrate_gmm(m.gmm, m.cfp, m.X_cal, m.y_cal, "density", **DEV)
    return (F.GMMSetDiagnoser(m.gmm, m.cfp, ch, levels, features=feats, **HOST), F.GMMSetDiagnoser(m.gmm, m.cfp, cd, levels, features=feats, **DEV))


def density_scores(F, m, X, backend):
    """s_c [n, C] and s_any [n] of rows under the mixture, as numpy."""
    mix = F._Mixture(m.gmm, m.cfp)
    if backend == "host":
        _, _, S, s_any, _ = mix.host(X, None, None, F.KINDS["density"], False, 0, 0, F.DRAW_TEST)
        return S, s_any
    cal0 = F.SetCalibration("density", mix.C, np.zeros(mix.C, np.int64), 0, 0, 0, False)
    r = mix.launch(X, None, None, cal0, None, 0, F.DRAW_TEST, None, ("scores",))
    return r["o"].scores.cpu().numpy(), r["any_score"].cpu().numpy()


def test_the_measured_allowance_still_holds(F, mixture):
    worst = 0.0
    for X in (mixture.X_cal, mixture.X_te, mixture.X_far):
        (Sh, ah), (Sd, ad) = density_scores(F, mixture, X, "host"), density_scores(F, mixture, X, "device")
        worst = max(worst, float(FC.float_distance(Sd, Sh).max()), float(FC.float_distance(ad, ah).max()))
    print("largest device-to-host distance of a density score: %.3f spacings (allowance %.1f)" % (worst, U_SPACINGS))
    assert 2.0 * worst <= U_SPACINGS


def test_the_fused_posterior_has_the_bytes_of_diagnose(F, mixture):
    import torch
    m = mixture
    saved, m.gmm.backend = m.gmm.backend, "device"
    try:
        wide = np.full((m.X_te.shape[0] + 3, 9), np.nan)
        cols = [7, 2, 4, 0]
        wide[:m.X_te.shape[0], cols] = m.X_te
        pick = np.concatenate([np.arange(0, m.X_te.shape[0], 3), [-1, wide.shape[0] + 5, m.X_te.shape[0] + 1]])     # outside, and a NaN row
        for kind in ("lac", "density"):
            cal = F.calibrate_gmm(m.gmm, m.cfp, m.X_cal, m.y_cal, kind, **DEV)
            d = F.GMMSetDiagnoser(m.gmm, m.cfp, cal, (0.9,), features=list(range(m.D)), **DEV)
            yp, pred, fs = d.predict(torch.from_numpy(m.X_te).cuda())
            want_p, want_y = m.gmm.diagnose(torch.from_numpy(m.X_te).cuda(), m.cfp)
            assert torch.equal(yp.view(torch.int64), want_p.view(torch.int64)) and torch.equal(pred, want_y)
            # in place with a gather list against packed, and two calls
            yq, predq, fq = d.predict(wide, columns=cols, row_index=pick)
            wq, wy = m.gmm.diagnose(wide, m.cfp, columns=cols, row_index=pick)
            assert yq.tobytes() == wq.tobytes() and np.array_equal(predq, wy)
            k = (m.X_te.shape[0] + 2) // 3
            assert fq.count[:k].tobytes() == fs.count.cpu().numpy()[::3].tobytes() and fq.missing[k:].all() and (fq.count[k:] == -1).all()
            again = d.predict(wide, columns=cols, row_index=pick)[2]
            same_sets(again, fq)
    finally:
        m.gmm.backend = saved


def test_density_counts_equal_the_host_outside_close_pairs(F, mixture):
    """A pair (row, class) is close when a host calibration score of the class lies within U_SPACINGS float64 spacings (at
    max(|s|, 1)) of the host's test score; there the device may count one entry more or fewer.  At most 1 % may be close."""
    m = mixture
    dh, dd = density_pair(F, m)
    X = np.concatenate([m.X_te, m.X_far])
    _, _, fh = dh.predict(X)
    _, _, fd = dd.predict(X)
    Sh, ah = density_scores(F, m, X, "host")
    close = np.zeros(Sh.shape, bool)
    tol = U_SPACINGS * np.spacing(np.maximum(np.abs(Sh), 1.0))
    for c in range(m.C):
        T = dh.cal.table(c)
        close[:, c] = np.searchsorted(T, Sh[:, c] - tol[:, c], "left") < np.searchsorted(T, Sh[:, c] + tol[:, c], "right")
    print("close pairs: %d of %d" % (int(close.sum()), close.size))
    assert close.mean() <= 0.01
    assert np.array_equal(fd.count[~close], fh.count[~close]) and np.array_equal(fd.missing, fh.missing)
    rows = ~close.any(axis=1)
    assert np.array_equal(fd.mask[rows], fh.mask[rows]) and np.array_equal(fd.size[rows], fh.size[rows])
    assert np.array_equal(dd.cal.n_cal, dh.cal.n_cal) and dd.cal.n_any == dh.cal.n_any
    # the far cluster through the fused path: every set empty
    far = slice(m.X_te.shape[0], None)
    assert (fd.count[far] == 0).all() and (fd.size[far] == 0).all() and fd.novel[far].all() and (fd.count_any[far] == 0).all()
    # every regime gives the device's own bytes
    for regime in ("lds", "sampled", "global"):
        dd.force_regime = regime
        same_sets(dd.predict(X)[2], fd)
    dd.force_regime = "auto"
    # a test row that is a calibration row of the same backend ties exactly: it counts itself
    own = dd.predict(m.X_cal)[2]
    assert (own.count[np.arange(m.y_cal.size), m.y_cal] >= 1).all() and (own.count_any >= 1).all()
    # tallies from the launch equal tallies counted from its sets
    y = np.concatenate([m.y_te, np.full(m.X_far.shape[0], 13)])
    rep = dd.evaluate(X, y)
    same_reports(rep, F.SetReport(F._host_tally(fd.mask, fd.size, fd.missing, y, m.C), m.C, dd.levels, fd.can_reject))
    assert rep.outside_n == m.X_far.shape[0] and (rep.outside_novel == rep.outside_n).all()


@pytest.mark.parametrize("kind", ["aps", "density"])
def test_update_in_chunks_equals_predict_on_the_whole_with_one_launch_per_chunk(F, mixture, kind, monkeypatch):
    import torch
    m = mixture
    cal = F.calibrate_gmm(m.gmm, m.cfp, m.X_cal, m.y_cal, kind, randomized=True, seed=8, **DEV)
    n = 1 + 2047 + 2048 + 2048 + 5
    rng = np.random.default_rng(0)
    res = np.zeros((n, 22))
    res[:, 13:17] = np.concatenate([m.X_te, m.X_far])[rng.integers(m.X_te.shape[0] + m.X_far.shape[0], size=n)]
    res = torch.from_numpy(res).cuda()
    d = F.GMMSetDiagnoser(m.gmm, m.cfp, cal, (0.9, 0.95), **DEV)
    whole = d.predict(res, columns=d.columns)
    launches = []
    real = F.call
    monkeypatch.setattr(F, "call", lambda name, *a, **k: (launches.append(name), real(name, *a, **k))[1])
    parts, lo = [], 0
    for size in (1, 2047, 2048, 2048 + 5):
        before = len(launches)
        parts.append(d.update(res[lo:lo + size]))
        lo += size
        assert launches[before:] == ["pinn_fs_gmm"] * (-(-size // 2048))
    assert d.n_seen == n
    for i in (0, 1):
        assert torch.equal(torch.cat([p[i] for p in parts]).view(torch.int64), whole[i].view(torch.int64))
    for name in ("count", "mask", "size", "novel", "missing"):
        assert torch.equal(torch.cat([getattr(p[2], name) for p in parts]), getattr(whole[2], name)), name
