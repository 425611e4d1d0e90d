"""CPU: the host backend of pinn_amd.temporal (sequential float64 recursions) against the two referees of hmm_cases.py, the
identities of the model, chunking, fitting and the claim the README makes for smoothing.  Gates as in hmm_cases.py; every
comparison prints its maxima before it asserts."""
import functools

import numpy as np
import pytest

import hmm_cases as H
from hmm_cases import check, logprob_atol, loglik_atol, rtol_of
from pinn_amd import temporal  # noqa: F401  (numpy only; without the module this file fails at import)

ATOL = 1e-290


def host(A, p0=None, prior=None):
    from pinn_amd import temporal
    return temporal.DeviceHMM(A, p0, prior, backend="host")


def tiny_cases():
    rng = np.random.default_rng(3)
    A = H.random_transitions(3, rng, stay=0.5)
    p0 = np.array([0.5, 0.3, 0.2])
    y = rng.random((6, 3)) + 0.05
    yield "dense", A, p0, y, None
    A0 = A.copy()
    A0[0, 2] = 0.0
    A0[0] /= A0[0].sum()
    y0 = y.copy()
    y0[3] = 0.0                                     # a missing row
    yield "zero in A, missing row", A0, p0, y0, np.array([0.2, 0.5, 0.3])


def compare_all(tag, hmm, y, want, n, S, seg=None, **rows):
    rt = rtol_of(n, S)
    alpha, L, _ = hmm.filter(y, seg_starts=seg, **rows)
    gamma, L2 = hmm.smooth(y, seg_starts=seg, **rows)
    xi, gsum, L3 = hmm.expected_counts(y, seg_starts=seg, **rows)
    alpha, gamma, xi, gsum = (np.asarray(v.cpu() if hasattr(v, "cpu") else v) for v in (alpha, gamma, xi, gsum))
    L, L2, L3 = (np.asarray(v.cpu() if hasattr(v, "cpu") else v) for v in (L, L2, L3))
    check(tag + " alpha", alpha, want["alpha"], rt, ATOL)
    check(tag + " gamma", gamma, want["gamma"], rt, ATOL)
    check(tag + " xi", xi, want["xi"], rt, ATOL)
    check(tag + " gamma_sum", gsum, want["gamma_sum"], rt, ATOL)
    la = loglik_atol(n, S, want["loglik"])
    for name, l in (("filter", L), ("smooth", L2), ("counts", L3)):
        check(tag + " loglik " + name, l, np.asarray(want["loglik"], dtype=float).reshape(-1), 0.0, la)
    return alpha, gamma, xi, gsum


def check_identities(tag, alpha, gamma, xi, gsum, n, S, seg=None):
    rt = rtol_of(n, S)
    check(tag + " rows of alpha", alpha.sum(axis=1), np.ones(n), rt)
    check(tag + " rows of gamma", gamma.sum(axis=1), np.ones(n), rt)
    check(tag + " rows of xi", xi.sum(axis=1), gsum, rt, ATOL)
    ends = [hi - 1 for _, hi in H.bounds_of(seg, n)]
    check(tag + " gamma = alpha at ends", gamma[ends], alpha[ends], rt, ATOL)


@pytest.mark.parametrize("case", list(tiny_cases()), ids=lambda c: c[0])
def test_enumeration_sequential_referee_and_host_agree(case):
    name, A, p0, y, prior = case
    b = H.emissions(y, prior)
    exact = H.brute_force(b, A, p0)
    seq = H.sequential(b, A, p0)
    vit = H.sequential_viterbi(b, A, p0)
    for k in ("alpha", "gamma", "xi"):
        check("referee " + k, seq[k], exact[k], 1e-13, 1e-300)
    check("referee loglik", seq["loglik"], [exact["loglik"]], 0, 1e-13)
    assert np.array_equal(vit["path"], exact["path"])
    check("referee path logprob", vit["logprob"], [exact["path_logprob"]], 0, 1e-13)
    hmm = host(A, p0, prior)
    exact["gamma_sum"] = exact["gamma"][:-1].sum(axis=0)
    alpha, gamma, xi, gsum = compare_all(name, hmm, y, exact, 6, 3)
    check_identities(name, alpha, gamma, xi, gsum, 6, 3)
    path, lp = hmm.viterbi(y)
    assert path.dtype == np.int64 and np.array_equal(path, exact["path"])
    check("path logprob", lp, [exact["path_logprob"]], 0, logprob_atol(6, exact["path_logprob"]))


@pytest.mark.parametrize("S,n,seg", [(5, 3000, [0, 1, 700, 2999]), (8, 1500, None), (2, 1000, [0, 500])])
def test_host_matches_the_sequential_referee_at_length(S, n, seg):
    A, p0, y, _ = H.random_case(n, S, seed=10 + S, seg_starts=seg)
    y[5] = np.nan
    y[n // 2: n // 2 + 3] = 0.0
    prior = np.linspace(1.0, 2.0, S) / np.linspace(1.0, 2.0, S).sum()
    b = H.emissions(y, prior)
    hmm = host(A, p0, prior)
    alpha, gamma, xi, gsum = compare_all("S=%d" % S, hmm, y, H.sequential(b, A, p0, seg), n, S, seg)
    check_identities("S=%d" % S, alpha, gamma, xi, gsum, n, S, seg)
    vit = H.sequential_viterbi(b, A, p0, seg)
    path, lp = hmm.viterbi(y, seg_starts=seg)
    assert np.array_equal(path, vit["path"])
    check("logprob", lp, vit["logprob"], 0, logprob_atol(n, vit["delta"]))


def test_left_to_right_chain_with_an_absorbing_state():
    A, p0, y, _ = H.random_case(800, 4, seed=5, A=H.left_to_right(4))
    b = H.emissions(y)
    hmm = host(A, p0)
    compare_all("left-to-right", hmm, y, H.sequential(b, A, p0), 800, 4)
    path, _ = hmm.viterbi(y)
    assert np.array_equal(path, H.sequential_viterbi(b, A, p0)["path"])
    assert np.all(np.diff(path) >= 0) and np.all(np.diff(path) <= 1)         # it can only stay or step


def test_trivial_models_are_exact():
    rng = np.random.default_rng(0)
    y1 = rng.random((50, 1)) + 0.1
    h1 = host(np.ones((1, 1)))
    alpha, L, _ = h1.filter(y1)
    gamma, _ = h1.smooth(y1)
    xi, gsum, _ = h1.expected_counts(y1)
    assert np.array_equal(alpha, np.ones((50, 1))) and np.array_equal(gamma, np.ones((50, 1)))
    assert xi[0, 0] == 49.0 and gsum[0] == 49.0 and np.array_equal(h1.viterbi(y1)[0], np.zeros(50, dtype=np.int64))
    check("S=1 loglik", L, [np.log(y1[:, 0]).sum()], 0, loglik_atol(50, 1, np.log(y1[:, 0]).sum()))
    # A = identity and a one-hot start: the state never moves
    y = rng.random((200, 4)) + 0.05
    hI = host(np.eye(4), np.array([0.0, 0.0, 1.0, 0.0]))
    for out in (hI.filter(y)[0], hI.smooth(y)[0]):
        assert np.array_equal(out, np.tile([0.0, 0.0, 1.0, 0.0], (200, 1)))
    assert np.array_equal(hI.viterbi(y)[0], np.full(200, 2))
    # every row of A equal to p0: no time coupling, the posterior is recovered row by row
    p0 = np.array([0.1, 0.2, 0.3, 0.4])
    hR = host(np.tile(p0, (4, 1)), p0)
    want = p0 * y / (p0 * y).sum(axis=1, keepdims=True)
    check("iid alpha", hR.filter(y)[0], want, rtol_of(200, 4))
    check("iid gamma", hR.smooth(y)[0], want, rtol_of(200, 4))


def test_emissions_are_scale_free_and_missing_rows_are_ones():
    A, p0, y, _ = H.random_case(300, 3, seed=2)
    hmm = host(A, p0)
    c = np.exp(np.random.default_rng(1).normal(0, 20, size=(300, 1)))
    a1, L1, _ = hmm.filter(y)
    a2, L2, _ = hmm.filter(y * c)
    check("scaled rows: alpha", a2, a1, rtol_of(300, 3))
    check("scaled rows: loglik", L2 - np.log(c).sum(), L1, 0, loglik_atol(300, 3, np.abs(L2) + np.abs(np.log(c)).sum()))
    assert np.array_equal(hmm.viterbi(y * c)[0], hmm.viterbi(y)[0])
    ym = y.copy()
    ym[[0, 17, 299]] = [[0, 0, 0], [0.2, -0.1, 0.9], [0.1, np.inf, 0.1]]
    y1 = y.copy()
    y1[[0, 17, 299]] = 1.0
    assert np.array_equal(hmm.smooth(ym)[0], hmm.smooth(y1)[0])


def test_helpers():
    from pinn_amd import temporal
    A = temporal.sticky_transitions(4, 0.97)
    assert A.shape == (4, 4) and np.allclose(A.sum(axis=1), 1.0) and np.allclose(np.diag(A), 0.97) and np.allclose(A[0, 1], 0.01)
    assert np.array_equal(temporal.sticky_transitions(1), np.ones((1, 1)))
    y = np.array([0, 0, 1, 1, 1, 2, 0, 0])
    T = temporal.transitions_from_labels(y, 3, seg_starts=[0, 6], pseudo_count=0.0)
    # 2 -> 0 crosses the segment start and is not counted, which leaves state 2 without a count: a uniform row
    assert np.allclose(T, [[2 / 3, 1 / 3, 0], [0, 2 / 3, 1 / 3], [1 / 3, 1 / 3, 1 / 3]])
    assert np.allclose(temporal.transitions_from_labels(y, 3, pseudo_count=1.0).sum(axis=1), 1.0)
    assert np.allclose(temporal.scaled_likelihood(np.array([[0.2, 0.8]]), [0.5, 0.25]), [[0.4, 3.2]])
    import pinn_amd
    assert pinn_amd.DeviceHMM is temporal.DeviceHMM and pinn_amd.TemporalDiagnoser is temporal.TemporalDiagnoser
    with pytest.raises(ValueError):
        temporal.DeviceHMM(np.ones((3, 3)))
    with pytest.raises(ValueError):
        temporal.DeviceHMM(np.eye(9))
    with pytest.raises(ValueError):
        host(np.eye(2)).filter(np.ones((4, 3)))
    with pytest.raises(ValueError):
        host(np.eye(2)).filter(np.ones((4, 2)), seg_starts=[1, 2])


def chunked(hmm, y, chunk):
    """filter and viterbi over consecutive chunks through the carry -> alpha, loglik, path, logprob, the last carries"""
    cf = cv = None
    alphas, paths = [], []
    for lo in range(0, len(y), chunk):
        a, L, cf = hmm.filter(y[lo:lo + chunk], carry_in=cf)
        p, lp, cv = hmm.viterbi(y[lo:lo + chunk], carry_in=cv, return_carry=True)
        alphas.append(a)
        paths.append(p)
    return alphas, L, paths, lp, cf, cv


def chunked_path_by_definition(vit, n, chunk):
    """What a chunked Viterbi returns, from the whole series' scores and backpointers: per chunk, the trace back from the
    lowest arg-max of the scores at the chunk's last row."""
    out = np.zeros(n, dtype=np.int64)
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        s = int(np.argmax(vit["delta"][hi - 1]))
        out[hi - 1] = s
        for t in range(hi - 1, lo, -1):
            s = vit["psi"][t, s]
            out[t - 1] = s
    return out


@pytest.mark.parametrize("chunk", [1, 100, 1024, 1976])
def test_chunks_through_the_carry_equal_the_whole_series(chunk):
    from pinn_amd import temporal
    n, S = 4000, 3
    A, p0, y, _ = H.random_case(n, S, seed=21)
    hmm = host(A, p0)
    alpha, L, _ = hmm.filter(y)
    vit = H.sequential_viterbi(H.emissions(y), A, p0)
    alphas, Lc, paths, lpc, cf, cv = chunked(hmm, y, chunk)
    check("chunked alpha", np.concatenate(alphas), alpha, rtol_of(n, S), ATOL)
    check("chunked loglik", Lc, L, 0, loglik_atol(n, S, L))
    check("chunked logprob", lpc, vit["logprob"], 0, logprob_atol(n, vit["delta"]))
    check("carried scores", cv[0, S + 1:], vit["delta"][-1], 0, logprob_atol(n, vit["delta"]))
    assert np.array_equal(np.concatenate(paths), chunked_path_by_definition(vit, n, chunk))
    mon = temporal.TemporalDiagnoser(hmm)
    got = [mon.update(y[lo:lo + chunk]) for lo in range(0, n, chunk)]
    check("online alpha", np.concatenate([g[0] for g in got]), alpha, rtol_of(n, S), ATOL)
    labels = np.concatenate([g[1] for g in got])
    assert np.array_equal(labels, alpha.argmax(axis=1)) and mon.n_seen == n and mon.switches == H.switches(labels)
    mon.reset()
    assert mon.n_seen == 0 and mon.switches == 0


def test_online_diagnoser_takes_rows_through_a_source():
    from pinn_amd import temporal

    class Source:
        def update(self, rows):
            p = rows[:, 2:5] / rows[:, 2:5].sum(axis=1, keepdims=True)
            return p, p.argmax(axis=1)

    A, p0, y, _ = H.random_case(500, 3, seed=4)
    rows = np.concatenate([np.zeros((500, 2)), 3.0 * y], axis=1)
    hmm = host(A, p0)
    mon = temporal.TemporalDiagnoser(hmm, source=Source())
    got = np.concatenate([mon.update(rows[lo:lo + 128])[0] for lo in range(0, 500, 128)])
    check("through a source", got, hmm.filter(y)[0], rtol_of(500, 3), ATOL)


# ---------------------------------------------------------------------------------------------- fitting
@functools.lru_cache(maxsize=None)
def recovery():
    return H.recovery_case()


@functools.lru_cache(maxsize=None)
def host_fit(n_iter=12):
    from pinn_amd import temporal
    A_true, p0, y, x, seg = recovery()
    return host(temporal.sticky_transitions(3, 0.9), p0).fit_transitions(y, seg_starts=seg, n_iter=n_iter, tol=0.0)


def test_log_likelihood_history_never_decreases_and_first_rises():
    _, _, y, _, _ = recovery()
    fit = host_fit()
    hist = fit.loglik_history_
    print("history", hist)
    assert fit.n_iter_ == 12 and len(hist) == 12 and not fit.converged_
    gate = loglik_atol(len(y), 3, hist)
    assert np.all(np.diff(hist) >= -gate)
    assert np.all(np.diff(hist[:4]) > gate)


def test_fit_recovers_the_sampled_chain():
    A_true, _, _, x, _ = recovery()
    fit = host_fit()
    visits = np.bincount(x, minlength=3)
    d = np.diag(A_true)
    se = np.sqrt(d * (1 - d) / visits)
    z = (np.diag(fit.transitions_) - d) / se
    print("fitted diagonal", np.diag(fit.transitions_), "z", z)
    assert np.all(np.abs(z) <= 5.0)
    assert np.allclose(fit.transitions_.sum(axis=1), 1.0, atol=1e-12)


def early_stop_tol(hist):
    """A tolerance that no gain of the history lies within a factor 2 of, between the 3rd and the last gain."""
    gains = np.abs(np.diff(hist))
    for k in range(3, len(gains)):
        tol = np.sqrt(gains[k - 1] * gains[k])
        if np.all((gains > 2 * tol) | (gains < tol / 2)):
            return tol
    raise AssertionError("no such tolerance: %s" % gains)


def test_early_stop_follows_the_gain_rule():
    from pinn_amd import temporal
    _, p0, y, _, seg = recovery()
    full = host_fit()
    tol = early_stop_tol(full.loglik_history_)
    gains = np.abs(np.diff(full.loglik_history_))
    k = int(np.flatnonzero(gains < tol)[0]) + 2          # the iteration whose gain is the first below tol
    fit = host(temporal.sticky_transitions(3, 0.9), p0).fit_transitions(y, seg_starts=seg, n_iter=12, tol=tol)
    print("tol", tol, "gains", gains, "stopped after", fit.n_iter_)
    assert fit.converged_ and fit.n_iter_ == k and len(fit.loglik_history_) == k
    assert np.array_equal(fit.loglik_history_, full.loglik_history_[:k])


def test_zeros_stay_zero_and_pseudo_counts_enter():
    A, p0, y, _ = H.random_case(600, 4, seed=8, A=H.left_to_right(4, 0.9))
    fit = host(A, p0).em_iterations(y, 3)
    assert np.array_equal(fit.transitions_ == 0.0, A == 0.0) and fit.transitions_[3, 3] == 1.0 and fit.n_iter_ == 3
    xi, _, _ = host(A, p0).expected_counts(y)
    one = host(A, p0).em_iterations(y, 1, pseudo_count=2.0)
    cnt = np.where(A > 0, xi + 2.0, 0.0)
    check("pseudo-counts", one.transitions_, cnt / cnt.sum(axis=1, keepdims=True), 1e-15)


def test_what_smoothing_buys():
    """README's claim: on the sampled chain the smoothed and the Viterbi labels make fewer errors and fewer switches than the
    per-row arg-max, and the filtered labels no more errors."""
    A_true, p0, y, x, seg = recovery()
    hmm = host(A_true, p0)
    per_row = y.argmax(axis=1)
    labels = {"per row": per_row, "filtered": hmm.filter(y, seg_starts=seg)[0].argmax(axis=1),
              "smoothed": hmm.smooth(y, seg_starts=seg)[0].argmax(axis=1), "viterbi": hmm.viterbi(y, seg_starts=seg)[0]}
    err = {k: int(np.count_nonzero(v != x)) for k, v in labels.items()}
    sw = {k: H.switches(v) for k, v in labels.items()}
    print("errors", err, "switches", sw, "true switches", H.switches(x))
    assert err["smoothed"] < err["per row"] and err["viterbi"] < err["per row"] and err["filtered"] <= err["per row"]
    assert sw["smoothed"] < sw["per row"] and sw["viterbi"] < sw["per row"]
