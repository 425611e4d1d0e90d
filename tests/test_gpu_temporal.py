"""GPU: the device backend of pinn_amd.temporal (csrc/pinn_hmm.hip) against the package's host backend (sequential float64
recursions, itself held to two referees in test_temporal_host.py).

Gates (hmm_cases.py; derived from the arithmetic, not from what the kernels give): alpha, gamma, xi and the fitted
A after one iteration rtol 4 n (S + 2) u with atol 1e-290; log-likelihoods atol 4 n (S + 2) u + 4 u |L|; paths exact, under a
condition on the inputs that is checked on the host run first: every arg-max decision of the sequential Viterbi has a margin of
at least 4 n u max |delta|.  Every comparison prints its maxima before it asserts.  T is the scan tile, R a thread's rows."""
import numpy as np
import pytest
import torch

import hmm_cases as H
from hmm_cases import check, logprob_atol, loglik_atol, rtol_of
from test_temporal_host import ATOL, check_identities, chunked, chunked_path_by_definition, compare_all, early_stop_tol, host, host_fit, recovery

pytestmark = pytest.mark.gpu

T, R = 1024, 16


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device(A, p0=None, prior=None):
    from pinn_amd import temporal
    assert (temporal.TILE, temporal.ROWS_PER_THREAD) == (T, R)
    return temporal.DeviceHMM(A, p0, prior, backend="device")


def host_reference(A, p0, y, seg=None, prior=None):
    """The host backend's outputs as compare_all wants them, and its path with the margin condition checked."""
    hmm = host(A, p0, prior)
    alpha, L, _ = hmm.filter(y, seg_starts=seg)
    gamma, _ = hmm.smooth(y, seg_starts=seg)
    xi, gsum, _ = hmm.expected_counts(y, seg_starts=seg)
    path, lp = hmm.viterbi(y, seg_starts=seg)
    vit = H.sequential_viterbi(H.emissions(y, prior), A, p0, seg)
    need = H.path_margin_needed(len(y), vit["delta"])
    print("arg-max margin %.3e, needed %.3e" % (vit["margin"], need))
    assert vit["margin"] >= need, "the case does not satisfy the margin condition: choose another seed"
    assert np.array_equal(vit["path"], path)
    return {"alpha": alpha, "gamma": gamma, "xi": xi, "gamma_sum": gsum, "loglik": L, "path": path, "logprob": lp}


def compare_device(tag, A, p0, y, seg=None, prior=None):
    n, S = y.shape
    want = host_reference(A, p0, y, seg, prior)
    d = device(A, p0, prior)
    yd = dev(y)
    alpha, gamma, xi, gsum = compare_all(tag, d, yd, want, n, S, seg)
    check_identities(tag, alpha, gamma, xi, gsum, n, S, seg)
    path, lp = d.viterbi(yd, seg_starts=seg)
    assert path.is_cuda and path.dtype == torch.int64
    check(tag + " logprob", lp.cpu().numpy(), want["logprob"], 0, logprob_atol(n, want["logprob"]))
    mism = np.flatnonzero(path.cpu().numpy() != want["path"])
    print(tag + " path mismatches", mism.size)
    assert mism.size == 0, mism[:10]
    return d, yd


@pytest.mark.parametrize("n", [1, 2, R - 1, R, R + 1, T - 1, T, T + 1, 2 * T + 1, 5 * T + 3])
def test_device_matches_host_at_every_size_and_state_count(n):
    for S in (1, 2, 3, 5, 8):
        A, p0, y, _ = H.random_case(n, S, seed=100 + S)
        compare_device("n=%d S=%d" % (n, S), A, p0, y)


SEGMENTS = {
    "row 0 only": [0],
    "every row": list(range(2 * T + 1)),
    "tile edges": [0, T, 2 * T],
    "T-1 and T+1": [0, T - 1, T + 1],
    "inside the last thread's run": [0, T - 5, T - 2, 2 * T - 1],
}


@pytest.mark.parametrize("name", list(SEGMENTS))
def test_segment_starts(name):
    n, S, seg = 2 * T + 1, 3, SEGMENTS[name]
    A, p0, y, _ = H.random_case(n, S, seed=31, seg_starts=seg)
    prior = np.array([0.5, 0.3, 0.2])
    compare_device(name, A, p0, y, seg, prior)


def test_structural_zeros_and_missing_rows():
    n, S = 5 * T + 3, 4
    A, p0, y, _ = H.random_case(n, S, seed=12, A=H.left_to_right(S, 0.999))
    compare_device("left-to-right", A, p0, y)
    seg = [0, 700, T, 3000]
    A, p0, y, _ = H.random_case(n, 3, seed=13, seg_starts=seg)
    y[700] = 0.0                                    # at a segment start
    y[T - 1:T + 1] = np.nan                         # at a tile edge
    y[T + 500:4 * T + 500] = [0.3, -1.0, 0.2]       # a run of 3 T rows
    compare_device("missing rows", A, p0, y, seg)


def test_exponent_bookkeeping_over_3000_rows_of_extreme_ratios():
    """Emissions with ratios of 1e-30 between states over 3000 consecutive rows: unscaled products would underflow by tens of
    thousands of decades.  The sequential referee (per-step normalisation) and the device must agree on the log-likelihood."""
    n, S = 3 * T + 7, 4
    rng = np.random.default_rng(17)
    A, p0, y, x = H.random_case(n, S, seed=17)
    y[40:3040] = np.where(np.arange(S)[None, :] == x[40:3040, None], 1.0, 1e-30) * 10.0 ** rng.integers(-40, 0, size=(3000, 1))
    d, yd = compare_device("1e-30 ratios", A, p0, y)
    ref = H.sequential(H.emissions(y), A, p0)
    _, L, _ = d.filter(yd)
    print("log-likelihood", float(L[0]), "referee", float(ref["loglik"][0]))
    assert float(ref["loglik"][0]) < -40000.0
    check("log-likelihood against the referee", L.cpu().numpy(), ref["loglik"], 0, loglik_atol(n, S, ref["loglik"]))


@pytest.mark.parametrize("chunk", [1, 100, T, T + 952])
def test_chunks_through_the_carry_equal_the_whole_series(chunk):
    from pinn_amd import temporal
    n, S = 2500, 3
    A, p0, y, _ = H.random_case(n, S, seed=21)
    want = host_reference(A, p0, y)
    vit = H.sequential_viterbi(H.emissions(y), A, p0)
    d, yd = device(A, p0), dev(y)
    alphas, Lc, paths, lpc, cf, cv = chunked(d, yd, chunk)
    assert cf.is_cuda and cv.is_cuda
    check("chunked alpha", torch.cat(alphas).cpu().numpy(), want["alpha"], rtol_of(n, S), ATOL)
    check("chunked loglik", Lc.cpu().numpy(), want["loglik"], 0, loglik_atol(n, S, want["loglik"]))
    check("chunked logprob", lpc.cpu().numpy(), want["logprob"], 0, logprob_atol(n, want["logprob"]))
    check("carried scores", cv[0, S + 1:].cpu().numpy(), vit["delta"][-1], 0, logprob_atol(n, vit["delta"]))
    assert np.array_equal(torch.cat(paths).cpu().numpy(), chunked_path_by_definition(vit, n, chunk))
    # the online form over the same chunks against one filter call
    mon = temporal.TemporalDiagnoser(d)
    got = [mon.update(yd[lo:lo + chunk]) for lo in range(0, n, chunk)]
    whole = d.filter(yd)[0]
    check("online alpha", torch.cat([g[0] for g in got]).cpu().numpy(), whole.cpu().numpy(), rtol_of(n, S), ATOL)
    labels = torch.cat([g[1] for g in got]).cpu().numpy()
    assert mon.n_seen == n and mon.switches == H.switches(labels)
    assert np.array_equal(labels, torch.cat([g[0] for g in got]).argmax(1).cpu().numpy())


def test_rows_read_in_place_equal_the_packed_copy():
    n, S = 2 * T + 1, 5
    A, p0, y, _ = H.random_case(n, S, seed=9)
    wide = np.random.default_rng(1).normal(size=(n, 3 + S + 2))
    wide[:, 3:3 + S] = y
    order = np.arange(n)
    order[T - 40:T + 60] = order[T - 40:T + 60][::-1].copy()     # a gather list that reverses a block across a tile edge
    d = device(A, p0)
    packed = dev(y[order])
    kw = dict(columns=list(range(3, 3 + S)), row_index=order)
    for name, a, b in (("filter", d.filter(dev(wide), **kw), d.filter(packed)), ("smooth", d.smooth(dev(wide), **kw), d.smooth(packed)),
                       ("viterbi", d.viterbi(dev(wide), **kw), d.viterbi(packed)),
                       ("counts", d.expected_counts(dev(wide), **kw), d.expected_counts(packed))):
        for u, v in zip(a, b):
            assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), name


def test_same_call_twice_gives_the_same_bytes_and_numpy_gives_numpy():
    n, S = 5 * T + 3, 8
    seg = [0, 1500, 4000]
    A, p0, y, _ = H.random_case(n, S, seed=3, seg_starts=seg)
    d, yd = device(A, p0), dev(y)
    calls = (lambda v: d.filter(v, seg_starts=seg), lambda v: d.smooth(v, seg_starts=seg), lambda v: d.viterbi(v, seg_starts=seg),
             lambda v: d.expected_counts(v, seg_starts=seg))
    for f in calls:
        first, second, plain = f(yd), f(yd), f(y)
        for u, v, w in zip(first, second, plain):
            assert isinstance(w, np.ndarray) and u.is_cuda
            assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes() == w.tobytes()


# ---------------------------------------------------------------------------------------------- fitting
def test_one_em_iteration_matches_the_host():
    from pinn_amd import temporal
    _, p0, y, _, seg = recovery()
    n, S = y.shape
    A0 = temporal.sticky_transitions(3, 0.9)
    h = host(A0, p0).em_iterations(y, 1, seg_starts=seg)
    d = device(A0, p0).em_iterations(dev(y), 1, seg_starts=seg)
    check("A after one iteration", d.transitions_, h.transitions_, rtol_of(n, S), ATOL)
    check("its log-likelihood", d.loglik_history_, h.loglik_history_, 0, loglik_atol(n, S, h.loglik_history_))
    assert d.n_iter_ == 1 and not d.converged_
    A4, p4, y4, _ = H.random_case(3000, 4, seed=8, A=H.left_to_right(4, 0.99))
    pc = np.full((4, 4), 0.5)
    h4 = host(A4, p4).em_iterations(y4, 1, pseudo_count=pc)
    d4 = device(A4, p4).em_iterations(dev(y4), 1, pseudo_count=pc)
    check("zeros and pseudo-counts", d4.transitions_, h4.transitions_, rtol_of(3000, 4), ATOL)
    assert np.array_equal(d4.transitions_ == 0.0, A4 == 0.0)


def test_device_fit_recovers_the_chain_and_its_history_never_decreases():
    from pinn_amd import temporal
    A_true, p0, y, x, seg = recovery()
    fit = device(temporal.sticky_transitions(3, 0.9), p0).fit_transitions(dev(y), seg_starts=seg, n_iter=12, tol=0.0)
    hist = fit.loglik_history_
    print("history", hist)
    gate = loglik_atol(len(y), 3, hist)
    assert fit.n_iter_ == 12 and len(hist) == 12 and np.all(np.diff(hist) >= -gate) and np.all(np.diff(hist[:4]) > gate)
    dg = np.diag(A_true)
    z = (np.diag(fit.transitions_) - dg) / np.sqrt(dg * (1 - dg) / np.bincount(x, minlength=3))
    print("fitted diagonal", np.diag(fit.transitions_), "z", z)
    assert np.all(np.abs(z) <= 5.0)


def test_device_fit_lies_within_the_fits_own_float64_noise_of_the_host_fit():
    """EM amplifies a perturbation by an unknown factor per iteration, so the distance between two fits cannot be derived:
    it is measured.  d = the largest entrywise difference between the sequential referee's fit in np.longdouble and in
    float64; the device must lie within 16 d of the host backend's fit (the factor allows for the scan tree's other
    association order)."""
    from pinn_amd import temporal
    _, p0, y, _, _ = recovery()
    y, n_iter = y[:4000], 4
    A0 = temporal.sticky_transitions(3, 0.9)
    b = H.emissions(y)
    A_ld, _ = H.referee_fit(b, A0, p0, None, n_iter, np.longdouble)
    A_64, _ = H.referee_fit(b, A0, p0, None, n_iter, np.float64)
    noise = float(np.max(np.abs(A_ld - A_64.astype(np.longdouble))))
    h = host(A0, p0).fit_transitions(y, n_iter=n_iter, tol=0.0)
    d = device(A0, p0).fit_transitions(dev(y), n_iter=n_iter, tol=0.0)
    dist = float(np.max(np.abs(d.transitions_ - h.transitions_)))
    print("float64 noise of the fit d = %.3e, device to host %.3e, host to float64 referee %.3e" %
          (noise, dist, np.max(np.abs(h.transitions_ - A_64))))
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 here"
    assert h.n_iter_ == d.n_iter_ == n_iter and dist <= 16.0 * noise


def test_early_stop_agrees_with_the_host_and_later_launches_do_nothing():
    from pinn_amd import temporal
    _, p0, y, _, seg = recovery()
    full = host_fit()
    tol = early_stop_tol(full.loglik_history_)
    h = host(temporal.sticky_transitions(3, 0.9), p0).fit_transitions(y, seg_starts=seg, n_iter=12, tol=tol)
    d = device(temporal.sticky_transitions(3, 0.9), p0).fit_transitions(dev(y), seg_starts=seg, n_iter=12, tol=tol)
    print("tol", tol, "host stopped after", h.n_iter_, "device after", d.n_iter_)
    assert h.converged_ and d.converged_ and d.n_iter_ == h.n_iter_ < 12
    assert len(d.loglik_history_) == d.n_iter_ and np.all(d._history_room[d.n_iter_:] == 0.0)
    print("history, device - host", d.loglik_history_ - h.loglik_history_)
