"""Shared by test_temporal_host.py and test_gpu_temporal.py: case builders, the gates and two referees that do not use the
package: (1) brute-force enumeration of all S^n state paths, exact marginals for tiny cases; (2) a sequential forward-backward
and Viterbi written straight from the recursions, in any numpy float type, the referee at length.

Gates, from the arithmetic: every quantity is a product or sum of non-negative numbers, one S x S combine
carries at most (S + 1) u per entry (u = 2^-53), a prefix of t rows at most t (S + 1) u in any association order.
rtol = 4 n (S + 2) u covers both sides and the final normalisation; atol 1e-290 for entries the power-of-two scaling lets
underflow; log-likelihood atol = 4 n (S + 2) u + 4 u |L|; Viterbi scores atol = 4 n u max |score| (logprob_atol)."""
import functools
import itertools

import numpy as np

U = 2.0 ** -53


def rtol_of(n, S):
    return 4.0 * n * (S + 2) * U


def loglik_atol(n, S, L):
    return rtol_of(n, S) + 4.0 * U * float(np.max(np.abs(L)))


def logprob_atol(n, scores):
    """Viterbi scores are sums of 2 n logarithms added one by one: each addition rounds by at most u max |score|, on either
    side, and the logarithms themselves by an ulp of theirs: 4 n u max |score|, the margin the exact path asks for."""
    scores = np.asarray(scores, dtype=float)
    finite = scores[np.isfinite(scores)]
    return 4.0 * n * U * float(np.max(np.abs(finite))) if finite.size else 0.0


def check(tag, got, want, rtol=0.0, atol=0.0):
    """Prints the maxima, then asserts |got - want| <= atol + rtol |want| elementwise (NaN never passes)."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if got.size == 0:
        return
    err = np.abs(got - want)
    rel = err / np.maximum(np.abs(want), 1e-300)
    print("%-34s max abs %.3e  max rel %.3e  (rtol %.3e atol %.3e)" % (tag, np.nanmax(err), np.nanmax(rel), rtol, atol))
    assert np.all(err <= atol + rtol * np.abs(want)), tag


def emissions(y_prob, prior=None):
    """The emission rule, restated: y / prior; a row that is all zero or holds a negative or non-finite value is all ones."""
    b = np.array(y_prob, dtype=float)
    if prior is not None:
        b = b / np.asarray(prior, dtype=float)[None, :]
    for t in range(b.shape[0]):
        r = b[t]
        if not np.all(np.isfinite(r)) or np.any(r < 0) or not np.any(r > 0):
            b[t] = 1.0
    return b


def bounds_of(seg_starts, n):
    starts = [0] if seg_starts is None or len(seg_starts) == 0 else [int(s) for s in seg_starts]
    return list(zip(starts, starts[1:] + [n]))


# ---------------------------------------------------------------------------------------------- referee 1: enumeration
def brute_force(b, A, p0):
    """One segment of n rows: dict with alpha [n, S], gamma [n, S], loglik, xi [S, S], path, path_logprob."""
    n, S = b.shape
    paths = list(itertools.product(range(S), repeat=n))

    def weight(p, upto):
        w = p0[p[0]] * b[0, p[0]]
        for t in range(1, upto):
            w *= A[p[t - 1], p[t]] * b[t, p[t]]
        return w

    w = np.array([weight(p, n) for p in paths])
    Z = w.sum()
    gamma, xi, alpha = np.zeros((n, S)), np.zeros((S, S)), np.zeros((n, S))
    for p, wp in zip(paths, w):
        for t in range(n):
            gamma[t, p[t]] += wp / Z
        for t in range(n - 1):
            xi[p[t], p[t + 1]] += wp / Z
    for t in range(n):
        for p in itertools.product(range(S), repeat=t + 1):
            alpha[t, p[t]] += weight(p, t + 1)
        alpha[t] /= alpha[t].sum()
    best = int(np.argmax(w))
    order = np.sort(w)
    assert order[-1] > order[-2] * (1 + 1e-9), "the case must have a unique best path"
    return {"alpha": alpha, "gamma": gamma, "loglik": np.log(Z), "xi": xi, "path": np.array(paths[best]), "path_logprob": np.log(w[best])}


# ---------------------------------------------------------------------------------------------- referee 2: sequential
def sequential(b, A, p0, seg_starts=None, dtype=np.float64):
    """Forward-backward with per-step normalisation, in `dtype`: alpha, gamma, loglik [n_seg], xi, gamma_sum."""
    b, A, p0 = np.asarray(b, dtype=dtype), np.asarray(A, dtype=dtype), np.asarray(p0, dtype=dtype)
    n, S = b.shape
    alpha, beta, gamma = np.zeros((n, S), dtype), np.zeros((n, S), dtype), np.zeros((n, S), dtype)
    xi, gsum, loglik = np.zeros((S, S), dtype), np.zeros(S, dtype), []
    for lo, hi in bounds_of(seg_starts, n):
        L = dtype(0)
        for t in range(lo, hi):
            a = p0 * b[t] if t == lo else (alpha[t - 1] @ A) * b[t]        # alpha_t(j) = sum_i alpha_{t-1}(i) A(i, j) b_t(j)
            c = a.sum()
            alpha[t] = a / c
            L += np.log(c)
        loglik.append(L)
        beta[hi - 1] = 1
        for t in range(hi - 2, lo - 1, -1):
            x = A @ (b[t + 1] * beta[t + 1])                               # beta_t(i) = sum_j A(i, j) b_{t+1}(j) beta_{t+1}(j)
            beta[t] = x / x.sum()
        for t in range(lo, hi):
            g = alpha[t] * beta[t]
            gamma[t] = g / g.sum()
        for t in range(lo, hi - 1):
            x = alpha[t][:, None] * A * (b[t + 1] * beta[t + 1])[None, :]
            xi += x / x.sum()
            gsum += gamma[t]
    return {"alpha": alpha, "gamma": gamma, "loglik": np.array(loglik, dtype), "xi": xi, "gamma_sum": gsum}


def sequential_viterbi(b, A, p0, seg_starts=None):
    """Log-domain Viterbi, the lowest maximising state on ties: path, logprob [n_seg], delta [n, S] and the smallest margin
    of any arg-max decision it took (backpointers and segment-end states; inf when no decision had a runner-up)."""
    n, S = b.shape
    with np.errstate(divide="ignore"):
        lA, lb, lp0 = np.log(A), np.log(b), np.log(p0)
    delta, psi, path, logprob = np.zeros((n, S)), np.zeros((n, S), dtype=np.int64), np.zeros(n, dtype=np.int64), []
    margin = np.inf

    def decide(v):
        nonlocal margin
        k = 0
        for i in range(1, len(v)):
            if v[i] > v[k]:
                k = i
        rest = [v[i] for i in range(len(v)) if i != k and np.isfinite(v[i])]
        if rest and np.isfinite(v[k]):
            margin = min(margin, v[k] - max(rest))
        return k

    for lo, hi in bounds_of(seg_starts, n):
        delta[lo] = lp0 + lb[lo]
        for t in range(lo + 1, hi):
            for j in range(S):
                v = [delta[t - 1, i] + lA[i, j] for i in range(S)]
                psi[t, j] = decide(v)
                delta[t, j] = v[psi[t, j]] + lb[t, j]
        s = decide(list(delta[hi - 1]))
        logprob.append(delta[hi - 1, s])
        path[hi - 1] = s
        for t in range(hi - 1, lo, -1):
            s = psi[t, s]
            path[t - 1] = s
    return {"path": path, "logprob": np.array(logprob), "delta": delta, "psi": psi, "margin": margin}


def path_margin_needed(n, delta):
    """m = 4 n u max |delta|: below it a rounding difference between two association orders could flip an arg-max."""
    return logprob_atol(n, delta)


def referee_fit(b, A0, p0, seg_starts, n_iter, dtype=np.float64):
    """n_iter Baum-Welch iterations for the transitions with the sequential referee in `dtype` (no pseudo-counts)."""
    A = np.asarray(A0, dtype=dtype)
    hist = []
    for _ in range(n_iter):
        r = sequential(b, A, p0, seg_starts, dtype)
        hist.append(r["loglik"].sum())
        cnt = np.where(A > 0, r["xi"], 0)
        tot = cnt.sum(axis=1, keepdims=True)
        A = np.where(tot > 0, cnt / np.where(tot > 0, tot, 1), A)
    return A, np.array(hist)


# ---------------------------------------------------------------------------------------------- cases
def random_transitions(S, rng, stay=0.9):
    A = rng.random((S, S)) + 0.05
    A = (1 - stay) * A / A.sum(axis=1, keepdims=True) + stay * np.eye(S)
    return A / A.sum(axis=1, keepdims=True)


def left_to_right(S, stay=0.97):
    """A chain with structural zeros: state i stays or moves to i + 1, the last state absorbs."""
    A = np.zeros((S, S))
    for i in range(S - 1):
        A[i, i], A[i, i + 1] = stay, 1 - stay
    A[S - 1, S - 1] = 1.0
    return A


def sample_chain(n, A, p0, seg_starts, rng):
    S = A.shape[0]
    x = np.zeros(n, dtype=np.int64)
    for lo, hi in bounds_of(seg_starts, n):
        x[lo] = rng.choice(S, p=p0)
        for t in range(lo + 1, hi):
            x[t] = rng.choice(S, p=A[x[t - 1]])
    return x


def noisy_posteriors(x, S, rng, strength=1.2, noise=1.0):
    """Per-row class posteriors of a noisy classifier: softmax(strength onehot(x) + noise N(0, 1))."""
    z = noise * rng.normal(size=(x.size, S))
    z[np.arange(x.size), x] += strength
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def random_case(n, S, seed, seg_starts=None, A=None):
    rng = np.random.default_rng(seed)
    A = random_transitions(S, rng) if A is None else A
    p0 = rng.random(S) + 0.2
    if A[0, -1] == 0.0 and S > 1:                   # a left-to-right chain begins in its first state
        p0 = np.zeros(S)
        p0[0] = 1.0
    p0 = p0 / p0.sum()
    x = sample_chain(n, A, p0, seg_starts, rng)
    return A, p0, noisy_posteriors(x, S, rng), x


TRUE_A3 = np.array([[0.98, 0.015, 0.005], [0.01, 0.98, 0.01], [0.004, 0.016, 0.98]])
RECOVERY_N, RECOVERY_SEGS, RECOVERY_SEED = 20000, [0, 9000], 7


@functools.lru_cache(maxsize=None)
def recovery_case():
    """The sampled chain of the fitting tests: 20 000 rows, S = 3, diagonal 0.98, two segments, informative but noisy
    emissions.  Returns A_true, p0, y_prob, states, seg_starts."""
    rng = np.random.default_rng(RECOVERY_SEED)
    p0 = np.full(3, 1.0 / 3)
    x = sample_chain(RECOVERY_N, TRUE_A3, p0, RECOVERY_SEGS, rng)
    return TRUE_A3, p0, noisy_posteriors(x, 3, rng, strength=2.0), x, RECOVERY_SEGS


def switches(labels):
    labels = np.asarray(labels)
    return int(np.count_nonzero(labels[1:] != labels[:-1]))
