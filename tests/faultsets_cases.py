"""Case builders shared by the fault-set tests (host and GPU): posteriors with known classes, the rows a ranking can get
wrong (ties, missing rows, empty classes), a fitted mixture with a far cluster, and the referees simpler than the module."""
import math
from fractions import Fraction

import numpy as np

KINDS = ("lac", "margin", "aps")


def posteriors(n, C, seed, quantise=None, alpha=1.0):
    """y_prob [n, C] from a Dirichlet law and a class drawn from each row, so that the rows of a class are exchangeable.
    quantise=q rounds every entry to a multiple of 1 / q (most scores then tie; an all-zero row is given to class 0)."""
    rng = np.random.default_rng(seed)
    P = rng.dirichlet(np.full(C, alpha), size=n)
    if quantise:
        P = np.round(P * quantise) / quantise
        P[~(P > 0).any(axis=1), 0] = 1.0 / quantise
    cum = np.cumsum(P / P.sum(axis=1, keepdims=True), axis=1)
    y = np.minimum((rng.random(n)[:, None] > cum).sum(axis=1), C - 1).astype(np.int64)
    return P, y


def spoil(P, seed, share=0.1):
    """Missing rows of every kind: NaN, +inf, a negative entry, all zeros."""
    rng = np.random.default_rng(seed)
    P = P.copy()
    idx = rng.choice(P.shape[0], size=max(4, int(P.shape[0] * share)), replace=P.shape[0] < 4)
    for i, j in enumerate(idx):
        k = i % 4
        if k == 0: P[j, rng.integers(P.shape[1])] = np.nan
        elif k == 1: P[j, rng.integers(P.shape[1])] = np.inf
        elif k == 2: P[j, rng.integers(P.shape[1])] = -0.25
        else: P[j] = 0.0
    return P, np.sort(np.unique(idx))


def with_class_sizes(sizes, C, seed, quantise=None):
    """Calibration posteriors in which class c has exactly sizes[c] rows (shuffled)."""
    rng = np.random.default_rng(seed)
    rows, ys = [], []
    for c, m in enumerate(sizes):
        P, _ = posteriors(m, C, seed + 17 * c + 1, quantise)
        rows.append(P)
        ys.append(np.full(m, c, np.int64))
    P, y = np.concatenate(rows), np.concatenate(ys)
    perm = rng.permutation(P.shape[0])
    return P[perm], y[perm]


def brute_scores(P, kind, u=None):
    """The scores by the definition's own words, one row and class at a time."""
    n, C = P.shape
    S = np.full((n, C), np.nan)
    for i in range(n):
        p = P[i]
        if not all(math.isfinite(v) and v >= 0 for v in p) or not any(v > 0 for v in p):
            continue
        for c in range(C):
            if kind == "lac":
                S[i, c] = 1.0 - p[c]
            elif kind == "margin":
                S[i, c] = -p[c] if C == 1 else max(p[k] for k in range(C) if k != c) - p[c]
            else:
                acc = 0.0
                for k in range(C):
                    if p[k] > p[c] or (p[k] == p[c] and k < c):
                        acc = acc + p[k]
                S[i, c] = acc + (1.0 if u is None else u[i]) * p[c]
    return S


def brute_counts(tables, S):
    """count [n, C] by a double loop over the calibration scores (-1 on rows whose scores are NaN)."""
    n, C = S.shape
    out = np.full((n, C), -1, np.int32)
    for i in range(n):
        if np.isnan(S[i]).any():
            continue
        for c in range(C):
            out[i, c] = sum(1 for t in tables[c].tolist() if t >= S[i, c])
    return out


def brute_tables(S, y, C):
    return [np.array(sorted(float(S[i, c]) + 0.0 for i in range(S.shape[0]) if y[i] == c and not np.isnan(S[i, c]))) for c in range(C)]


def kmin_exact(n_c, level):
    return math.floor((1 - Fraction(float(level))) * (n_c + 1))


def hits_region(m, n_c, kmin, mass=Fraction(1, 10 ** 6)):
    """[lo, hi]: the central region of the hits among m fresh exchangeable rows, each tail of mass at most `mass` / 2.  The
    coverage given the calibration is Beta(n_c + 1 - kmin, kmin), so the hits are beta-binomial:
    P(h) = C(h + a - 1, h) C(m - h + b - 1, m - h) / C(m + a + b - 1, m) with a = n_c + 1 - kmin, b = kmin."""
    a, b = n_c + 1 - kmin, kmin
    den = math.comb(m + a + b - 1, m)
    pmf = [Fraction(math.comb(h + a - 1, h) * math.comb(m - h + b - 1, m - h), den) for h in range(m + 1)]
    assert sum(pmf) == 1
    lo, acc = 0, Fraction(0)
    while acc + pmf[lo] <= mass / 2:
        acc += pmf[lo]
        lo += 1
    hi, acc = m, Fraction(0)
    while acc + pmf[hi] <= mass / 2:
        acc += pmf[hi]
        hi -= 1
    return lo, hi


class MixtureCase:
    """Four classes in D = 4 features around well separated centres, a mixture of K = 8 components fitted on the host on a
    training split, its label map, a calibration split, a test split, and a cluster 25 sigma away from every centre."""

    def __init__(self, seed=0, n_per=260, C=4, K=8, D=4, ld=None, backend="host"):
        from pinn_amd.diagnosis import DeviceGMM
        rng = np.random.default_rng(seed)
        self.C, self.K, self.D = C, K, D
        centres = rng.normal(size=(C, D)) * 5.0
        X = np.concatenate([centres[c] + rng.normal(size=(n_per, D)) for c in range(C)])
        y = np.repeat(np.arange(C, dtype=np.int64), n_per)
        perm = rng.permutation(X.shape[0])
        X, y = X[perm], y[perm]
        a, b = X.shape[0] // 3, 2 * X.shape[0] // 3
        self.X_fit, self.y_fit, self.X_cal, self.y_cal, self.X_te, self.y_te = X[:a], y[:a], X[a:b], y[a:b], X[b:], y[b:]
        self.X_far = centres[rng.integers(C, size=64)] + rng.normal(size=(64, D)) + 25.0 * np.sqrt(D) * np.sign(rng.normal(size=D))
        self.gmm = DeviceGMM(K, random_state=seed, backend=backend).fit(self.X_fit)
        self.cfp = self.gmm.label_map(self.X_fit, self.y_fit, C)


def float_distance(a, b):
    """|a - b| in float64 spacings at max(|a|, |b|, 1); 0 where both are the same infinity."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(a - b) / np.spacing(np.maximum(np.maximum(np.abs(a), np.abs(b)), 1.0))
    return np.where(a == b, 0.0, d)


def mp_density_scores(X, weights, means, covariances, comp_map, digits=50):
    """s_c [n, C] and s_any [n] of the module's docstring, one row and class at a time at `digits` digits from the mixture's
    weights, means and covariances (not from its precisions_cholesky): the Gaussian log density by an explicit inverse and
    determinant, log(sum_k w_k m_kc N_k(x)) - log(sum_k w_k m_kc) over the components with m_kc > 0.  Returned as floats."""
    import mpmath as mp
    mp.mp.dps = digits
    K, D = means.shape
    C = comp_map.shape[1]
    inv = [mp.matrix(covariances[k].tolist()) ** -1 for k in range(K)]
    logdet = [mp.log(mp.det(mp.matrix(covariances[k].tolist()))) for k in range(K)]
    S, A = np.empty((X.shape[0], C)), np.empty(X.shape[0])
    for i in range(X.shape[0]):
        dens = []
        for k in range(K):
            d = mp.matrix([mp.mpf(float(X[i, j])) - mp.mpf(float(means[k, j])) for j in range(D)])
            q = (d.T * inv[k] * d)[0]
            dens.append(mp.mpf(float(weights[k])) * mp.exp(-(D * mp.log(2 * mp.pi) + logdet[k] + q) / 2))
        A[i] = float(-mp.log(mp.fsum(dens)))
        for c in range(C):
            ks = [k for k in range(K) if comp_map[k, c] > 0]
            pi = mp.fsum(mp.mpf(float(weights[k])) * mp.mpf(float(comp_map[k, c])) for k in ks)
            S[i, c] = float("inf") if not ks or pi == 0 else float(-(mp.log(mp.fsum(dens[k] * mp.mpf(float(comp_map[k, c])) for k in ks)) - mp.log(pi)))
    return S, A
