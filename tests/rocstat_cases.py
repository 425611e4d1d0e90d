"""Shared inputs of the ROC-inference tests and their oracle: the definitions themselves, in Python integers and Fractions.

The reference has no counterpart (script 02 prints one AUC per group), so the oracle is the O(m n) double loop over
psi(x, y) = 1, 1/2, 0 for x >, ==, < y (kept doubled: 2, 1, 0), the textbook sample covariance (ddof = 1) of V10 and V01, and
for the bootstrap the same double loop over the drawn rows, with the draws recovered from Philox by the documented keying."""
from fractions import Fraction

import numpy as np

SIZES = [(2, 2), (7, 13), (60, 180), (130, 127)]
VARIANTS = ["continuous", "quarter", "eighth", "equal", "separated", "zeros"]
DRAW_BOOT = 2                           # the bootstrap's Philox draw kind (include/pinn_hip.h: PINN_AUC_DRAW_BOOT)

_cache = {}


def make_case(m, n, variant="continuous", K=1, seed=0, shifts=None):
    """(y [N] of 0 / 1 in a shuffled order, scores [K, N]); classifier k's positives are shifted by shifts[k]."""
    key = (m, n, variant, K, seed, None if shifts is None else tuple(shifts))
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng([seed, m, n, K])
    y = np.zeros(m + n, dtype=np.int64)
    y[:m] = 1
    y = rng.permutation(y)
    sh = np.asarray(shifts if shifts is not None else [1.5 / (1 + k) for k in range(K)], dtype=np.float64)
    s = rng.normal(size=(K, m + n)) + sh[:, None] * y
    if variant == "quarter":
        s = np.round(s * 4) / 4
    elif variant == "eighth":
        s = np.round(s * 8) / 8
    elif variant == "equal":
        s = np.full_like(s, 0.25)
    elif variant == "separated":
        s = np.where(y == 1, 1.0 + np.abs(s), -1.0 - np.abs(s))
    elif variant == "zeros":                      # half the rows at +0.0, one of them at -0.0, the rest rounded to 1/2
        s = np.round(s * 2) / 2
        zero = rng.random(m + n) < 0.5
        zero[:2] = True
        s[:, zero] = 0.0
        s[:, np.flatnonzero(zero)[0]] = -0.0
        assert np.signbit(s[0, np.flatnonzero(zero)[0]])
    elif variant != "continuous":
        raise KeyError(variant)
    _cache[key] = (y, s)
    return y, s


def brute_components(y, s):
    """a [K][m], b [K][n] as lists of Python integers by the double loop: a[i] = sum_j 2 psi(pos_i, neg_j), b[j] likewise."""
    pos, neg = np.flatnonzero(y == 1), np.flatnonzero(y != 1)
    A, B = [], []
    for k in range(s.shape[0]):
        sp, sn = s[k][pos].tolist(), s[k][neg].tolist()
        A.append([sum(2 if x > v else (1 if x == v else 0) for v in sn) for x in sp])
        B.append([sum(2 if x > v else (1 if x == v else 0) for x in sp) for v in sn])
    return A, B


def textbook_cov(A, B):
    """(theta [K], cov [K][K]) as Fractions: cov = S10 / m + S01 / n, the sample covariances (ddof = 1) of V10 = a / (2 n)
    and V01 = b / (2 m) about their means."""
    K, m, n = len(A), len(A[0]), len(B[0])
    V10 = [[Fraction(v, 2 * n) for v in A[k]] for k in range(K)]
    V01 = [[Fraction(v, 2 * m) for v in B[k]] for k in range(K)]
    theta = [sum(V10[k], Fraction(0)) / m for k in range(K)]
    assert theta == [sum(V01[k], Fraction(0)) / n for k in range(K)]

    def scov(U, k, l, cnt):
        return sum(((x - theta[k]) * (z - theta[l]) for x, z in zip(U[k], U[l])), Fraction(0)) / (cnt - 1)

    cov = [[scov(V10, k, l, m) / m + scov(V01, k, l, n) / n for l in range(K)] for k in range(K)]
    return theta, cov


def philox_draws(seed, resample, stratum, size):
    """The positions a resample draws in a stratum, one Philox call per draw through the package's host twin, in Python
    integers: draw t reads words 2 (t & 1) and 2 (t & 1) + 1 of the call at the counter (t >> 1, resample, DRAW_BOOT, stratum)
    under the key (seed low, seed high); position = (bits * size) >> 64."""
    from pinn_amd.anomaly import philox4x32_10
    out = []
    for t in range(size):
        w = philox4x32_10(t >> 1, resample, DRAW_BOOT, stratum, seed & 0xFFFFFFFF, seed >> 32)
        bits = int(w[2 * (t & 1)]) | (int(w[2 * (t & 1) + 1]) << 32)
        out.append((bits * size) >> 64)
    return out


def brute_resample_u2(y, s_k, seed, resample):
    """U2* of one resample of one classifier by the double loop over its drawn rows."""
    pos, neg = np.flatnonzero(y == 1), np.flatnonzero(y != 1)
    sn = [float(s_k[neg[i]]) for i in philox_draws(seed, resample, 0, len(neg))]
    sp = [float(s_k[pos[i]]) for i in philox_draws(seed, resample, 1, len(pos))]
    return sum(2 if x > v else (1 if x == v else 0) for x in sp for v in sn)


def holm_reference(p):
    """Holm's step-down adjusted p-values, ten lines."""
    p = list(p)
    order = sorted(range(len(p)), key=lambda i: p[i])
    adj, running = [0.0] * len(p), 0.0
    for rank, i in enumerate(order):
        running = max(running, min(1.0, (len(p) - rank) * p[i]))
        adj[i] = running
    return adj
