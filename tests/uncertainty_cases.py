"""Case builders shared by the uncertainty tests (host and GPU): results-shaped arrays with known laws, the rows a select or
a tiled pass can get wrong, and the referees that both test files use."""
import math

import numpy as np

Y_TRUE, Y_PRED, ALE, EPI, LABEL = 8, 9, 10, 11, 17
MASK64 = (1 << 64) - 1


def results_array(n, seed, ld=22, n_labels=13, understate=1.0, s_lo=0.8, s_hi=2.0):
    """y_true = y_pred + understate * s * eps with eps ~ N(0, 1) and s^2 = ale^2 + epi^2, s_lo <= ale, epi <= s_hi (so v >= 1.28 and
    every nll term is positive at the defaults); labels 0 .. n_labels - 1 in runs, as a recording has them."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, ld))
    A[:, ALE] = rng.uniform(s_lo, s_hi, n)
    A[:, EPI] = rng.uniform(s_lo, s_hi, n)
    s = np.sqrt(A[:, ALE] ** 2 + A[:, EPI] ** 2)
    A[:, Y_PRED] = rng.normal(3.0, 0.5, n)
    A[:, Y_TRUE] = A[:, Y_PRED] + understate * s * rng.normal(size=n)
    if ld > LABEL:
        A[:, LABEL] = (np.arange(n) * n_labels) // max(n, 1)
    return A


def spoil(A, seed, share=0.05):
    """Rows that are not valid, of every kind: NaN / inf in y_true and y_pred, a NaN, negative-variance and zero-variance
    uncertainty, labels that are NaN, negative, beyond the table and fractional."""
    rng = np.random.default_rng(seed)
    A = A.copy()
    n = A.shape[0]
    kinds = 10
    idx = rng.choice(n, size=max(kinds, int(n * share)), replace=n < kinds)
    for i, j in enumerate(idx):
        k = i % kinds
        if k == 0: A[j, Y_TRUE] = np.nan
        elif k == 1: A[j, Y_PRED] = np.inf
        elif k == 2: A[j, ALE] = np.nan
        elif k == 3: A[j, ALE] = 0.0; A[j, EPI] = 0.0               # v = 0
        elif k == 4: A[j, EPI] = np.inf
        elif k == 5: A[j, LABEL] = np.nan
        elif k == 6: A[j, LABEL] = -1.0
        elif k == 7: A[j, LABEL] = 1000.0
        elif k == 8: A[j, LABEL] = A[j, LABEL] + 0.5                 # truncates to the same label: still valid
        elif k == 9: A[j, Y_TRUE] = -np.inf
    return A


def key_to_double(key):
    key = int(key) & MASK64
    bits = (key & (MASK64 >> 1)) if key >> 63 else (~key & MASK64)
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


def double_to_key(x):
    x = float(x) + 0.0
    bits = int(np.array([x], dtype=np.float64).view(np.uint64)[0])
    return (~bits & MASK64) if bits >> 63 else (bits | (1 << 63))


def bit_split_values(bit, count, rng):
    """`count` finite doubles whose 64-bit keys agree above `bit` and differ at and below it, both values of `bit` present."""
    while True:
        hi = int(rng.integers(0, 1 << 62)) << 2 | int(rng.integers(0, 4))
        hi = (hi >> (bit + 1)) << (bit + 1) if bit < 63 else 0
        vals = []
        for i in range(4 * count):
            low = (int(rng.integers(0, 1 << 62)) << 2 | int(rng.integers(0, 4))) & ((1 << (bit + 1)) - 1)
            low = (low & ~(1 << bit)) | ((i & 1) << bit)
            x = key_to_double(hi | low)
            if math.isfinite(x):
                vals.append(x)
            if len(vals) == count:
                return np.array(vals, dtype=np.float64)


def bit_split_array(bits, count, seed, ld=3):
    """One group per entry of `bits` (label = its position): column 0 the values, column 1 the label."""
    rng = np.random.default_rng(seed)
    A = np.zeros((len(bits) * count, ld))
    for g, b in enumerate(bits):
        A[g * count:(g + 1) * count, 0] = bit_split_values(b, count, rng)
        A[g * count:(g + 1) * count, 1] = g
    return A[rng.permutation(A.shape[0])]


def brute_rank(n_g, level, conformal):
    if n_g == 0:
        return 0
    if conformal:
        return int(math.ceil(float(n_g + 1) * level))
    return min(max(int(math.ceil(float(n_g) * level)), 1), n_g)


def brute_quantile(scores, level, conformal):
    """sorted(scores)[k - 1] with the stated k; NaN for no scores, +inf for k beyond them."""
    k = brute_rank(len(scores), level, conformal)
    if not scores:
        return float("nan"), k
    return (float("inf") if k > len(scores) else sorted(scores)[k - 1]), k


def ulp_distance(x, ref):
    """|x - ref| in units of the float64 spacing at |ref| (ref: floats rounded from a higher-precision referee)."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return np.abs(x - ref) / np.spacing(np.abs(ref))


def mp_terms(z, v, s, digits=50):
    """Phi(z), nll and crps of the module's docstring from the float64 z, v, s taken as exact, evaluated at `digits` digits;
    returned as mpmath numbers."""
    import mpmath as mp
    mp.mp.dps = digits
    phi, nll, crps = [], [], []
    for zi, vi, si in zip(np.asarray(z).tolist(), np.asarray(v).tolist(), np.asarray(s).tolist()):
        zi, vi, si = mp.mpf(zi), mp.mpf(vi), mp.mpf(si)
        P = mp.erfc(-zi / mp.sqrt(2)) / 2
        pdf = mp.exp(-zi * zi / 2) / mp.sqrt(2 * mp.pi)
        phi.append(P)
        nll.append((mp.log(2 * mp.pi) + mp.log(vi) + zi * zi) / 2)
        crps.append(si * (zi * (2 * P - 1) + 2 * pdf - 1 / mp.sqrt(mp.pi)))
    return phi, nll, crps


def mp_ulp_distance(x, ref_mp):
    """Distance of every float64 value of x from the mpmath number of ref_mp, in float64 spacings at |ref|."""
    import mpmath as mp
    return np.array([float(abs(mp.mpf(xi) - ri) / mp.mpf(float(np.spacing(abs(float(ri))))))
                     for xi, ri in zip(np.asarray(x, np.float64).tolist(), ref_mp)])


def sum_depth(n, tile, max_blocks, items=8):
    """Additions a term can pass through in the device's sum of n rows: the lane tree of a wave (6), the wave's steps in row
    order (items per tile, the tiles of a workgroup), the 4 waves (3), the workgroups in index order (blocks - 1)."""
    tiles = max(1, -(-n // tile))
    blocks = min(tiles, max_blocks)
    return 6 + items * (-(-tiles // blocks)) + 3 + (blocks - 1)
