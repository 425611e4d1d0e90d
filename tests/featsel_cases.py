"""Data and helpers shared by the feature-selection tests (test_featsel_host.py, test_featsel_abi.py, test_gpu_featsel.py).

Every array is a synthetic results array of 22 columns (column 17 the label 0..12, columns 18..21 unused), so that rows are
read in place with a leading dimension that is not the number of features.  Nothing here depends on the code under test."""
import numpy as np

BINARY = "normal:0 | fault:1,2,3,4,5,6,7,8,9,10,11,12"
FIVE = "normal:0 | flooding:1,2,3 | oxygen_starvation:4,5,6 | membrane_drying:7,8,9 | hydrogen_starvation:10,11,12"
THIRTEEN = " | ".join("c%d:%d" % (k, k) for k in range(13))
SPECS = {2: BINARY, 5: FIVE, 13: THIRTEEN}
LABEL = 17
POOL5 = (0, 3, 11, 12, 8)                      # x0, x3, epi, res, y_true: 25 subsets of sizes 1..3
TIED = 5                                       # a column with two distinct values: heavily tied scores

# the planted-signal case: the labels come from a logistic model on the two named columns, the rest of the pool is noise
PLANTED_POOL = ("x0", "x3", "x5", "epi", "res", "pV")
PLANTED_PAIR = (3, 11)                         # x3, epi in pool order
PLANTED_N, PLANTED_SEED, PLANTED_STRENGTH, PLANTED_A, PLANTED_TEST_SIZE = 600, 3, 6.0, 0.2, 0.5


def class_of(label, C):
    label = np.asarray(label, dtype=np.int64)
    return {2: (label > 0).astype(np.int64), 5: (label + 2) // 3, 13: label}[C]


def results_array(n, seed, shift=0.6):
    """[n, 22]: the labels 0..12 occur in rows 0..12 and again in rows 13..25; the feature columns are noise of column-dependent scale and offset plus a
    class-dependent shift whose size varies from column to column (so subsets differ in how hard their fit is); column
    TIED takes two values, correlated with the label."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 13, n)
    lab[:13] = lab[13:26] = np.arange(13)
    A = rng.normal(size=(n, 22)) * rng.uniform(0.5, 3.0, 22) + rng.normal(size=22) * 5.0
    A += (shift * rng.uniform(0.0, 4.0, 22) * rng.normal(size=(13, 22)))[lab]
    A[:, TIED] = ((lab > 0) ^ (rng.random(n) < 0.3)).astype(np.float64)
    A[:, LABEL] = lab
    return A


def split_of(n, seed, frac=0.5):
    """(idx_train, idx_val) among n >= 26 rows of results_array: rows 0..12 train, rows 13..25 validate (so both sides hold
    every label), the rest is shuffled and the first `frac` of it trains."""
    rest = 26 + np.random.default_rng(seed).permutation(n - 26)
    k = int(frac * len(rest))
    return np.concatenate([np.arange(13), rest[:k]]).astype(np.int64), np.concatenate([np.arange(13, 26), rest[k:]]).astype(np.int64)


def planted(n=PLANTED_N, seed=PLANTED_SEED, strength=PLANTED_STRENGTH, a=PLANTED_A):
    """[n, 22] of standard normal columns, except epi = u + a v and x3 = u - a v for independent standard normal u, v, and
    P(fault) = sigmoid(strength v): a logistic model on (epi - x3) / (2 a).  Either column alone says little about v
    (correlation a / sqrt(1 + a^2)), the pair says everything."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, 22))
    u, v = rng.normal(size=n), rng.normal(size=n)
    A[:, 11], A[:, 3] = u + a * v, u - a * v
    fault = rng.random(n) < 1.0 / (1.0 + np.exp(-strength * v))
    A[:, LABEL] = np.where(fault, rng.integers(1, 13, n), 0)
    return A


def auc_of(truth, score):
    """AUC by counting pairs, ties as halves: the test's own statement."""
    pos, neg = score[truth], score[~truth]
    gt = (pos[:, None] > neg[None, :]).sum()
    eq = (pos[:, None] == neg[None, :]).sum()
    return (gt + 0.5 * eq) / (len(pos) * len(neg))


def bootstrap_margin(truth, y_idx, pf_a, pf_b, p_a, p_b, n_boot=400, seed=0):
    """(AUC margin, log-loss margin) of model a over model b on the validation rows, each divided by the bootstrap
    standard error of the paired difference (rows resampled with replacement)."""
    rng = np.random.default_rng(seed)
    n = len(truth)
    la, lb = -np.log(p_a[np.arange(n), y_idx]), -np.log(p_b[np.arange(n), y_idx])
    d_auc, d_ll = [], []
    for _ in range(n_boot):
        r = rng.integers(0, n, n)
        if truth[r].all() or not truth[r].any():
            continue
        d_auc.append(auc_of(truth[r], pf_a[r]) - auc_of(truth[r], pf_b[r]))
        d_ll.append(lb[r].mean() - la[r].mean())
    return ((auc_of(truth, pf_a) - auc_of(truth, pf_b)) / np.std(d_auc), (lb.mean() - la.mean()) / np.std(d_ll))
