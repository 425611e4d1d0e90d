"""Shared builders of the change-point tests: rows with a shifted second half, a brute force over every admissible partition
with costs summed directly (no prefix sums), the rounding bound that decides which cases are kept, and the case lists."""
import functools
import itertools
import json
import os

import numpy as np

EPS = np.finfo(np.float64).eps
VAR_FLOOR = 1e-3                         # of the brute-force cases: it bounds how far an error in SS moves log v and SS / v
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "changepoint_immediate_pruning.json")


def shifted_rows(seed, n, D, level=0.0):
    """Gaussian rows [n, D] whose second half is shifted by 1 to 3 standard deviations per column."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, D)) + level
    X[n // 2:] += rng.uniform(1.0, 3.0, size=D) * rng.choice([-1.0, 1.0], size=D)
    return X


def results_like(X, ld=None, first=0):
    """The rows X in columns first .. first + D of a wider float64 array (the results array's shape), the rest filled."""
    n, D = X.shape
    ld = max(first + D + 2, 6) if ld is None else ld
    A = np.full((n, ld), 7.5)
    A[:, first:first + D] = X
    return A, list(range(first, first + D))


def piece_cost(Z, s, t, kind, var_floor):
    """C(s, t) from the rows themselves: two-pass sums in extended precision."""
    x = np.asarray(Z[s:t], dtype=np.longdouble)
    ss = ((x - x.mean(axis=0)) ** 2).sum(axis=0)
    if kind == "mean":
        return float(ss.sum())
    ln = np.longdouble(t - s)
    v = np.maximum(ss / ln, np.longdouble(var_floor))
    return float((ln * np.log(v) + ss / v).sum())


def partitions(m, min_len, max_len):
    """Every tuple of change points 0 < tau_1 < ... < tau_k < m with all pieces in [min_len, max_len]."""
    hi = m if not max_len else max_len

    def rec(start):
        if min_len <= m - start <= hi:
            yield ()
        for nxt in range(start + min_len, min(start + hi, m - min_len) + 1):
            for rest in rec(nxt):
                yield (nxt,) + rest
    return rec(0)


def brute_force(Z, beta, kind, min_len, max_len=None, var_floor=VAR_FLOOR):
    """(best penalised cost, its change points, the runner-up's penalised cost or inf, partitions tried)."""
    m = Z.shape[0]
    cost = functools.lru_cache(maxsize=None)(lambda s, t: piece_cost(Z, s, t, kind, var_floor))
    scored = []
    for taus in partitions(m, min_len, max_len):
        edges = (0,) + taus + (m,)
        scored.append((sum(cost(a, b) for a, b in zip(edges, edges[1:])) + beta * len(taus), taus))
    scored.sort()
    if not scored:
        return np.inf, (), np.inf, 0
    return scored[0][0], scored[0][1], scored[1][0] if len(scored) > 1 else np.inf, len(scored)


def rounding_bound(Z, beta, kind, var_floor=VAR_FLOOR):
    """How far a penalised cost computed from float64 prefix sums of the centred rows can lie from the exact one.

    With c the rows centred on the first and SQ the sum of all c^2: a prefix sum of n terms is off by at most n eps SQ, so
    is S^2 / len (at most Q by Cauchy-Schwarz); an SS takes two differences of prefix sums and one such quotient, 6 n eps SQ
    with the roundings of the expression itself.  A partition has at most n pieces and D columns share SQ: 6 n^2 eps SQ, and
    the n additions of the recursion add n eps (SQ + n beta).  For "meanvar" an error e in SS moves len log v + SS / v by at
    most 2 e / var_floor (v >= var_floor), and each of the n D logarithms, at most len |log v| <= n * 40, is off by a few eps."""
    n, D = Z.shape
    c = Z - Z[0]
    SQ = float((c * c).sum())
    b = 6.0 * n * n * EPS * SQ + n * EPS * (SQ + n * beta)
    if kind == "meanvar":
        b = 2.0 * b / var_floor + 4.0 * n * D * n * 40.0 * EPS
    return 2.0 * b                        # both the brute force's runner-up and the solver's optimum may be off


def host_cases():
    """The cases of the brute-force comparison: n = 6 .. 14, D = 1 .. 3, both kinds, min_len 1 .. 3, with and without max_len.
    Returns (kept cases, generated, dropped): a case is dropped when the runner-up is within the rounding bound of the best."""
    kept, generated = [], 0
    for n, D, kind, min_len, with_max in itertools.product(range(6, 15), (1, 2, 3), ("mean", "meanvar"), (1, 2, 3), (False, True)):
        if kind == "meanvar" and min_len < 2:
            continue
        generated += 1
        Z = shifted_rows(1000 * n + 100 * D + 10 * min_len + with_max, n, D)
        beta = 1.5 * (D + 1) if kind == "mean" else 1.0 * (2 * D + 1)
        max_len = max(min_len + 1, n // 2 + 1) if with_max else None
        best, taus, second, tried = brute_force(Z, beta, kind, min_len, max_len)
        if not best < np.inf or second - best <= rounding_bound(Z, beta, kind):
            continue
        kept.append(dict(Z=Z, n=n, D=D, kind=kind, min_len=min_len, max_len=max_len, beta=beta, best=best, taus=taus, second=second))
    return kept, generated, generated - len(kept)


@functools.lru_cache(maxsize=None)
def cached_host_cases():
    return host_cases()


def golden_case():
    with open(GOLDEN) as f:
        g = json.load(f)
    g["Z"] = np.asarray(g["rows"], dtype=np.float64)
    return g
