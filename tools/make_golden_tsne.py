"""Generate tests/golden/g_tsne.npz: scikit-learn 1.7's exact t-SNE taken apart, for tests/test_embedding_host.py.

Build machine only: needs scikit-learn and scipy.  No test imports this file.  The fixture holds arrays only.
Rows: synthetic, shaped like the four posterior columns pV, pT, pH, pO of the results array (values in (0, 1), 4 classes):
`X` [257, 4] with `y`, and two small cases at n = 65, `X1` [65, 1] and `X8` [65, 8].  Perplexity 20 (script 03's) throughout.

Per case (suffix "", "1", "8"), as condensed upper triangles: `P_sk` (scikit-learn's `_joint_probabilities`), `P_root` (per row
scipy's brentq on the entropy equation in float64 from float64 distances, then the same symmetrisation in numpy), and
`m_P` = max |P_sk - P_root| / max P, which carries scikit-learn's float32 distances and its tolerance of 1e-5.

For the main case: `Y_pca` (PCA(svd_solver="arpack"), scaled to std 1e-4 of the first column); three states `s<k>_Y`,
`s<k>_update`, `s<k>_gains` before iterations k = 10, 260 and 900 of a float64 run of `_gradient_descent`'s rule on P_sk under
`_tsne`'s schedule (the rule is restated here to reach the update and the gains, and the restatement is asserted to give
`_gradient_descent`'s bytes over the first phase); at each state `_kl_divergence`'s `s<k>_kl12`, `s<k>_grad12`, `s<k>_kl1`,
`s<k>_grad1` and the state after one further iteration `s<k>_next_Y`, `_update`, `_gains` (momentum and exaggeration of
the state's phase, learning rate `lr`); `trust` = trustworthiness of the run's final embedding `Y_final` for 5 and 10
neighbours; and for the end-to-end band `band_kl`, `band_trust` [8]: the KL scikit-learn would report and the
trustworthiness (10 neighbours) of 8 runs of the whole schedule from Y_pca on P_sk (1 + 1e-13 u), u uniform in [-1, 1],
with `band_factor` (2 unless no seed passes, see below).

Asserted here, with the next seed tried on failure: no stored state comes within a factor 1e3 of the floor Q = max(w / Z,
eps) that the package does not apply; no |update x gradient| below 1e-30 at the stored states (no sign tie); every one of
the 8 runs lies inside the band built from the other seven: KL <= max + f (max - min), trustworthiness >= min - f (max - min).

`--time` prints scikit-learn's wall times (exact and Barnes-Hut) for tools/time_tsne.py's sizes; nothing is stored.
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g_tsne.npz")
PERPLEXITY, EXAG, EPS, STATES, RUNS = 20.0, 12.0, np.finfo(np.double).eps, (10, 260, 900), 8


def make_rows(rng, n, D, n_classes=4):
    """Posterior-like columns: class c is high in column c mod D, everything squeezed into (0, 1)."""
    y = rng.integers(n_classes, size=n)
    centre = -2.0 * np.ones((n_classes, D))
    for c in range(n_classes):
        centre[c, c % D] = 2.0 + 0.5 * (c // D)
    X = 1.0 / (1.0 + np.exp(-(centre[y] + 0.7 * rng.standard_normal((n, D)))))
    return X, y


def p_root(X, perplexity):
    from scipy.optimize import brentq
    from scipy.spatial.distance import squareform
    n = X.shape[0]
    d = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    cond = np.zeros((n, n))
    target = np.log(perplexity)
    for i in range(n):
        di = np.delete(d[i], i)
        di = di - di.min()

        def f(lb):
            e = np.exp(-np.exp(lb) * di)
            s = e.sum()
            return np.log(s) + np.exp(lb) * (di * e).sum() / s - target
        lb = brentq(f, -40.0, 40.0, xtol=1e-15, rtol=4 * EPS, maxiter=500)
        e = np.exp(-np.exp(lb) * di)
        cond[i, np.arange(n) != i] = e / e.sum()
    P = cond + cond.T
    return np.maximum(squareform(P, checks=False) / max(P.sum(), EPS), EPS)


def p_sklearn(X, perplexity):
    from sklearn.manifold._t_sne import _joint_probabilities
    from sklearn.metrics import pairwise_distances
    return np.asarray(_joint_probabilities(pairwise_distances(X, metric="euclidean", squared=True), perplexity, 0), dtype=np.float64)


def step(p, update, gains, P, alpha, momentum, lr, n):
    """One iteration of _gradient_descent (scikit-learn 1.7): returns the error it computed, p, update, gains."""
    from sklearn.manifold._t_sne import _kl_divergence
    err, grad = _kl_divergence(p, P * alpha, 1, n, 2)
    inc = update * grad < 0.0
    gains = gains.copy()
    gains[inc] += 0.2
    gains[~inc] *= 0.8
    np.clip(gains, 0.01, np.inf, out=gains)
    grad *= gains
    update = momentum * update - lr * grad
    return err, p + update, update, gains, np.linalg.norm(grad)


def run_schedule(P, Y0, lr, n, max_iter=1000, no_progress=300, min_grad=1e-7, keep=()):
    """_tsne's two phases with _gradient_descent's checks.  Returns Y, the error last computed, the last iteration, and
    the states (p, update, gains) before the iterations in `keep`."""
    p, states, err, i = Y0.ravel().copy(), {}, np.finfo(float).max, 0
    start = 0
    for alpha, momentum, stop_at, nwp in ((EXAG, 0.5, 250, 250), (1.0, 0.8, max_iter, no_progress)):
        update, gains = np.zeros_like(p), np.ones_like(p)
        best, best_it = np.finfo(float).max, start
        for i in range(start, stop_at):
            if i in keep:
                states[i] = (p.copy(), update.copy(), gains.copy())
            err, p, update, gains, gnorm = step(p, update, gains, P, alpha, momentum, lr, n)
            if (i + 1) % 50 == 0:
                if err < best:
                    best, best_it = err, i
                elif i - best_it > nwp:
                    break
                if gnorm <= min_grad:
                    break
        start = i + 1
    return p.reshape(n, 2), err, i, states


def build(seed):
    from scipy.spatial.distance import pdist, squareform
    from sklearn.decomposition import PCA
    from sklearn.manifold import trustworthiness
    from sklearn.manifold._t_sne import _gradient_descent, _kl_divergence
    rng = np.random.default_rng(seed)
    out = {"seed": np.int64(seed), "perplexity": np.float64(PERPLEXITY)}
    X, y = make_rows(rng, 257, 4)
    X1, _ = make_rows(rng, 65, 1)
    X8, _ = make_rows(rng, 65, 8)
    out.update(X=X, y=y.astype(np.int64), X1=X1, X8=X8)
    for sfx, rows in (("", X), ("1", X1), ("8", X8)):
        Psk, Pr = p_sklearn(rows, PERPLEXITY), p_root(rows, PERPLEXITY)
        out["P_sk" + sfx], out["P_root" + sfx] = Psk, Pr
        out["m_P" + sfx] = np.float64(np.abs(Psk - Pr).max() / Pr.max())
        print("case %r: m_P = %.3e" % (sfx, out["m_P" + sfx]))
    n, P = 257, out["P_sk"]
    lr = max(n / EXAG / 4.0, 50.0)
    Y0 = PCA(n_components=2, svd_solver="arpack", random_state=seed).fit_transform(X)
    Y0 = Y0 / np.std(Y0[:, 0]) * 1e-4
    out.update(Y_pca=Y0, lr=np.float64(lr))

    # the restated rule gives _gradient_descent's bytes
    ref, _, _ = _gradient_descent(_kl_divergence, Y0.ravel().copy(), it=0, max_iter=250, n_iter_check=50, n_iter_without_progress=250,
                                  momentum=0.5, learning_rate=lr, min_gain=0.01, min_grad_norm=1e-7, verbose=0,
                                  args=[P * EXAG, 1, n, 2])
    p, u, g = Y0.ravel().copy(), np.zeros(2 * n), np.ones(2 * n)
    for _ in range(250):
        _, p, u, g, _ = step(p, u, g, P, EXAG, 0.5, lr, n)
    assert np.array_equal(p, ref), "the restated update rule differs from _gradient_descent"

    Yf, _, last, states = run_schedule(P, Y0, lr, n, keep=STATES)
    if sorted(states) != list(STATES):
        return None, "the run stopped at iteration %d, before a stored state" % last
    for k in STATES:
        p, u, g = states[k]
        alpha, mom = (EXAG, 0.5) if k < 250 else (1.0, 0.8)
        kl12, g12 = _kl_divergence(p, P * EXAG, 1, n, 2)
        kl1, g1 = _kl_divergence(p, P, 1, n, 2)
        ga = g12 if alpha == EXAG else g1
        if np.abs(u * ga).min() < 1e-30:
            return None, "a sign tie at state %d" % k
        w = 1.0 / (1.0 + pdist(p.reshape(n, 2), "sqeuclidean"))
        if w.min() / (2.0 * w.sum()) < 1e3 * EPS:
            return None, "state %d comes within 1e3 of the floor of Q" % k
        _, pn, un, gn, _ = step(p, u, g, P, alpha, mom, lr, n)
        out.update({"s%d_Y" % k: p.reshape(n, 2), "s%d_update" % k: u.reshape(n, 2), "s%d_gains" % k: g.reshape(n, 2),
                    "s%d_kl12" % k: np.float64(kl12), "s%d_grad12" % k: g12.reshape(n, 2), "s%d_kl1" % k: np.float64(kl1),
                    "s%d_grad1" % k: g1.reshape(n, 2), "s%d_next_Y" % k: pn.reshape(n, 2), "s%d_next_update" % k: un.reshape(n, 2),
                    "s%d_next_gains" % k: gn.reshape(n, 2)})
    out["Y_final"] = Yf
    out["trust"] = np.array([trustworthiness(X, Yf, n_neighbors=k) for k in (5, 10)])

    kls, trs = np.zeros(RUNS), np.zeros(RUNS)
    for r in range(RUNS):
        Pp = P * (1.0 + 1e-13 * rng.uniform(-1.0, 1.0, size=P.shape))
        Yr, kls[r], _, _ = run_schedule(Pp, Y0, lr, n)
        w = 1.0 / (1.0 + pdist(Yr, "sqeuclidean"))
        if w.min() / (2.0 * w.sum()) < 1e3 * EPS:
            return None, "run %d ends within 1e3 of the floor of Q" % r
        trs[r] = trustworthiness(X, Yr, n_neighbors=10)
    print("seed %d: KL %s\n  trustworthiness %s" % (seed, kls, trs))

    def inside(f):
        for r in range(RUNS):
            ok, ot = np.delete(kls, r), np.delete(trs, r)
            if kls[r] > ok.max() + f * (ok.max() - ok.min()) or trs[r] < ot.min() - f * (ot.max() - ot.min()):
                return False
        return True
    out.update(band_kl=kls, band_trust=trs)
    return out, inside


def timing():
    from sklearn.manifold import TSNE
    from sklearn.manifold._t_sne import _kl_divergence
    rng = np.random.default_rng(0)
    for n in (2048, 11000):
        X, _ = make_rows(rng, n, 4)
        t0 = time.perf_counter()
        TSNE(perplexity=20, init="pca", random_state=42, method="barnes_hut").fit(X)
        print("n = %d  Barnes-Hut, 1000 iterations: %.1f s" % (n, time.perf_counter() - t0))
        if n <= 2048:
            t0 = time.perf_counter()
            TSNE(perplexity=20, init="pca", random_state=42, method="exact").fit(X)
            print("n = %d  exact, 1000 iterations: %.1f s" % (n, time.perf_counter() - t0))
        else:                                   # a full exact run takes hours: three objective evaluations, times 1000
            P = np.full(n * (n - 1) // 2, 1.0 / (n * (n - 1)))
            p = 1e-4 * rng.standard_normal(2 * n)
            t0 = time.perf_counter()
            for _ in range(3):
                _kl_divergence(p, P, 1, n, 2)
            dt = (time.perf_counter() - t0) / 3
            print("n = %d  exact: %.2f s per objective evaluation, %.0f s for 1000 (extrapolated)" % (n, dt, 1000 * dt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="print scikit-learn's wall times and write nothing")
    args = ap.parse_args()
    warnings.filterwarnings("ignore")
    if args.time:
        return timing()
    fallback = None
    for seed in range(10):
        out, res = build(seed)
        if out is None:
            print("seed %d rejected: %s" % (seed, res))
            continue
        if res(2.0):
            out["band_factor"] = np.float64(2.0)
            break
        print("seed %d rejected: a run lies outside the band of the other seven" % seed)
        fallback = fallback or (out, res)
    else:
        if fallback is None:
            sys.exit("no seed gave a usable fixture")
        out, res = fallback
        f = 2.0
        while not res(f):
            f *= 2.0
        out["band_factor"] = np.float64(f)
        print("no seed in 0..9 passes at factor 2: seed %d with factor %g" % (int(out["seed"]), f))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
