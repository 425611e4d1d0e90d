"""What the tests of pinn_amd.explain share: the referee, the models it explains and the cases.

The referee does not use the module's formula: for D <= 4 it is the average of marginal contributions over all D!
orderings, for D = 8 (8! orderings are too many) the subset formula with math.factorial weights, both in float64 numpy on
hybrid rows built by np.where.  Its model functions are the package's host backends: DeviceGMM(..., backend="host").diagnose
and a float64 forward of a network's own weights."""
import itertools
import math

import numpy as np


def coalition_values(f, X, Bg):
    """{S as a bit mask: v(S) [n, C]}: the mean over the background of f on the hybrid rows."""
    n, D = X.shape
    B = Bg.shape[0]
    vals = {}
    for S in range(1 << D):
        mask = np.array([(S >> i) & 1 for i in range(D)], dtype=bool)
        H = np.where(mask[None, None, :], X[:, None, :], Bg[None, :, :]).reshape(n * B, D)
        F = np.asarray(f(H), dtype=np.float64).reshape(n, B, -1)
        vals[S] = F.mean(axis=1)
    return vals


def referee(f, X, Bg):
    """(phi [n, D, C], base [C], fx [n, C]) in float64: all orderings for D <= 4, the subset formula above."""
    X, Bg = np.asarray(X, dtype=np.float64), np.asarray(Bg, dtype=np.float64)
    n, D = X.shape
    v = coalition_values(f, X, Bg)
    C = v[0].shape[1]
    phi = np.zeros((n, D, C))
    if D <= 4:
        for order in itertools.permutations(range(D)):
            S = 0
            for j in order:
                phi[:, j, :] += v[S | (1 << j)] - v[S]
                S |= 1 << j
        phi /= math.factorial(D)
    else:
        for j in range(D):
            for S in range(1 << D):
                if not (S >> j) & 1:
                    s = bin(S).count("1")
                    phi[:, j, :] += math.factorial(s) * math.factorial(D - s - 1) / math.factorial(D) * (v[S | (1 << j)] - v[S])
    return phi, v[0][0].copy(), v[(1 << D) - 1]


def random_mixture(K, D, C, seed, iid_feature=None):
    """A host-backend DeviceGMM holding random parameters (components a few standard deviations apart, full covariances) and
    a random label map [K, C].  iid_feature: that feature has the same mean and variance in every component and no
    covariance with the others, so the posterior does not depend on it."""
    from pinn_amd import diagnosis
    rng = np.random.default_rng(seed)
    means = rng.normal(0.0, 2.0, (K, D))
    cov = np.empty((K, D, D))
    for k in range(K):
        A = rng.normal(0.0, 1.0, (D, D)) * 0.4 + np.eye(D)
        cov[k] = A @ A.T * rng.uniform(0.5, 1.5)
    if iid_feature is not None:
        j = iid_feature
        means[:, j] = 0.3
        cov[:, j, :] = 0.0
        cov[:, :, j] = 0.0
        cov[:, j, j] = 1.7
    w = rng.uniform(0.5, 1.5, K)
    g = diagnosis.DeviceGMM(K, backend="host")
    g.weights_, g.means_, g.covariances_ = w / w.sum(), means, cov
    g.precisions_cholesky_ = diagnosis._host_factor(cov)
    g.n_iter_, g.converged_, g.lower_bound_, g.lower_bound_changes_ = 1, True, 0.0, []
    cfp = rng.uniform(0.0, 1.0, (K, C)) ** 3
    cfp /= cfp.sum(axis=1, keepdims=True)
    return g, cfp


def mixture_rows(g, n, seed, pad=0):
    """n rows drawn around the mixture's means; pad: that many columns of other numbers before and after each feature block,
    to be read through a column list.  Returns (array, columns)."""
    rng = np.random.default_rng(seed)
    K, D = g.means_.shape
    z = rng.integers(K, size=n)
    X = g.means_[z] + rng.normal(0.0, 1.2, (n, D))
    if not pad:
        return X, list(range(D))
    arr = rng.normal(0.0, 1.0, (n, D + 2 * pad))
    cols = list(rng.permutation(D + 2 * pad)[:D])
    arr[:, cols] = X
    return arr, [int(c) for c in cols]


def host_diagnose(g, cfp):
    return lambda Z: g.diagnose(Z, cfp)[0]


def device_copy(g):
    """A device-backend mixture holding exactly the parameters of the host one."""
    from pinn_amd import diagnosis
    d = diagnosis.DeviceGMM(g.n_components, backend="device")
    d.weights_, d.means_, d.covariances_, d.precisions_cholesky_ = (a.copy() for a in (g.weights_, g.means_, g.covariances_,
                                                                                        g.precisions_cholesky_))
    d.n_iter_, d.converged_, d.lower_bound_, d.lower_bound_changes_ = 1, True, 0.0, []
    return d


def net_forward_f64(params, x):
    """DNN.forward in eval mode (01:421-438) in float64 numpy; params in the oracle's order.  Returns [n, 2] = (u, logvar)."""
    P = [np.asarray(p.detach().cpu().numpy(), dtype=np.float64) for p in params]
    n_hidden = (len(P) - 8) // 2
    h = np.asarray(x, dtype=np.float64)
    for l in range(n_hidden):
        h = np.tanh(h @ P[2 * l].T + P[2 * l + 1])
    k = 2 * n_hidden
    u = h @ P[k].T + P[k + 1]
    v = np.tanh(h @ P[k + 2].T + P[k + 3])
    v = np.tanh(v @ P[k + 4].T + P[k + 5])
    z = v @ P[k + 6].T + P[k + 7]
    return np.concatenate([u, np.log(np.logaddexp(0.0, z) + 1e-6)], axis=1)


def report(what, got, want, gate):
    """Print the largest deviation before the caller asserts on it."""
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max()) if np.size(want) else 0.0
    print("%s: max err %.3e (gate %.3e)" % (what, err, gate))
    return err
