"""What the selection tests share: the grid of the fixture sweep, the host referee's sweep (computed once per process and
never changed), the conditions the selections rest on, and the host's k-means++ picks with their margins."""
import functools

import numpy as np

from conftest import load_golden

GRID_K = (2, 4, 8, 12, 16, 20, 24, 32)
SEEDS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def fixture():
    return load_golden("g_gmm.npz")


@functools.lru_cache(maxsize=None)
def host_sweep():
    from pinn_amd import selection
    G = fixture()
    return selection.gmm_sweep(G["X_tr"], GRID_K, SEEDS, X_val=G["X_te"], backend="host")


def best_bic_per_K(sw):
    return {int(K): float(np.min(sw.bic[sw.n_components == K])) for K in np.unique(sw.n_components)}


def check_conditions(sw, margins, tol=1e-3):
    """The input conditions of the fixture selections; each is asserted, none is skipped.  `margins`: per candidate the
    smallest ||change| - tol| of the host referee's iterations."""
    per_K = sorted(best_bic_per_K(sw).values())
    gap = per_K[1] - per_K[0]
    print("BIC gap between the best K and the runner-up %.1f (needs >= 100); converged %d of %d; status set %d; smallest "
          "convergence margin %.3e (needs >= 1e-8)" % (gap, int(sw.converged.sum()), len(sw), int((sw.status != 0).sum()), min(margins)))
    assert gap >= 100.0
    assert sw.converged.all() and (sw.status == 0).all()
    assert min(margins) >= 1e-8


@functools.lru_cache(maxsize=None)
def host_margins(tol=1e-3):
    sw = host_sweep()
    return tuple(float(np.min(np.abs(np.abs(np.array(sw.model(i).lower_bound_changes_)) - tol))) for i in range(len(sw)))


def check_selections(sw, G):
    """bic, aic and val_score pick K = 8; lower_bound over the seeds of K = 20 picks seed 1; the selected model diagnoses
    the held-out rows no worse than (20, seed 1)."""
    picks = {c: int(sw.n_components[sw.best(c)]) for c in ("bic", "aic", "val_score")}
    print("picked K:", picks)
    assert picks == {"bic": 8, "aic": 8, "val_score": 8}
    at20 = np.flatnonzero(sw.n_components == 20)
    lb = np.where(sw.status[at20] == 0, sw.lower_bound[at20], -np.inf)
    print("lower bounds at K = 20, seeds %s: %s" % (sw.seed[at20], lb))
    assert int(sw.seed[at20[np.argmax(lb)]]) == 1
    ref = int(at20[list(sw.seed[at20]).index(1)])
    m = sw.diagnosis_metrics(G["X_tr"], G["y_tr"], G["X_te"], G["y_te"], 4)
    sel = sw.best("bic")
    print("held-out accuracy: selected (K=%d, seed %d) %.4f, (20, seed 1) %.4f" % (sw.n_components[sel], sw.seed[sel], m[sel]["accuracy"],
                                                                                 m[ref]["accuracy"]))
    assert m[sel]["accuracy"] >= m[ref]["accuracy"]


def clustered(n, K, D, seed, spread=3.0):
    """n rows around K centres with unequal feature scales."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, spread, (K, D))
    return centres[rng.integers(K, size=n)] + rng.normal(0.0, 1.0, (n, D)) * rng.uniform(0.5, 1.5, D)


def nested(n, seed):
    """n rows in four groups 40 or more apart, three of them split into two clusters 8 sigma apart: four and seven
    components are both natural, responsibilities are all but 0 or 1 and an EM iteration does not amplify a rounding
    error, so the sensitivity gate (floor 1e-13) stays above the rounding of a sum of n terms (sqrt(n) x 1.1e-16)."""
    rng = np.random.default_rng(seed)
    sup = np.array([[40.0, 0, 0, 0], [0, 40.0, 0, 0], [0, 0, 40.0, 0], [-40.0, -40.0, 0, 40.0]])
    centres = np.concatenate([sup[:1], sup[1:] + 4.0, sup[1:] - 4.0])
    return centres[rng.integers(7, size=n)] + rng.normal(0.0, 1.0, (n, 4)) * rng.uniform(0.5, 1.5, 4)


def duplicated_rows():
    """50 rows around the origin and two identical rows far from them: with two or more components the pair gets a
    component of its own, whose covariance has no Cholesky factor when reg_covar is 0."""
    rng = np.random.default_rng(0)
    return np.concatenate([rng.normal(size=(50, 3)), np.full((2, 3), 9.0)])


def host_picks(X, K, seed):
    """The k-means++ picks of the host referee (DeviceGMM._host_own_labels' draws) and the smallest pick margin
    |c[pick or pick - 1] - u total| / total over the draws (inf when K is 1 or a total is 0, where nothing is compared)."""
    n = X.shape[0]
    rng = np.random.default_rng(seed)
    picks = [int(rng.integers(n))]
    d2 = ((X - X[picks[0]]) ** 2).sum(axis=1)
    margin = np.inf
    for _ in range(1, K):
        u = float(rng.random())
        c = np.cumsum(d2)
        p = int(min(np.searchsorted(c, u * c[-1], side="right"), n - 1))
        if c[-1] > 0:
            near = [abs(c[p] - u * c[-1])] + ([abs(c[p - 1] - u * c[-1])] if p > 0 else [])
            margin = min(margin, min(near) / c[-1])
        picks.append(p)
        d2 = np.minimum(d2, ((X - X[p]) ** 2).sum(axis=1))
    return picks, margin
