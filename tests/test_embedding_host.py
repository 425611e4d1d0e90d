"""CPU: the host backend of pinn_amd.embedding (exact t-SNE) against tests/golden/g_tsne.npz (tools/make_golden_tsne.py).

The checkers take a backend and are shared with tests/test_gpu_embedding.py.  Trajectories and end points are no target (a
float64 exact run moves by percents of KL when P is perturbed by 1e-13); the gates are:
  1  entropy: every row of the conditional distribution, recomputed here from the returned beta, has |H - log perp| <= 1e-10
  2  |P - P_root| <= 1e-9 max P (brentq's root in float64, propagated)
  3  |P - P_sk| <= 2 m_P max P (m_P: the fixture's own distance between scikit-learn's P and the root)
  4  P symmetric bit for bit, zero diagonal, |sum P - 1| <= n^2 eps
  5  every raw sum of a pair pass within 1e-12 x the sum of its absolute terms of the host backend (n <= 600: the worst-case
     summation error is 600 x 1.1e-16)
  6  KL and gradient against scikit-learn's stored values within the same bound
  7  one iteration from each stored state: gains exactly, update and Y within lr x gain x (the gradient's tolerance)
  8  the schedule as a state machine (here: against what scikit-learn's rules name; on the GPU: host against device)
  9  plumbing, 10 trustworthiness <= 1e-12, 11 the end-to-end band of the reference's own spread, 12 the script helpers.
Every comparison prints its maxima before it asserts."""
import numpy as np
import pytest

EPS = 2.220446049250313e-16
STATES = (10, 260, 900)
SHAPES = [(5, 4, 2.0), (64, 1, 20.0), (65, 8, 20.0), (257, 4, 20.0), (600, 4, 30.0)]       # n, D, perplexity


@pytest.fixture(scope="module")
def G(golden):
    return golden("g_tsne.npz")


@pytest.fixture(scope="module")
def E():
    from pinn_amd import embedding
    return embedding


def full(c):
    """A condensed upper triangle as the symmetric matrix with a zero diagonal."""
    n = int(round((1 + np.sqrt(1 + 8 * c.size)) / 2))
    P = np.zeros((n, n))
    P[np.triu_indices(n, 1)] = c
    return P + P.T


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def draw_rows(n, D, seed=0):
    """Posterior-like rows in (0, 1) around 4 class centres."""
    rng = np.random.default_rng(1000 * n + 10 * D + seed)
    y = rng.integers(4, size=n)
    centre = -2.0 * np.ones((4, D))
    for c in range(4):
        centre[c, c % D] = 2.0 + 0.5 * (c // D)
    return 1.0 / (1.0 + np.exp(-(centre[y] + 0.7 * rng.standard_normal((n, D))))), y


def row_entropy(X, beta):
    """Entropy (nats) of p_{j|i} ~ exp(-beta_i |x_i - x_j|^2), j != i, recomputed from beta."""
    n = X.shape[0]
    d = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    off = ~np.eye(n, dtype=bool)
    d = d - np.where(off, d, np.inf).min(axis=1)[:, None]
    with np.errstate(invalid="ignore"):                                         # beta = inf (a row without a root) gives nan
        e = np.exp(-beta[:, None] * d) * off
        s = e.sum(axis=1)
        return np.log(s) + beta * (d * e).sum(axis=1) / s


def check_structure(P, X, beta, perplexity, tag):
    n = P.shape[0]
    dH = np.abs(row_entropy(X, beta) - np.log(perplexity)).max()
    dsum = abs(P.sum() - 1.0)
    print("%s: max |H - log perp| = %.3e, |sum P - 1| = %.3e (bound %.3e), min off-diagonal P = %.3e"
          % (tag, dH, dsum, n * n * EPS, P[~np.eye(n, dtype=bool)].min()))
    assert dH <= 1e-10                                                          # gate 1
    assert P.tobytes() == np.ascontiguousarray(P.T).tobytes()                   # gate 4
    assert np.all(np.diag(P) == 0.0) and P[~np.eye(n, dtype=bool)].min() >= EPS
    assert dsum <= n * n * EPS


def check_affinities_fixture(G, E, backend, sfx, wrap=lambda a: a):
    X = G["X" + sfx]
    P, beta, H = (host(a) for a in E.joint_probabilities(wrap(X), float(G["perplexity"]), backend=backend))
    check_structure(P, X, beta, float(G["perplexity"]), "fixture case %r" % sfx)
    Pr, Ps, mP = full(G["P_root" + sfx]), full(G["P_sk" + sfx]), float(G["m_P" + sfx])
    d_root, d_sk = np.abs(P - Pr).max() / Pr.max(), np.abs(P - Ps).max() / Pr.max()
    print("  max |P - P_root| / max P = %.3e (bound 1e-9), max |P - P_sk| / max P = %.3e (bound %.3e)" % (d_root, d_sk, 2 * mP))
    assert d_root <= 1e-9                                                       # gate 2
    assert d_sk <= 2 * mP                                                       # gate 3
    assert np.abs(H - np.log(float(G["perplexity"]))).max() <= 1e-10
    return P


def check_affinities_shape(E, backend, n, D, perplexity, wrap=lambda a: a):
    X, _ = draw_rows(n, D)
    P, beta, _ = (host(a) for a in E.joint_probabilities(wrap(X), perplexity, backend=backend))
    check_structure(P, X, beta, perplexity, "n = %d, D = %d" % (n, D))
    return X, P


def sums_bound(ref):
    return 1e-12 * ref["abs_row_sums"]


def grad_tolerance(ref, alpha):
    """What the bound of the raw sums allows the gradient 4 (alpha A - R / Z) to move by, per element."""
    A = ref["abs_row_sums"]
    return 1e-12 * 4.0 * (alpha * A[:, 1:3] + A[:, 3:5] / ref["Z"])


def kl_tolerance(ref, alpha):
    A = ref["abs_row_sums"].sum(axis=0)
    return 1e-12 * alpha * (A[5] + abs(np.log(alpha)) * A[7] + A[6] + A[7] * abs(np.log(ref["Z"])) + A[7] * A[0] / ref["Z"])


def check_raw_sums(E, backend, P, Y, alpha, tag, wrap=lambda a: a):
    ref = E.kl_and_gradient(P, Y, alpha, backend="host")
    r = E.kl_and_gradient(wrap(P), wrap(Y), alpha, backend=backend)
    d = np.abs(host(r["row_sums"]) - ref["row_sums"])
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(ref["abs_row_sums"] > 0, d / ref["abs_row_sums"], 0.0), axis=0)
    print("%s, alpha %g: max |sum - host| / sum |terms| per column = %s (bound 1e-12)" % (tag, alpha, np.array2string(worst, precision=2)))
    assert np.all(d <= sums_bound(ref))                                         # gate 5
    dg, dk = np.abs(host(r["grad"]) - ref["grad"]), abs(r["kl"] - ref["kl"])
    print("  against the host: max |grad diff| / tolerance = %.3e, |KL diff| = %.3e (tolerance %.3e)"
          % ((dg / grad_tolerance(ref, alpha)).max(), dk, kl_tolerance(ref, alpha)))
    assert np.all(dg <= grad_tolerance(ref, alpha)) and dk <= kl_tolerance(ref, alpha)
    return r, ref


def check_stored_states(G, E, backend, wrap=lambda a: a):
    P = full(G["P_sk"])
    for k in STATES:
        for alpha, sfx in ((12.0, "12"), (1.0, "1")):
            r, ref = check_raw_sums(E, backend, P, G["s%d_Y" % k], alpha, "state %d" % k, wrap)
            dg, dk = np.abs(host(r["grad"]) - G["s%d_grad%s" % (k, sfx)]), abs(r["kl"] - float(G["s%d_kl%s" % (k, sfx)]))
            print("  against scikit-learn: max |grad diff| / tolerance = %.3e, |KL diff| = %.3e (tolerance %.3e, KL %.6f)"
                  % ((dg / grad_tolerance(ref, alpha)).max(), dk, kl_tolerance(ref, alpha), r["kl"]))
            assert np.all(dg <= grad_tolerance(ref, alpha))                     # gate 6
            assert dk <= kl_tolerance(ref, alpha)


def check_one_iteration(G, E, backend):
    P, lr = full(G["P_sk"]), float(G["lr"])
    for k in STATES:
        alpha = 12.0 if k < 250 else 1.0
        st = E.new_state(G["s%d_Y" % k], iteration=k, update=G["s%d_update" % k], gains=G["s%d_gains" % k])
        out, h = E.descend(P, st, 1, learning_rate=lr, backend=backend)
        ref = E.kl_and_gradient(P, G["s%d_Y" % k], alpha, backend="host")
        bound = lr * out["gains"] * grad_tolerance(ref, alpha)
        du, dy = np.abs(out["update"] - G["s%d_next_update" % k]), np.abs(out["Y"] - G["s%d_next_Y" % k])
        print("one iteration from state %d: gains equal: %s, max |update diff| / bound = %.3e, max |Y diff| / bound = %.3e"
              % (k, np.array_equal(out["gains"], G["s%d_next_gains" % k]), (du / bound).max(), (dy / bound).max()))
        assert h["iteration"] == k + 1 and h["n_iter"] == k and not h["done"]
        assert np.array_equal(out["gains"], G["s%d_next_gains" % k])           # gate 7
        assert np.all(du <= bound) and np.all(dy <= bound)


def small_problem(G, E):
    """P of the fixture's n = 65, D = 8 case and a drawn start of scale 1e-4."""
    return full(G["P_sk8"]), 1e-4 * np.random.default_rng(7).standard_normal((65, 2))


def run(E, backend, P, st, n_iter, **kw):
    return E.descend(P, st, n_iter, backend=backend, **kw)


def ints(E, h):
    return {k: h[k] for k in E.HEADER_INTEGERS}


def same_state(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("Y", "update", "gains"))


def case_max_iter_250(E, backend, P, Y0):
    out, h = run(E, backend, P, E.new_state(Y0), 300, max_iter=250, learning_rate=50.0)
    return out, h


def case_boundary(E, backend, P, Y0):
    at250, h250 = run(E, backend, P, E.new_state(Y0), 250, max_iter=300, learning_rate=50.0)
    end, hend = run(E, backend, P, at250, 100, max_iter=300, learning_rate=50.0)
    return at250, h250, end, hend


def stationary_start(E):
    """Two clusters of three points, descended on the host (no exaggeration) until the gradient norm is below 1e-10."""
    rng = np.random.default_rng(3)
    X = np.concatenate([rng.standard_normal((3, 2)) * 0.3, rng.standard_normal((3, 2)) * 0.3 + 1.0])
    P, _, _ = E.joint_probabilities(X, 4.0, backend="host")
    st, h = E.descend(P, E.new_state(1e-2 * rng.standard_normal((6, 2)), iteration=250), 3000, max_iter=5250, learning_rate=1.0,
                      n_iter_without_progress=5000, min_grad_norm=1e-10, backend="host")
    g = E.kl_and_gradient(P, st["Y"], backend="host")["grad_norm"]
    print("stationary start: %d iterations, stop %r, |grad| = %.3e" % (h["n_iter"] - 249, E.STOP_NAMES[h["stop"]], g))
    assert g < 1e-7
    return P, st["Y"]


def case_stationary(E, backend, P, Y):
    return run(E, backend, P, E.new_state(Y, iteration=250), 200, max_iter=1000, learning_rate=1.0, min_grad_norm=1e-7)


def case_no_progress(E, backend, P, Y0):
    """550 iterations at the usual learning rate, then the same state with a learning rate of 1e6: the error rises above the
    best one and stays there, and the rule `iteration - best iteration > 50` ends the run at a check."""
    st, h0 = run(E, backend, P, E.new_state(Y0), 550, max_iter=1000, learning_rate=50.0, n_iter_without_progress=50)
    out, h = run(E, backend, P, st, 450, max_iter=1000, learning_rate=1e6, n_iter_without_progress=50)
    return h0, out, h


# ---------------------------------------------------------------------------------------------- the host backend
@pytest.mark.parametrize("sfx", ["", "1", "8"])
def test_host_affinities_against_root_and_reference(G, E, sfx):
    check_affinities_fixture(G, E, "host", sfx)


@pytest.mark.parametrize("n,D,perplexity", SHAPES)
def test_host_affinities_structure(E, n, D, perplexity):
    check_affinities_shape(E, "host", n, D, perplexity)


def test_host_kl_and_gradient_at_stored_states(G, E):
    check_stored_states(G, E, "host")


def test_host_one_iteration_from_stored_states(G, E):
    check_one_iteration(G, E, "host")


def test_host_state_machine(G, E):
    P, Y0 = small_problem(G, E)
    out, h = case_max_iter_250(E, "host", P, Y0)
    print("max_iter 250:", ints(E, h))
    assert h["done"] and h["n_iter"] == 249 and h["phase"] == 0 and E.STOP_NAMES[h["stop"]] == "max_iter"
    more, h2 = run(E, "host", P, out, 100, max_iter=250, learning_rate=50.0)
    assert same_state(out, more) and h2 == h                                    # after done nothing changes

    at250, h250, end, hend = case_boundary(E, "host", P, Y0)
    print("max_iter 300 at 250:", ints(E, h250), "\n  at the end:", ints(E, hend))
    assert h250["iteration"] == 250 and h250["phase"] == 1 and h250["n_iter"] == 249 and not h250["done"]
    assert h250["best_iteration"] == 250 and h250["best_error"] == np.finfo(np.float64).max and E.STOP_NAMES[h250["stop1"]] == "max_iter"
    assert np.all(at250["update"] == 0.0) and np.all(at250["gains"] == 1.0)
    assert at250["Y"].tobytes() == out["Y"].tobytes()                           # the same 250 iterations
    assert hend["done"] and hend["n_iter"] == 299 and E.STOP_NAMES[hend["stop"]] == "max_iter"

    Ps, Ys = stationary_start(E)
    out, h = case_stationary(E, "host", Ps, Ys)
    print("stationary start:", ints(E, h), "grad norm %.3e" % h["grad_norm"])
    assert h["done"] and h["n_iter"] == 299 and E.STOP_NAMES[h["stop"]] == "min_grad_norm"

    h0, out, h = case_no_progress(E, "host", P, Y0)
    print("no progress: at 550", ints(E, h0), "\n  at the end", ints(E, h), "best error %.6f, last error %.6f" % (h["best_error"], h["error"]))
    assert not h0["done"] and h0["iteration"] == 550 and h0["best_iteration"] == 549
    assert h["done"] and E.STOP_NAMES[h["stop"]] == "no_progress" and h["phase"] == 1
    assert h["n_iter"] == 649 and h["best_iteration"] == 549 and h["error"] >= h["best_error"]     # 599 - 549 = 50 is not yet more than 50


def test_host_plumbing(G, E):
    X = G["X"][:65]
    kw = dict(perplexity=20, n_iter=250, init="random", random_state=5, backend="host")
    a = E.DeviceTSNE(**kw).fit(X)
    assert a.max_iter == 250 and a.n_iter_ == 249 and a.learning_rate_ == 50.0 and a.n_features_in_ == 4
    assert isinstance(a.embedding_, np.ndarray) and a.embedding_.shape == (65, 2)
    wide = np.full((90, 22), np.nan)
    perm = np.random.default_rng(0).permutation(90)[:65]
    wide[perm[:, None], np.array([13, 14, 15, 16])[None, :]] = X
    b = E.DeviceTSNE(**kw).fit(wide, columns=[13, 14, 15, 16], row_index=perm)
    assert a.embedding_.tobytes() == b.embedding_.tobytes() and a.kl_divergence_ == b.kl_divergence_
    P, _, _ = E.joint_probabilities(X, 20, backend="host")
    ref = E.kl_and_gradient(P, a.embedding_, backend="host")
    print("kl_divergence_ %.12f, kl_and_gradient %.12f" % (a.kl_divergence_, ref["kl"]))
    assert abs(a.kl_divergence_ - ref["kl"]) <= kl_tolerance(ref, 1.0)
    bad = X.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        E.DeviceTSNE(**kw).fit(bad)
    with pytest.raises(ValueError):
        E.DeviceTSNE(perplexity=65, backend="host").fit(X)
    with pytest.raises(NotImplementedError, match="approximates"):
        E.DeviceTSNE(method="barnes_hut")
    with pytest.raises(NotImplementedError):
        E.DeviceTSNE(n_components=3)
    with pytest.raises(NotImplementedError):
        E.DeviceTSNE(metric="cosine")
    with pytest.raises(NotImplementedError):
        E.DeviceTSNE(**kw).fit(np.random.default_rng(0).random((65, 9)))
    assert E.DeviceTSNE(verbose=1, learning_rate=10.0)._lr(1000) == 10.0 and E.DeviceTSNE()._lr(11000) == 11000 / 12.0 / 4.0


def test_pca_initialisation(G, E):
    X = G["X"]
    Y = E._host_pca(X)
    lam = np.sort(np.linalg.eigvalsh(np.cov(X.T)))[::-1]
    bound = 1e3 * EPS * lam[0] / min(lam[0] - lam[1], lam[1] - lam[2]) * np.abs(G["Y_pca"]).max()     # eigenvectors move by eps |C| / gap
    d = np.abs(Y - G["Y_pca"]).max()
    print("PCA start: max |Y - scikit-learn's| = %.3e (bound %.3e), std of column 0 = %.6e" % (d, bound, Y[:, 0].std()))
    assert d <= bound and abs(Y[:, 0].std() - 1e-4) <= 1e-18


def test_trustworthiness(G, E):
    for k, ref in zip((5, 10), G["trust"]):
        t = E.trustworthiness(G["X"], G["Y_final"], n_neighbors=k)
        print("trustworthiness(%d) = %.15f, scikit-learn %.15f" % (k, t, ref))
        assert abs(t - ref) <= 1e-12                                            # gate 10
    with pytest.raises(ValueError):
        E.trustworthiness(G["X"][:10], G["Y_final"][:10], n_neighbors=5)


def check_end_to_end(G, E, backend, wrap=lambda a: a):
    f = float(G["band_factor"])
    kl_hi = G["band_kl"].max() + f * (G["band_kl"].max() - G["band_kl"].min())
    tr_lo = G["band_trust"].min() - f * (G["band_trust"].max() - G["band_trust"].min())
    m = E.DeviceTSNE(backend=backend, **E.TSNE_TEST_PARAMS).fit(wrap(G["X"]))
    t = E.trustworthiness(G["X"], host(m.embedding_), n_neighbors=10)
    print("end to end (%s): KL %.6f (at most %.6f; the reference's runs %.6f .. %.6f), trustworthiness %.6f (at least %.6f), n_iter_ %d"
          % (backend, m.kl_divergence_, kl_hi, G["band_kl"].min(), G["band_kl"].max(), t, tr_lo, m.n_iter_))
    assert m.kl_divergence_ <= kl_hi and t >= tr_lo                             # gate 11
    return m


def test_host_end_to_end_band(G, E):
    check_end_to_end(G, E, "host")


def results_array(G):
    """A results array [120, 22] with the fixture's rows in the posterior columns, labels with unmapped values, NaN rows."""
    rng = np.random.default_rng(11)
    res = rng.random((120, 22))
    res[:, 13:17] = G["X"][:120]
    res[:, 17] = rng.choice([0, 1, 2, 3, 7, 99], size=120)
    res[[5, 50], 14] = np.nan
    res[17, 16] = np.inf
    return res, {0: 0, 1: 1, 2: 1, 3: 2}


def check_helpers(G, E, backend, wrap=lambda a: a):
    from pinn_amd.diagnosis import extract_X_y
    res, label_map = results_array(G)
    X2, y2 = extract_X_y(res, [13, 15], label_map, backend="host")
    xy, y, used = E.scatter_by_features(wrap(res), [13, 15], label_map, backend=backend)
    assert used is False and host(xy).tobytes() == X2.tobytes() and np.array_equal(host(y), y2)
    X4, y4 = extract_X_y(res, [13, 14, 15, 16], label_map, backend="host")
    xy, y, used = E.scatter_by_features(wrap(res), [13, 14, 15, 16], label_map, backend=backend, max_iter=250)
    ref = E.DeviceTSNE(backend=backend, **{**E.TSNE_PARAMS, "max_iter": 250}).fit_transform(wrap(X4))
    print("scatter_by_features: %d of %d rows kept" % (len(y4), len(res)))
    assert used is True and np.array_equal(host(y), y4) and host(xy).shape == (len(y4), 2) and len(y4) < 120 - 3
    assert host(xy).tobytes() == host(ref).tobytes()
    assert E.TSNE_TEST_PARAMS == dict(n_components=2, perplexity=20, learning_rate="auto", init="pca", random_state=42, n_iter=1000)
    assert E.TSNE_PARAMS == dict(n_components=2, perplexity=30, learning_rate="auto", init="pca", random_state=49)
    y_pred = np.arange(len(y4)) % 3
    emb, groups = E.tsne_of_test_samples(wrap(X4), y_pred, backend=backend, n_iter=250)
    ref = E.DeviceTSNE(backend=backend, **{**E.TSNE_TEST_PARAMS, "n_iter": 250}).fit_transform(wrap(X4))
    assert host(emb).tobytes() == host(ref).tobytes() and sorted(groups) == [0, 1, 2]
    assert np.array_equal(np.sort(np.concatenate([groups[c] for c in groups])), np.arange(len(y4)))


def duplicated_rows(G):
    """The fixture's first 40 rows with row 0 repeated 25 times (more than the perplexity of 20) and row 1 three times."""
    X = G["X"][:40].copy()
    X[2:26] = X[0]
    X[26:28] = X[1]
    return X


def check_duplicates(G, E, backend, wrap=lambda a: a):
    """Rows with at least `perplexity` exact duplicates have no root; they get the limit, 1 / m on their duplicates."""
    X = duplicated_rows(G)
    P, beta, H = (host(a) for a in E.joint_probabilities(wrap(X), 20.0, backend=backend))
    n = 40
    copies = np.array([0] + list(range(2, 26)))
    d = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    m = (d == d.min(axis=1)[:, None]).sum(axis=1)                               # copies are exact: so are these equalities
    dup, rest = np.flatnonzero(m >= 20), np.flatnonzero(m < 20)
    print("duplicates (%s): rows without a root %s (m = %s), beta of row 0 %r, entropy %.6f (log 24 = %.6f)"
          % (backend, dup.tolist(), sorted(set(m[dup].tolist())), beta[0], H[0], np.log(24.0)))
    assert set(copies) <= set(dup) and np.all(m[copies] == 24) and {1, 26, 27} <= set(rest)     # a row nearest to the copies has m = 25
    assert np.all(np.isinf(beta[dup])) and np.all(H[dup] == np.log(m[dup])) and np.all(np.isfinite(beta[rest]))
    assert np.abs(row_entropy(X, beta)[rest] - np.log(20.0)).max() <= 1e-10     # the three copies of row 1 have a root
    assert P.tobytes() == np.ascontiguousarray(P.T).tobytes() and np.all(np.diag(P) == 0.0) and abs(P.sum() - 1.0) <= n * n * EPS
    # p_{j|i} of a duplicated row is 1 / 24 on the other copies and 0 elsewhere: P among the copies is 2 / 24 / (2 n)
    block = P[np.ix_(copies, copies)][~np.eye(25, dtype=bool)]
    assert np.abs(block - 1.0 / 24.0 / n).max() <= 4 * EPS / n
    m = E.DeviceTSNE(perplexity=20, n_iter=250, init="random", random_state=1, backend=backend).fit(wrap(X))
    assert np.isfinite(host(m.embedding_)).all() and np.isfinite(m.kl_divergence_)
    return P


def test_host_duplicated_rows(G, E):
    check_duplicates(G, E, "host")


def test_auto_backend_rule(G, E, monkeypatch):
    """backend="auto": the device for a host array of at least AUTO_DEVICE_ROWS rows when a GPU is present, else the host."""
    assert E.AUTO_DEVICE_ROWS == 256 and E.AUTO_DEVICE_ROWS <= E.MAX_ROWS
    small, large = np.zeros((255, 4)), np.zeros((256, 4))
    for present, want in ((True, "device"), (False, "host")):
        monkeypatch.setattr(E._device, "_gpu_present", lambda: present)
        assert E._pick_backend("auto", small) == "host" and E._pick_backend("auto", large) == want
        assert E._pick_backend("auto", np.zeros((9000, 22)), 100) == "host"        # rows picked by a gather list count
        assert E._pick_backend("auto", np.zeros((100, 22)), 300) == want
        assert E._pick_backend("host", large) == "host" and E._pick_backend("device", small) == "device"
    with pytest.raises(ValueError):
        E._pick_backend("gpu", large)
    monkeypatch.setattr(E._device, "_gpu_present", lambda: False)
    m = E.DeviceTSNE(perplexity=20, n_iter=250, init="random", random_state=1).fit(G["X"][:65])
    assert m.backend == "auto" and m.backend_ == "host"


def test_shape_errors(G, E):
    P, Y = full(G["P_sk8"]), np.zeros((65, 2))
    for backend in ("host", "device"):                                          # raised before a backend is touched
        with pytest.raises(ValueError, match="P must be"):
            E.kl_and_gradient(P[:, :60], Y, backend=backend)
        with pytest.raises(ValueError, match="Y must be"):
            E.kl_and_gradient(P, Y[:60], backend=backend)
        with pytest.raises(ValueError, match="P must be"):
            E.descend(P[:60], E.new_state(Y), 1, backend=backend)
        with pytest.raises(ValueError, match="state"):
            E.descend(P, E.new_state(Y[:60]), 1, backend=backend)


def test_host_script_helpers(G, E):
    check_helpers(G, E, "host")                                                 # gate 12


def test_module_needs_numpy_only():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import pinn_amd.embedding as e; "
            "assert 'sklearn' not in sys.modules and 'torch' not in sys.modules and 'scipy' not in sys.modules; print(e.TSNE_PARAMS)")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code % root], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
