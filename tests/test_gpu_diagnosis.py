"""GPU: the device backend of pinn_amd.diagnosis (csrc/pinn_gmm.hip) against tests/golden/g_gmm.npz and against the
package's host backend (float64 numpy, scikit-learn's formulas, covariances in two passes).

Gates (from the reference's own sensitivity and the arithmetic, not from what the kernels give): a full fit
within 10 x the sensitivity of the referee to 1e-13 relative input noise (not below 1e-13) with n_iter_ equal; one EM
iteration: every moment sum within 1e-12 x the sum of its absolute terms, log_prob_norm atol 1e-10, resp atol 1e-9;
covariances of data offset by 1e4 sigma within 1e-10 of each matrix's largest entry.  In-place and gathered reads, repeated
calls and chunked diagnosis are compared bit for bit.  Every comparison prints its maxima before it asserts."""
import types

import numpy as np
import pytest
import torch

from test_diagnosis_host import check_fit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(golden):
    return golden("g_gmm.npz")


@pytest.fixture(scope="module")
def D():
    from pinn_amd import diagnosis
    return diagnosis


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def as_numpy_model(gmm):
    return types.SimpleNamespace(weights_=host(gmm.weights_), means_=host(gmm.means_), covariances_=host(gmm.covariances_),
                                 precisions_cholesky_=host(gmm.precisions_cholesky_), n_iter_=gmm.n_iter_, converged_=gmm.converged_,
                                 lower_bound_=gmm.lower_bound_)


def clustered(n, K, Dm, seed, spread=4.0):
    """n rows around K centres with unequal feature scales; returns X and the centre of every row."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, spread, (K, Dm))
    z = rng.integers(K, size=n)
    X = centres[z] + rng.normal(0.0, 1.0, (n, Dm)) * rng.uniform(0.5, 1.5, Dm)
    return X, z


def soft_resp(n, K, z, seed):
    """Half of every row's weight on its own centre, half spread at random: every component sees every row, so that no
    covariance is decided by two or three rows."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.0, 1.0, (n, K))
    r = 0.5 * r / r.sum(axis=1, keepdims=True)
    r[np.arange(n), z] += 0.5
    return r


def copy_params(D, src, K, **kw):
    """A device-backend mixture holding exactly the parameters of `src`."""
    g = D.DeviceGMM(K, backend="device", **kw)
    g.weights_, g.means_, g.covariances_, g.precisions_cholesky_ = (a.copy() for a in (src.weights_, src.means_, src.covariances_,
                                                                                        src.precisions_cholesky_))
    g.n_iter_, g.converged_, g.lower_bound_, g.lower_bound_changes_ = src.n_iter_, src.converged_, src.lower_bound_, []
    return g


def rel_cov(a, b):
    return (np.abs(a - b) / np.abs(b).max(axis=(1, 2), keepdims=True)).max()


def test_device_matches_reference_fixture(G, D):
    kw = dict(random_state=42, n_components=20, backend="device", labels_init=G["labels_init"])
    y_prob, y_pred, gmm, cfp = D.fit_gmm_and_get_probabilities(G["X_tr"], G["y_tr"], G["X_te"], 4, **kw)
    for a in (y_prob, y_pred, cfp, gmm.weights_, gmm.means_, gmm.covariances_, gmm.precisions_cholesky_):
        assert isinstance(a, np.ndarray)
    check_fit(G, gmm, y_prob, y_pred, cfp, "device, numpy in")
    t_prob, t_pred, tg, t_cfp = D.fit_gmm_and_get_probabilities(dev(G["X_tr"]), dev(G["y_tr"]), dev(G["X_te"]), 4, **kw)
    for a in (t_prob, t_pred, t_cfp, tg.weights_, tg.means_, tg.covariances_, tg.precisions_cholesky_):
        assert isinstance(a, torch.Tensor) and a.is_cuda
    check_fit(G, as_numpy_model(tg), host(t_prob), host(t_pred), host(t_cfp), "device, tensor in")
    assert host(t_prob).tobytes() == y_prob.tobytes() and host(tg.covariances_).tobytes() == gmm.covariances_.tobytes()
    # first E-step of the fixture
    g0 = D.DeviceGMM(20, labels_init=G["labels_init"], max_iter=0, backend="device").fit(G["X_tr"])
    e_l = np.abs(g0.score_samples(G["X_tr"]) - G["log_prob_norm0"]).max()
    e_r = np.abs(g0.predict_proba(G["X_tr"])[:300] - G["resp0_head"]).max()
    print("first E-step: log_prob_norm err %.3e (gate 1e-10), resp err %.3e (gate 1e-9)" % (e_l, e_r))
    assert g0.n_iter_ == 0 and e_l <= 1e-10 and e_r <= 1e-9
    assert abs(g0.score(G["X_tr"]) - float(np.mean(G["log_prob_norm0"]))) <= 1e-10
    assert np.array_equal(gmm.predict(G["X_te"]), gmm.predict_proba(G["X_te"]).argmax(axis=1))


CASES = [(1, 1, 1), (63, 4, 2), (64, 20, 4), (65, 32, 8), (2049, 1, 2), (2049, 32, 1), (100003, 20, 4), (100003, 4, 8), (1000000, 20, 4)]


@pytest.mark.parametrize("n,K,Dm", CASES)
def test_one_em_iteration_against_the_host(D, n, K, Dm):
    X, z = clustered(n, K, Dm, seed=n + K + Dm)
    R = soft_resp(n, K, z, seed=n)
    gh = D.DeviceGMM(K, resp_init=R, max_iter=0, backend="host").fit(X)
    # the initial M-step itself (two passes on both sides)
    gi = D.DeviceGMM(K, resp_init=R, max_iter=0, backend="device").fit(X)
    e_w, e_m = np.abs(gi.weights_ - gh.weights_).max(), np.abs(gi.means_ - gh.means_).max() / max(np.abs(gh.means_).max(), 1e-300)
    e_c = rel_cov(gi.covariances_, gh.covariances_)
    print("n=%d K=%d D=%d init: weights %.3e means %.3e covariances %.3e (gates 1e-13, 1e-13, 1e-12)" % (n, K, Dm, e_w, e_m, e_c))
    assert e_w <= 1e-13 and e_m <= 1e-13 and e_c <= 1e-12
    # one iteration from identical parameters
    gd = copy_params(D, gh, K)
    Xd = dev(X)
    lpn_h, resp_h = gh.score_samples(X), gh.predict_proba(X)
    e_l = np.abs(host(gd.score_samples(Xd)) - lpn_h).max()
    e_r = np.abs(host(gd.predict_proba(Xd)) - resp_h).max()
    mom_h, abs_h = gh.em_iterations(X, 1, return_moments=True)
    mom_d = host(gd.em_iterations(Xd, 1, return_moments=True))
    ratio = (np.abs(mom_d - mom_h) / np.maximum(abs_h, 1e-300)).max()
    print("  log_prob_norm %.3e (gate 1e-10)  resp %.3e (gate 1e-9)  moments %.3e of sum|terms| (gate 1e-12)" % (e_l, e_r, ratio))
    assert e_l <= 1e-10 and e_r <= 1e-9
    assert np.all(np.abs(mom_d - mom_h) <= 1e-12 * abs_h)
    assert gd.n_iter_ == gh.n_iter_ == 1 and abs(gd.lower_bound_ - gh.lower_bound_) <= 1e-10
    e_c = rel_cov(host(gd.covariances_), gh.covariances_)
    print("  after the M-step: covariances %.3e means %.3e" % (e_c, np.abs(host(gd.means_) - gh.means_).max()))
    assert e_c <= 1e-10


@pytest.mark.parametrize("n", [2049, 100003])
def test_full_fit_against_the_host(D, n):
    K, Dm, tol = 8, 4, 1e-3
    for seed in range(5):
        X, z = clustered(n, K, Dm, seed=100 + seed, spread=2.0)
        rng = np.random.default_rng(seed)
        lab = np.where(rng.uniform(size=n) < 0.3, rng.integers(K, size=n), z)      # 30 % of the rows start in a random component

        def fit(Xf, backend="host"):
            return D.DeviceGMM(K, labels_init=lab, tol=tol, backend=backend).fit(Xf)
        ref = fit(X)
        ch = np.array(ref.lower_bound_changes_)
        if ref.converged_ and np.min(np.abs(np.abs(ch) - tol)) >= 1e-8:
            break
    else:
        pytest.fail("no draw met the convergence-margin condition")

    def dist(g, h):
        return np.array([np.abs(host(g.weights_) - h.weights_).max(), np.abs(host(g.means_) - h.means_).max() / np.abs(h.means_).max(),
                         rel_cov(host(g.covariances_), h.covariances_), abs(g.lower_bound_ - h.lower_bound_)])
    sens = np.zeros(4)
    prng = np.random.default_rng(999)
    for _ in range(5):
        p = fit(X * (1.0 + 1e-13 * prng.uniform(-1.0, 1.0, X.shape)))
        assert p.n_iter_ == ref.n_iter_
        sens = np.maximum(sens, dist(p, ref))
    gate = np.maximum(10.0 * sens, 1e-13)
    got = fit(X, "device")
    err = dist(got, ref)
    print("n=%d seed %d: n_iter host %d device %d" % (n, seed, ref.n_iter_, got.n_iter_))
    for name, e, g_ in zip(("weights", "means", "covariances", "lower_bound"), err, gate):
        print("  %-12s err %.3e  gate %.3e" % (name, e, g_))
    assert got.n_iter_ == ref.n_iter_ and got.converged_
    assert np.all(err <= gate)


def test_offsets_do_not_cancel(D):
    """Every feature shifted by 1e4 of its standard deviation: raw second moments would lose 1.8e-7 of a covariance here."""
    n, K, Dm = 20011, 4, 4
    X, z = clustered(n, K, Dm, seed=5)
    X = X + 1e4 * X.std(axis=0)
    R = soft_resp(n, K, z, seed=6)
    gh = D.DeviceGMM(K, resp_init=R, max_iter=0, backend="host").fit(X)
    gi = D.DeviceGMM(K, resp_init=R, max_iter=0, backend="device").fit(X)
    e0 = rel_cov(gi.covariances_, gh.covariances_)
    gd = copy_params(D, gh, K)
    gh.em_iterations(X, 1)
    gd.em_iterations(X, 1)
    e1 = rel_cov(gd.covariances_, gh.covariances_)
    print("offset 1e4 sigma: covariances init %.3e, after one iteration %.3e (gate 1e-10)" % (e0, e1))
    assert e0 <= 1e-10 and e1 <= 1e-10


def test_in_place_columns_and_gather_equal_the_packed_copy(D):
    n, K = 30011, 6
    rng = np.random.default_rng(2)
    a = rng.normal(size=(n, 22))
    Xc, z = clustered(n, K, 4, seed=3)
    cols = [13, 14, 15, 16]
    a[:, cols] = Xc
    idx = np.sort(rng.choice(n, size=20001, replace=False))
    lab = z[idx]
    ad, packed = dev(a), dev(a[idx][:, cols])
    g1 = D.DeviceGMM(K, labels_init=lab, backend="device").fit(ad, columns=cols, row_index=dev(idx))
    g2 = D.DeviceGMM(K, labels_init=lab, backend="device").fit(packed)
    assert g1.n_iter_ == g2.n_iter_ and g1.n_iter_ >= 1
    assert host(g1._state).tobytes() == host(g2._state).tobytes()
    p1 = g1._posterior(ad, cols, dev(idx), want=("log_prob_norm", "resp"))
    p2 = g2._posterior(packed, want=("log_prob_norm", "resp"))
    for k in p1:
        assert host(p1[k]).tobytes() == host(p2[k]).tobytes()
    m1 = g1.label_map(ad, dev(lab % 4), 4, columns=cols, row_index=dev(idx))
    m2 = g2.label_map(packed, dev(lab % 4), 4)
    assert host(m1).tobytes() == host(m2).tobytes()
    # a gather index outside the array reads nothing: NaN out, nothing else disturbed
    bad = dev(np.array([0, n + 5, 1, -1], dtype=np.int64))
    r = host(g1._posterior(ad, cols, bad, want=("resp",))["resp"])
    assert np.isnan(r[[1, 3]]).all() and np.isfinite(r[[0, 2]]).all()


def test_identical_calls_give_identical_bytes(G, D):
    def run():
        out = D.fit_gmm_and_get_probabilities(dev(G["X_tr"]), dev(G["y_tr"]), dev(G["X_te"]), 4, random_state=7, n_components=20,
                                              backend="device")
        return [host(out[0]), host(out[1]), host(out[2]._state), host(out[3])], out[2]
    a, gmm = run()
    b, _ = run()
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    # the package's own initialisation meets the reference's own spread (gates as on the host)
    (lb_min, lb_max), (acc_min, acc_max) = G["lb_range"], G["acc_range"]
    acc = float((a[1] == G["y_te"]).mean())
    print("own initialisation on the device: lower bound %.4f (reference %.4f-%.4f), accuracy %.4f (reference %.4f-%.4f), n_iter %d"
          % (gmm.lower_bound_, lb_min, lb_max, acc, acc_min, acc_max, gmm.n_iter_))
    assert gmm.converged_ and gmm.lower_bound_ >= lb_min - (lb_max - lb_min) and acc >= acc_min - (acc_max - acc_min)


def test_fault_diagnoser_chunks_equal_one_call(D):
    K, C = 12, 4
    sizes = [1, 7, 4096, 100003]
    n = sum(sizes)
    Xc, z = clustered(n, K, 4, seed=11, spread=3.0)
    a = np.random.default_rng(12).normal(size=(n, 22))
    cols = D.parse_features(D.DEFAULT_FEATURES)
    a[:, cols] = Xc
    gmm = D.DeviceGMM(K, labels_init=z[:20000], backend="host").fit(Xc[:20000])
    cfp = gmm.label_map(Xc[:20000], z[:20000] % C, C)
    want_p, want_y = gmm.diagnose(Xc, cfp)
    top = np.sort(want_p, axis=1)
    clear = (top[:, -1] - top[:, -2]) >= 1e-6
    assert (~clear).mean() <= 1e-3                 # a condition on the draw, checked on the host result alone
    ad = dev(a)
    diag = D.FaultDiagnoser(gmm, cfp, backend="device")
    probs, preds, o = [], [], 0
    for s in sizes:
        p, y = diag.update(ad[o:o + s])
        assert p.is_cuda and p.shape == (s, C) and y.shape == (s,)
        probs.append(p)
        preds.append(y)
        o += s
    probs, preds = host(torch.cat(probs)), host(torch.cat(preds))
    err = np.abs(probs - want_p).max()
    print("FaultDiagnoser over chunks %s: y_prob err %.3e (gate 1e-9), rows inside the decision margin %d" % (sizes, err, (~clear).sum()))
    assert diag.n_seen == n and err <= 1e-9 and np.array_equal(preds[clear], want_y[clear])
    gdev = copy_params(D, gmm, K)
    whole_p, whole_y = gdev.diagnose(ad, dev(cfp), columns=cols)
    assert host(whole_p).tobytes() == probs.tobytes() and np.array_equal(host(whole_y), preds)
    resp_d = host(gdev.predict_proba(ad, columns=cols))
    assert np.abs(resp_d - gmm.predict_proba(Xc)).max() <= 1e-9


def test_extract_X_y_on_the_device(G, D):
    a = np.zeros((G["results_cols"].shape[0], 22))
    a[:, [13, 14, 15, 16, 17]] = G["results_cols"]
    mapping, _ = D.build_label_mapper(D.parse_group_spec(D.DEFAULT_GROUP_SPEC))
    X, y, kept = D.extract_X_y(dev(a), [13, 14, 15, 16], mapping, return_index=True)
    assert X.is_cuda and y.is_cuda and kept.is_cuda
    assert np.array_equal(host(kept), G["kept_rows"]) and np.array_equal(host(X)[G["idx_tr"]], G["X_tr"])
    assert np.array_equal(host(y)[G["idx_te"]], G["y_te"])
    m = D.classification_metrics(y, y, 4)
    assert m["accuracy"] == 1.0 and m["macro_f1"] == 1.0


def test_singular_component_raises_value_error(D):
    """Two duplicated rows own a component and reg_covar is 0: an arithmetic condition reported through the status word."""
    rng = np.random.default_rng(0)
    X = np.concatenate([rng.normal(size=(50, 3)), np.full((2, 3), 9.0)])
    lab = np.array([0] * 50 + [1, 1])
    gmm = D.DeviceGMM(2, labels_init=lab, reg_covar=0.0, backend="device")
    with pytest.raises(ValueError):
        gmm.fit(X)
    assert np.isfinite(host(gmm._state)[8:]).all() and not hasattr(gmm, "means_")
    ok = D.DeviceGMM(2, labels_init=lab, reg_covar=1e-6, backend="device").fit(X)      # the same rows with the default regularisation
    assert np.isfinite(ok.covariances_).all() and ok.n_iter_ >= 1
