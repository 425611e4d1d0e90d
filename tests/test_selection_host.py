"""CPU: pinn_amd.selection on the host backend (the referee of the device sweep), its criteria against scikit-learn's, the
fixture selections of the grid K in {2, 4, 8, 12, 16, 20, 24, 32} x seeds 0-2, and the host checks of the
pinn_gmm_batch_* entry points (no device needed: every call fails, or sizes something, on the host).  Every comparison
prints its figures before it asserts."""
import ctypes

import numpy as np
import pytest

import selection_cases as SC


@pytest.fixture(scope="module")
def S():
    from pinn_amd import selection
    return selection


def test_exports():
    import pinn_amd
    from pinn_amd import selection
    assert pinn_amd.gmm_sweep is selection.gmm_sweep and pinn_amd.select_gmm is selection.select_gmm
    assert pinn_amd.GMMSweep is selection.GMMSweep


def test_host_sweep_is_the_loop_of_host_fits(S):
    from pinn_amd.diagnosis import DeviceGMM
    G, sw = SC.fixture(), SC.host_sweep()
    assert list(sw.n_components) == [K for K in SC.GRID_K for _ in SC.SEEDS] and list(sw.seed) == list(SC.SEEDS) * len(SC.GRID_K)
    for K, seed in ((4, 1), (20, 2), (8, 0)):
        i = int(np.flatnonzero((sw.n_components == K) & (sw.seed == seed))[0])
        ref = DeviceGMM(K, random_state=seed, backend="host").fit(G["X_tr"])
        m = sw.model(i)
        for name in ("weights_", "means_", "covariances_", "precisions_cholesky_"):
            assert getattr(m, name).tobytes() == getattr(ref, name).tobytes(), (K, seed, name)
        print("K=%d seed %d: n_iter %d / %d, lower bound %.12f / %.12f" % (K, seed, sw.n_iter[i], ref.n_iter_, sw.lower_bound[i], ref.lower_bound_))
        assert sw.n_iter[i] == m.n_iter_ == ref.n_iter_ and bool(sw.converged[i]) == m.converged_ == ref.converged_
        assert sw.lower_bound[i] == m.lower_bound_ == ref.lower_bound_
        assert sw.loglik[i] == ref.score_samples(G["X_tr"]).sum() and sw.val_score[i] == ref.score(G["X_te"])
    # the rows of a wider array, read through columns and gather lists, are the same candidates
    wide = np.full((2700, 7), np.nan)
    tr, te = np.arange(0, 2 * 1349, 2), np.arange(1, 901, 2)
    wide[np.ix_(tr, [5, 1, 2, 6])] = G["X_tr"]
    wide[np.ix_(te, [5, 1, 2, 6])] = G["X_te"]
    a = S.gmm_sweep(wide, (4, 8), (1,), columns=[5, 1, 2, 6], row_index=tr, val_index=te, backend="host")
    sel = [int(np.flatnonzero((sw.n_components == K) & (sw.seed == 1))[0]) for K in (4, 8)]
    for name in ("n_iter", "lower_bound", "loglik", "bic", "aic", "val_score"):
        assert getattr(a, name).tobytes() == getattr(sw, name)[sel].tobytes(), name
    with pytest.raises(ValueError):
        S.gmm_sweep(G["X_tr"], (2,), (0,), val_index=[0], X_val=G["X_te"], backend="host")
    with pytest.raises(ValueError):
        sw.best("accuracy")
    with pytest.raises(ValueError):
        S.gmm_sweep(G["X_tr"][:50], (2,), (0,), backend="host").best("val_score")


def test_criteria_against_scikit_learn(S):
    mixture = pytest.importorskip("sklearn.mixture")
    G, sw = SC.fixture(), SC.host_sweep()
    X = G["X_tr"]
    worst = 0.0
    for i in range(0, len(sw), 2):
        m = sw.model(i)
        sk = mixture.GaussianMixture(n_components=int(sw.n_components[i]), covariance_type="full")
        sk.weights_, sk.means_, sk.covariances_, sk.precisions_cholesky_ = m.weights_, m.means_, m.covariances_, m.precisions_cholesky_
        assert sk._n_parameters() == sw.n_parameters[i]
        for got, want in ((sw.aic[i], sk.aic(X)), (sw.bic[i], sk.bic(X))):
            worst = max(worst, abs(got - want) / abs(want))
    print("aic / bic against scikit-learn: largest relative difference %.3e (gate 1e-12)" % worst)
    assert worst <= 1e-12
    assert np.array_equal(S.n_parameters([1, 20], 4), [4 + 10, 20 * 4 + 20 * 10 + 19])


def test_fixture_selection(S):
    G, sw = SC.fixture(), SC.host_sweep()
    SC.check_conditions(sw, SC.host_margins())
    SC.check_selections(sw, G)
    per_K = SC.best_bic_per_K(sw)
    print("best BIC per K:", per_K)
    for K, want in ((2, -8686.7), (8, -11582.6), (20, -10529.4), (32, -9509.0)):       # the figures of DESIGN 3g's table
        assert abs(per_K[K] - want) <= 0.05
    # select_gmm is the sweep plus the pick; n_init's rule is criterion="lower_bound" over the seeds of one K
    g, sw20 = S.select_gmm(G["X_tr"], (20,), SC.SEEDS, criterion="lower_bound", backend="host")
    assert g.random_state == 1 and g.n_components == 20 and g.lower_bound_ == sw20.lower_bound.max()
    with pytest.raises(ValueError):
        S.select_gmm(G["X_tr"], (2,), (0,), criterion="loglik", backend="host")


def test_singular_candidate_on_the_host(S):
    """Two identical rows form a cluster of their own; with reg_covar=0 its covariance has no Cholesky factor."""
    X = SC.duplicated_rows()
    sw = S.gmm_sweep(X, (2, 1), (1,), reg_covar=0.0, backend="host")
    print("status", sw.status, "bic", sw.bic)
    assert list(sw.status) == [1, 0] and np.isnan(sw.bic[0]) and np.isfinite(sw.bic[1])
    assert sw.best("bic") == 1
    with pytest.raises(ValueError, match="positive definite"):
        sw.model(0)
    assert sw.diagnosis_metrics(X, np.zeros(52, int), X, np.zeros(52, int), 2)[0] is None
    g, _ = S.select_gmm(X, (2, 1), (1,), reg_covar=0.0, backend="host")
    assert g.n_components == 1


# ---------------------------------------------------------------------------------------------- the C ABI's host checks
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    return _lib.load(build_if_missing=False)


E_ARG, E_WS = -1, -3
ONE, ODD = 0x1000, 0x1004                 # addresses that are never dereferenced: every call below fails on the host
BIG = 1 << 40


def _calls(lib):
    """name -> function of keyword overrides; the defaults pass every host check but the one under test."""
    cols = (ctypes.c_int * 2)(0, 1)

    def make(name, tail):
        def f(**kw):
            a = dict(arr=ONE, ld=2, n_arr=100, cols=cols, D=2, ridx=None, n=10, B=2, ncomp=(3, 5), maxc=5, state=ONE, ws=ONE, ws_bytes=BIG,
                     first=ONE, u=ONE, picks=None, labels=ONE, sums=ONE, iters=1)
            a.update(kw)
            nc = None if a["ncomp"] is None else (ctypes.c_int * len(a["ncomp"]))(*a["ncomp"])
            head = [a["arr"], a["ld"], a["n_arr"], a["cols"], a["D"], a["ridx"], a["n"], a["B"], nc, a["maxc"]]
            return getattr(lib, name)(*(head + [a[t] if isinstance(t, str) else t for t in tail] + [a["ws"], a["ws_bytes"], None]))
        return f
    return {
        "pinn_gmm_batch_seed": make("pinn_gmm_batch_seed", ["first", "u", "state", "picks"]),
        "pinn_gmm_batch_kmeans": make("pinn_gmm_batch_kmeans", ["iters", "state", "labels"]),
        "pinn_gmm_batch_mstep_init": make("pinn_gmm_batch_mstep_init", ["labels", 1e-6, "state"]),
        "pinn_gmm_batch_em": make("pinn_gmm_batch_em", ["iters", 1e-3, 1e-6, "state"]),
        "pinn_gmm_batch_score": make("pinn_gmm_batch_score", ["state", "sums"]),
    }


def test_batch_entry_points_check_their_arguments_on_the_host(lib):
    need = lib.pinn_gmm_batch_workspace_bytes(10, 2, 5, 2)
    assert need > 0
    for name, f in _calls(lib).items():
        bad = {
            "NULL state": dict(state=None), "NULL workspace": dict(ws=None), "NULL array": dict(arr=None), "NULL n_comp": dict(ncomp=None),
            "n_batch 0": dict(B=0), "n_batch 1025": dict(B=1025, ncomp=(1,) * 1025), "n_comp 0": dict(ncomp=(3, 0)),
            "n_comp above max_comp": dict(ncomp=(6, 5)), "max_comp 33": dict(maxc=33, ncomp=(3, 33)), "max_comp 0": dict(maxc=0),
            "n_feat 9": dict(D=9), "no rows": dict(n=0), "misaligned state": dict(state=ODD), "misaligned workspace": dict(ws=ODD),
            "misaligned array": dict(arr=ODD), "misaligned gather list": dict(ridx=ODD),
        }
        if name == "pinn_gmm_batch_seed":
            bad.update({"NULL first": dict(first=None), "NULL uniforms": dict(u=None), "misaligned uniforms": dict(u=ODD),
                        "misaligned picks": dict(picks=ODD)})
        if name in ("pinn_gmm_batch_kmeans", "pinn_gmm_batch_mstep_init"):
            bad.update({"NULL labels": dict(labels=None), "misaligned labels": dict(labels=ODD)})
        if name in ("pinn_gmm_batch_kmeans", "pinn_gmm_batch_em"):
            bad.update({"negative iterations": dict(iters=-1)})
        if name == "pinn_gmm_batch_score":
            bad.update({"NULL sums": dict(sums=None), "misaligned sums": dict(sums=ODD)})
        for what, kw in bad.items():
            assert f(**kw) == E_ARG, (name, what)
        assert f(ws_bytes=need - 1) == E_WS, name
        assert f(ws_bytes=0) == E_WS, name
        assert f(B=1024, ncomp=(5,) * 1024, ws_bytes=need) == E_WS, name        # sized for 2 candidates, asked for 1024


def test_batch_sizes(lib):
    from pinn_amd import _lib
    assert _lib.GMM_MAX_BATCH == 1024
    for K, D in ((1, 1), (20, 4), (32, 8)):
        assert lib.pinn_gmm_batch_state_stride(K, D) == lib.pinn_gmm_state_bytes(K, D) > 0
    for K, D in ((0, 4), (33, 4), (20, 0), (20, 9)):
        assert lib.pinn_gmm_batch_state_stride(K, D) == 0
        assert lib.pinn_gmm_batch_workspace_bytes(1000, 4, K, D) == 0
    for n, B in ((-1, 4), (1000, 0), (1000, 1025)):
        assert lib.pinn_gmm_batch_workspace_bytes(n, B, 20, 4) == 0
    one = lib.pinn_gmm_batch_workspace_bytes(1349, 1, 32, 4)
    assert one > 0 and lib.pinn_gmm_batch_workspace_bytes(1349, 1024, 32, 4) == 1024 * one
    assert lib.pinn_gmm_batch_workspace_bytes(1349, 1, 32, 4) < lib.pinn_gmm_batch_workspace_bytes(131073, 1, 32, 4)
    # a candidate's block holds its partial sums (11 workgroups at 1349 rows) and the seeding's distances, not 1024 blocks' worth
    assert one < lib.pinn_gmm_workspace_bytes(1349, 32, 4) // 16
