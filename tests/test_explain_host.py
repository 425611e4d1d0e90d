"""CPU: the host backend of pinn_amd.explain (float64 numpy, the subset formula) against the orderings referee of
explain_cases.py and against the properties an exact Shapley value has.  Every comparison prints its maxima before it
asserts."""
import numpy as np
import pytest

from explain_cases import host_diagnose, mixture_rows, random_mixture, referee, report


@pytest.fixture(scope="module")
def E():
    from pinn_amd import explain
    return explain


def smooth(W):
    """An elementwise model (no BLAS: a row's value does not depend on the rows around it) with interactions."""
    def f(Z):
        Z = np.asarray(Z, dtype=np.float64)
        out = np.zeros((Z.shape[0], W.shape[1]))
        for c in range(W.shape[1]):
            lin = np.zeros(Z.shape[0])
            prod = np.ones(Z.shape[0])
            for i in range(Z.shape[1]):
                lin = lin + W[i, c] * Z[:, i]
                prod = prod * np.cos(0.3 * (i + 1) * Z[:, i] + c)
            out[:, c] = np.tanh(lin) + 0.5 * prod
        return out
    return f


@pytest.mark.parametrize("D", [1, 2, 4])
def test_host_backend_against_the_orderings_referee(E, D):
    g, cfp = random_mixture(5, D, 3, seed=D)
    X, _ = mixture_rows(g, 7, seed=10 + D)
    Bg, _ = mixture_rows(g, 9, seed=20 + D)
    r = E.shapley_diagnosis(g, cfp, X, Bg, backend="host")
    phi, base, fx = referee(host_diagnose(g, cfp), X, Bg)
    assert r.phi.shape == (7, D, 3) and r.base.shape == (3,) and r.fx.shape == (7, 3) and r.phi.dtype == np.float64
    e = [report("D=%d %s" % (D, n), a, b, 1e-13) for n, a, b in (("phi", r.phi, phi), ("base", r.base, base), ("fx", r.fx, fx))]
    assert max(e) <= 1e-13
    # the generic entry point with the same model is the same computation
    r2 = E.shapley_values(host_diagnose(g, cfp), X, Bg, backend="host")
    assert r2.phi.tobytes() == r.phi.tobytes() and r2.base.tobytes() == r.base.tobytes()


def test_efficiency_and_one_feature(E):
    rng = np.random.default_rng(0)
    for D in (1, 3, 8):
        f = smooth(rng.normal(0.0, 1.0, (D, 2)) * 3.0)
        X, Bg = rng.normal(0, 1, (4, D)), rng.normal(0, 1, (6, D))
        r = E.shapley_values(f, X, Bg, backend="host")
        gap = np.abs(r.phi.sum(axis=1) - (r.fx - r.base)) / np.maximum(1.0, np.abs(r.fx))
        print("D=%d efficiency gap %.3e (gate 1e-13)" % (D, gap.max()))
        assert gap.max() <= 1e-13
        assert report("fx", r.fx, f(X), 1e-15) <= 1e-15
        if D == 1:
            assert np.array_equal(r.phi[:, 0, :], r.fx - r.base)
        if D == 8:
            phi, base, fx = referee(f, X, Bg)
            assert report("D=8 phi against the subset referee", r.phi, phi, 1e-13) <= 1e-13


def test_linear_model_gives_the_closed_form(E):
    rng = np.random.default_rng(1)
    D, C = 5, 3
    W, c0 = rng.normal(0, 1, (D, C)), rng.normal(0, 1, C)
    X, Bg = rng.normal(0, 2, (6, D)), rng.normal(0, 2, (11, D))
    r = E.shapley_values(lambda Z: Z @ W + c0, X, Bg, backend="host")
    want = W[None, :, :] * (X - Bg.mean(axis=0))[:, :, None]
    rel = np.abs(r.phi - want).max() / np.abs(want).max()
    print("linear model: relative error %.3e (gate 1e-12)" % rel)
    assert rel <= 1e-12
    # a model with one output may return [m]
    r1 = E.shapley_values(lambda Z: Z @ W[:, 0] + c0[0], X, Bg, backend="host")
    assert r1.phi.shape == (6, D, 1) and r1.base.shape == (1,) and r1.fx.shape == (6, 1)
    assert np.abs(r1.phi[:, :, 0] - want[:, :, 0]).max() / np.abs(want).max() <= 1e-12


def test_an_ignored_feature_gets_nothing(E):
    rng = np.random.default_rng(2)
    D = 4
    W = rng.normal(0, 1, (D, 2)) * 2.0
    inner = smooth(W[[0, 1, 3]])
    f = lambda Z: inner(np.asarray(Z)[:, [0, 1, 3]])
    X, Bg = rng.normal(0, 1, (5, D)), rng.normal(0, 1, (8, D))
    r = E.shapley_values(f, X, Bg, backend="host")
    bound = 1e-15 * np.abs(f(np.concatenate([X, Bg]))).max()
    print("ignored feature: max |phi_2| %.3e (gate %.3e), max |phi| %.3e" % (np.abs(r.phi[:, 2]).max(), bound, np.abs(r.phi).max()))
    assert np.abs(r.phi[:, 2]).max() <= bound and np.abs(r.phi).max() > 1e-3


def test_chunking_and_a_single_background_row(E):
    rng = np.random.default_rng(3)
    D = 3
    f = smooth(rng.normal(0, 1, (D, 2)))
    X, Bg = rng.normal(0, 1, (5, D)), rng.normal(0, 1, (4, D))
    whole = E.shapley_values(f, X, Bg, backend="host")
    calls = []
    counted = lambda Z: (calls.append(Z.shape[0]), f(Z))[1]
    one = E.shapley_values(counted, X, Bg, backend="host", max_hybrid_rows=1)
    assert calls == [8 * 4] * 5                                   # one row per chunk
    for a, b in zip(whole, one):
        assert a.tobytes() == b.tobytes()
    # B = 1: v(S) is f of one hybrid row
    r = E.shapley_values(f, X, Bg[:1], backend="host")
    phi, base, fx = referee(f, X, Bg[:1])
    assert report("B=1 phi", r.phi, phi, 1e-14) <= 1e-14 and np.array_equal(r.base, f(Bg[:1])[0])
    # columns and gather lists read the same rows as the packed copy
    arr = rng.normal(0, 1, (9, 6))
    idx = np.array([7, 0, 3])
    a = E.shapley_values(f, arr, arr, columns=[4, 1, 2], row_index=idx, background_index=[1, 2, 8, 5], backend="host")
    b = E.shapley_values(f, arr[idx][:, [4, 1, 2]], arr[[1, 2, 8, 5]][:, [4, 1, 2]], backend="host")
    assert a.phi.tobytes() == b.phi.tobytes()
    # float32 hybrid rows reach the model as float32
    seen = []
    E.shapley_values(lambda Z: (seen.append(Z.dtype), f(Z))[1], X, Bg, backend="host", dtype="float32")
    assert seen == [np.dtype(np.float32)]


def test_errors(E):
    rng = np.random.default_rng(4)
    f1 = lambda Z: np.asarray(Z).sum(axis=1)
    with pytest.raises(ValueError, match="features"):
        E.shapley_values(f1, rng.normal(0, 1, (2, 9)), rng.normal(0, 1, (2, 9)), backend="host")
    with pytest.raises(ValueError, match="outputs"):
        E.shapley_values(lambda Z: np.zeros((Z.shape[0], 17)), rng.normal(0, 1, (2, 2)), rng.normal(0, 1, (2, 2)), backend="host")
    bad = rng.normal(0, 1, (3, 2))
    bad[1, 0] = np.inf
    with pytest.raises(ValueError, match="finite"):
        E.shapley_values(f1, rng.normal(0, 1, (2, 2)), bad, backend="host")
    for wrong in (lambda Z: np.zeros(Z.shape[0] + 1), lambda Z: np.zeros((2, Z.shape[0])), lambda Z: np.zeros((Z.shape[0], 1, 1))):
        with pytest.raises(ValueError, match="shape"):
            E.shapley_values(wrong, rng.normal(0, 1, (3, 2)), rng.normal(0, 1, (3, 2)), backend="host")
    with pytest.raises(ValueError):
        E.shapley_values(f1, rng.normal(0, 1, (2, 2)), rng.normal(0, 1, (0, 2)), backend="host")
    with pytest.raises(ValueError, match="dtype"):
        E.shapley_values(f1, rng.normal(0, 1, (2, 2)), rng.normal(0, 1, (2, 2)), backend="host", dtype="float16")
    with pytest.raises(ValueError, match="backend"):
        E.shapley_values(f1, rng.normal(0, 1, (2, 2)), rng.normal(0, 1, (2, 2)), backend="gpu")


def test_summaries_and_lazy_export(E):
    import pinn_amd
    assert pinn_amd.shapley_values is E.shapley_values and pinn_amd.DiagnosisExplainer is E.DiagnosisExplainer
    phi = np.zeros((2, 3, 2))
    phi[:, 0, 0], phi[:, 1, 0], phi[:, 2, 1] = [1.0, -3.0], [0.5, 0.5], [-2.0, -2.0]
    imp = E.global_importance(phi)
    assert imp.shape == (3, 2) and np.array_equal(imp[:, 0], [2.0, 0.5, 0.0])
    top = E.top_features(phi, ["pV", "pT", "pH"], ["flooding", "drying"], topn=2)
    assert [t["class"] for t in top] == ["flooding", "drying"]
    assert top[0]["importance"] == [("pV", 2.0), ("pT", 0.5)] and top[0]["positive"][0] == ("pT", 0.5) and top[0]["negative"][0] == ("pV", -1.0)
    assert top[1]["importance"][0] == ("pH", 2.0) and E.top_features(phi, ["a", "b", "c"], [], topn=0) == []
    # the weights of phi_j = sum_S c_j(S) v(S): they cancel over j for every proper coalition and their absolute values sum to 2
    for D in range(1, 9):
        c = E.coalition_weights(D)
        assert np.abs(np.abs(c).sum(axis=1) - 2.0).max() <= 1e-14 and np.abs(c[:, 1:-1].sum(axis=0)).sum() <= 1e-13


def test_explainer_on_the_host_follows_the_diagnoser(E):
    from pinn_amd import diagnosis
    g, cfp = random_mixture(4, 4, 4, seed=5)
    cols = diagnosis.parse_features(diagnosis.DEFAULT_FEATURES)
    rng = np.random.default_rng(6)
    res, bgr = rng.normal(0, 1, (6, 18)), rng.normal(0, 1, (5, 18))
    res[:, cols], bgr[:, cols] = mixture_rows(g, 6, seed=7)[0], mixture_rows(g, 5, seed=8)[0]
    ex = E.DiagnosisExplainer(g, cfp, bgr, backend="host")
    phi, y_prob = ex.update(res)
    want = E.shapley_diagnosis(g, cfp, res, bgr, columns=cols, backend="host")
    assert phi.tobytes() == want.phi.tobytes() and ex.n_seen == 6 and np.array_equal(ex.base, want.base)
    y_ref, _ = diagnosis.FaultDiagnoser(g, cfp, backend="host").update(res)
    assert report("y_prob against FaultDiagnoser", y_prob, y_ref, 1e-15) <= 1e-15
    # the feature columns alone serve as the background too
    phi2, _ = E.DiagnosisExplainer(g, cfp, bgr[:, cols], backend="host").update(res)
    assert phi2.tobytes() == phi.tobytes()


def test_entry_points_refuse_bad_arguments_on_the_host():
    """PINN_E_ARG (-1) and PINN_E_WORKSPACE (-3) as make_rows' callers give them, before any launch: the addresses are never
    dereferenced, so this needs no device."""
    import ctypes
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    lib = _lib.load(build_if_missing=False)
    E_ARG, E_WS = -1, -3
    al, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    cols = (ctypes.c_int * 4)(0, 1, 2, 3)
    x = lambda n=10, D=4, arr=al: (arr, 4, 100, cols, D, None, n)
    bg = lambda B=50, D=4, arr=al: (arr, 4, 100, cols, D, None, B)
    need = lib.pinn_shap_gmm_workspace_bytes(10, 50, 4, 4)
    staged = 32 * (8 + 36 + 2 + 16) * 8                                  # the mixture as the fused kernel reads it
    assert need == staged + 256 * ((50 * 4 * 8 + 255) // 256) + 256 * ((2 * 10 * 4 * 4 * 8 + 255) // 256)
    assert lib.pinn_shap_gmm_workspace_bytes(10, 0, 4, 4) == 0 and lib.pinn_shap_gmm_workspace_bytes(10, 50, 9, 4) == 0
    assert lib.pinn_shap_gmm_workspace_bytes(10, 50, 4, 17) == 0
    tail = lambda ws=al, wb=need, C=4, phi=al: (20, al, al, C, phi, al, al, ws, wb, None)
    assert lib.pinn_shap_gmm(*x(), *bg(), *tail(wb=need - 1)) == E_WS
    assert lib.pinn_shap_gmm(*x(), *bg(), *tail(ws=None)) == E_ARG
    assert lib.pinn_shap_gmm(*x(), *bg(), *tail(phi=odd)) == E_ARG
    assert lib.pinn_shap_gmm(*x(), *bg(), *tail(C=17)) == E_ARG
    assert lib.pinn_shap_gmm(*x(), *bg(B=0), *tail()) == E_ARG
    assert lib.pinn_shap_gmm(*x(), *bg(D=3), *tail()) == E_ARG                 # the two heads differ in their columns
    assert lib.pinn_shap_gmm(*x(arr=odd), *bg(), *tail()) == E_ARG
    assert lib.pinn_shap_gmm(*x(n=101), *bg(), *tail(wb=1 << 30)) == E_ARG      # more positions than rows, no gather list
    assert lib.pinn_shap_gmm(*x(n=0), *bg(), *tail()) == 0                      # nothing to do
    assert lib.pinn_shap_hybrid(*x(), *bg(), 5, 6, 1, al, None) == E_ARG        # the chunk leaves the rows
    assert lib.pinn_shap_hybrid(*x(), *bg(), 0, 5, 1, None, None) == E_ARG
    assert lib.pinn_shap_hybrid(*x(), *bg(), 0, 5, 1, odd, None) == E_ARG and lib.pinn_shap_hybrid(*x(), *bg(), 0, 0, 0, odd, None) == 0
    assert lib.pinn_shap_reduce(al, 1, 5, 9, 50, 4, al, al, al, None) == E_ARG
    assert lib.pinn_shap_reduce(al, 1, 5, 4, 0, 4, al, al, al, None) == E_ARG
    assert lib.pinn_shap_reduce(None, 1, 5, 4, 50, 4, al, al, al, None) == E_ARG
    assert lib.pinn_shap_reduce(odd, 1, 5, 4, 50, 4, al, al, al, None) == E_ARG and lib.pinn_shap_reduce(al, 0, 0, 4, 50, 4, al, None, al, None) == 0
