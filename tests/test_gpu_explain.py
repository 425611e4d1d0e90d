"""GPU: pinn_amd.explain on the device (csrc/pinn_shap.hip) against the float64 referee of explain_cases.py (all D!
orderings for D <= 4, the subset formula for D = 8; its models are the package's host backends).

Gates, from the definitions and the package's own gates, not from what the kernels give.  phi = sum_S c_j(S) v(S) with
sum_S |c_j(S)| = 2, so an error delta in every model evaluation moves phi by at most 2 delta.  The fused kernel: the package
holds responsibilities to atol 1e-9 (test_gpu_diagnosis.py); the sum over K components and the renormalisation give
|delta y_prob| <= 2 K 1e-9, hence phi within 4 K 1e-9 and base, fx within 2 K 1e-9; efficiency within 1e-12.  The voltage
network: twice the forward's gate, rtol = atol = 2e-5 against max |f|.  Reads in place, repeated calls, chunked updates and
host arrays are compared bit for bit.  Every comparison prints its maxima before it asserts."""

import numpy as np
import pytest
import torch

from explain_cases import device_copy, host_diagnose, mixture_rows, net_forward_f64, random_mixture, referee, report

pytestmark = pytest.mark.gpu

TILE, BLOCK, MAX_SPLIT = 128, 32, 32


@pytest.fixture(scope="module")
def E():
    from pinn_amd import explain
    assert (explain.TILE, explain.BG_BLOCK, explain.MAX_SPLIT) == (TILE, BLOCK, MAX_SPLIT)
    return explain


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def check_against_referee(tag, r, ref, K):
    phi, base, fx = ref
    e_phi = report("%s phi" % tag, host(r.phi), phi, 4 * K * 1e-9)
    e_base = report("%s base" % tag, host(r.base), base, 2 * K * 1e-9)
    e_fx = report("%s fx" % tag, host(r.fx), fx, 2 * K * 1e-9)
    gap = np.abs(host(r.phi).sum(axis=1) - (host(r.fx) - host(r.base))).max()
    print("%s efficiency gap %.3e (gate 1e-12)" % (tag, gap))
    assert e_phi <= 4 * K * 1e-9 and e_base <= 2 * K * 1e-9 and e_fx <= 2 * K * 1e-9 and gap <= 1e-12


# n: 1, tile - 1, tile + 1; B: 1, one LDS block - 1, one block + 1, and more than MAX_SPLIT blocks (two blocks to a split);
# D = 4 with K in 1, 20, 32 and C in 2, 4, 16 (one and four class passes) and 5 (a partial pass); D = 8, 3 and 1
FUSED = [(1, 1, 4, 1, 2), (TILE - 1, BLOCK - 1, 4, 20, 4), (TILE + 1, BLOCK + 1, 4, 32, 16), (TILE + 1, 1, 4, 20, 2),
         (1, BLOCK + 1, 4, 32, 4), (TILE - 1, BLOCK + 1, 4, 1, 16), (2, MAX_SPLIT * BLOCK + 7, 4, 20, 4), (4, 2 * BLOCK + 8, 3, 5, 5),
         (5, 33, 8, 32, 4), (3, 5, 1, 3, 2)]


@pytest.fixture(scope="module")
def fused_case():
    """One case computed once: the mixture, its rows and the referee's answer, shared and left unchanged."""
    cache = {}

    def get(case):
        if case not in cache:
            n, B, D, K, C = case
            g, cfp = random_mixture(K, D, C, seed=sum(case))
            X, _ = mixture_rows(g, n, seed=n + 1)
            Bg, _ = mixture_rows(g, B, seed=B + 2)
            cache[case] = (g, cfp, X, Bg, referee(host_diagnose(g, cfp), X, Bg))
        return cache[case]
    return get


@pytest.mark.parametrize("case", FUSED)
def test_fused_kernel_against_the_referee(E, fused_case, case):
    n, B, D, K, C = case
    g, cfp, X, Bg, ref = fused_case(case)
    r = E.shapley_diagnosis(device_copy(g), dev(cfp), dev(X), dev(Bg))
    assert r.phi.is_cuda and r.phi.shape == (n, D, C) and r.base.shape == (C,) and r.fx.shape == (n, C) and r.phi.dtype == torch.float64
    check_against_referee("fused n=%d B=%d D=%d K=%d C=%d" % case, r, ref, K)
    if D == 1:
        assert np.array_equal(host(r.phi)[:, 0, :], host(r.fx) - host(r.base))
    # fx is the diagnosis itself
    assert host(r.fx).tobytes() == host(device_copy(g).diagnose(dev(X), dev(cfp))[0]).tobytes()


@pytest.mark.parametrize("case", [FUSED[1], FUSED[7], FUSED[8]])
def test_fused_path_against_the_generic_path(E, fused_case, case):
    n, B, D, K, C = case
    g, cfp, X, Bg, ref = fused_case(case)
    gd, cd = device_copy(g), dev(cfp)
    r = E.shapley_values(lambda Z: gd.diagnose(Z, cd)[0], dev(X), dev(Bg), max_hybrid_rows=1 << 16)
    check_against_referee("generic n=%d B=%d D=%d K=%d C=%d" % case, r, ref, K)
    f = E.shapley_diagnosis(gd, cd, dev(X), dev(Bg))
    assert report("fused against generic", host(f.phi), host(r.phi), 4 * K * 1e-9) <= 4 * K * 1e-9


def test_a_feature_the_posterior_ignores(E):
    K, D, C, j = 20, 4, 4, 2
    g, cfp = random_mixture(K, D, C, seed=77, iid_feature=j)
    X, _ = mixture_rows(g, 9, seed=1)
    Bg, _ = mixture_rows(g, BLOCK + 1, seed=2)
    r = E.shapley_diagnosis(device_copy(g), dev(cfp), dev(X), dev(Bg))
    phi = host(r.phi)
    print("independent feature: max |phi_j| %.3e (gate %.3e), max |phi| %.3e" % (np.abs(phi[:, j]).max(), 4 * K * 1e-9, np.abs(phi).max()))
    assert np.abs(phi[:, j]).max() <= 4 * K * 1e-9 and np.abs(phi).max() > 1e-3


# ---------------------------------------------------------------------------------------------- the generic kernels
def heads(E, arr, cols, ridx, bg, bcols, bidx):
    from pinn_amd._device import _DevRows
    return _DevRows(torch, dev(arr), cols, ridx), _DevRows(torch, dev(bg), bcols, bidx)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_hybrid_rows_equal_numpy_where(E, dtype):
    from pinn_amd._device import call
    rng = np.random.default_rng(0)
    arr, bg = rng.normal(0, 1, (9, 7)), rng.normal(0, 1, (6, 5))
    cols, bcols, ridx, bidx = [5, 0, 3], [1, 4, 2], [8, 2, 2, 6, 0], [3, 0, 5, 1]
    D, B, row0, m = 3, 4, 1, 3
    a, b = heads(E, arr, cols, ridx, bg, bcols, bidx)
    out = torch.full((m * 8 * B, D), -1.0, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    call("pinn_shap_hybrid", *a.head(), *b.head(), row0, m, int(dtype == np.float64), out)
    X, Bg = arr[ridx][:, cols][row0:row0 + m], bg[bidx][:, bcols]
    masks = ((np.arange(8)[:, None] >> np.arange(D)[None, :]) & 1).astype(bool)
    want = np.where(masks[None, :, None, :], X[:, None, None, :], Bg[None, None, :, :]).reshape(-1, D).astype(dtype)
    assert host(out).tobytes() == want.tobytes()


def test_reduce_kernel_linear_model_and_float64_sums(E):
    from pinn_amd._device import call
    rng = np.random.default_rng(1)
    n, D, B, C = 3, 5, 37, 3
    W, c0 = rng.normal(0, 1, (D, C)), rng.normal(0, 1, C)
    X, Bg = rng.normal(0, 2, (n, D)), rng.normal(0, 2, (B, D))
    r = E.shapley_values(lambda Z: Z @ dev(W) + dev(c0), dev(X), dev(Bg))
    want = W[None, :, :] * (X - Bg.mean(axis=0))[:, :, None]
    rel = np.abs(host(r.phi) - want).max() / np.abs(want).max()
    print("reduce kernel, linear model: relative error %.3e (gate 1e-12)" % rel)
    assert rel <= 1e-12
    # float32 outputs are summed in float64: 1 followed by 4096 values of 2^-30, which a float32 sum leaves at 1
    B = 4097
    f = np.full((2 * B, 1), 2.0 ** -30, dtype=np.float32)
    f[0, 0] = 1.0
    f[B:, 0] = 0.25                                              # the full coalition: f(x)
    lost = np.float32(0.0)
    for v in f[:B, 0]:
        lost = np.float32(lost + v)
    assert lost == np.float32(1.0)
    phi, base, fx = (torch.empty(s, dtype=torch.float64, device="cuda") for s in ((1, 1, 1), (1,), (1, 1)))
    call("pinn_shap_reduce", dev(f), 0, 1, 1, B, 1, phi, base, fx)
    exact = (1.0 + 4096 * 2.0 ** -30) / B
    print("float32 outputs: base %.17g, float64 sum %.17g, float32 sum %.17g" % (float(base[0]), exact, float(lost) / B))
    assert float(base[0]) == exact and float(fx[0, 0]) == 0.25 and float(phi[0, 0, 0]) == 0.25 - exact


# ---------------------------------------------------------------------------------------------- the voltage network
@pytest.mark.parametrize("layers,kernels", [([8, 128, 128, 128, 1], "auto"), ([8, 64, 200, 48, 1], "general")])
def test_voltage_attributions(E, layers, kernels):
    from gnet_helpers import model, params
    m, ds = model(layers, 64, kernels=kernels)
    x = ds[0][:3].to(torch.float32)
    bg = ds[0][10:15].to(torch.float32)
    f64 = lambda Z: net_forward_f64(params(m.dnn), Z)
    ref_phi, ref_base, ref_fx = referee(f64, x.numpy().astype(np.float64), bg.numpy().astype(np.float64))
    scale = np.abs(f64(np.concatenate([x.numpy(), bg.numpy()]).astype(np.float64))).max()
    gate = 2e-5 + 2e-5 * scale
    for mode in (True, False):
        m.dnn.train(mode)
        r = E.shapley_values(E.voltage_predictor(m), x.cuda(), bg.cuda(), dtype="float32")
        assert m.dnn.training is mode
        assert r.phi.shape == (3, 8, 2)
        e = [report("%s %s train=%s %s" % (layers, kernels, mode, n), host(a), b, gate)
             for n, a, b in (("phi", r.phi, ref_phi), ("base", r.base, ref_base), ("fx", r.fx, ref_fx))]
        assert max(e) <= gate
    u_only = E.shapley_values(E.voltage_predictor(m, outputs=("u",)), x.cuda(), bg.cuda(), dtype="float32")
    assert host(u_only.phi).tobytes() == host(r.phi[:, :, :1].contiguous()).tobytes()


# ---------------------------------------------------------------------------------------------- bit for bit
@pytest.fixture(scope="module")
def stream_case():
    """A results array [n, 18] whose feature columns hold mixture rows, and a background of the same kind."""
    from pinn_amd import diagnosis
    g, cfp = random_mixture(20, 4, 4, seed=3)
    cols = diagnosis.parse_features(diagnosis.DEFAULT_FEATURES)
    rng = np.random.default_rng(4)
    n, B = 1 + (TILE - 1) + (TILE + 1), BLOCK + 1
    res, bgr = rng.normal(0, 1, (n, 18)), rng.normal(0, 1, (B, 18))
    res[:, cols], bgr[:, cols] = mixture_rows(g, n, seed=5)[0], mixture_rows(g, B, seed=6)[0]
    return g, cfp, cols, res, bgr


def test_repeated_calls_and_reads_in_place(E, stream_case):
    g, cfp, cols, res, bgr = stream_case
    gd, cd, rd, bd = device_copy(g), dev(cfp), dev(res), dev(bgr)
    a = E.shapley_diagnosis(gd, cd, rd, bd, columns=cols)
    b = E.shapley_diagnosis(gd, cd, rd, bd, columns=cols)
    for u, v in zip(a, b):
        assert host(u).tobytes() == host(v).tobytes()
    ridx, bidx = np.array([5, 200, 0, 77, 5]), np.array([30, 2, 2, 9])
    c = E.shapley_diagnosis(gd, cd, rd, bd, columns=cols, row_index=ridx, background_index=bidx)
    d = E.shapley_diagnosis(gd, cd, dev(res[ridx][:, cols]), dev(bgr[bidx][:, cols]))
    for u, v in zip(c, d):
        assert host(u).tobytes() == host(v).tobytes()
    # the generic path likewise
    pred = lambda Z: gd.diagnose(Z, cd)[0]
    e = E.shapley_values(pred, rd, bd, columns=cols, row_index=ridx, background_index=bidx)
    f = E.shapley_values(pred, dev(res[ridx][:, cols]), dev(bgr[bidx][:, cols]), max_hybrid_rows=1)
    h = E.shapley_values(pred, rd, bd, columns=cols, row_index=ridx, background_index=bidx)
    for u, v, w in zip(e, f, h):
        assert host(u).tobytes() == host(v).tobytes() == host(w).tobytes()


def test_explainer_chunks_equal_one_call(E, stream_case):
    from pinn_amd import diagnosis
    g, cfp, cols, res, bgr = stream_case
    gd, rd = device_copy(g), dev(res)
    whole = E.shapley_diagnosis(gd, dev(cfp), rd, dev(bgr), columns=cols)
    ex = E.DiagnosisExplainer(gd, cfp, bgr)
    fd = diagnosis.FaultDiagnoser(gd, dev(cfp))
    at = 0
    for m in (1, TILE - 1, TILE + 1):
        phi, y_prob = ex.update(rd[at:at + m])
        assert phi.is_cuda and host(phi).tobytes() == host(whole.phi[at:at + m]).tobytes()
        assert host(y_prob).tobytes() == host(whole.fx[at:at + m]).tobytes() == host(fd.update(rd[at:at + m])[0]).tobytes()
        assert host(ex.base).tobytes() == host(whole.base).tobytes()
        at += m
    assert at == res.shape[0] == ex.n_seen


def test_host_array_in_gives_numpy_out(E, stream_case):
    g, cfp, cols, res, bgr = stream_case
    gd = device_copy(g)
    t = E.shapley_diagnosis(gd, dev(cfp), dev(res[:9]), dev(bgr), columns=cols)
    h = E.shapley_diagnosis(gd, cfp, res[:9], bgr, columns=cols, backend="device")
    for u, v in zip(t, h):
        assert isinstance(v, np.ndarray) and host(u).tobytes() == v.tobytes()
    pred = lambda Z: gd.diagnose(Z, dev(cfp))[0]
    t = E.shapley_values(pred, dev(res[:9]), dev(bgr), columns=cols)
    h = E.shapley_values(pred, res[:9], bgr, columns=cols, backend="device")
    for u, v in zip(t, h):
        assert isinstance(v, np.ndarray) and host(u).tobytes() == v.tobytes()


def test_positions_that_read_nothing(E, stream_case):
    from pinn_amd._device import _DevRows, _torch_lib
    g, cfp, cols, res, bgr = stream_case
    gd, cd, rd, bd = device_copy(g), dev(cfp), dev(res[:20]), dev(bgr)
    ridx = np.array([3, 20, 7, -1, 0])
    r = E.shapley_diagnosis(gd, cd, rd, bd, columns=cols, row_index=ridx)
    ok = E.shapley_diagnosis(gd, cd, rd, bd, columns=cols, row_index=np.array([3, 7, 0]))
    phi, fx = host(r.phi), host(r.fx)
    assert np.isnan(phi[[1, 3]]).all() and np.isnan(fx[[1, 3]]).all()
    assert phi[[0, 2, 4]].tobytes() == host(ok.phi).tobytes() and fx[[0, 2, 4]].tobytes() == host(ok.fx).tobytes()
    assert host(r.base).tobytes() == host(ok.base).tobytes()
    # the Python side refuses a background that is not finite or a gather list that leaves it, once
    with pytest.raises(ValueError, match="background_index"):
        E.shapley_diagnosis(gd, cd, rd, bd, columns=cols, background_index=[0, bgr.shape[0]])
    bad = bgr.copy()
    bad[4, cols[1]] = np.nan
    with pytest.raises(ValueError, match="finite"):
        E.shapley_diagnosis(gd, cd, rd, dev(bad), columns=cols)
    # the kernel itself: a background position outside its array makes the outputs NaN
    tl = _torch_lib()
    out = E._device_diagnosis(tl[0], tl[2], gd, cd, _DevRows(torch, rd, cols), _DevRows(torch, bd, cols, [0, bgr.shape[0], 1]))
    assert all(bool(torch.isnan(a).all()) for a in out)
