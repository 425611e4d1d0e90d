"""GPU: the physics residuals under torch autograd -- pinn_residuals_backward / pinn_net_f_t_backward (csrc/pinn_residuals.hip)
against the reference's recorded gradients and torch autograd of the oracle, and the physics_autograd surface of
PhysicsInformedNN ("lambdas": the reference's own graph; "full": rows, halo and the DNN's weights too)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pinn_oracle as O
from conftest import ScalerFromArrays, load_golden

NAMES = O.LAMBDA_NAMES
COLS = {"V": ["FV", "VACT", "VOHM", "VCONC", "ENERNST", "VEST5", "I", "VOUT5"], "T": ["FT", "TPRED", "TOUT"],
        "H": ["FH", "ACTH", "TGTH", "ITOT"], "O": ["FO", "ACTO", "TGTO", "QO2", "O2FLOW"]}
FLAG = {"V": 1, "T": 2, "H": 4, "O": 8}
REL = 2e-4          # the DNN autograd yardstick (tests/test_gpu_autograd.py)


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


def _dev():
    return torch.device("cuda:0")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _aff(sx, sy):
    import hip_helpers as hh
    return hh.affine_struct(sx, sy)


# ---------------------------------------------------------------------------------------------------------------------------
# C entry points
def res_backward(lib, x, u, aff, lam, g, flags=None, want_gx=True, want_gu=True):
    """pinn_residuals_backward with upstream g = {column name: [n] tensor} -> (glambda [17], gu, gx) float64 numpy."""
    from pinn_amd import _lib
    n = x.shape[0]
    if flags is None:
        flags = sum(FLAG[t] for t, cs in COLS.items() if any(c in g for c in cs))
    gbuf = torch.full((_lib.NCOLS, n), float("nan"), device=_dev())      # absent columns are poisoned: they must not be read
    gmask = 0
    for name, v in g.items():
        gbuf[_lib.C[name]] = torch.as_tensor(v, dtype=torch.float32).reshape(n).to(_dev())
        gmask |= 1 << _lib.C[name]
    gl = torch.full((17,), float("nan"), device=_dev())
    gu = torch.full((n,), float("nan"), device=_dev()) if want_gu else None
    gx = torch.full((n, 8), float("nan"), device=_dev()) if want_gx else None
    work = torch.full((lib.pinn_residuals_workspace_bytes(),), 0xFF, dtype=torch.uint8, device=_dev())
    _lib.check(lib.pinn_residuals_backward(_ptr(x), _ptr(u), ctypes.byref(aff), _ptr(lam), flags, n, _ptr(gbuf), n, gmask, _ptr(gl), _ptr(gu),
                                           _ptr(gx), _ptr(work), work.numel(), _stream()), "pinn_residuals_backward")
    torch.cuda.synchronize()
    f = lambda t: None if t is None else t.cpu().numpy().astype(np.float64)
    return f(gl), f(gu), f(gx)


def res_forward(lib, x, u, aff, lam, flags=15):
    from pinn_amd import _lib
    n = x.shape[0]
    cols = torch.zeros(_lib.NCOLS, n, device=_dev())
    _lib.check(lib.pinn_residuals(_ptr(x), _ptr(u), None, ctypes.byref(aff), _ptr(lam), flags, n, _ptr(cols), n, None, None, 0, _stream()),
               "pinn_residuals")
    return cols


def euler_backward(lib, x, u, aff, lam, gf=None, gp=None, gr=None, halo=None):
    """pinn_net_f_t_backward -> (glambda, gu, gx, gx_halo, gu_halo) float64 numpy."""
    from pinn_amd import _lib
    n = x.shape[0]
    d = lambda v: None if v is None else torch.as_tensor(v, dtype=torch.float32).reshape(n).to(_dev()).contiguous()
    gf, gp, gr = d(gf), d(gp), d(gr)
    xh = uh = gxh = guh = None
    if halo is not None:
        xh = halo[0].reshape(8).to(_dev()).contiguous()
        uh = halo[1].reshape(1).to(_dev()).contiguous()
        gxh = torch.full((8,), float("nan"), device=_dev())
        guh = torch.full((1,), float("nan"), device=_dev())
    gl = torch.full((17,), float("nan"), device=_dev())
    gu = torch.full((n,), float("nan"), device=_dev())
    gx = torch.full((n, 8), float("nan"), device=_dev())
    work = torch.empty(lib.pinn_residuals_workspace_bytes(), dtype=torch.uint8, device=_dev())
    _lib.check(lib.pinn_net_f_t_backward(_ptr(x), _ptr(u), _ptr(xh), _ptr(uh), ctypes.byref(aff), _ptr(lam), n, _ptr(gf), _ptr(gp), _ptr(gr),
                                         _ptr(gl), _ptr(gu), _ptr(gx), _ptr(gxh), _ptr(guh), _ptr(work), work.numel(), _stream()),
               "pinn_net_f_t_backward")
    torch.cuda.synchronize()
    f = lambda t: None if t is None else t.cpu().numpy().astype(np.float64)
    return f(gl), f(gu), f(gx), f(gxh), f(guh)


# ---------------------------------------------------------------------------------------------------------------------------
# referees: torch autograd of the oracle, `real` = denorm(x) requiring grad, the DNN output restated as a differentiable input
def _columns(real, u, lam, y_min, y_scale, tags):
    out = {}
    v_out = ((u - torch.as_tensor(y_min, dtype=u.dtype)) / torch.as_tensor(y_scale, dtype=u.dtype)) / 5
    if "V" in tags:
        r = O.net_f_V(real, u.detach().float(), y_min, y_scale, lam)
        out.update(FV=r[0] + r[8] / 5 - v_out, VACT=r[1], VOHM=r[2], VCONC=r[3], ENERNST=r[4], VEST5=r[5], I=r[6], VOUT5=v_out * 5)
    if "T" in tags:
        out.update(zip(COLS["T"], O.net_f_T_simple(real, lam)))
    if "H" in tags:
        out.update(zip(COLS["H"], O.net_f_H(real, lam)[:4]))
    if "O" in tags:
        out.update(zip(COLS["O"], O.net_f_O(real, lam)))
    return out


def referee(xn, un, lamv, sx, sy, g, dtype):
    """-> (glambda [17], gu [n], gx [n, 8]) float64 numpy of sum_c (g_c * col_c).sum()."""
    mn, sc = O.scaler_affine(sx)
    y_min, y_scale = O.scaler_affine(sy)
    real = torch.tensor(O.denorm(xn, mn, sc), dtype=dtype, requires_grad=True)
    u = torch.tensor(np.asarray(un, np.float32).reshape(-1, 1), dtype=dtype, requires_grad=True)
    lam = {k: torch.tensor([v], dtype=dtype, requires_grad=True) for k, v in zip(NAMES, lamv)}
    cols = _columns(real, u, lam, y_min, y_scale, {t for t, cs in COLS.items() if any(c in g for c in cs)})
    L = sum((torch.as_tensor(np.asarray(v), dtype=dtype).reshape(-1, 1) * cols[k]).sum() for k, v in g.items())
    gs = torch.autograd.grad(L, [real, u] + [lam[k] for k in NAMES], allow_unused=True)
    z = lambda t, shape: np.zeros(shape) if t is None else t.detach().double().numpy()
    n = real.shape[0]
    gx = z(gs[0], (n, 8)) / sc
    return np.array([0.0 if t is None else float(t) for t in gs[2:]]), z(gs[1], (n, 1)).reshape(-1), gx


def _within(got, r64, r32, what, rel=1e-5):
    """The gradient yardstick: |got - float64| <= 2 x |float32 torch - float64| + a small atol, per column / entry."""
    got, r64, r32 = (np.asarray(a, np.float64) for a in (got, r64, r32))
    if got.ndim == 1 and got.shape[0] == 17:                 # parameter gradients: entry by entry
        err, e32, scale = np.abs(got - r64), np.abs(r32 - r64), np.abs(r64)
    else:                                                    # per column, max over rows
        g2, a2, b2 = (a.reshape(a.shape[0], -1) for a in (got, r64, r32))
        err, e32, scale = np.abs(g2 - a2).max(0), np.abs(b2 - a2).max(0), np.abs(a2).max(0)
    ok = err <= 2 * e32 + rel * scale + 1e-30
    assert np.all(ok), (what, err[~ok], e32[~ok], scale[~ok])


def _golden_rows(si):
    """The fixture's edge rows with its parameter set `si` (0, 1), or with one of the sets of tests/residual_referee.py ("A", "B", "D":
    the oxygen target clamped, so the inclusive clamp mask is 0 on those rows; "C": lambda_O3 = 0, the sign is 0)."""
    g = load_golden("g_resid.npz")
    sx, sy = ScalerFromArrays(g, "sx."), ScalerFromArrays(g, "sy.")
    x = torch.from_numpy(g["x"]).to(_dev())
    u = torch.from_numpy(g["u_eval"]).reshape(-1).to(_dev())
    if isinstance(si, str):
        import residual_referee as rr
        lam = torch.from_numpy(rr.param_sets()[si].copy()).to(_dev())
    else:
        lam = torch.tensor(g["s%d.lambdas" % si], dtype=torch.float32).to(_dev())
    return g, sx, sy, x, u, lam


def _synthetic(n, seed=0):
    from pinn_amd import synth
    ds = synth.make_dataset(n, (), seed=seed)
    x = ds[0].to(_dev()).contiguous()
    gen = torch.Generator().manual_seed(seed + 1)
    u = (torch.rand(n, generator=gen) * 1.6 - 0.8).to(_dev())
    return ds[4], ds[5], x, u


def _upstream(names, n, seed):
    gen = torch.Generator().manual_seed(seed)
    return {c: torch.randn(n, generator=gen).numpy() for c in names}


ALL = sum(COLS.values(), [])
SUBSETS = [ALL, ["FV"], ["VACT", "ENERNST", "I"], ["VOUT5"], ["VEST5", "VCONC"], ["FT"], ["TPRED", "TOUT"], ["FH"], ["ACTH", "TGTH", "ITOT"],
           ["FO"], ["ACTO", "QO2"], ["TGTO", "O2FLOW"], ["FV", "FT", "FH", "FO"]]


# 1. against the reference's recorded gradients
@pytest.mark.parametrize("si", [0, 1])
def test_backward_golden_lambda_grads(lib, si):
    from pinn_amd import _lib
    g, sx, sy, x, u, lam = _golden_rows(si)
    aff = _aff(sx, sy)
    n = x.shape[0]
    cols = res_forward(lib, x, u, aff, lam)
    for tag, fcol in (("V", "FV"), ("T", "FT"), ("H", "FH"), ("O", "FO")):
        gl, _, _ = res_backward(lib, x, u, aff, lam, {fcol: 2 * cols[_lib.C[fcol]] / n}, want_gx=False, want_gu=False)
        want = g["s%d.%s.grad" % (si, tag)]
        for k in range(17):
            assert abs(gl[k] - want[k]) <= 1e-4 * abs(want[k]) + 1e-9, (tag, NAMES[k], gl[k], want[k])
    # train_lambda(dnn_para=False): mean((y - (V_est5 s + m))^2) -> upstream on V_est5
    y = torch.from_numpy(g["y"]).reshape(-1).to(_dev())
    vn = cols[_lib.C["VEST5"]] * aff.vn_scale + aff.vn_min
    gl, _, _ = res_backward(lib, x, u, aff, lam, {"VEST5": -2.0 * (y - vn) * aff.vn_scale / n}, want_gx=False, want_gu=False)
    want = g["s%d.Vn.grad" % si]
    for k in range(17):
        assert abs(gl[k] - want[k]) <= 1e-4 * abs(want[k]) + 1e-9, ("Vn", NAMES[k], gl[k], want[k])


# 2. against a float64 referee, every column and subsets, golden rows and a multi-workgroup synthetic set
@pytest.mark.parametrize("case", ["golden0", "golden1", "synthetic", "goldenA", "goldenB", "goldenD"])
def test_backward_vs_float64_referee(lib, case):
    if case.startswith("golden"):
        g, sx, sy, x, u, lam = _golden_rows(int(case[-1]) if case[-1].isdigit() else case[-1])
    else:
        sx, sy, x, u = _synthetic(100003)
        lam = torch.tensor([O.LAMBDA_INIT[k] for k in NAMES], dtype=torch.float32).to(_dev())
    aff = _aff(sx, sy)
    n = x.shape[0]
    xn, un, lamv = x.cpu().numpy(), u.cpu().numpy(), lam.cpu().numpy()
    subsets = SUBSETS if case != "synthetic" else [ALL, ["FV", "FT", "FH", "FO"], ["VOUT5", "TGTO"]]
    for i, names in enumerate(subsets):
        up = _upstream(names, n, 100 + i)
        got = res_backward(lib, x, u, aff, lam, up)
        r64 = referee(xn, un, lamv, sx, sy, up, torch.float64)
        r32 = referee(xn, un, lamv, sx, sy, up, torch.float32)
        for what, a, b, c in zip(("glambda", "gu", "gx"), got, r64, r32):
            if what == "gu" and "V" not in {t for t, cs in COLS.items() if any(cn in names for cn in cs)}:
                assert np.all(a == 0.0)
                continue
            _within(a, b, c, (case, names, what))


def test_backward_nan_rows_like_torch(lib):
    """I >= lambda_3: the voltage model's log of a negative number (01:758-761).  NaN exactly where float32 torch autograd has it."""
    g, sx, sy, x, u, lam = _golden_rows(0)
    lam = lam.clone()
    lam[2] = 1.0                        # every row with I > 270 A is a NaN row
    aff = _aff(sx, sy)
    n = x.shape[0]
    lamv = lam.cpu().numpy()
    for i, names in enumerate([ALL, COLS["V"], ["VACT", "ENERNST"], ["FV"]]):
        up = _upstream(names, n, 7 + i)
        got = res_backward(lib, x, u, aff, lam, up)
        r32 = referee(x.cpu().numpy(), u.cpu().numpy(), lamv, sx, sy, up, torch.float32)
        for what, a, b in zip(("glambda", "gu", "gx"), got, r32):
            assert np.array_equal(np.isnan(a), np.isnan(b)), (names, what, np.argwhere(np.isnan(a) != np.isnan(b))[:5])
            fin = ~np.isnan(b)
            np.testing.assert_allclose(a[fin], b[fin], rtol=1e-3, atol=1e-3 * (np.abs(b[fin]).max() + 1e-30), err_msg=str((names, what)))
        if "FV" in names or "VCONC" in names:
            assert np.isnan(got[2][:, 5]).any()


def test_backward_sign_zero_like_torch(lib):
    """lambda_O3 = 0 (set C): the threshold |lambda_O3| is 0, every row is past it, and d|x|/dx at 0 is 0 in torch.  Where float32 torch
    autograd has a gradient and where it has exactly none, so has the kernel."""
    import residual_referee as rr
    assert rr.edge_stats("C")["o_sgn"] == 0.0 and rr.edge_stats("C")["o_lin"] == 0
    g, sx, sy, x, u, lam = _golden_rows("C")
    aff = _aff(sx, sy)
    n = x.shape[0]
    lamv = lam.cpu().numpy()
    for i, names in enumerate([ALL, COLS["O"], ["FO"], ["TGTO"]]):
        up = _upstream(names, n, 17 + i)
        got = res_backward(lib, x, u, aff, lam, up)
        r32 = referee(x.cpu().numpy(), u.cpu().numpy(), lamv, sx, sy, up, torch.float32)
        for what, a, b in zip(("glambda", "gu", "gx"), got, r32):
            assert np.array_equal(np.isnan(a), np.isnan(b)), (names, what, np.argwhere(np.isnan(a) != np.isnan(b))[:5])
            fin = ~np.isnan(b)
            np.testing.assert_allclose(a[fin], b[fin], rtol=1e-3, atol=1e-3 * (np.abs(b[fin]).max() + 1e-30), err_msg=str((names, what)))
        k = NAMES.index("lambda_O3")
        assert got[0][k] == 0.0 and r32[0][k] == 0.0, (got[0][k], r32[0][k])
        assert got[0][NAMES.index("lambda_O1")] != 0.0          # (the target itself is live: lambda_O1 + lambda_O2 0 / 100, inside the clamp)


# 3. determinism, row windows, shards
def test_backward_deterministic_windows_and_shards(lib):
    sx, sy, x, u = _synthetic(300007, seed=3)
    lam = torch.tensor([O.LAMBDA_INIT[k] for k in NAMES], dtype=torch.float32).to(_dev())
    aff = _aff(sx, sy)
    n = x.shape[0]
    up = _upstream(ALL, n, 5)
    a = res_backward(lib, x, u, aff, lam, up)
    b = res_backward(lib, x, u, aff, lam, up)
    for s, t in zip(a, b):
        assert np.array_equal(s, t)
    lo, hi = 12345, 212345
    w = res_backward(lib, x[lo:hi], u[lo:hi], aff, lam, {k: v[lo:hi] for k, v in up.items()})
    assert np.array_equal(w[1], a[1][lo:hi]) and np.array_equal(w[2], a[2][lo:hi])
    cuts = [0, 1000, 77777, 150000, n]
    tot = np.zeros(17)
    for s, e in zip(cuts[:-1], cuts[1:]):
        tot += res_backward(lib, x[s:e], u[s:e], aff, lam, {k: v[s:e] for k, v in up.items()}, want_gx=False, want_gu=False)[0]
    np.testing.assert_allclose(tot, a[0], rtol=1e-6, atol=1e-6 * np.abs(a[0]).max())


# 4. the Euler model
def euler_referee(xn, un, lamv, sx, sy, gf, gp, gr, dtype):
    """torch autograd of O.net_f_T with the DNN output of rows t-1 restated as a differentiable input."""
    mn, sc = O.scaler_affine(sx)
    y_min, y_scale = O.scaler_affine(sy)
    real = torch.tensor(O.denorm(xn, mn, sc), dtype=dtype, requires_grad=True)
    u = torch.tensor(np.asarray(un, np.float32).reshape(-1, 1), dtype=dtype, requires_grad=True)
    lam = {k: torch.tensor([v], dtype=dtype, requires_grad=True) for k, v in zip(NAMES, lamv)}
    f, tp, tr = O.net_f_T(real, u[:-1].detach().float(), y_min, y_scale, lam)
    # O.net_f_T detaches u: add its term back, Q_el's -I V_cell lT4 dt / lT2
    i_prev = (real[:-1, 0:1] / 270 + 0.00001) * 270
    v_cell = ((u[:-1] - float(y_min[0])) / float(y_scale[0])) / 5
    v_const = v_cell.detach()
    delta = torch.cat([torch.zeros(1, 1, dtype=dtype), (-(i_prev * v_cell) + i_prev * v_const) * lam["lambda_T4"] / lam["lambda_T2"] * 0.1])
    tp = tp + delta
    f = f - delta
    gt = lambda v: torch.as_tensor(np.asarray(v), dtype=dtype).reshape(-1, 1)
    L = (gt(gf) * f).sum() + (gt(gp) * tp).sum() + (gt(gr) * tr).sum()
    gs = torch.autograd.grad(L, [real, u] + [lam[k] for k in NAMES], allow_unused=True)
    n = real.shape[0]
    gx = gs[0].detach().double().numpy() / sc
    return np.array([0.0 if t is None else float(t) for t in gs[2:]]), gs[1].detach().double().numpy().reshape(-1), gx


@pytest.mark.parametrize("case", ["golden0", "golden1", "synthetic"])
def test_euler_backward_vs_referee_and_halo(lib, case):
    if case.startswith("golden"):
        g, sx, sy, x, u, lam = _golden_rows(int(case[-1]))
    else:
        sx, sy, x, u = _synthetic(70001, seed=4)
        lam = torch.tensor([O.LAMBDA_INIT[k] for k in NAMES], dtype=torch.float32).to(_dev())
    aff = _aff(sx, sy)
    n = x.shape[0]
    up = _upstream(["f", "p", "r"], n, 9)
    got = euler_backward(lib, x, u, aff, lam, up["f"], up["p"], up["r"])
    xn, un, lamv = x.cpu().numpy(), u.cpu().numpy(), lam.cpu().numpy()
    r64 = euler_referee(xn, un, lamv, sx, sy, up["f"], up["p"], up["r"], torch.float64)
    r32 = euler_referee(xn, un, lamv, sx, sy, up["f"], up["p"], up["r"], torch.float32)
    for what, a, b, c in zip(("glambda", "gu", "gx"), got[:3], r64, r32):
        _within(a, b, c, (case, what))
    assert got[1][-1] == 0.0
    # lambda_T1..T4 of mean(f^2) against the oracle's own autograd (u constant)
    lamt = {k: torch.tensor([v], requires_grad=True) for k, v in zip(NAMES, lamv)}
    mn, sc = O.scaler_affine(sx)
    real = torch.from_numpy(O.denorm(xn, mn, sc))
    f = O.net_f_T(real, torch.from_numpy(un.reshape(-1, 1))[:-1], *O.scaler_affine(sy), lamt)[0]
    gs = torch.autograd.grad(torch.mean(f ** 2), [lamt[k] for k in NAMES], allow_unused=True)
    fk = torch.empty(3, n, device=_dev())
    _lib_check_net_f_t(lib, x, u, aff, lam, fk)
    gl = euler_backward(lib, x, u, aff, lam, gf=2 * fk[0] / n)[0]
    for k, t in enumerate(gs):
        if t is None:
            assert gl[k] == 0.0
        else:
            assert abs(gl[k] - float(t)) <= 1e-4 * abs(float(t)) + 1e-9, (NAMES[k], gl[k], float(t))
    # halo shards: the concatenation, the halo gradients added to the previous shard's last row, equals the whole series
    cut = n // 2 + 1
    a = euler_backward(lib, x[:cut], u[:cut], aff, lam, up["f"][:cut], up["p"][:cut], up["r"][:cut])
    b = euler_backward(lib, x[cut:], u[cut:], aff, lam, up["f"][cut:], up["p"][cut:], up["r"][cut:], halo=(x[cut - 1], u[cut - 1:cut]))
    gx = np.concatenate([a[2], b[2]])
    gu = np.concatenate([a[1], b[1]])
    gx[cut - 1] += b[3]
    gu[cut - 1] += b[4][0]
    assert np.all(np.abs(gx - got[2]) <= 1e-6 * np.abs(got[2]) + 1e-6 * np.abs(got[2]).max(0)), np.abs(gx - got[2]).max(0)
    np.testing.assert_allclose(gu, got[1], rtol=1e-6, atol=1e-6 * np.abs(got[1]).max())
    # each shard's float32 sum is rounded on its own: the bound is relative to the two parts
    assert np.all(np.abs(a[0] + b[0] - got[0]) <= 1e-6 * (np.abs(a[0]) + np.abs(b[0]) + np.abs(got[0])) + 1e-9), (a[0] + b[0], got[0])


def _lib_check_net_f_t(lib, x, u, aff, lam, out):
    from pinn_amd import _lib
    n = x.shape[0]
    _lib.check(lib.pinn_net_f_t(_ptr(x), _ptr(u), None, None, ctypes.byref(aff), _ptr(lam), n, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                _stream()), "pinn_net_f_t")


# ---------------------------------------------------------------------------------------------------------------------------
# the module
def _golden_model(name="g_resid.npz", si=0, **kw):
    import pinn_amd
    g = load_golden(name)
    sx, sy = ScalerFromArrays(g, "sx."), ScalerFromArrays(g, "sy.")
    m = pinn_amd.PhysicsInformedNN(torch.from_numpy(g["x"]), torch.from_numpy(g["y"]), [8, 128, 128, 128, 1], sx, sy, p=0.2, logvar=True,
                                   precision="fp32", **kw)
    m.verbose = False
    sd = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w.")}
    missing, unexpected = m.dnn.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("lambda") for k in missing)
    if "s%d.lambdas" % si in g:
        with torch.no_grad():
            for k, v in zip(NAMES, g["s%d.lambdas" % si]):
                getattr(m, k).fill_(float(v))
    m.dnn.eval()
    return m, g, sx, sy


def _clear_grads(m):
    for k in NAMES:
        getattr(m, k).grad = None
    m.dnn.zero_grad(set_to_none=True)
    m.x.grad = None


# 5. "lambdas" mode
@pytest.mark.parametrize("si", [0, 1])
def test_module_lambdas_mode_golden(si):
    m, g, sx, sy = _golden_model(si=si, physics_autograd="lambdas")
    assert m.physics_autograd == "lambdas"
    real = torch.from_numpy(O.denorm(g["x"], *O.scaler_affine(sx)))
    lam = {k: torch.tensor([float(v)], requires_grad=True) for k, v in zip(NAMES, g["s%d.lambdas" % si])}
    ymin, yscale = O.scaler_affine(sy)
    oracle = {"V": O.net_f_V(real, torch.from_numpy(g["u_eval"]), ymin, yscale, lam), "T": O.net_f_T_simple(real, lam),
              "H": O.net_f_H(real, lam), "O": O.net_f_O(real, lam)}
    fns = {"V": m.net_f_V, "T": m.net_f_T_simple, "H": m.net_f_H, "O": m.net_f_O}
    for tag, fn in fns.items():
        m.physics_autograd = False
        plain = fn(m.X, sx)
        m.physics_autograd = "lambdas"
        _clear_grads(m)
        res = fn(m.X, sx)
        assert [bool(r.requires_grad) for r in res] == [bool(r.requires_grad) for r in oracle[tag]], tag
        for a, b in zip(plain, res):
            assert torch.equal(a.detach(), b.detach()), tag
        torch.mean(res[0] ** 2).backward()
        got = np.array([0.0 if getattr(m, k).grad is None else float(getattr(m, k).grad) for k in NAMES])
        assert np.array_equal(np.array([getattr(m, k).grad is None for k in NAMES]), g["s%d.%s.grad_none" % (si, tag)]), tag
        want = g["s%d.%s.grad" % (si, tag)]
        for k in range(17):
            assert abs(got[k] - want[k]) <= 1e-4 * abs(want[k]) + 1e-9, (tag, NAMES[k], got[k], want[k])
        assert m.x.grad is None and all(p.grad is None for n, p in m.dnn.named_parameters() if not n.startswith("lambda"))
        with torch.no_grad():
            assert all(r.grad_fn is None for r in fn(m.X, sx) if not isinstance(r, torch.nn.Parameter))
    assert m.net_f_V(m.X, sx)[7] is m.lambda_3 and m.net_f_H(m.X, sx)[4] is m.lambda_H3
    # the Euler model: lambda_T1..T4, u a constant
    _clear_grads(m)
    f = m.net_f_T(m.X, sx)[0]
    assert f.grad_fn is not None
    torch.mean(f ** 2).backward()
    ft = O.net_f_T(real, torch.from_numpy(g["u_eval"])[:-1], ymin, yscale, lam)[0]
    gs = torch.autograd.grad(torch.mean(ft ** 2), [lam[k] for k in NAMES], allow_unused=True)
    for k, t in zip(NAMES, gs):
        assert (getattr(m, k).grad is None) == (t is None), k
        if t is not None:
            assert abs(float(getattr(m, k).grad) - float(t)) <= 2e-4 * abs(float(t)) + 1e-9, (k, float(getattr(m, k).grad), float(t))
    assert all(p.grad is None for n, p in m.dnn.named_parameters() if not n.startswith("lambda"))


def test_module_lambdas_mode_frozen_and_train_masks():
    m, g, sx, sy = _golden_model(physics_autograd="lambdas")
    m.lambda_2.requires_grad = False
    res = m.net_f_V(m.X, sx)
    assert [r.requires_grad for r in res[:7]] == [True, False, True, True, False, True, False] and not res[8].requires_grad
    _clear_grads(m)
    torch.mean(res[0] ** 2).backward()
    assert m.lambda_2.grad is None and m.lambda_1.grad is not None and m.lambda_3.grad is not None
    m.lambda_2.requires_grad = True
    # train mode: the DNN inside draws the masks it draws with physics_autograd=False
    m.dnn.train()
    c0 = m.dnn._fwd_counter
    a = m.net_f_V(m.X, sx)[0]
    m.physics_autograd = False
    m.dnn._fwd_counter = c0
    b = m.net_f_V(m.X, sx)[0]
    assert torch.equal(a.detach(), b) and m.dnn._fwd_counter == c0 + 1
    # the reference's clamp idiom keeps working (the Parameter is re-pointed, then re-gathered)
    m.physics_autograd = "lambdas"
    m.dnn.eval()
    m.lambda_1.data = torch.clamp(m.lambda_1.data + 1.0, 0.0, 0.5)
    _clear_grads(m)
    f = m.net_f_V(m.X, sx)[0]
    torch.mean(f ** 2).backward()
    assert float(m._lambda[0]) == 0.5 and m.lambda_1.grad is not None


# 6. the reference's four stage loops, in plain torch over the model's surface
STAGE_KEYS = [("lambdaF", "lambda", False), ("lambdaT", "lambda", True), ("thermal", "thermal", None), ("hydrogen", "hydrogen", None),
              ("oxygen", "oxygen", None)]


@pytest.mark.parametrize("key,stage,dnn_para", STAGE_KEYS)
def test_reference_stage_loops_golden(key, stage, dnn_para):
    from torch.optim.lr_scheduler import StepLR
    m, g, sx, sy = _golden_model("g_traj.npz", physics_autograd="lambdas")
    names, lr0, gamma, bounds = O.STAGES[stage]
    for k in NAMES:
        getattr(m, k).requires_grad = k in names
    params = [getattr(m, k) for k in names]
    opt = torch.optim.Adam(params, lr=lr0)
    sched = StepLR(opt, step_size=1000, gamma=gamma)
    with torch.no_grad():
        u_pred = m.net_u(m.x)[0]
    y = m.u
    lo, hi = -1.0, 1.0
    dmin = torch.tensor(sy.data_min_, dtype=torch.float32, device=y.device)
    dmax = torch.tensor(sy.data_max_, dtype=torch.float32, device=y.device)
    scale_y = (hi - lo) / (dmax - dmin + 1e-12)
    min_y = lo - dmin * scale_y
    traj = []
    for epoch in range(50):
        if stage == "lambda":
            res = m.net_f_V(m.X, sx)
            physics = torch.mean(res[0] ** 2) if dnn_para else torch.mean((y - (res[5] * scale_y + min_y)) ** 2)
            loss = physics + torch.mean((y - u_pred) ** 2)
        else:
            fn = {"thermal": m.net_f_T_simple, "hydrogen": m.net_f_H, "oxygen": m.net_f_O}[stage]
            loss = torch.mean(fn(m.X, sx)[0] ** 2)
        opt.zero_grad()
        loss.backward()
        opt.step()
        for p, (a, b) in zip(params, bounds):
            p.data = torch.clamp(p.data, a, b)
        sched.step()
        traj.append(m._lambdas().cpu().numpy().astype(np.float64))
    for k in (1, 2, 5, 50):
        want = g["%s.k%d" % (key, k)]
        for j, n in enumerate(NAMES):
            tol = 5e-5 * abs(want[j]) + 5e-6 * abs(O.LAMBDA_INIT[n])
            assert abs(traj[k - 1][j] - want[j]) <= tol, (key, k, n, traj[k - 1][j], want[j])


# 7. "full" mode: residual losses reach the weights and X
def _pack_bits(passes, widths):
    out = []
    for masks in passes:
        parts = []
        for m_, w in zip(masks, widths):
            m_ = np.asarray(m_, dtype=np.uint8)
            m_ = np.concatenate([m_, np.zeros((m_.shape[0], (-w) % 32), np.uint8)], axis=1)
            parts.append(np.packbits(m_, axis=-1, bitorder="little"))
        out.append(np.ascontiguousarray(np.concatenate(parts, axis=-1)).view(np.int32))
    return torch.from_numpy(np.stack(out).copy())


def _cpu_full_loss(P, x, y, sx, sy, lamv, p_list, masks):
    """aleatoric_loss + mean(f_V^2) + mean(f_T_euler^2) on the CPU (O.mlp_forward + the restated residuals), three DNN passes."""
    mn, sc = O.scaler_affine(sx)
    y_min, y_scale = O.scaler_affine(sy)
    u0, lv = O.mlp_forward(P, x, p_list, masks[0])
    loss = O.aleatoric_loss(y, u0, lv)
    real = ((x.double() - torch.from_numpy(mn)) / torch.from_numpy(sc)).float()
    lam = {k: lamv[k] for k in NAMES}
    u1, _ = O.mlp_forward(P, x, p_list, masks[1])
    fV = _columns(real, u1, lam, y_min, y_scale, {"V"})["FV"]
    u2, _ = O.mlp_forward(P, x, p_list, masks[2])
    f, _, _ = O.net_f_T(real, u2[:-1].detach(), y_min, y_scale, lam)
    i_prev = (real[:-1, 0:1] / 270 + 0.00001) * 270
    v_cell = ((u2[:-1] - float(y_min[0])) / float(y_scale[0])) / 5
    delta = torch.cat([torch.zeros(1, 1), (-(i_prev * v_cell) + i_prev * v_cell.detach()) * lam["lambda_T4"] / lam["lambda_T2"] * 0.1])
    return loss + torch.mean(fV ** 2) + torch.mean((f - delta) ** 2)


def _close(got, want, what, rel=REL):
    scale = float(want.abs().max()) + 1e-30
    err = float((got - want).abs().max())
    assert np.isfinite(err) and err <= rel * scale + 1e-6 * scale, (what, err, scale)


@pytest.mark.parametrize("layers,kw", [([8, 128, 128, 128, 1], {}), ([8, 64, 200, 48, 1], dict(kernels="general"))])
@pytest.mark.parametrize("train", [False, True])
def test_module_full_mode_vs_cpu_autograd(layers, kw, train):
    import pinn_amd
    from pinn_amd import synth
    n = 300
    ds = synth.make_dataset(n, (), seed=2)
    torch.manual_seed(0)
    m = pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=True, seed=5, autograd=True,
                                   physics_autograd="full", **kw)
    m.verbose = False
    names = O.param_names(len(layers) - 2)
    named = dict(m.dnn.named_parameters())
    P = [named[k].detach().cpu().clone().requires_grad_(True) for k in names]
    widths = list(layers[1:-1]) + [layers[-2] // 2]
    p_list = [0.2] * len(widths)
    if train:
        gen = np.random.default_rng(3)
        passes = [[gen.random((n, w)) > 0.2 for w in widths] for _ in range(3)]
        m.dnn.inject_masks(_pack_bits(passes, widths))
        m.dnn.train()
    else:
        passes = [None] * 3
        m.dnn.eval()
    _clear_grads(m)
    X = ds[0].to(_dev()).clone().requires_grad_(True)
    u, lv = m.net_u(X)
    L = m.aleatoric_loss(m.u, u, lv) + torch.mean(m.net_f_V(X, ds[4])[0] ** 2) + torch.mean(m.net_f_T(X, ds[4])[0] ** 2)
    L.backward()
    xc = ds[0].clone().requires_grad_(True)
    lamc = {k: torch.tensor([v], requires_grad=True) for k, v in O.LAMBDA_INIT.items()}
    Lc = _cpu_full_loss(P, xc, ds[1], ds[4], ds[5], lamc, p_list if train else None, passes)
    gs = torch.autograd.grad(Lc, P + [xc] + [lamc[k] for k in NAMES], allow_unused=True)
    for k, gw in zip(names, gs):
        _close(named[k].grad.cpu(), gw, (layers, train, k))
    _close(X.grad.cpu(), gs[len(P)], (layers, train, "X"))
    for k, t in zip(NAMES, gs[len(P) + 1:]):
        assert (getattr(m, k).grad is None) == (t is None), k
        if t is not None:
            _close(getattr(m, k).grad.cpu(), t, k)


def test_module_full_mode_coupled_adam_and_halo():
    import pinn_amd
    from pinn_amd import synth
    n = 256
    layers = [8, 128, 128, 128, 1]
    ds = synth.make_dataset(n, (), seed=6)
    torch.manual_seed(1)
    m = pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=True, autograd=True, physics_autograd="full")
    m.verbose = False
    m.dnn.eval()
    names = O.param_names(3)
    named = dict(m.dnn.named_parameters())
    lam_names = ["lambda_1", "lambda_2", "lambda_3", "lambda_T1", "lambda_T2", "lambda_T3", "lambda_T4"]
    P = [named[k].detach().cpu().clone().requires_grad_(True) for k in names]
    lamc = {k: torch.tensor([v], requires_grad=k in lam_names) for k, v in O.LAMBDA_INIT.items()}
    opt = torch.optim.Adam([named[k] for k in names] + [getattr(m, k) for k in lam_names], lr=1e-3)
    optc = torch.optim.Adam(P + [lamc[k] for k in lam_names], lr=1e-3)
    X = m.x
    for _ in range(3):
        opt.zero_grad()
        u, lv = m.net_u(X)
        (m.aleatoric_loss(m.u, u, lv) + torch.mean(m.net_f_V(X, ds[4])[0] ** 2) + 1e-6 * torch.mean(m.net_f_T(X, ds[4])[0] ** 2)).backward()
        opt.step()
        optc.zero_grad()
        xc = ds[0].clone()
        u0, lv0 = O.mlp_forward(P, xc)
        # the same loss on the CPU, the Euler term weighted 1e-6 (its scale is ~1e10 at the initial thermal parameters)
        real = ((xc.double() - torch.from_numpy(O.scaler_affine(ds[4])[0])) / torch.from_numpy(O.scaler_affine(ds[4])[1])).float()
        y_min, y_scale = O.scaler_affine(ds[5])
        fV = _columns(real, u0, lamc, y_min, y_scale, {"V"})["FV"]
        f, _, _ = O.net_f_T(real, u0[:-1].detach(), y_min, y_scale, lamc)
        i_prev = (real[:-1, 0:1] / 270 + 0.00001) * 270
        v_cell = ((u0[:-1] - float(y_min[0])) / float(y_scale[0])) / 5
        delta = torch.cat([torch.zeros(1, 1), (-(i_prev * v_cell) + i_prev * v_cell.detach()) * lamc["lambda_T4"] / lamc["lambda_T2"] * 0.1])
        (O.aleatoric_loss(ds[1], u0, lv0) + torch.mean(fV ** 2) + 1e-6 * torch.mean((f - delta) ** 2)).backward()
        optc.step()
    for k, p in zip(names, P):
        np.testing.assert_allclose(named[k].detach().cpu().numpy(), p.detach().numpy(), rtol=5e-4, atol=5e-6, err_msg=k)
    for k in lam_names:
        np.testing.assert_allclose(float(getattr(m, k).detach()), float(lamc[k].detach()), rtol=5e-4, err_msg=k)
    assert m.x.grad is not None and bool(torch.isfinite(m.x.grad).all())
    # halo tensors that require grad receive the gradient of the row before the shard
    cut = 100
    x = ds[0].to(_dev())
    xs = x.clone().requires_grad_(True)
    _clear_grads(m)
    full = m.net_f_T(xs, ds[4])[0]
    (full ** 2).sum().backward()
    want_x = xs.grad.clone()
    with torch.no_grad():
        uh = m.net_u(x[cut - 1:cut])[0].reshape(1)
    xh = x[cut - 1].clone().requires_grad_(True)
    uh = uh.clone().requires_grad_(True)
    xb = x[cut:].clone().requires_grad_(True)
    hi = m.net_f_T(xb, ds[4], halo=(xh, uh))[0]
    (hi ** 2).sum().backward()
    assert xh.grad is not None and uh.grad is not None
    np.testing.assert_allclose(xb.grad.cpu().numpy(), want_x[cut:].cpu().numpy(), rtol=1e-5, atol=1e-6 * float(want_x.abs().max()))
    xa = x[:cut].clone().requires_grad_(True)
    lo = m.net_f_T(xa, ds[4])[0]
    (lo ** 2).sum().backward()
    # the halo row's total: its own shard's gradient + the DNN path of uh + the direct halo gradient
    u_probe = x[cut - 1:cut].clone().requires_grad_(True)
    m.net_u(u_probe)[0].reshape(1).backward(uh.grad)
    tot = xa.grad[cut - 1] + xh.grad + u_probe.grad[0]
    np.testing.assert_allclose(tot.cpu().numpy(), want_x[cut - 1].cpu().numpy(), rtol=1e-4, atol=1e-5 * float(want_x.abs().max()))


# 8. errors, and the library's trainers afterwards
def test_errors_and_trainers_after_physics_autograd(tmp_path):
    import pinn_amd
    from pinn_amd import report, synth
    ds = synth.make_dataset(400, (), seed=0)
    layers = [8, 128, 128, 128, 1]
    mk = lambda **kw: pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=True, seed=3, **kw)
    with pytest.raises(ValueError):
        mk(physics_autograd="full")                       # needs dnn.autograd
    with pytest.raises(ValueError):
        mk(physics_autograd="yes")
    with pytest.raises(ValueError):
        mk(physics_autograd=True)
    m = mk()
    assert m.physics_autograd is False
    with pytest.raises(ValueError):
        m.physics_autograd = "full"
    m.dnn.autograd = True
    m.physics_autograd = "full"
    m.dnn.autograd = False
    with pytest.raises(ValueError):
        m.net_f_V(m.X, ds[4])
    m.physics_autograd = "lambdas"
    f = m.net_f_H(m.X, ds[4])[0]
    with pytest.raises(RuntimeError):
        torch.autograd.grad(f.sum(), m.lambda_H1, create_graph=True)
    for fn, lam in ((m.net_f_H, m.lambda_H1), (m.net_f_T, m.lambda_T1)):
        f = fn(m.X, ds[4])[0]
        with torch.no_grad():
            lam.mul_(1.0)                                  # an in-place change between forward and backward
        with pytest.raises(RuntimeError):
            f.sum().backward()
    # bf16 nets: "lambdas" mode works (u is a constant there)
    b16 = mk(precision="bf16", physics_autograd="lambdas")
    b16.dnn.eval()
    f = b16.net_f_V(b16.X, ds[4])[0]
    torch.mean(f ** 2).backward()
    assert b16.lambda_1.grad is not None and torch.isfinite(b16.lambda_1.grad).all()

    # user physics autograd, then the library's trainers: bitwise what a fresh model loaded from a checkpoint does
    a = mk(physics_autograd="lambdas")
    a.verbose = False
    a.dnn.eval()
    opt = torch.optim.Adam([a.lambda_H1, a.lambda_H2, a.lambda_O1], lr=1e-2)
    for _ in range(3):
        opt.zero_grad()
        (torch.mean(a.net_f_H(a.X, ds[4])[0] ** 2) + torch.mean(a.net_f_O(a.X, ds[4])[0] ** 2)).backward()
        opt.step()
    path = str(tmp_path / "a.pt")
    report.save_checkpoint(a, path)
    b = mk()
    b.verbose = False
    report.load_checkpoint(b, path)
    assert torch.equal(a._lambdas(), b._lambdas())
    a.train_dnn(3)
    b.train_dnn(3)
    assert torch.equal(a.dnn.flat_params(), b.dnn.flat_params())
    for call in (lambda mm: mm.train_lambda(3), lambda mm: mm.train_thermal(3), lambda mm: mm.train_hydrogen(3), lambda mm: mm.train_oxygen(3)):
        call(a)
        call(b)
        assert torch.equal(a._lambdas(), b._lambdas())
