"""The optimizer kernel (pinn_adam_step, pinn_adam_update.h) one step at a time against a float64 Adam, its NaN / inf behaviour
against torch's CPU Adam, and the five optimizer routes of the C ABI against each other bit for bit."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pinn_oracle as O

FP32, BF16, X6, G6 = 0, 1, 2, 3
E_ARCH = -2


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


def _states(n, step, seed):
    """fp32 p, g, m, v (v >= 0) mixing: |g| from 1e-3 to 1e18 of both signs and -0.0 with moments of matching size; g = 0
    with m = v = 0; |g| ~ 1e-30 (g^2 underflows, denom is eps); and sqrt(v') / sqrt(bc2) ~ 1e-8 (eps decides the step).
    The first elements cover one category each, so that n = 1 and 3 see the edge cases too."""
    rng = np.random.default_rng(seed)
    bc2s = math.sqrt(1.0 - 0.999 ** step)
    cat = rng.integers(0, 6, size=n)
    cat[:6] = [2, 1, 3, 0, 4, 5][:min(n, 6)]
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    mag = 10.0 ** rng.uniform(-3, 18, n)
    g = sign * mag
    m = g * rng.uniform(-1.5, 1.5, n)
    v = g * g * rng.uniform(0.0, 2.0, n)
    p = rng.normal(0.0, 1.0, n) * 10.0 ** rng.uniform(-3, 3, n)
    z = cat == 1                                    # g = 0, m = v = 0
    g[z], m[z], v[z] = 0.0, 0.0, 0.0
    t = cat == 2                                    # g^2 underflows
    g[t] = sign[t] * 10.0 ** rng.uniform(-31, -29, t.sum())
    v[t] = 0.0
    m[t] = g[t] * rng.uniform(-1, 1, t.sum())
    e = cat == 3                                    # sqrt(v') / bc2_sqrt ~ 1e-8
    tgt = (1e-8 * rng.uniform(0.3, 3.0, e.sum()) * bc2s) ** 2
    g[e] = sign[e] * 1e-9 * rng.uniform(0, 1, e.sum())
    v[e] = np.maximum(tgt - 0.001 * g[e] ** 2, 0.0) / 0.999
    m[e] = 1e-8 * rng.uniform(-1, 1, e.sum())
    nz = cat == 4                                   # -0.0
    g[nz] = -0.0
    out = [a.astype(np.float32) for a in (p, g, m, v)]
    out[1][nz] = np.float32(-0.0)
    return out


def adam_kernel(lib, p, g, m, v, lr, step):
    import hip_helpers as hh
    from pinn_amd import _lib
    P, G, M, V = (torch.from_numpy(a.copy()).to(hh.dev()) for a in (p, g, m, v))
    _lib.check(lib.pinn_adam_step(hh.ptr(P), hh.ptr(G), hh.ptr(M), hh.ptr(V), p.size, lr, step, hh.stream()), "pinn_adam_step")
    torch.cuda.synchronize()
    return P.cpu().numpy(), M.cpu().numpy(), V.cpu().numpy()


U = 2.0 ** -23                                       # one fp32 ulp, relative (an upper bound: ulp(x) <= 2^-23 |x|)
C01 = abs(float(np.float32(0.1)) / 0.1 - 1.0)        # the constants the kernel holds in fp32
C001 = max(abs(float(np.float32(0.001)) / 0.001 - 1.0), abs(float(np.float32(0.999)) / 0.999 - 1.0))
CEPS = abs(float(np.float32(1e-8)) / 1e-8 - 1.0)
TINY = 2.0 ** -126                                    # results that underflow round to 0 or a subnormal


@pytest.mark.parametrize("step", [1, 2, 1000, 58009])
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 2048 * 256 + 5])
def test_adam_step_against_float64(lib, n, step):
    """One pinn_adam_step against float64 Adam (O.AdamState's formula) on the same fp32 inputs, lr = O.steplr(0.01, 0.8, 1000,
    step - 1) as float64 (the reference's lr; the kernel takes it as fp32).  The bound counts the kernel's operations
    (pinn_adam_update.h), one ulp (U = 2^-23 relative) per fp32 rounding, plus each fp32 constant's own error:
      m' = fma(0.1f, g - m, m):               |dm| <= U |m'| + 0.1 |g - m| (U + C01)
      v' = fma(0.001f g, g, 0.999f v):        |dv| <= v' (2U + C001)
      denom = sqrtf(v') / bc2_sqrt + 1e-8f:   relative (2U + C001) / 2 + U (sqrt) + U (bc2_sqrt) + U (divide) + U (add),
                                              the eps term with CEPS
      p' = fma(-step_size, m' / denom, p):    |dp| <= U |p'| + step_size (|dm| / denom + |m' / denom| (e_denom + U))
                                              + |update| 2U (lr and step_size to fp32)
    each x 1.01 for second-order terms, + 2^-126 for underflow.  2048 * 256 + 5 elements pass the 2048-block cap, so the
    grid-stride loop runs twice."""
    lr = O.steplr(0.01, 0.8, 1000, step - 1)
    p, g, m, v = _states(n, step, seed=n + step)
    kp, km, kv = adam_kernel(lib, p, g, m, v, lr, step)
    P, G, M, V = (a.astype(np.float64) for a in (p, g, m, v))
    bc1, bc2 = 1.0 - 0.9 ** step, 1.0 - 0.999 ** step
    m1 = 0.9 * M + 0.1 * G
    v1 = 0.999 * V + 0.001 * G * G
    d1 = np.sqrt(v1) / math.sqrt(bc2)
    den = d1 + 1e-8
    step_size = lr / bc1
    upd = step_size * m1 / den
    p1 = P - upd
    bm = 1.01 * (U * np.abs(m1) + 0.1 * np.abs(G - M) * (U + C01)) + TINY
    bv = 1.01 * v1 * (2 * U + C001) + TINY
    e_den = (d1 * ((2 * U + C001) / 2 + 3 * U) + 1e-8 * CEPS) / den + U
    bp = 1.01 * (U * np.abs(p1) + step_size * (bm / den + np.abs(m1 / den) * (e_den + U)) + np.abs(upd) * 2 * U) + TINY
    worst = {}
    for name, got, ref, b in (("m", km, m1, bm), ("v", kv, v1, bv), ("p", kp, p1, bp)):
        err = np.abs(got.astype(np.float64) - ref)
        assert np.isfinite(got).all(), name
        r = err / b
        i = int(np.argmax(r))
        worst[name] = float(r[i])
        assert r[i] <= 1.0, (name, i, float(got[i]), float(ref[i]), float(err[i]), float(b[i]), float(g[i]), float(m[i]), float(v[i]))
    print("adam n=%d step=%d worst error / bound: m %.3f v %.3f p %.3f" % (n, step, worst["m"], worst["v"], worst["p"]))


@pytest.mark.parametrize("step", [1, 1000])
def test_adam_step_nonfinite_gradients(lib, step):
    """g = NaN / +inf / -inf: p, m and v carry torch's CPU fp32 Adam (foreach=False) NaN / inf pattern element by element, and
    every other element equals the kernel's result on the same vector with those gradients zeroed."""
    n = 257
    lr = O.steplr(0.01, 0.8, 1000, step - 1)
    p, g, m, v = _states(n, step, seed=7 + step)
    g = np.clip(g, -1e6, 1e6)
    m = np.clip(m, -1e6, 1e6)
    v = np.clip(v, 0, 1e12)
    bad = np.zeros(n, bool)
    bad[[3, 17, 64, 100, 255, 256]] = True
    gb = g.copy()
    gb[[3, 64, 255]] = np.nan
    gb[[17, 256]] = np.inf
    gb[100] = -np.inf
    kp, km, kv = adam_kernel(lib, p, gb, m, v, lr, step)
    g0 = gb.copy()
    g0[bad] = 0.0
    cp, cm, cv = adam_kernel(lib, p, g0, m, v, lr, step)
    tp = torch.from_numpy(p.copy())
    opt = torch.optim.Adam([tp], lr=lr, foreach=False)
    opt.state[tp] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
    tp.grad = torch.from_numpy(gb.copy())
    opt.step()
    ref = {"p": tp.detach().numpy(), "m": opt.state[tp]["exp_avg"].numpy(), "v": opt.state[tp]["exp_avg_sq"].numpy()}
    for name, got, clean in (("p", kp, cp), ("m", km, cm), ("v", kv, cv)):
        r = ref[name]
        for f in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(f(got), f(r)), (name, f.__name__, np.nonzero(f(got))[0], np.nonzero(f(r))[0])
        assert np.array_equal(got[~bad].view(np.int32), clean[~bad].view(np.int32)), name


# ---- the five routes ---------------------------------------------------------------------------------------------------
ROUTE_FAMILIES = [(X6, 256, 3), (G6, 256, 3), (FP32, 128, 3), (BF16, 128, 3), (X6, 512, 2)]
N_ROWS, N_STEPS, STREAM0 = 1000, 5, 11


def _lr(k):
    return O.steplr(0.01, 0.8, 2, k - 1)        # changes within the five steps, so the coefficient table's index shows


def _setup(H, nh):
    import hip_helpers as hh
    from pinn_amd import synth
    P = O.init_params([8] + [H] * nh + [1], seed=31)
    ds = synth.make_dataset(N_ROWS, (), seed=32)
    return hh.flat_params(P, H, nh).to(hh.dev()), ds[0].contiguous().to(hh.dev()), ds[1].reshape(-1).contiguous().to(hh.dev())


def _run_route(lib, route, prec, H, nh, fp0, x, y):
    """Five optimizer steps through one route; returns (params, m, v, last grads, last loss, counter or None)."""
    import hip_helpers as hh
    from pinn_amd import _lib
    net = hh.make_net(lib, H, nh, prec)
    wb = lib.pinn_train_workspace_bytes(ctypes.byref(net), N_ROWS)
    work = torch.full((wb,), 0xFF, dtype=torch.uint8, device=hh.dev())
    fp = fp0.clone()
    m, v = torch.zeros_like(fp), torch.zeros_like(fp)
    grads = torch.full_like(fp, float("nan"))
    loss = torch.full((4,), float("nan"), dtype=torch.float64, device=hh.dev())
    counter = torch.zeros(1, dtype=torch.int32, device=hh.dev()) if route in ("iii", "iv") else None
    coeffs = None
    if counter is not None:
        tab = np.zeros(2 * N_STEPS, np.float32)
        ss, bs = ctypes.c_float(), ctypes.c_float()
        for k in range(1, N_STEPS + 1):
            lib.pinn_adam_coeffs(_lr(k), k, ctypes.byref(ss), ctypes.byref(bs))
            tab[2 * k - 2], tab[2 * k - 1] = ss.value, bs.value
        coeffs = torch.from_numpy(tab).to(hh.dev())
    n_par = fp.numel()
    for k in range(1, N_STEPS + 1):
        drop = hh.dropout_struct(1, [0.2] * (nh + 1), seed=77, stream_id=STREAM0 if counter is not None else STREAM0 + k - 1)
        drop.d_step_counter = counter.data_ptr() if counter is not None else None
        common = (ctypes.byref(net), hh.ptr(fp), hh.ptr(x), hh.ptr(y), N_ROWS, N_ROWS, ctypes.byref(drop), hh.ptr(grads), hh.ptr(loss),
                  hh.ptr(work), wb)
        if route == "i":
            _lib.check(lib.pinn_mlp_train_grads(*common, hh.stream()), "grads")
            _lib.check(lib.pinn_adam_step(hh.ptr(fp), hh.ptr(grads), hh.ptr(m), hh.ptr(v), n_par, _lr(k), k, hh.stream()), "adam")
        elif route == "ii":
            _lib.check(lib.pinn_mlp_train_step(*common, hh.ptr(m), hh.ptr(v), _lr(k), k, hh.stream()), "train_step")
        elif route == "iii":
            rc = lib.pinn_mlp_train_grads(*common, hh.stream())
            if H > 256:
                assert rc == E_ARCH        # the layer-by-layer kernels take their pass index by value
                return None
            _lib.check(rc, "grads + counter")
            _lib.check(lib.pinn_adam_step_dev(hh.ptr(fp), hh.ptr(grads), hh.ptr(m), hh.ptr(v), n_par, hh.ptr(coeffs), hh.ptr(counter),
                                              hh.stream()), "adam_dev")
        else:
            _lib.check(lib.pinn_mlp_train_step_dev(*common, hh.ptr(m), hh.ptr(v), hh.ptr(coeffs), hh.stream()), "train_step_dev")
    torch.cuda.synchronize()
    return fp, m, v, grads, loss, (int(counter.item()) if counter is not None else None)


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32)


@pytest.mark.parametrize("fam", ROUTE_FAMILIES, ids=lambda f: "prec%d-H%d-nh%d" % f)
def test_optimizer_routes_bitwise(lib, fam):
    """Five PHILOX-dropout steps: (i) train_grads + adam_step, (ii) train_step, (iii) train_grads with d_step_counter +
    adam_step_dev over a pinn_adam_coeffs table (fused nets; a wide net refuses the counter with PINN_E_ARCH), (iv)
    train_step_dev (fused F32X6 / _G6).  Parameters, m, v, last gradients and loss are equal bit for bit; counters read 5."""
    prec, H, nh = fam
    fp0, x, y = _setup(H, nh)
    routes = ["i", "ii", "iii"] + (["iv"] if prec in (X6, G6) and H <= 256 else [])
    ref = _run_route(lib, "i", prec, H, nh, fp0, x, y)
    assert torch.isfinite(ref[0]).all() and not torch.equal(ref[0], fp0)
    for r in routes[1:]:
        out = _run_route(lib, r, prec, H, nh, fp0, x, y)
        if out is None:
            assert r == "iii" and H > 256
            continue
        for name, a, b in zip(("params", "m", "v", "grads", "loss"), out[:5], ref[:5]):
            assert torch.equal(_bits(a), _bits(b)), (r, name)
        if r in ("iii", "iv"):
            assert out[5] == N_STEPS, (r, out[5])


def test_gnet_train_step_equals_grads_plus_adam(lib):
    """pinn_gnet_train_step == pinn_gnet_train_grads + pinn_adam_step, five steps of an unequal-width general net."""
    import hip_helpers as hh
    from pinn_amd import _lib, layout, synth
    layers = [8, 100, 60, 1]
    offs, total = layout.general_offsets(layers)
    P = O.init_params(layers, seed=5)
    f = torch.zeros(total, dtype=torch.float32)
    for (_, shape, off), t in zip(offs, P):
        f[off:off + t.numel()] = t.reshape(-1)
    fp0 = f.to(hh.dev())
    ds = synth.make_dataset(N_ROWS, (), seed=6)
    x, y = ds[0].contiguous().to(hh.dev()), ds[1].reshape(-1).contiguous().to(hh.dev())
    net = _lib.GNet(layers)
    assert lib.pinn_gnet_param_count(ctypes.byref(net)) == total
    wb = lib.pinn_gnet_workspace_bytes(ctypes.byref(net), N_ROWS, 0)
    res = []
    for fused in (False, True):
        fp = fp0.clone()
        m, v = torch.zeros_like(fp), torch.zeros_like(fp)
        grads = torch.full_like(fp, float("nan"))
        loss = torch.full((4,), float("nan"), dtype=torch.float64, device=hh.dev())
        work = torch.full((wb,), 0xFF, dtype=torch.uint8, device=hh.dev())
        for k in range(1, N_STEPS + 1):
            d = hh.dropout_struct(1, [0.2] * (len(layers) - 1), seed=9, stream_id=k - 1)
            common = (ctypes.byref(net), hh.ptr(fp), hh.ptr(x), hh.ptr(y), N_ROWS, N_ROWS, ctypes.byref(d), hh.ptr(grads), hh.ptr(loss),
                      hh.ptr(work), wb)
            if fused:
                _lib.check(lib.pinn_gnet_train_step(*common, hh.ptr(m), hh.ptr(v), _lr(k), k, hh.stream()), "gnet_train_step")
            else:
                _lib.check(lib.pinn_gnet_train_grads(*common, hh.stream()), "gnet_train_grads")
                _lib.check(lib.pinn_adam_step(hh.ptr(fp), hh.ptr(grads), hh.ptr(m), hh.ptr(v), total, _lr(k), k, hh.stream()), "adam")
        torch.cuda.synchronize()
        res.append((fp, m, v, grads, loss))
    assert torch.isfinite(res[0][0]).all() and not torch.equal(res[0][0], fp0)
    for name, a, b in zip(("params", "m", "v", "grads", "loss"), res[1], res[0]):
        assert torch.equal(_bits(a), _bits(b)), name
