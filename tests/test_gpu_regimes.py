"""GPU parity away from initialisation: every kernel family in the weight regimes of tests/regimes.py -- saturated layers, both signs
of logvar, var at its 1e-6 floor, both sides of z > 20 -- with a different dropout probability per module, Philox masks with a seed
>= 2^32, a non-zero stream and a non-zero row offset, on row counts ragged against 16, 64 and 128.

The referee is always the oracle in float64; test_regimes_host.py proves on the CPU that each case reaches its branch and that torch's
own float32 stays within half of every gate used here.  The gates are the project's own, from the existing parity test of the same
family and entry point: forward and MC mean rtol = atol = 1e-5, a_u rtol 1e-4, e_u rtol 1e-3 + atol 2e-6, loss and mse 2e-5 relative,
every gradient tensor and dL/dx 2e-4 * max |ref| + 1e-6 * max |ref|, f32x6 / f32x6g6 gradients also within 2e-5 * max of the exact-fp32
kernels', bf16-mixed the two-level gates of test_gpu_bf16.py.  Every comparison prints its ratio to the bound before it asserts (run with
-s to read them), and every output must be finite.

No case uses the K-times-torch form of test_gradient_error_no_worse_than_torch_fp32: measured ratios are in DESIGN.md."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gnet_helpers as G
import hip_helpers as hh
import pinn_oracle as O
import regimes as R

REGIME_NAMES = list(R.REGIMES)
# (precision, layers): exact fp32, f32x6 and f32x6g6 on the fused nets; the wide net on the two split-operand precisions
FP32_FAMILIES = [(p, l) for p in (0, 2, 3) for l in R.FUSED_NETS] + [(p, l) for p in (2, 3) for l in R.WIDE_NETS]
FAMILY_IDS = ["prec%d-%s" % (p, "x".join(map(str, l))) for p, l in FP32_FAMILIES]


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


def _ratio(what, got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|), printed, then asserted <= 1; got must be finite."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    want = np.asarray(want, dtype=np.float64).reshape(-1)
    assert np.isfinite(got).all(), what
    r = float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())
    print("%-70s ratio to bound %.3f" % (what, r))
    assert r <= 1.0, (what, r)


def _tensor(what, got, want, rel=2e-4, floor=1e-6):
    """The project's per-tensor rule: max |err| <= rel * max |ref| + floor * max |ref|."""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double()
    assert bool(torch.isfinite(got).all()), what
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    bound = rel * scale + floor * scale
    print("%-70s err %.3e  scale %.3e  ratio to bound %.3f" % (what, err, scale, err / (bound + 1e-300)))
    assert err <= bound, (what, err, scale)


def _loss(what, l, n, ref_loss, ref_mse, rel=2e-5):
    l = l.cpu().numpy()
    assert np.isfinite(l).all(), what
    loss, mse = (l[0] + 0.01 * l[1]) / n, l[2] / n
    print("%-70s loss ratio %.3f  mse ratio %.3f" % (what, abs(loss - ref_loss) / (rel * abs(ref_loss)), abs(mse - ref_mse) / (rel * abs(ref_mse))))
    assert abs(loss - ref_loss) <= rel * abs(ref_loss), (what, loss, ref_loss)
    assert abs(mse - ref_mse) <= rel * abs(ref_mse), (what, mse, ref_mse)


def _fused(c):
    """(H, n_hidden, flat parameters, x, y) of a case on the device, fused layout."""
    H, nh = c.layers[1], c.k
    return H, nh, hh.flat_params(c.P, H, nh).to(hh.dev()), c.x.to(hh.dev()), c.y.reshape(-1).to(hh.dev()).contiguous()


def _hdrop(c, stream=R.STREAM):
    return hh.dropout_struct(1, c.pl, seed=R.SEED, stream_id=stream, row_offset=R.ROW0)


# ---------------------------------------------------------------------------------------------------------------------------
# fused exact fp32, f32x6, f32x6g6 and the wide nets: pinn_mlp_forward, pinn_mc_dropout, pinn_mlp_train_grads
@pytest.mark.parametrize("regime", REGIME_NAMES)
@pytest.mark.parametrize("prec,layers", FP32_FAMILIES, ids=FAMILY_IDS)
def test_forward(lib, prec, layers, regime):
    c = R.case(layers, regime)
    H, nh, fp, xd, _ = _fused(c)
    tag = "%s prec %d %s forward " % (layers, prec, regime)
    u, lv = hh.forward(lib, H, nh, fp, xd, None, precision=prec)
    _ratio(tag + "eval u", u.cpu(), c.eval64[0], 1e-5, 1e-5)
    _ratio(tag + "eval logvar", lv.cpu(), c.eval64[1], 1e-5, 1e-5)
    u, lv = hh.forward(lib, H, nh, fp, xd, _hdrop(c), precision=prec)
    _ratio(tag + "philox u", u.cpu(), c.train64[0], 1e-5, 1e-5)
    _ratio(tag + "philox logvar", lv.cpu(), c.train64[1], 1e-5, 1e-5)


@pytest.mark.parametrize("regime", REGIME_NAMES)
@pytest.mark.parametrize("prec,layers", FP32_FAMILIES, ids=FAMILY_IDS)
def test_mc_dropout(lib, prec, layers, regime):
    """T = 6: the x6 kernels run even and odd passes on two waves, three passes each."""
    from pinn_amd import _lib
    c = R.case(layers, regime)
    H, nh, fp, xd, _ = _fused(c)
    out = torch.full((3, c.n), float("nan"), device=hh.dev())
    net = hh.make_net(lib, H, nh, prec)
    d = _hdrop(c, R.MC_STREAM)
    _lib.check(lib.pinn_mc_dropout(ctypes.byref(net), hh.ptr(fp), hh.ptr(xd), c.n, ctypes.byref(d), R.MC_T, hh.ptr(out[0]), hh.ptr(out[1]),
                                   hh.ptr(out[2]), hh.stream()), "pinn_mc_dropout")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    tag = "%s prec %d %s mc " % (layers, prec, regime)
    _ratio(tag + "pred_mean", o[0], c.mc64[0], 1e-5, 1e-5)
    _ratio(tag + "a_u", o[1], c.mc64[1], 1e-4, 0.0)
    _ratio(tag + "e_u", o[2], c.mc64[2], 1e-3, 2e-6)


@pytest.mark.parametrize("regime", REGIME_NAMES)
@pytest.mark.parametrize("prec,layers", FP32_FAMILIES, ids=FAMILY_IDS)
def test_train_grads(lib, prec, layers, regime):
    c = R.case(layers, regime)
    H, nh, fp, xd, yd = _fused(c)
    tag = "%s prec %d %s train " % (layers, prec, regime)
    grads, loss = hh.train_grads(lib, H, nh, fp, xd, yd, _hdrop(c), precision=prec)
    lo, mse, go = c.nll64
    _loss(tag, loss, c.n, lo, mse)
    for name, g, w in zip(O.param_names(nh), hh.unflat(grads.cpu(), H, nh), go):
        _tensor(tag + name, g, w)
    if prec and H <= 256:       # the split-operand families against the exact-fp32 kernels (test_train_grads_x6_vs_oracle_autograd)
        g0, l0 = hh.train_grads(lib, H, nh, fp, xd, yd, _hdrop(c), precision=0)
        scale = float(g0.abs().max())
        err = float((grads - g0).abs().max())
        print("%-70s ratio to bound %.3f" % (tag + "vs exact fp32", err / (2e-5 * scale)))
        assert err <= 2e-5 * scale
        np.testing.assert_allclose(loss.cpu().numpy()[:3], l0.cpu().numpy()[:3], rtol=2e-6)


# ---------------------------------------------------------------------------------------------------------------------------
# bf16-mixed: the two-level gates of test_gpu_bf16.py (tight against the oracle under the same rounding policy, which is float32
# arithmetic by construction; loose against the float64 oracle)
@pytest.mark.parametrize("regime", R.BF16_REGIMES)
@pytest.mark.parametrize("layers", R.BF16_NETS, ids=lambda l: "x".join(map(str, l)))
def test_bf16_forward(lib, layers, regime):
    c = R.case(layers, regime, bf16=True)
    H, nh, fp, xd, _ = _fused(c)
    tag = "%s bf16 %s forward " % (layers, regime)
    for train, ref in ((False, c.eval64), (True, c.train64)):
        u, lv = hh.forward(lib, H, nh, fp, xd, _hdrop(c) if train else None, precision=1)
        with torch.no_grad():
            ub, lvb = O.mlp_forward(c.P, c.x, c.pl if train else None, c.masks if train else None, bf16=True)
        mode = "philox " if train else "eval "
        _ratio(tag + mode + "u, same policy", u.cpu(), ub, 2e-3, 2e-3)
        _ratio(tag + mode + "logvar, same policy", lv.cpu(), lvb, 2e-3, 2e-3)
        eu = float(np.abs(u.cpu().numpy() - ref[0]).max()) / (2e-2 * max(float(np.abs(ref[0]).max()), 1.0))
        elv = float(np.abs(lv.cpu().numpy() - ref[1]).max()) / 5e-2
        print("%-70s ratio to bound u %.3f logvar %.3f" % (tag + mode + "vs float64", eu, elv))
        assert eu <= 1.0 and elv <= 1.0


@pytest.mark.parametrize("regime", R.BF16_REGIMES)
@pytest.mark.parametrize("layers", R.BF16_NETS, ids=lambda l: "x".join(map(str, l)))
def test_bf16_train_grads(lib, layers, regime):
    c = R.case(layers, regime, bf16=True)
    H, nh, fp, xd, yd = _fused(c)
    tag = "%s bf16 %s train " % (layers, regime)
    grads, loss = hh.train_grads(lib, H, nh, fp, xd, yd, _hdrop(c), precision=1)
    l = loss.cpu().numpy()
    assert np.isfinite(l).all()
    got = (l[0] + 0.01 * l[1]) / c.n
    with torch.no_grad():
        ub, lvb = O.mlp_forward(c.P, c.x, c.pl, c.masks, bf16=True)
        lb = O.aleatoric_loss(c.y, ub, lvb).item()
    lo, _, go = c.nll64
    print("%-70s ratio to bound: same policy %.3f  float64 %.3f" % (tag + "loss", abs(got - lb) / (2e-3 * abs(lb) + 2e-4),
                                                                  abs(got - lo) / (2e-2 * abs(lo) + 2e-3)))
    assert abs(got - lb) <= 2e-3 * abs(lb) + 2e-4
    assert abs(got - lo) <= 2e-2 * abs(lo) + 2e-3
    for name, g, w in zip(O.param_names(nh), hh.unflat(grads.cpu(), H, nh), go):
        _tensor(tag + name, g, w, rel=5e-2, floor=0.0)
        g, w = g.double(), w.double()
        cos = float((g * w).sum() / (g.norm() * w.norm() + 1e-30))
        assert cos > 0.998, (name, cos)


# ---------------------------------------------------------------------------------------------------------------------------
# the general family: pinn_gnet_forward, _mc_dropout, _train_grads, _backward, _backward2
def _gdrop(c, stream=R.STREAM):
    return hh.dropout_struct(1, c.pl, seed=R.SEED, stream_id=stream, row_offset=R.ROW0)


def _general(c):
    return G.flat(c.layers, c.P), c.x.to(hh.dev()).contiguous(), c.y.reshape(-1).to(hh.dev()).contiguous()


@functools.lru_cache(maxsize=None)
def _upstream(n):
    return G.upstream(n, n, with_v=True)          # g_u, g_lv [n], v [n, 8]


@functools.lru_cache(maxsize=None)
def _vjp_ref(c, with_lv):
    gu, glv, _ = _upstream(c.n)
    return R.vjp64(c.P, c.x, gu, glv if with_lv else None, c.pl, c.masks)


def _check_general_forward(lib, c, tag):
    fp, xd, _ = _general(c)
    u, lv = G.forward(lib, c.layers, fp, xd)
    _ratio(tag + "eval u", u, c.eval64[0], 1e-5, 1e-5)
    _ratio(tag + "eval logvar", lv, c.eval64[1], 1e-5, 1e-5)
    u, lv = G.forward(lib, c.layers, fp, xd, _gdrop(c))
    _ratio(tag + "philox u", u, c.train64[0], 1e-5, 1e-5)
    _ratio(tag + "philox logvar", lv, c.train64[1], 1e-5, 1e-5)


def _check_general_train(lib, c, tag):
    fp, xd, yd = _general(c)
    g, loss = G.train_grads(lib, c.layers, fp, xd, yd, _gdrop(c))
    lo, mse, go = c.nll64
    _loss(tag, loss, c.n, lo, mse)
    for name, a, w in zip(O.param_names(c.k), G.unflat(c.layers, g), go):
        _tensor(tag + name, a, w)


def _check_general_backward(lib, c, tag):
    fp, xd, _ = _general(c)
    gu, glv, _ = _upstream(c.n)
    gud, glvd = gu.to(hh.dev()), glv.to(hh.dev())
    for with_lv in (True, False):
        g, dx = G.backward(lib, c.layers, fp, xd, gud, glvd if with_lv else None, _gdrop(c))
        wp, wx = _vjp_ref(c, with_lv)
        t = tag + ("" if with_lv else "no g_lv ")
        for name, a, w in zip(O.param_names(c.k), G.unflat(c.layers, g), wp):
            if not with_lv and name.startswith("var_layers"):
                assert float(w.abs().max()) == 0.0 and float(a.abs().max()) == 0.0, (t, name)
            else:
                _tensor(t + name, a, w)
        _tensor(t + "dL/dx", dx, wx)


def _check_general_backward2(lib, c, tag):
    fp, xd, _ = _general(c)
    gu, glv, vx = _upstream(c.n)
    got = G.backward2(lib, c.layers, fp, xd, gu.to(hh.dev()), glv.to(hh.dev()), vx.to(hh.dev()), _gdrop(c))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    wp, wx, wgu, wglv = G.oracle2(c.P, c.x, gu, glv, vx, c.pl, c.masks)
    for name, a, w in zip(O.param_names(c.k), G.unflat(c.layers, got["grads"]), wp):
        if name == "predict.bias":
            assert float(w.abs().max()) == 0.0 and float(a.abs().max()) == 0.0, (c.layers, tag, name)      # exactly zero
        else:
            _tensor("%s %s %s" % (c.layers, tag, name), a, w)
    assert float(G.padding(c.layers, got["grads"]).abs().sum()) == 0.0
    _tensor("%s %s dS/dx" % (c.layers, tag), got["gx"], wx)
    _tensor("%s %s ud" % (c.layers, tag), got["ggu"], wgu)
    _tensor("%s %s lvd" % (c.layers, tag), got["gglv"], wglv)


GENERAL_IDS = ["x".join(map(str, l)) for l in R.GENERAL_NETS]


@pytest.mark.parametrize("regime", REGIME_NAMES)
@pytest.mark.parametrize("layers", R.GENERAL_NETS, ids=GENERAL_IDS)
def test_general_forward(lib, layers, regime):
    _check_general_forward(lib, R.case(layers, regime), "%s general %s forward " % (layers, regime))


@pytest.mark.parametrize("regime", REGIME_NAMES)
@pytest.mark.parametrize("layers", R.GENERAL_NETS, ids=GENERAL_IDS)
def test_general_mc_dropout(lib, layers, regime):
    c = R.case(layers, regime)
    fp, xd, _ = _general(c)
    o = G.mc(lib, layers, fp, xd, _gdrop(c, R.MC_STREAM), R.MC_T)
    tag = "%s general %s mc " % (layers, regime)
    _ratio(tag + "pred_mean", o[0], c.mc64[0], 1e-5, 1e-5)
    _ratio(tag + "a_u", o[1], c.mc64[1], 1e-4, 0.0)
    _ratio(tag + "e_u", o[2], c.mc64[2], 1e-3, 2e-6)


@pytest.mark.parametrize("regime", REGIME_NAMES)
@pytest.mark.parametrize("layers", R.GENERAL_NETS, ids=GENERAL_IDS)
def test_general_train_grads(lib, layers, regime):
    _check_general_train(lib, R.case(layers, regime), "%s general %s train " % (layers, regime))


@pytest.mark.parametrize("regime", REGIME_NAMES)
@pytest.mark.parametrize("layers", R.GENERAL_NETS, ids=GENERAL_IDS)
def test_general_backward(lib, layers, regime):
    """With g_lv and without it (NULL: the variance head gets no gradient at all), both with dL/dx."""
    _check_general_backward(lib, R.case(layers, regime), "%s general %s backward " % (layers, regime))


@pytest.mark.parametrize("regime", REGIME_NAMES)
@pytest.mark.parametrize("layers", R.GENERAL_NETS, ids=GENERAL_IDS)
def test_general_backward2(lib, layers, regime):
    _check_general_backward2(lib, R.case(layers, regime), "%s backward2" % regime)


# kMaxWidth as an output width and as an input width, h_k // 4 == 2 and h_k // 2 == 2, at 129 rows
@pytest.mark.parametrize("regime", R.EDGE_REGIMES)
@pytest.mark.parametrize("layers", R.EDGE_NETS, ids=["x".join(map(str, l)) for l in R.EDGE_NETS])
@pytest.mark.parametrize("entry", ["forward", "train_grads", "backward", "backward2"])
def test_general_widest_layers(lib, entry, layers, regime):
    c = R.case(layers, regime, 129)
    tag = "%s general %s %s " % (layers, regime, entry)
    {"forward": _check_general_forward, "train_grads": _check_general_train, "backward": _check_general_backward,
     "backward2": _check_general_backward2}[entry](lib, c, tag)


def test_general_mc_exact_across_a_chunk_boundary(lib):
    """[8,2048,8,1], 97 rows, T = 120: infer_layout holds (256 MiB / (4 * (3 * 2048 + 2))) / 64 * 64 = 10 880 virtual rows, the call has
    97 * 121 = 11 737, so it takes two chunks and the cut falls inside stochastic pass 111 (10 880 = 112 * 97 + 16).  The moments of
    every row against the float64 oracle on the same Philox masks, and a row window bitwise equal to the same rows of the full call."""
    from pinn_amd import _lib
    layers, n, T = R.CHUNK_NET, R.CHUNK_ROWS, R.CHUNK_T
    net = ctypes.byref(_lib.GNet(layers))
    cap = ((256 << 20) // (4 * (3 * 2048 + 2))) // 64 * 64
    assert cap == 10880 and cap < n * (T + 1) <= 2 * cap and cap == 112 * n + 16
    # the workspace stops growing at one chunk: ten times the passes need no more bytes, a tenth of them fewer
    assert lib.pinn_gnet_workspace_bytes(net, n, T) == lib.pinn_gnet_workspace_bytes(net, n, 10 * T)
    assert lib.pinn_gnet_workspace_bytes(net, n, T // 10) < lib.pinn_gnet_workspace_bytes(net, n, T)
    c = R.case(layers, "sign", n)
    fp, xd, _ = _general(c)
    o = G.mc(lib, layers, fp, xd, _gdrop(c, R.MC_STREAM), T)
    masks = R.philox_masks_passes(layers, n, c.pl, [R.MC_STREAM + t for t in range(T)])
    pm, au, eu = R.mc_reference(c.P, c.x, c.pl, T, lambda t: masks[t])
    tag = "%s general sign mc T=%d " % (layers, T)
    _ratio(tag + "pred_mean", o[0], pm, 1e-5, 1e-5)
    _ratio(tag + "a_u", o[1], au, 1e-4, 0.0)
    _ratio(tag + "e_u", o[2], eu, 1e-3, 2e-6)
    a, b = 16, 81           # the first chunk ends at row 16 of pass 111: a window that starts there
    d = _gdrop(c, R.MC_STREAM)
    d.row_offset = R.ROW0 + a
    w = G.mc(lib, layers, fp, xd[a:b].contiguous(), d, T)
    assert np.array_equal(w, o[:, a:b])
