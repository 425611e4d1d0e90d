"""GPU parity of the general (any layers list) exact-fp32 kernels, csrc/pinn_general.hip, through the C ABI and the model surface."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pinn_oracle as O
from gnet_helpers import SHAPES, data, forward, mc, pack_bits, train_grads
from gnet_helpers import dev as _dev, drop as _drop, flat as _flat, model as _model, philox_masks as _philox_masks
from gnet_helpers import unflat as _unflat, widths as _widths

RTOL = ATOL = 1e-5
_pack_bits = functools.partial(pack_bits, passes=True)      # a list over passes
_data = functools.partial(data, with_y=True)                # (x, y)


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


def _check_grads(layers, got, want, rtol):
    for name, g, w in zip(O.param_names(len(layers) - 2), _unflat(layers, got), want):
        scale = float(w.abs().max()) + 1e-30
        err = float((g - w).abs().max())
        assert err <= rtol * scale + 1e-6 * scale, (layers, name, err, scale)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", SHAPES)
def test_forward_eval_and_philox_vs_oracle(lib, layers):
    P = O.init_params(layers, seed=sum(layers))
    fp = _flat(layers, P)
    rows = [1, 15, 17, 1000] + ([12000] if layers[1] == 2000 else [])     # 12 000 rows > one inference chunk of [8, 2000, 300, 1]
    for n in rows:
        x, _ = _data(n, seed=n)
        xd = x.to(_dev()).contiguous()
        u, lv = forward(lib, layers, fp, xd)
        with torch.no_grad():
            ue, le = O.mlp_forward(P, x)
        np.testing.assert_allclose(u.numpy(), ue.numpy().reshape(-1), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(lv.numpy(), le.numpy().reshape(-1), rtol=RTOL, atol=ATOL)
        seed, stream, row0 = 123456789012, 7, 999
        u, lv = forward(lib, layers, fp, xd, _drop(1, layers, 0.2, seed, stream, row0))
        with torch.no_grad():
            ue, le = O.mlp_forward(P, x, [0.2] * (len(layers) - 1), _philox_masks(layers, seed, stream, row0, n, 0.2))
        np.testing.assert_allclose(u.numpy(), ue.numpy().reshape(-1), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(lv.numpy(), le.numpy().reshape(-1), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("layers", SHAPES[:4])
def test_forward_injected_bits_vs_oracle(lib, layers):
    P = O.init_params(layers, seed=1)
    n = 333
    x, _ = _data(n, seed=2)
    gen = torch.Generator().manual_seed(3)
    masks = [(torch.rand(n, w, generator=gen) >= 0.3).numpy() for w in _widths(layers)]
    bits = _pack_bits([masks]).to(_dev())
    u, lv = forward(lib, layers, _flat(layers, P), x.to(_dev()), _drop(2, layers, 0.3, bits=bits))
    with torch.no_grad():
        ue, le = O.mlp_forward(P, x, [0.3] * (len(layers) - 1), masks)
    np.testing.assert_allclose(u.numpy(), ue.numpy().reshape(-1), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(lv.numpy(), le.numpy().reshape(-1), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("layers,n", [(SHAPES[0], 1000), (SHAPES[1], 777), (SHAPES[2], 129), (SHAPES[3], 64), (SHAPES[4], 300),
                                      (SHAPES[5], 1000)])
def test_grads_vs_oracle_autograd(lib, layers, n):
    P = O.init_params(layers, seed=n)
    x, y = _data(n, seed=5)
    seed, stream, row0 = 987654321987, 42, 12345
    pl = [0.2] * (len(layers) - 1)
    g, loss = train_grads(lib, layers, _flat(layers, P), x.to(_dev()), y.to(_dev()), _drop(1, layers, 0.2, seed, stream, row0))
    masks = _philox_masks(layers, seed, stream, row0, n, 0.2)
    lo, mse, go, _, _ = O.nll_loss_and_grads(P, x, y.reshape(-1, 1), pl, masks)
    l = loss.numpy()
    assert abs((l[0] + 0.01 * l[1]) / n - lo.item()) <= 2e-5 * abs(lo.item())
    assert abs(l[2] / n - mse.item()) <= 2e-5 * abs(mse.item())
    _check_grads(layers, g, go, rtol=2e-4)


def test_grads_several_chunks(lib):
    """Training gradients and loss sums across chunk edges.  train_layout keeps 78 keep words + 2 * 2016 (d pre ping-pong) + 2 (du, dz)
    + 2016 + 320 + 160 + 96 (activations, padded to 32) = 6704 floats per row of [8, 2000, 300, 1], so a chunk is
    (512 MiB / (4 * 6704)) / 64 * 64 = 19 968 rows and 50 000 rows take three: 19 968 + 19 968 + 10 064.  The loss partials of chunk c
    start at block 1248 c, and finalize_kernel sums 3 * 1248 of them.  Same oracle and bounds as test_grads_vs_oracle_autograd."""
    from pinn_amd import _lib
    layers, n = [8, 2000, 300, 1], 50000
    assert ((512 << 20) // (4 * 6704)) // 64 * 64 == 19968 and 2 * 19968 < n <= 3 * 19968
    # one chunk's activations cap the workspace: beyond it only the loss partials grow, 4 B per row
    net = ctypes.byref(_lib.GNet(layers))
    wb, wb_half = lib.pinn_gnet_workspace_bytes(net, n, 0), lib.pinn_gnet_workspace_bytes(net, n // 2, 0)
    assert 0 < wb - wb_half < 0.01 * wb_half, (wb, wb_half)
    P = O.init_params(layers, seed=4)
    x, y = _data(n, seed=6)
    seed, stream, row0 = 5, 3, 17          # test_backward_several_chunks' stream: gnet_helpers.philox_masks draws the masks once
    g, loss = train_grads(lib, layers, _flat(layers, P), x.to(_dev()), y.to(_dev()), _drop(1, layers, 0.2, seed, stream, row0))
    lo, mse, go, _, _ = O.nll_loss_and_grads(P, x, y.reshape(-1, 1), [0.2] * 3, _philox_masks(layers, seed, stream, row0, n, 0.2))
    l = loss.numpy()
    got_lo, got_mse = (l[0] + 0.01 * l[1]) / n, l[2] / n
    print("loss %.3f of its bound, mse %.3f" % (abs(got_lo - lo.item()) / (2e-5 * abs(lo.item())),
                                                abs(got_mse - mse.item()) / (2e-5 * abs(mse.item()))))
    for name, a, w in zip(O.param_names(len(layers) - 2), _unflat(layers, g), go):
        print("%-24s %.3f of its bound" % (name, float((a - w).abs().max()) / (2e-4 * float(w.abs().max()) + 1e-6 * float(w.abs().max()))))
    assert abs(got_lo - lo.item()) <= 2e-5 * abs(lo.item())
    assert abs(got_mse - mse.item()) <= 2e-5 * abs(mse.item())
    _check_grads(layers, g, go, rtol=2e-4)


def test_grads_deterministic_shard_additive_and_windows(lib):
    layers, N = [8, 64, 200, 48, 1], 1536
    P = O.init_params(layers, seed=3)
    fp = _flat(layers, P)
    x, y = _data(N, seed=9)
    x, y = x.to(_dev()).contiguous(), y.to(_dev()).contiguous()
    mk = lambda off: _drop(1, layers, 0.2, 77, 5, off)
    g1, l1 = train_grads(lib, layers, fp, x, y, mk(0))
    g2, l2 = train_grads(lib, layers, fp, x, y, mk(0))
    assert torch.equal(g1, g2) and torch.equal(l1, l2)
    cut = 640
    ga, la = train_grads(lib, layers, fp, x[:cut].contiguous(), y[:cut].contiguous(), mk(0), n_global=N)
    gb, lb = train_grads(lib, layers, fp, x[cut:].contiguous(), y[cut:].contiguous(), mk(cut), n_global=N)
    assert (ga + gb - g1).abs().max().item() <= 2e-5 * g1.abs().max().item()
    np.testing.assert_allclose((la + lb).numpy()[:3], l1.numpy()[:3], rtol=1e-6)
    # a row window alone is bitwise the same rows inside the larger call (forward and MC)
    a, b = 333, 1001
    u_all, lv_all = forward(lib, layers, fp, x, mk(0))
    u_w, lv_w = forward(lib, layers, fp, x[a:b].contiguous(), mk(a))
    assert torch.equal(u_all[a:b], u_w) and torch.equal(lv_all[a:b], lv_w)
    m_all = mc(lib, layers, fp, x, mk(0), 5)
    m_w = mc(lib, layers, fp, x[a:b].contiguous(), mk(a), 5)
    assert np.array_equal(m_all[:, a:b], m_w)


def test_mc_recorded_masks_vs_oracle(lib):
    layers, n, T, p = [8, 100, 100, 1], 200, 4, 0.4
    P = O.init_params(layers, seed=8)
    x, _ = _data(n, seed=1)
    gen = torch.Generator().manual_seed(11)
    passes = [[(torch.rand(n, w, generator=gen) >= p).numpy() for w in _widths(layers)] for _ in range(T)]
    bits = _pack_bits(passes).to(_dev())
    o = mc(lib, layers, _flat(layers, P), x.to(_dev()), _drop(2, layers, p, bits=bits), T)
    pm, au, eu = O.mc_dropout(P, x, p, T, lambda t: passes[t])
    np.testing.assert_allclose(o[0], pm, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(o[1], au, rtol=1e-4, atol=ATOL)
    np.testing.assert_allclose(o[2], eu, rtol=1e-3, atol=1e-5)


def test_mc_T2000_band_vs_bernoulli(lib):
    """The Philox stream at the reference's setting (T = 2000, p = 0.4) against the oracle on torch-bernoulli masks, on 256 rows:
    the means of e_u and a_u over the rows agree within 3 standard errors of their difference."""
    layers, N, NREF, T, p = [8, 32, 32, 32, 1], 4096, 256, 2000, 0.4
    P = O.init_params(layers, seed=3)
    x, _ = _data(N, seed=4)
    o = mc(lib, layers, _flat(layers, P), x.to(_dev()), _drop(1, layers, p, 2024, 1), T)
    gen = torch.Generator().manual_seed(7)
    mk = lambda t: [(torch.rand(NREF, w, generator=gen) >= p).numpy() for w in _widths(layers)]
    pm, au, eu = O.mc_dropout(P, x[:NREF], p, T, mk)
    np.testing.assert_allclose(o[0][:NREF], pm, rtol=RTOL, atol=ATOL)
    for name, col, ref in (("e_u", o[2], eu), ("a_u", o[1], au)):
        diff = col[:NREF].astype(np.float64) - ref.astype(np.float64)
        se = diff.std(ddof=1) / np.sqrt(NREF)
        assert abs(diff.mean() / se) < 3.0, (name, diff.mean() / se)
        assert abs(col[NREF:].mean() / col[:NREF].mean() - 1) < 0.1


def _net_params(m):
    return [p.detach().cpu().clone() for n, p in m.dnn.named_parameters() if not n.startswith("lambda")]


def test_train_dnn_injected_masks_vs_adam_oracle(lib):
    layers, n, steps = [8, 64, 200, 48, 1], 500, 3
    m, ds = _model(layers, n, kernels="general")
    P = _net_params(m)
    gen = torch.Generator().manual_seed(5)
    passes = [[(torch.rand(n, w, generator=gen) >= 0.2).numpy() for w in _widths(layers)] for _ in range(steps)]
    m.dnn.inject_masks(_pack_bits(passes))
    m.train_dnn(steps)
    ps = [p.clone().requires_grad_(True) for p in P]
    adam = O.AdamState(ps)
    for t in range(steps):
        _, _, go, _, _ = O.nll_loss_and_grads([p.detach() for p in ps], ds[0], ds[1], [0.2] * 4, passes[t])
        with torch.no_grad():
            adam.step(ps, go, O.steplr(0.01, 0.8, 1000, t))
    for (name, got), want in zip([(k, v) for k, v in m.dnn.named_parameters() if not k.startswith("lambda")], ps):
        w = want.detach()
        assert float((got.detach().cpu() - w).abs().max()) <= 1e-4 * (float(w.abs().max()) + 1e-3), name


def test_general_vs_fused_fp32_on_reference_net(lib):
    layers, n = [8, 256, 256, 256, 1], 1500
    mg, ds = _model(layers, n, kernels="general")
    ma, _ = _model(layers, n, precision="fp32")
    assert torch.equal(mg.dnn.flat_params(), ma.dnn.flat_params())
    x = ds[0].to(_dev())
    for m in (mg, ma):
        m.dnn.eval()
    ug = mg.dnn(x)[0].cpu().numpy()
    ua = ma.dnn(x)[0].cpu().numpy()
    np.testing.assert_allclose(ug, ua, rtol=RTOL, atol=ATOL)
    for m in (mg, ma):
        m.dnn.train()
    ug, lg = mg.dnn(x)
    ua, la = ma.dnn(x)        # same forward counter -> same Philox masks
    np.testing.assert_allclose(ug.cpu().numpy(), ua.cpu().numpy(), rtol=RTOL, atol=ATOL)
    og = [t.cpu().numpy() for t in mg.mc_dropout(x, 8)]
    oa = [t.cpu().numpy() for t in ma.mc_dropout(x, 8)]
    for a, b in zip(og, oa):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5)
    mg.train_dnn(3)
    ma.train_dnn(3)
    pg, pa = mg.dnn.flat_params().cpu(), ma.dnn.flat_params().cpu()
    assert float((pg - pa).abs().max()) <= 1e-4 * float(pa.abs().max())


def test_end_to_end_general_model(lib, tmp_path):
    import pinn_amd
    from pinn_amd import synth
    layers = [8, 64, 32, 16, 1]
    m, ds = _model(layers, 3000, kernels="general")
    assert m.dnn.kernels == "general" and m.dnn.widths == [64, 32, 16] and m.dnn.precision == "fp32"
    m.train_dnn(20)
    m.train_dnn(4, batch_size=1024)
    m.train_lambda(5, False)
    m.train_lambda(5, True)
    m.train_thermal(5)
    m.train_hydrogen(5)
    m.train_oxygen(5)
    u, lv = m.predict(ds[0], ds[4])
    assert u.shape == (3000, 1) and np.all(np.isfinite(u)) and np.all(np.isfinite(lv))
    arr = pinn_amd.create_comprehensive_results_array_v2(m, ds, mc_times=8, dropout=0.2)
    assert arr.ndim == 2 and arr.shape[0] > 0 and arr.shape[1] == 22 and np.all(np.isfinite(arr))
    path = str(tmp_path / "ck.pt")
    pinn_amd.save_checkpoint(m, path)
    m2, _ = _model(layers, 3000, kernels="general", seed=99)
    pinn_amd.load_checkpoint(m2, path)
    m.train_dnn(3)
    m2.train_dnn(3)
    assert torch.equal(m.dnn.flat_params(), m2.dnn.flat_params())
    m3, _ = _model([8, 64, 32, 8, 1], 3000, kernels="general")
    with pytest.raises(ValueError):
        pinn_amd.load_checkpoint(m3, path)


def test_constructor_surface(lib):
    import pinn_amd
    from pinn_amd import synth
    ds = synth.make_dataset(500, (), seed=0)
    with pytest.raises(ValueError):
        pinn_amd.PhysicsInformedNN(ds[0], ds[1], [8, 100, 100, 1], ds[4], ds[5], p=0.2, logvar=True)
    with pytest.raises(ValueError):
        pinn_amd.PhysicsInformedNN(ds[0], ds[1], [8, 100, 100, 1], ds[4], ds[5], p=0.2, logvar=True, kernels="general", precision="f32x6")
    m = pinn_amd.PhysicsInformedNN(ds[0], ds[1], [8, 100, 100, 1], ds[4], ds[5], p=0.2, logvar=True, kernels="general")
    m.verbose = False
    m.train_dnn(5)
    m.dnn.set_precision("fp32")
    with pytest.raises(ValueError):
        m.dnn.set_precision("bf16")
    m.dnn.check_range()
    u, _ = m.predict(ds[0], ds[4])
    assert np.all(np.isfinite(u))
    # the reference's keys and shapes after torch.manual_seed(0)
    layers = [8, 96, 48, 20, 1]
    torch.manual_seed(0)
    sd = pinn_amd.DNN(0.2, True, layers, kernels="general").state_dict()
    want = O.init_params(layers, seed=0)
    assert list(sd.keys()) == O.param_names(3)
    for k, w in zip(sd.keys(), want):
        assert tuple(sd[k].shape) == tuple(w.shape), k
