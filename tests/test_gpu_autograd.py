"""GPU: the DNN under torch autograd -- pinn_gnet_backward (csrc/pinn_general.hip) against the CPU oracle's autograd, and the
autograd=True surface of pinn_amd.DNN / PhysicsInformedNN for every kernel family."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pinn_oracle as O
from conftest import ScalerFromArrays, load_golden, unpack_mask
from gnet_helpers import SHAPES, backward, oracle_vjp
from gnet_helpers import data as _data, dev as _dev, drop as _drop, flat as _flat, model as _model, pack_bits as _pack_bits
from gnet_helpers import params as _params, philox_masks as _philox_masks, unflat as _unflat, upstream as _upstream, widths as _widths

REL = 2e-4          # per tensor: max |err| <= REL * max |ref|  (test_gpu_general._check_grads)


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


def _close(got, want, what):
    scale = float(want.abs().max()) + 1e-30
    err = float((got - want).abs().max())
    assert np.isfinite(err) and err <= REL * scale + 1e-6 * scale, (what, err, scale)


def _check(layers, got_flat, got_dx, want_p, want_dx):
    for name, g, w in zip(O.param_names(len(layers) - 2), _unflat(layers, got_flat), want_p):
        _close(g, w, (layers, name))
    if want_dx is not None:
        _close(got_dx, want_dx, (layers, "dx"))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the C ABI against the oracle
@pytest.mark.parametrize("layers", SHAPES)
def test_backward_vs_oracle_eval_philox_bits(lib, layers):
    P = O.init_params(layers, seed=sum(layers) + 1)
    fp = _flat(layers, P)
    pl = [0.2] * (len(layers) - 1)
    for n in (1, 17, 1000):
        x = _data(n, seed=n + 3)
        xd = x.to(_dev()).contiguous()
        gu, glv = _upstream(n, n)
        gud, glvd = gu.to(_dev()), glv.to(_dev())
        # eval
        g, dx = backward(lib, layers, fp, xd, gud, glvd)
        wp, wx = oracle_vjp(P, x, gu, glv)
        _check(layers, g, dx, wp, wx)
        # Philox: seed >= 2^32, stream != 0, row_offset != 0
        seed, stream, row0 = 123456789012, 7, 999
        g, dx = backward(lib, layers, fp, xd, gud, glvd, _drop(1, layers, 0.2, seed, stream, row0))
        wp, wx = oracle_vjp(P, x, gu, glv, pl, _philox_masks(layers, seed, stream, row0, n, 0.2))
        _check(layers, g, dx, wp, wx)
        # g_lv = NULL, same masks
        g, dx = backward(lib, layers, fp, xd, gud, None, _drop(1, layers, 0.2, seed, stream, row0))
        wp, wx = oracle_vjp(P, x, gu, None, pl, _philox_masks(layers, seed, stream, row0, n, 0.2))
        _check(layers, g, dx, wp, wx)
        # injected bits
        gen = torch.Generator().manual_seed(n)
        masks = [(torch.rand(n, w, generator=gen) >= 0.3).numpy() for w in _widths(layers)]
        bits = _pack_bits(masks).to(_dev())
        g, dx = backward(lib, layers, fp, xd, gud, glvd, _drop(2, layers, 0.3, bits=bits))
        wp, wx = oracle_vjp(P, x, gu, glv, [0.3] * (len(layers) - 1), masks)
        _check(layers, g, dx, wp, wx)


# 2. more rows than one training chunk
def test_backward_several_chunks(lib):
    layers, n = [8, 2000, 300, 1], 50000
    P = O.init_params(layers, seed=4)
    x = _data(n, seed=6)
    gu, glv = _upstream(n, 8)
    seed, stream, row0 = 5, 3, 17
    g, dx = backward(lib, layers, _flat(layers, P), x.to(_dev()).contiguous(), gu.to(_dev()), glv.to(_dev()),
                     _drop(1, layers, 0.2, seed, stream, row0))
    wp, wx = oracle_vjp(P, x, gu, glv, [0.2] * 3, _philox_masks(layers, seed, stream, row0, n, 0.2))
    _check(layers, g, dx, wp, wx)
    # every row's dx against the tensor's scale, the largest |dx| of any row (a row's own scale: test_gpu_general_referee.py)
    err = (dx - wx).abs().max(dim=1).values
    assert bool(torch.all(err <= REL * wx.abs().max() + 1e-6)), float(err.max())


# 3. determinism: repeat, row windows, shards
def test_backward_deterministic_windows_and_shards(lib):
    layers, N = [8, 64, 200, 48, 1], 1536
    P = O.init_params(layers, seed=3)
    fp = _flat(layers, P)
    x = _data(N, seed=9).to(_dev()).contiguous()
    gu, glv = (t.to(_dev()) for t in _upstream(N, 1))
    mk = lambda off: _drop(1, layers, 0.2, 77, 5, off)
    g1, x1 = backward(lib, layers, fp, x, gu, glv, mk(0))
    g2, x2 = backward(lib, layers, fp, x, gu, glv, mk(0))
    assert torch.equal(g1, g2) and torch.equal(x1, x2)
    a, b = 333, 1001
    _, xw = backward(lib, layers, fp, x[a:b].contiguous(), gu[a:b].contiguous(), glv[a:b].contiguous(), mk(a))
    assert torch.equal(xw, x1[a:b])
    cut = 640
    ga, _ = backward(lib, layers, fp, x[:cut].contiguous(), gu[:cut].contiguous(), glv[:cut].contiguous(), mk(0), want_dx=False)
    gb, _ = backward(lib, layers, fp, x[cut:].contiguous(), gu[cut:].contiguous(), glv[cut:].contiguous(), mk(cut), want_dx=False)
    assert (ga + gb - g1).abs().max().item() <= 2e-5 * g1.abs().max().item()


# ---------------------------------------------------------------------------------------------------------------------------
# the module surface
def _check_module(dnn, layers, x, gu, glv, masks, p=0.2):
    P = [t.detach().cpu() for t in _params(dnn)]
    wp, wx = oracle_vjp(P, x.detach().cpu(), gu.cpu(), glv.cpu(), [p] * (len(layers) - 1), masks)
    for t, w, name in zip(_params(dnn), wp, O.param_names(dnn.n_hidden)):
        _close(t.grad.cpu(), w, (layers, name))
    _close(x.grad.cpu(), wx, (layers, "x"))


# 4. the module, every kernel family
@pytest.mark.parametrize("layers,kw", [
    ([8, 64, 200, 48, 1], dict(kernels="general")),
    ([8, 128, 128, 128, 1], dict(precision="f32x6")),
    ([8, 256, 256, 256, 1], dict(precision="fp32")),
    ([8, 256, 256, 256, 1], dict(precision="f32x6g6")),
    ([8, 512, 512, 1], dict(precision="f32x6")),
])
def test_module_grads_every_family(layers, kw):
    import pinn_amd
    n = 700
    m, ds = _model(layers, n=n, autograd=True, **kw)
    dnn = m.dnn
    dnn.train()
    x = ds[0].to(_dev()).clone().requires_grad_(True)
    gu, glv = (t.to(_dev()) for t in _upstream(n, 2))
    dnn.zero_grad(set_to_none=True)
    c0 = dnn._fwd_counter
    u, lv = dnn(x)
    assert u.grad_fn is not None and lv.grad_fn is not None
    (gu.reshape(-1, 1) * u + glv.reshape(-1, 1) * lv).sum().backward()
    _check_module(dnn, layers, x, gu, glv, _philox_masks(layers, dnn.seed, 0x80000000 + c0 + 1, 0, n, 0.2))
    # through net_u of a shard (row_offset != 0): the masks of global rows [row_offset, row_offset + n)
    off = 4321
    ms = pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=True, seed=13, row_offset=off,
                                    n_global=off + n, autograd=True, **kw)
    ms.verbose = False
    ms.dnn.load_state_dict({k: v for k, v in dnn.state_dict().items() if not k.startswith("lambda")}, strict=False)
    ms.dnn.train()
    ms.dnn.zero_grad(set_to_none=True)
    x2 = ds[0].to(_dev()).clone().requires_grad_(True)
    c0 = ms.dnn._fwd_counter
    u, lv = ms.net_u(x2)
    (gu.reshape(-1, 1) * u + glv.reshape(-1, 1) * lv).sum().backward()
    _check_module(ms.dnn, layers, x2, gu, glv, _philox_masks(layers, 13, 0x80000000 + c0 + 1, off, n, 0.2))


# 5. surface semantics
def test_surface_semantics():
    n = 300
    layers = [8, 128, 128, 128, 1]
    m, ds = _model(layers, n=n)
    dnn = m.dnn
    assert dnn.autograd is False
    x = ds[0].to(_dev()).contiguous()
    xg = x.clone().requires_grad_(True)
    for train in (False, True):
        dnn.train(train)
        dnn.autograd = False
        dnn._fwd_counter = 5
        u0, lv0 = dnn(x)
        assert u0.grad_fn is None
        dnn.autograd = True
        dnn._fwd_counter = 5
        u1, lv1 = dnn(xg)
        assert u1.grad_fn is not None
        assert torch.equal(u0, u1.detach()) and torch.equal(lv0, lv1.detach())
        with torch.no_grad():
            u2, lv2 = dnn(xg)
        assert u2.grad_fn is None and lv2.grad_fn is None

    # two backward calls accumulate to 2x (eval: same masks)
    dnn.eval()
    gu, glv = (t.to(_dev()).reshape(-1, 1) for t in _upstream(n, 4))
    dnn.zero_grad(set_to_none=True)
    xg.grad = None
    u, lv = dnn(xg)
    L = (gu * u + glv * lv).sum()
    L.backward(retain_graph=True)
    one = [p.grad.clone() for p in _params(dnn)] + [xg.grad.clone()]
    L.backward()
    two = [p.grad for p in _params(dnn)] + [xg.grad]
    assert all(torch.equal(b, 2 * a) for a, b in zip(one, two))

    # two training forwards, one backward: the sum of each with its own masks
    dnn.train()
    dnn.zero_grad(set_to_none=True)
    xg.grad = None
    c0 = dnn._fwd_counter
    u1, lv1 = dnn(xg)
    u2, lv2 = dnn(xg)
    ((gu * u1 + glv * lv1).sum() + (gu * u2 + glv * lv2).sum()).backward()
    P = [t.detach().cpu() for t in _params(dnn)]
    pl = [0.2] * 4
    wa, xa = oracle_vjp(P, ds[0], gu.cpu(), glv.cpu(), pl, _philox_masks(layers, dnn.seed, 0x80000000 + c0 + 1, 0, n, 0.2))
    wb, xb = oracle_vjp(P, ds[0], gu.cpu(), glv.cpu(), pl, _philox_masks(layers, dnn.seed, 0x80000000 + c0 + 2, 0, n, 0.2))
    for t, a, b, name in zip(_params(dnn), wa, wb, O.param_names(3)):
        _close(t.grad.cpu(), a + b, name)
    _close(xg.grad.cpu(), xa + xb, "x")

    # logvar=False: a constant zero logvar
    import pinn_amd
    m2 = pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=False, autograd=True)
    u, lv = m2.dnn(xg)
    assert u.grad_fn is not None and lv.grad_fn is None and not lv.requires_grad and float(lv.abs().sum()) == 0.0
    u.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in _params(m2.dnn))


# 6. the reference's own loop (01:931-955) in plain torch reproduces G7
def test_reference_train_dnn_loop_golden():
    import hip_helpers as hh
    import pinn_amd
    from torch.optim.lr_scheduler import StepLR
    g = load_golden("g_train.npz")
    sc = load_golden("g_traj.npz")
    sx, sy = ScalerFromArrays(sc, "sx."), ScalerFromArrays(sc, "sy.")
    H = 128
    self = pinn_amd.PhysicsInformedNN(torch.from_numpy(g["x"]), torch.from_numpy(g["y"]), [8, H, H, H, 1], sx, sy, p=0.2, logvar=True,
                                      autograd=True)
    self.verbose = False
    sd = {k[len("w0."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w0.")}
    missing, unexpected = self.dnn.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("lambda") for k in missing)
    per_step = [[unpack_mask(g["mask%d_s%d" % (l, s)], 128 if l < 3 else 64) for l in range(4)] for s in range(3)]
    self.dnn.inject_masks(hh.pack_mask_bits(per_step))

    for param in self.dnn.parameters():
        param.requires_grad = True
    self.lambda_1.requires_grad = False
    self.lambda_2.requires_grad = False
    self.lambda_3.requires_grad = False
    self.lambda_4.requires_grad = False
    optimizer_Adam = torch.optim.Adam(self.dnn.parameters(), lr=0.01)
    scheduler_Adam = StepLR(optimizer_Adam, step_size=1000, gamma=0.8)
    self.dnn.train()
    for epoch in range(3):
        u_pred, log_var = self.net_u(self.x)
        loss = self.aleatoric_loss(self.u, u_pred, log_var)
        optimizer_Adam.zero_grad()
        loss.backward()
        optimizer_Adam.step()
        scheduler_Adam.step()

    sd = self.dnn.state_dict()
    for n in O.param_names(3):
        np.testing.assert_allclose(sd[n].cpu().numpy(), g["w3." + n], rtol=5e-4, atol=5e-6, err_msg=n)
    assert self.x.grad is not None and bool(torch.isfinite(self.x.grad).all())


# 7. the library's trainers are untouched by user autograd
def test_library_trainers_after_user_autograd(tmp_path):
    from pinn_amd import report
    layers = [8, 128, 128, 128, 1]
    a, ds = _model(layers, n=500, autograd=True)
    opt = torch.optim.Adam(a.dnn.parameters(), lr=1e-3)
    a.dnn.train()
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        u, lv = a.net_u(a.x)
        a.aleatoric_loss(a.u, u, lv).backward()
        opt.step()
    opt.zero_grad(set_to_none=True)
    path = str(tmp_path / "a.pt")
    report.save_checkpoint(a, path)
    b, _ = _model(layers, n=500)
    report.load_checkpoint(b, path)
    a.train_dnn(3)
    b.train_dnn(3)
    assert torch.equal(a.dnn.flat_params(), b.dnn.flat_params())


# 8. errors
def test_errors():
    import pinn_amd
    from pinn_amd import synth
    ds = synth.make_dataset(200, (), seed=0)
    layers = [8, 256, 256, 256, 1]
    with pytest.raises(ValueError):
        pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=True, precision="bf16", autograd=True)
    m = pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=True, precision="bf16")
    with pytest.raises(ValueError):
        m.dnn.autograd = True
    m = pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=True, autograd=True)
    with pytest.raises(ValueError):
        m.dnn.set_precision("bf16")
    x = ds[0].to(_dev()).clone().requires_grad_(True)
    u, lv = m.dnn(x)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(u.sum(), x, create_graph=True)
    u, lv = m.dnn(x)
    with torch.no_grad():
        _params(m.dnn)[0].mul_(1.0)
    with pytest.raises(RuntimeError):
        (u.sum() + lv.sum()).backward()
