"""GPU: the DNN differentiated twice -- pinn_gnet_backward2 (csrc/pinn_general.hip) and the autograd="double" surface of
pinn_amd.DNN / PhysicsInformedNN for every kernel family.

The referee is always the oracle's mlp_forward in float64 under torch's own double autograd on the CPU:
    dx = grad([u, lv], x, [g_u, g_lv], create_graph=True);  grad(dx, [g_u, g_lv, x] + params, v, allow_unused=True)
Bound: the project's per-tensor rule, max |err| <= 2e-4 * max |ref| + 1e-6 * max |ref| (test_gpu_general._check_grads, REL of
test_gpu_autograd.py); torch's own float32 double autograd of the same oracle sits about 40 times inside it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pinn_oracle as O
from gnet_helpers import SHAPES, backward2, oracle2
from gnet_helpers import data as _data, dev as _dev, drop as _drop, flat as _flat, model as _model, pack_bits as _pack_bits
from gnet_helpers import padding as _padding, params as _params, philox_masks as _philox_masks, ptr as _ptr, stream as _stream
from gnet_helpers import unflat as _unflat, upstream, widths as _widths

REL = 2e-4
_upstream = functools.partial(upstream, with_v=True)      # g_u, g_lv and v


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


def _close(got, want, what):
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    print("%-50s err %.3e  scale %.3e  ratio to bound %.3f" % (what, err, scale, err / (REL * scale + 1e-6 * scale + 1e-300)))
    assert np.isfinite(err) and err <= REL * scale + 1e-6 * scale, (what, err, scale)


def _check(layers, got, ref, tag=""):
    wp, wx, wgu, wglv = ref
    k = len(layers) - 2
    if got.get("grads") is not None:
        for name, g, w in zip(O.param_names(k), _unflat(layers, got["grads"]), wp):
            if name == "predict.bias":
                assert float(w.abs().max()) == 0.0 and float(g.abs().max()) == 0.0, (layers, tag, name)      # exactly zero
            else:
                _close(g, w, "%s %s %s" % (layers, tag, name))
        assert float(_padding(layers, got["grads"]).abs().sum()) == 0.0
    if got.get("gx") is not None:
        _close(got["gx"], wx, "%s %s dS/dx" % (layers, tag))
    if got.get("ggu") is not None:
        _close(got["ggu"], wgu, "%s %s ud" % (layers, tag))
    if got.get("gglv") is not None:
        _close(got["gglv"], wglv, "%s %s lvd" % (layers, tag))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the C entry point against the oracle: eval, Philox masks, injected masks; 1, 63 and 1000 rows
@pytest.mark.parametrize("layers", SHAPES)
def test_backward2_vs_oracle_eval_philox_bits(lib, layers):
    P = O.init_params(layers, seed=sum(layers) + 1)
    fp = _flat(layers, P)
    pl = [0.2] * (len(layers) - 1)
    for n in (1, 63, 1000):
        x = _data(n, seed=n + 3)
        xd = x.to(_dev()).contiguous()
        gu, glv, vx = _upstream(n, n)
        gud, glvd, vxd = gu.to(_dev()), glv.to(_dev()), vx.to(_dev())
        # eval
        _check(layers, backward2(lib, layers, fp, xd, gud, glvd, vxd), oracle2(P, x, gu, glv, vx), "eval n=%d" % n)
        # Philox: seed >= 2^32, stream != 0, row_offset != 0
        seed, stream, row0 = 123456789012, 7, 999
        masks = _philox_masks(layers, seed, stream, row0, n, 0.2)
        _check(layers, backward2(lib, layers, fp, xd, gud, glvd, vxd, _drop(1, layers, 0.2, seed, stream, row0)),
               oracle2(P, x, gu, glv, vx, pl, masks), "philox n=%d" % n)
        # g_lv = NULL, same masks
        got = backward2(lib, layers, fp, xd, gud, None, vxd, _drop(1, layers, 0.2, seed, stream, row0))
        _check(layers, got, oracle2(P, x, gu, None, vx, pl, masks), "philox no-glv n=%d" % n)
        # injected bits
        gen = torch.Generator().manual_seed(n)
        masks = [(torch.rand(n, w, generator=gen) >= 0.3).numpy() for w in _widths(layers)]
        bits = _pack_bits(masks).to(_dev())
        _check(layers, backward2(lib, layers, fp, xd, gud, glvd, vxd, _drop(2, layers, 0.3, bits=bits)),
               oracle2(P, x, gu, glv, vx, [0.3] * (len(layers) - 1), masks), "bits n=%d" % n)


# more rows than one chunk of the double backward's layout (about 9.8e3 rows for this net)
def test_backward2_several_chunks(lib):
    from pinn_amd import _lib
    layers, n = [8, 2000, 300, 1], 23000
    net = _lib.GNet(layers)
    # the workspace stops growing at one chunk: two chunks' rows need no more than a hundred chunks' rows
    assert lib.pinn_gnet_backward2_workspace_bytes(ctypes.byref(net), n) == lib.pinn_gnet_backward2_workspace_bytes(ctypes.byref(net), 100 * n)
    assert lib.pinn_gnet_backward2_workspace_bytes(ctypes.byref(net), n // 4) < lib.pinn_gnet_backward2_workspace_bytes(ctypes.byref(net), n)
    P = O.init_params(layers, seed=4)
    x = _data(n, seed=6)
    gu, glv, vx = _upstream(n, 8)
    seed, stream, row0 = 5, 3, 17
    got = backward2(lib, layers, _flat(layers, P), x.to(_dev()).contiguous(), gu.to(_dev()), glv.to(_dev()), vx.to(_dev()),
                    _drop(1, layers, 0.2, seed, stream, row0))
    ref = oracle2(P, x, gu, glv, vx, [0.2] * 3, _philox_masks(layers, seed, stream, row0, n, 0.2))
    _check(layers, got, ref, "chunks")
    # every row's dS/dx against the tensor's scale
    wx = ref[1]
    err = (got["gx"].double() - wx).abs().max(dim=1).values
    assert bool(torch.all(err <= REL * wx.abs().max() + 1e-6)), float(err.max())


# 2. determinism: repeat, row windows, shards, NULL outputs
def test_backward2_deterministic_windows_shards_and_null_outputs(lib):
    layers, N = [8, 64, 200, 48, 1], 1536
    P = O.init_params(layers, seed=3)
    fp = _flat(layers, P)
    x = _data(N, seed=9).to(_dev()).contiguous()
    gu, glv, vx = (t.to(_dev()) for t in _upstream(N, 1))
    mk = lambda off: _drop(1, layers, 0.2, 77, 5, off)
    a1 = backward2(lib, layers, fp, x, gu, glv, vx, mk(0))
    a2 = backward2(lib, layers, fp, x, gu, glv, vx, mk(0))
    assert all(torch.equal(a1[k], a2[k]) for k in a1)
    a, b = 333, 1001
    w = backward2(lib, layers, fp, x[a:b].contiguous(), gu[a:b].contiguous(), glv[a:b].contiguous(), vx[a:b].contiguous(), mk(a),
                  want=("gx", "ggu", "gglv"))
    assert w["grads"] is None
    assert torch.equal(w["gx"], a1["gx"][a:b]) and torch.equal(w["ggu"], a1["ggu"][a:b]) and torch.equal(w["gglv"], a1["gglv"][a:b])
    cut = 640
    ga = backward2(lib, layers, fp, x[:cut].contiguous(), gu[:cut].contiguous(), glv[:cut].contiguous(), vx[:cut].contiguous(), mk(0),
                   want=("grads",))["grads"]
    gb = backward2(lib, layers, fp, x[cut:].contiguous(), gu[cut:].contiguous(), glv[cut:].contiguous(), vx[cut:].contiguous(), mk(cut),
                   want=("grads",))["grads"]
    for name, s, whole in zip(O.param_names(3), _unflat(layers, ga + gb), _unflat(layers, a1["grads"])):
        scale = float(whole.abs().max())
        assert float((s - whole).abs().max()) <= REL * scale + 1e-6 * scale, name
    # NULL outputs leave the others unchanged, one at a time and alone
    for k in a1:
        rest = tuple(q for q in a1 if q != k)
        got = backward2(lib, layers, fp, x, gu, glv, vx, mk(0), want=rest)
        assert all(torch.equal(got[q], a1[q]) for q in rest), k
        only = backward2(lib, layers, fp, x, gu, glv, vx, mk(0), want=(k,))
        assert torch.equal(only[k], a1[k]), k


def test_backward2_zero_rows_zeroes_grads(lib):
    from pinn_amd import _lib
    layers = [8, 64, 200, 48, 1]
    net = _lib.GNet(layers)
    total = lib.pinn_gnet_param_count(ctypes.byref(net))
    fp = torch.zeros(total, device=_dev())
    g = torch.full((total,), float("nan"), device=_dev())
    _lib.check(lib.pinn_gnet_backward2(ctypes.byref(net), _ptr(fp), None, 0, None, None, None, None, _ptr(g), None, None, None, None, 0,
                                       _stream()), "pinn_gnet_backward2")
    torch.cuda.synchronize()
    assert float(g.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# the module surface
def _oracle_loss(P, x, y, masks, w, layers, p=0.2):
    """float64 on the CPU: the loss of test 3 under torch's double autograd -> (parameter gradients, x gradient)."""
    P = [t.detach().double().clone().requires_grad_(True) for t in P]
    x = x.detach().double().clone().requires_grad_(True)
    u, lv = O.mlp_forward(P, x, [p] * (len(layers) - 1), masks)
    du_dx, = torch.autograd.grad(u.sum(), x, create_graph=True)
    dlv_dx, = torch.autograd.grad(lv.sum(), x, create_graph=True)
    loss = O.aleatoric_loss(y.double(), u, lv) + w * torch.mean(du_dx[:, 0] ** 2) + w * torch.mean(dlv_dx ** 2)
    g = torch.autograd.grad(loss, P + [x])
    return g[:-1], g[-1]


FAMILIES = [
    ([8, 64, 200, 48, 1], dict(kernels="general")),
    ([8, 128, 128, 128, 1], dict(precision="f32x6")),
    ([8, 256, 256, 256, 1], dict(precision="fp32")),
    ([8, 256, 256, 256, 1], dict(precision="f32x6g6")),
    ([8, 512, 512, 1], dict(precision="f32x6")),
]


# 3. the module, every kernel family: a loss that contains du/dx and dlogvar/dx moves every parameter as the float64 oracle says
@pytest.mark.parametrize("layers,kw", FAMILIES)
def test_module_double_backward_every_family(layers, kw):
    n, w = 700, 0.5
    m, ds = _model(layers, n=n, autograd="double", **kw)
    dnn = m.dnn
    assert dnn.autograd == "double"
    dnn.train()
    x = ds[0].to(_dev()).clone().requires_grad_(True)
    y = ds[1].to(_dev())
    dnn.zero_grad(set_to_none=True)
    c0 = dnn._fwd_counter
    u, lv = dnn(x)
    du_dx, = torch.autograd.grad(u.sum(), x, create_graph=True)
    dlv_dx, = torch.autograd.grad(lv.sum(), x, create_graph=True)
    assert du_dx.grad_fn is not None and dlv_dx.grad_fn is not None
    loss = m.aleatoric_loss(y, u, lv) + w * torch.mean(du_dx[:, 0] ** 2) + w * torch.mean(dlv_dx ** 2)
    loss.backward()
    masks = _philox_masks(layers, dnn.seed, 0x80000000 + c0 + 1, 0, n, 0.2)
    wp, wx = _oracle_loss([t.detach().cpu() for t in _params(dnn)], ds[0], ds[1], masks, w, layers)
    for t, ref, name in zip(_params(dnn), wp, O.param_names(dnn.n_hidden)):
        _close(t.grad.cpu(), ref, "%s %s %s" % (layers, kw, name))
    _close(x.grad.cpu(), wx, "%s %s x" % (layers, kw))


# an upstream gradient that depends on the weights: d/dx of u^2 has g_u = 2 u, whose own gradient is ud
def test_module_upstream_depends_on_weights():
    layers, n = [8, 64, 200, 48, 1], 500
    m, ds = _model(layers, n=n, autograd="double", kernels="general")
    dnn = m.dnn
    dnn.train()
    x = ds[0].to(_dev()).clone().requires_grad_(True)
    dnn.zero_grad(set_to_none=True)
    c0 = dnn._fwd_counter
    u, lv = dnn(x)
    d, = torch.autograd.grad((u ** 2).sum() + (lv ** 2).sum(), x, create_graph=True)
    torch.mean(d ** 2).backward()
    masks = _philox_masks(layers, dnn.seed, 0x80000000 + c0 + 1, 0, n, 0.2)
    P = [t.detach().cpu().double().requires_grad_(True) for t in _params(dnn)]
    xo = ds[0].double().clone().requires_grad_(True)
    uo, lvo = O.mlp_forward(P, xo, [0.2] * 4, masks)
    do, = torch.autograd.grad((uo ** 2).sum() + (lvo ** 2).sum(), xo, create_graph=True)
    ref = torch.autograd.grad(torch.mean(do ** 2), P + [xo])
    for t, r, name in zip(_params(dnn), ref[:-1], O.param_names(3)):
        _close(t.grad.cpu(), r, "g(theta) " + name)
    _close(x.grad.cpu(), ref[-1], "g(theta) x")


# 4. unchanged behaviour
def test_double_mode_leaves_first_order_bitwise():
    n = 300
    layers = [8, 128, 128, 128, 1]
    m, ds = _model(layers, n=n)
    dnn = m.dnn
    x = ds[0].to(_dev()).contiguous()
    gu, glv, _ = (t.to(_dev()) for t in _upstream(n, 4))
    gu, glv = gu.reshape(-1, 1), glv.reshape(-1, 1)
    res = {}
    for train in (False, True):
        dnn.train(train)
        dnn.autograd = False
        dnn._fwd_counter = 5
        u0, lv0 = dnn(x)
        for mode in (True, "double"):
            dnn.autograd = mode
            assert dnn.autograd == mode and type(dnn.autograd) is type(mode)
            dnn._fwd_counter = 5
            xg = x.clone().requires_grad_(True)
            dnn.zero_grad(set_to_none=True)
            u, lv = dnn(xg)
            assert u.grad_fn is not None
            assert torch.equal(u0, u.detach()) and torch.equal(lv0, lv.detach())          # outputs: bit-identical to autograd=False
            (gu * u + glv * lv).sum().backward()
            res[(train, mode)] = [p.grad.clone() for p in _params(dnn)] + [xg.grad.clone()]
            if mode == "double":      # under create_graph=True: a dL/dx with a grad_fn, parameter gradients the same numbers
                dnn._fwd_counter = 5
                dnn.zero_grad(set_to_none=True)
                xg.grad = None
                u, lv = dnn(xg)
                (gu * u + glv * lv).sum().backward(create_graph=True)
                assert xg.grad.grad_fn is not None
                got = [p.grad.detach() for p in _params(dnn)] + [xg.grad.detach()]
                assert all(torch.equal(a, b) for a, b in zip(got, res[(train, mode)]))
                dnn.zero_grad(set_to_none=True)
                xg.grad = None
        assert all(torch.equal(a, b) for a, b in zip(res[(train, True)], res[(train, "double")]))      # plain backward: bit-identical


def test_library_trainers_and_mc_after_double_backward():
    import pinn_amd
    layers = [8, 128, 128, 128, 1]
    a, ds = _model(layers, n=500, autograd="double")
    b, _ = _model(layers, n=500)
    assert torch.equal(a.dnn.flat_params(), b.dnn.flat_params())
    a.dnn.train()
    x = ds[0].to(_dev()).clone().requires_grad_(True)
    u, lv = a.dnn(x)
    du_dx, = torch.autograd.grad(u.sum(), x, create_graph=True)
    grads = torch.autograd.grad(a.aleatoric_loss(a.u, u, lv) + torch.mean(torch.relu(du_dx[:, 0]) ** 2), _params(a.dnn))
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    a.dnn.zero_grad(set_to_none=True)
    a.dnn._fwd_counter = b.dnn._fwd_counter
    a.train_dnn(3)
    b.train_dnn(3)
    assert torch.equal(a.dnn.flat_params(), b.dnn.flat_params())
    ra = pinn_amd.get_MC_samples(a, ds[2], ds[4], mc_times=4, dropout=0.4)
    rb = pinn_amd.get_MC_samples(b, ds[2], ds[4], mc_times=4, dropout=0.4)
    assert all(np.array_equal(p, q) for p, q in zip(ra, rb))


def test_monotonicity_penalty_trains_with_adam():
    """The use the mode exists for: a penalty on a column of du/dx beside aleatoric_loss, stepped by torch.optim.Adam."""
    m, ds = _model([8, 64, 200, 48, 1], n=600, autograd="double", kernels="general")
    m.dnn.eval()
    opt = torch.optim.Adam(m.dnn.parameters(), lr=1e-3)
    x = m.x.detach().clone().requires_grad_(True)
    pen = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        u, lv = m.net_u(x)
        du_dx, = torch.autograd.grad(u.sum(), x, create_graph=True)
        penalty = torch.mean(du_dx[:, 0] ** 2)
        (1e-3 * m.aleatoric_loss(m.u, u, lv) + penalty).backward()
        opt.step()
        pen.append(float(penalty.detach()))
    # descent on a loss the penalty dominates must lower the penalty; it could not move at all if du/dx carried no graph
    assert np.isfinite(pen).all() and pen[-1] < pen[0], (pen[0], pen[-1])


# errors
def test_errors_double_mode():
    import pinn_amd
    from pinn_amd import synth
    ds = synth.make_dataset(200, (), seed=0)
    layers = [8, 256, 256, 256, 1]
    mk = lambda **kw: pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=True, **kw)
    with pytest.raises(ValueError):
        mk(precision="bf16", autograd="double")
    with pytest.raises(ValueError):
        mk(autograd="twice")
    m = mk(precision="bf16")
    with pytest.raises(ValueError):
        m.dnn.autograd = "double"
    m = mk(autograd="double", physics_autograd="full")          # "full" accepts a net in "double" mode
    assert m.dnn.autograd == "double" and m.physics_autograd == "full"
    with pytest.raises(ValueError):
        m.dnn.set_precision("bf16")
    with pytest.raises(ValueError):
        m.dnn.autograd = "twice"
    assert m.dnn.autograd == "double"
    x = ds[0].to(_dev()).clone().requires_grad_(True)
    # True mode still raises on create_graph=True
    m.dnn.autograd = True
    u, lv = m.dnn(x)
    with pytest.raises(RuntimeError, match="once-differentiable"):
        torch.autograd.grad(u.sum(), x, create_graph=True)
    m.dnn.autograd = "double"
    # a cotangent on a parameter gradient
    w0 = _params(m.dnn)[0]
    u, lv = m.dnn(x)
    gw, = torch.autograd.grad(u.sum(), w0, create_graph=True)
    with pytest.raises(RuntimeError, match="parameter gradient"):
        gw.sum().backward()
    # a third derivative
    u, lv = m.dnn(x)
    d1, = torch.autograd.grad(u.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        d2, = torch.autograd.grad((d1 ** 2).sum(), x, create_graph=True)
        torch.autograd.grad((d2 ** 2).sum(), x)
    # an in-place parameter change between the passes: torch's version error
    u, lv = m.dnn(x)
    d1, = torch.autograd.grad(u.sum(), x, create_graph=True)
    with torch.no_grad():
        w0.mul_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (d1 ** 2).sum().backward()
