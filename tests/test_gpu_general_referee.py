"""GPU: the general (any layers list) kernels of csrc/pinn_general.hip held to the float64 referee of tests/gnet_referee.py, element by
element: every output element against its own absolute sum, at the widths, depths and row counts the kernels' geometry makes edges
(64 x 64 tiles, K slabs of 32, widths padded to 32, the bias column of the weight-gradient tile, slice seams with a ragged last slice).
The referee, the band, its floors and the mutants that must fall outside it are proven on the CPU by test_gnet_referee_host.py; nothing
here was set from a device's output.  Every comparison prints its ratio to the band (<= 1 passes) before it asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gnet_referee as G
from gnet_helpers import backward, backward2, dev, flat, forward, pack_bits, padding, train_grads, unflat

IDS = ["-".join(map(str, s[1:-1])) if len(s) < 8 else "k8" for s in G.EDGE_SHAPES]


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


def _device(c):
    """The case's inputs on the device: flat parameters, x, y, g_u, g_lv, v and the dropout struct (with its packed bits kept alive)."""
    bits = pack_bits(c.masks).to(dev()) if c.mode == "bits" else None
    d = dict(fp=flat(c.layers, c.P), x=c.x.to(dev()).contiguous(), y=c.y.to(dev()).contiguous(), gu=c.gu.to(dev()), glv=c.glv.to(dev()),
             vx=c.vx.to(dev()).contiguous(), bits=bits)
    d["drop"] = c.drop(bits)
    return d


def _grads(c, g):
    """Flat gradient -> tensors in O.param_names order; the entries that belong to no tensor must be exactly 0."""
    assert float(padding(c.layers, g).abs().sum()) == 0.0, (c.layers, c.n, c.mode, "padding of the flat gradient")
    return [t.numpy() for t in unflat(c.layers, g)]


def _hold(c, what, ratios, out):
    """ratios: {output: ratio to its band}.  Printed; what is outside is added to `out`, which the test asserts empty after its last case,
    so that a miss does not hide the cases after it."""
    worst = max(ratios, key=ratios.get)
    print("%-28s n=%-3d %-6s %-10s worst %.3f (%s)  %s" % (c.layers if c.k < 8 else "k8", c.n, c.mode, what, ratios[worst], worst,
                                                          " ".join("%.2f" % v for v in ratios.values())))
    out += [(c.n, c.mode, what, k, round(v, 3)) for k, v in ratios.items() if not v <= 1.0]
    return ratios[worst]


@pytest.mark.parametrize("layers", G.EDGE_SHAPES, ids=IDS)
def test_forward_vs_referee(lib, layers):
    """pinn_gnet_forward: u and logvar of every row by the row's own absolute sums."""
    worst, out = 0.0, []
    for c in G.cases(layers):
        d = _device(c)
        u, lv = forward(lib, layers, d["fp"], d["x"], d["drop"])
        res = dict(u=u.numpy(), lv=lv.numpy())
        worst = max(worst, _hold(c, "forward", {o: c.ratio(res, "vjp_u", o) for o in ("u", "lv")}, out))
    print("%s forward: worst eps / band %.3f" % (layers, worst))
    assert not out, (layers, out)


@pytest.mark.parametrize("layers", G.EDGE_SHAPES, ids=IDS)
def test_train_grads_vs_referee(lib, layers):
    """pinn_gnet_train_grads: every gradient element by its absolute sum over the rows; the three loss sums by the sum of their rows'
    float32 errors (gnet_referee's docstring has the bound and why)."""
    worst, out = 0.0, []
    for c in G.cases(layers):
        assert (c.rows, c.slices, c.slice_rows) == G.SLICES[c.n]
        d = _device(c)
        g, loss = train_grads(lib, layers, d["fp"], d["x"], d["y"], d["drop"])
        res = dict(grads=_grads(c, g))
        ratios = {o: c.ratio(res, "train", o) for o in c.names}
        ratios["loss sums"] = c.sums_ratio(loss.numpy()[:3])
        worst = max(worst, _hold(c, "train", ratios, out))
    print("%s train_grads: worst eps / band %.3f" % (layers, worst))
    assert not out, (layers, out)


@pytest.mark.parametrize("layers", G.EDGE_SHAPES, ids=IDS)
def test_backward_vs_referee(lib, layers):
    """pinn_gnet_backward with g_u and g_lv, and with g_lv = NULL: gradients and dx."""
    worst, out = 0.0, []
    for c in G.cases(layers):
        d = _device(c)
        for kind, glv in (("vjp", d["glv"]), ("vjp_u", None)):
            g, dx = backward(lib, layers, d["fp"], d["x"], d["gu"], glv, d["drop"])
            res = dict(grads=_grads(c, g), dx=dx.numpy())
            worst = max(worst, _hold(c, "backward" if glv is not None else "backward, no g_lv",
                                     {o: c.ratio(res, kind, o) for o in c.names + ["dx"]}, out))
    print("%s backward: worst eps / band %.3f" % (layers, worst))
    assert not out, (layers, out)


@pytest.mark.parametrize("layers", G.EDGE_SHAPES, ids=IDS)
def test_backward2_vs_referee(lib, layers):
    """pinn_gnet_backward2 against torch's float64 double autograd: parameter gradients scaled by the first-order absolute sums under
    (|g_u|, |g_lv|), gx / ggu / gglv by their row's largest reference value; with g_lv and with g_lv = NULL.

    The floors of these five classes were first measured with one float32 order that on widths up to 32 was torch's own run; at those
    floors a device sat at 1.01 .. 1.83 of the band in six tensors of four lists (gglv of [8, 31, 1] at 289 rows: a row whose reference
    cancels 7400-fold, the device's error 3.7e-8 against a median of 0.076), and so did the CPU's own restatements once they were
    independent (test_float32_restatement_inside_half_the_band).  At the floors those settle the device is at 0.17 .. 0.80."""
    worst, out = 0.0, []
    for c in G.cases(layers, G.rows2_of(layers)):
        assert G.train_layout(layers, c.n, 2)[:3] == G.SLICES[c.n]
        d = _device(c)
        for with_glv in (True, False):
            got = backward2(lib, layers, d["fp"], d["x"], d["gu"], d["glv"] if with_glv else None, d["vx"], d["drop"])
            res = dict(grads=_grads(c, got["grads"]), gx=got["gx"].numpy(), ggu=got["ggu"].numpy(), gglv=got["gglv"].numpy())
            worst = max(worst, _hold(c, "backward2" if with_glv else "backward2, no g_lv",
                                     {o: c.ratio2(res, o, with_glv) for o in c.names + ["gx", "ggu", "gglv"]}, out))
    print("%s backward2: worst eps / band %.3f" % (layers, worst))
    assert not out, (layers, out)
