"""CPU: the float64 referee and the band of the general kernels (tests/gnet_referee.py) before any device sees them -- the referee
against torch's double autograd, the slice arithmetic against the library's workspace query, the float32 restatement inside half the
band on every case (what settles the floor), and every mutant of the referee outside it."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import gnet_referee as G
import pinn_oracle as O

IDS = ["-".join(map(str, s[1:-1])) if len(s) < 8 else "k8" for s in G.EDGE_SHAPES]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    return _lib.load(build_if_missing=False)


def _autograd64(c, kind):
    """torch double autograd of O.mlp_forward -> (u, lv, grads, dx or None) as numpy float64."""
    P = [p.double() for p in c.P]
    x = c.x.double()
    if kind == "train":
        _, _, g, u, lv = O.nll_loss_and_grads(P, x, c.y.double().reshape(-1, 1), c.ps, c.masks)
        return u.numpy().reshape(-1), lv.numpy().reshape(-1), [t.numpy() for t in g], None
    P = [p.clone().requires_grad_(True) for p in P]
    x = x.clone().requires_grad_(True)
    u, lv = O.mlp_forward(P, x, c.ps, c.masks)
    outs, gos = [u], [c.gu.double().reshape(-1, 1)]
    if kind == "vjp":
        outs.append(lv)
        gos.append(c.glv.double().reshape(-1, 1))
    g = torch.autograd.grad(outs, P + [x], gos, allow_unused=True)
    g = [(torch.zeros_like(t) if gi is None else gi).numpy() for gi, t in zip(g, P + [x])]
    return u.detach().numpy().reshape(-1), lv.detach().numpy().reshape(-1), g[:-1], g[-1]


@pytest.mark.parametrize("layers", G.EDGE_SHAPES, ids=IDS)
def test_referee_matches_torch_double_autograd(layers):
    """Forward, nll_loss_and_grads, the VJP with free g_u / g_lv and with g_lv = None: every element within 1e-12 of its own absolute
    sum plus its tensor's largest element (two float64 programs differ by 1e-16 times the cancellation of the layers above, which a
    last product's absolute sum does not see: 1.2e-12 of it on one row of [8, 63, 64, 64, 1]); 1e-12 is 2e-5 u.  O.mlp_forward casts
    its masks to float32, which is exact for 0 / 1, and its dropout scale is the float32 one in both."""
    worst = 0.0
    for c in G.cases(layers):
        for kind in ("train", "vjp", "vjp_u"):
            R, M = c.ref(kind)
            u, lv, g, dx = _autograd64(c, kind)
            want = dict(u=u, lv=lv, grads=g, dx=dx)
            for name in c.outputs(kind):
                ref = np.asarray(c.pick(want, name), dtype=np.float64)
                e = G.eps(c.pick(R, name), ref, c.pick(M, name) + np.abs(ref).max())[0]
                worst = max(worst, e)
                assert e <= 1e-12, (layers, c.n, c.mode, kind, name, e)
        R, _ = c.ref("train")
        lo, mse, _, _, _ = O.nll_loss_and_grads([p.double() for p in c.P], c.x.double(), c.y.double().reshape(-1, 1), c.ps, c.masks)
        assert abs((R["sums"][0] + 0.01 * R["sums"][1]) / c.n - lo.item()) <= 1e-12 * abs(lo.item())
        assert abs(R["sums"][2] / c.n - mse.item()) <= 1e-12 * abs(mse.item())
    print("%s: largest |referee - autograd| / M = %.2e" % (layers, worst))


@pytest.mark.parametrize("layers", G.EDGE_SHAPES, ids=IDS)
def test_slice_counts_and_workspace_query(lib, layers):
    """The slice count every case states (G.SLICES, from the arithmetic of train_layout / slice_plan) is what the restated layout gives,
    and the restated layout is the library's: the workspace bytes contain slices * gradient floats."""
    from pinn_amd import _lib
    net = ctypes.byref(_lib.GNet(layers))
    for n in G.rows_of(layers):
        for ns in (1, 2):
            rows, slices, slice_rows, nbytes = G.train_layout(layers, n, ns)
            assert (rows, slices, slice_rows) == G.SLICES[n], (layers, n, ns)
            assert slice_rows % 32 == 0 and (slices - 1) * slice_rows < rows <= slices * slice_rows
            if ns == 1:
                assert lib.pinn_gnet_workspace_bytes(net, n, 0) == max(nbytes, G.infer_layout(layers, n)), (layers, n)
            else:
                assert lib.pinn_gnet_backward2_workspace_bytes(net, n) == nbytes, (layers, n)
    # the ragged last slices the row counts were chosen for
    assert [n - (G.SLICES[n][1] - 1) * G.SLICES[n][2] for n in (257, 289, 321)] == [97, 129, 65]


@pytest.mark.parametrize("layers", G.EDGE_SHAPES, ids=IDS)
def test_float32_restatement_inside_half_the_band(layers):
    """What settles the floors: numpy float32 with K in slabs of 32 and the rows per slice, then across slices, is a correct float32
    implementation in the kernels' kind of order, so it must lie inside HALF the band (ratio <= 0.5) on every case, output and upstream.
    Likewise the loss sums, and for the double backward torch's float32 double autograd with every product in K slabs of 8, 16, 32, 64
    and 128 (a contraction within one slab by rounded products and torch's reduction).  Printed:
    the worst ratio per entry point, and per class of output the floors (largest, rms; in u) that would put it at exactly half."""
    worst = collections.defaultdict(float)
    need = collections.defaultdict(lambda: (0.0, 0.0))
    out = []                                    # what lies outside half the band

    def note(entry, cls, ratio, nd, what):
        worst[entry] = max(worst[entry], ratio)
        need[cls] = tuple(max(p, q) for p, q in zip(need[cls], nd))
        if ratio > 0.5:
            out.append(what + (round(ratio, 3),))

    for c in G.cases(layers):
        for kind in ("train", "vjp", "vjp_u"):
            r = c.restated(kind)
            for name in c.outputs(kind):
                note(kind, G.klass(name, c.n), c.ratio(r, kind, name), G.need(c.eps_of(r, kind, name), c.eps_torch(kind, name)),
                     (c.n, c.mode, kind, name))
        s = c.sums_ratio(c.restated("train")["sums"])
        worst["sums"] = max(worst["sums"], s)
        need["sums"] = (max(need["sums"][0], c.sums_ratio(c.restated("train")["sums"], G.sum_need)),) * 2
        if s > 0.5:
            out.append((c.n, c.mode, "loss sums", round(s, 3)))
        if c.n in G.rows2_of(layers):
            for with_glv in (True, False):
                t = c.torch2(with_glv)
                for order in G.ORDERS2:
                    r = c.torch2(with_glv, order)
                    # a restatement that is torch's own run bit for bit measures nothing: slabs of 32 on widths up to 32 once were, and
                    # put the floors of [8, 31, 1] at 0.  (Sums of at most 8 addends, all of [8, 4, 1], can still coincide.)
                    same = all(np.array_equal(c.pick(r, o), c.pick(t, o)) for o in c.names + ["gx", "ggu", "gglv"])
                    assert not same or max(layers[1:-1]) <= 8 or c.n == 1, (c.n, c.mode, order)
                    for name in c.names + ["gx", "ggu", "gglv"]:
                        note("backward2", G.klass(name, c.n, True), c.ratio2(r, name, with_glv),
                             G.need(c.eps2_of(r, name, with_glv), c.eps2_of(t, name, with_glv)),
                             (c.n, c.mode, "backward2", with_glv, order, name))
    print("%s: worst ratio to the band %s; floors at half the band, in u: %s"
          % (layers, {k: round(v, 3) for k, v in worst.items()}, {k: tuple(round(q, 1) for q in v) for k, v in need.items()}))
    assert not out, (layers, out)


def test_floors_follow_the_recorded_needs():
    """FLOORS is NEED by the stated rule: 4 u where the restatement needed no more, else twice the need rounded up to two digits."""
    def rule(v):
        if v <= 4:
            return 4
        digits = 10 ** max(0, int(np.floor(np.log10(2 * v))) - 1)
        return int(np.ceil(2 * v / digits - 1e-9) * digits)
    assert set(G.FLOORS) == set(G.NEED)
    for cls in G.NEED:
        assert G.FLOORS[cls] == tuple(rule(v) for v in G.NEED[cls]), (cls, G.FLOORS[cls], [rule(v) for v in G.NEED[cls]])


@pytest.mark.parametrize("layers", G.EDGE_SHAPES, ids=IDS)
def test_band_has_teeth(layers):
    """Every mutant of the referee leaves the band (ratio > 1) in at least one output it touches, on every case that admits it.
    Printed per mutant: the smallest such ratio over the cases, and on how many cases the suite's earlier rule (every output within
    2e-4 of its tensor's largest element) would have let the mutant through."""
    low = collections.defaultdict(lambda: np.inf)
    old = collections.defaultdict(lambda: [0, 0])
    for c in G.cases(layers):
        R, _ = c.ref("vjp")
        for kind, name, res, touched in G.mutants(c):
            same = [o for o in c.outputs("vjp") if np.shape(c.pick(res, o)) == np.shape(c.pick(R, o))]
            old[kind][1] += 1
            old[kind][0] += all(G.old_rule(c.pick(res, o), c.pick(R, o)) <= 1.0 for o in same)
            moved = [o for o in touched if not np.array_equal(c.pick(res, o), c.pick(R, o))]
            if not moved:       # nothing to see: every touched output is exactly zero in the referee (one row, its units all dropped)
                assert not any(np.any(c.pick(R, o)) for o in touched if o in c.names), (layers, c.n, c.mode, name)
                continue
            ratio = max(c.ratio(res, "vjp", o) for o in moved)
            low[kind] = min(low[kind], ratio)
            assert ratio > 1.0, (layers, c.n, c.mode, name, moved, ratio)
    for kind in low:
        print("%s %-10s smallest ratio to the band %.3g; passes the 2e-4-of-max rule on %d of %d cases"
              % (layers, kind, low[kind], old[kind][0], old[kind][1]))


TANH_REL = (1.3777387721347623e-05, -0.00010976991325151175, 0.0004508132115006447, -0.0013538711937144399, 0.003541822312399745,
            -0.008846853859722614, 0.021866105496883392, -0.05396784096956253, 0.13333331048488617, -0.3333333432674408)


def test_absolute_error_tanh_leaves_half_the_band():
    """The finding of the first device run, kept on the CPU.  With tanh_f32's formula 1 - 2 / (e^{2x} + 1) for every argument (absolute
    error 1.5e-7), which the general kernels' layer epilogue used until then, the same float32 restatement that sits inside half the band
    with a float32 tanh leaves it on the narrow and the deep list: u of a row is a dot product over activations far below 1, and an
    absolute error in them is a large one beside their absolute sum: 1.24 and 0.96 of the band (the device: 1.003 and 1.10).  With the
    epilogue's tanh_rel (odd polynomial below 1, the formula from there on) restated here it is back inside half.  The formula itself:
    relative error about 8000 u at |x| = 1e-4; tanh_rel within 2 u below 1 and within 2 u of float32 above.  The polynomial's coefficients
    are read out of csrc/pinn_general.hip, so this restates what the kernel evaluates."""
    import os
    import re
    import pinn_amd
    src = open(os.path.join(os.path.dirname(pinn_amd.__file__), "csrc", "pinn_general.hip")).read()
    body = src[src.index("float tanh_rel(float x)"):src.index("template <int MODE, int NS>")]
    coef = [float(v) for v in re.findall(r"(-?[0-9.]+e?-?[0-9]*)f[;)]", body.split("return")[0])]
    assert tuple(coef) == TANH_REL and "fabsf(x) < 1.0f" in body, coef

    def tanh_rel(v):
        v = np.asarray(v, dtype=np.float32)
        v2, p = v * v, np.float32(TANH_REL[0])
        for cf in TANH_REL[1:]:
            p = p * v2 + np.float32(cf)
        return np.where(np.abs(v) < 1.0, v + v * (v2 * p), G.kernel_tanh(v)).astype(np.float32)

    x = np.linspace(1e-4, 4.0, 400001, dtype=np.float32)
    ref = np.tanh(x.astype(np.float64))
    rel = lambda t, m: float((np.abs(t - ref) / ref)[m].max() / G.U)
    lo, hi = x < 1.0, x >= 1.0
    print("relative error in u on [1e-4, 1): tanh_f32's formula %.0f, tanh_rel %.2f; on [1, 4]: %.2f"
          % (rel(G.kernel_tanh(x), lo), rel(tanh_rel(x), lo), rel(tanh_rel(x), hi)))
    assert rel(G.kernel_tanh(x), lo) > 1000 and rel(tanh_rel(x), lo) <= 2.0 and rel(tanh_rel(x), hi) <= 2.0
    for layers in ([8, 65, 5, 1], [8, 16, 8, 40, 24, 72, 12, 36, 20, 1]):
        worst = {"formula": 0.0, "tanh_rel": 0.0}
        for c in G.cases(layers):
            for key, fn in (("formula", G.kernel_tanh), ("tanh_rel", tanh_rel)):
                r = c.restated("vjp_u", fn)
                worst[key] = max(worst[key], c.ratio(r, "vjp_u", "u"))
        print("%s: u of the float32 restatement, worst ratio to the band: %s" % (layers, worst))
        assert worst["formula"] > 0.9 and worst["tanh_rel"] <= 0.5, (layers, worst)
