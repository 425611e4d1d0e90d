"""CPU proof of what test_gpu_bf16.py holds the fused bf16/fp32-mixed kernels to: O.bf16_train_step (the kernels' rounding policy with a
manual backward) is a correct backward, its forward is the existing same-policy statement, and the band of bf16_policy.py -- defined
from the float64 reference and float32 restatements alone -- is narrow enough that a dropped row or a wrong dropout scale falls outside
it.  The second half repeats every proof for the wide nets' statement, O.bf16_wide_train_step, on the wide table (with a skipped 16-row
and 128-row tile, two exchanged gradient blocks and the route each case reaches).  Run with -s to see, per case: E_t, R_t, the float32
orders' largest error in flip units and every mutant's ratio to the band."""
import numpy as np
import pytest
import torch

import bf16_policy as B
import pinn_oracle as O


def _draw(H, nh, n, seed):
    from pinn_amd import synth
    P = O.init_params([8] + [H] * nh + [1], seed=seed)
    ds = synth.make_dataset(max(n, 2), (), seed=seed + 1)
    pl = B.p_list(nh)
    masks = O.philox_masks_for_net(B.SEED, B.STREAM, B.ROW0, n, H, nh, pl)
    return P, ds[0][:n].contiguous(), ds[1][:n].contiguous(), pl, masks


@pytest.mark.parametrize("H,nh,n", [(128, 2, 1), (256, 1, 17), (128, 3, 333), (256, 2, 129)])
@pytest.mark.parametrize("with_masks", [False, True])
def test_manual_backward_is_autograd(H, nh, n, with_masks):
    """Rounding off, float64: loss and all 2 nh + 8 gradients equal autograd on the oracle's forward to 1e-12 of each tensor's largest
    element, with and without masks, one p per module."""
    P, x, y, pl, masks = _draw(H, nh, n, 7)
    pl, masks = (pl, masks) if with_masks else (None, None)
    sums, grads, _ = O.bf16_train_step(P, x, y, pl, masks, torch.float64, rounding=False)
    lo, mse, want, _, _ = O.nll_loss_and_grads([p.double() for p in P], x.double(), y.double(), pl, masks)
    assert abs((sums[0] + 0.01 * sums[1]) / n - float(lo)) <= 1e-12 * abs(float(lo))
    assert abs(sums[2] / n - float(mse)) <= 1e-12 * abs(float(mse))
    worst = 0.0
    for name, g, w in zip(O.param_names(nh), grads, want):
        err = float((g.reshape(w.shape) - w).abs().max()) / float(w.abs().max())
        worst = max(worst, err)
        assert err <= 1e-12, (name, err)
    print("manual backward vs float64 autograd, H %d nh %d rows %d masks %s: worst %.1e of the tensor's max" % (H, nh, n, with_masks, worst))


@pytest.mark.parametrize("H,nh,n", [(128, 2, 1), (256, 1, 65), (128, 3, 333), (256, 3, 200)])
@pytest.mark.parametrize("with_masks", [False, True])
def test_forward_is_the_existing_statement(H, nh, n, with_masks):
    """Rounding on, float32, unchunked: (u, logvar) bit-equal to mlp_forward(bf16=True), and the three loss sums are those of its
    outputs (aleatoric_loss)."""
    P, x, y, pl, masks = _draw(H, nh, n, 9)
    pl, masks = (pl, masks) if with_masks else (None, None)
    sums, _, det = O.bf16_train_step(P, x, y, pl, masks, torch.float32)
    with torch.no_grad():
        u, lv = O.mlp_forward(P, x, pl, masks, bf16=True)
        lo = O.aleatoric_loss(y, u, lv).item()
    assert torch.equal(det["u"], u) and torch.equal(det["logvar"], lv)
    assert abs((sums[0] + 0.01 * sums[1]) / n - lo) <= 1e-5 * abs(lo)


def test_chunked_product_is_the_product():
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(37, 333, generator=g, dtype=torch.float64) - 0.5, torch.rand(333, 19, generator=g, dtype=torch.float64) - 0.5
    for c in B.ORDERS:
        assert float((O._mm_chunked(a, b, c) - a @ b).abs().max()) <= 1e-13
    # and in float32 the orders do differ: E_t measures something
    a, b = a.float(), b.float()
    assert any(not torch.equal(O._mm_chunked(a, b, c), a @ b) for c in B.ORDERS[:-1])


@pytest.mark.parametrize("name", B.CASE_IDS)
def test_band_has_teeth(name):
    """For every case the GPU test runs: a float64 reference with the last row (grid-cap case: the last full 64-row tile) left out of
    every row sum lies outside band_t for more than half of the gradient tensors, by >= 5x in the median tensor; with the variance
    head's dropout scale taken from layer 0 it lies outside for Wv0, bv0 and Wv1.  A cap on what the GPU test can hide, from the
    reference alone."""
    c = B.case(name)
    b = c.band
    print("\n%s: H %d, nh %d, %d rows, mode %d, seed %d; float32 orders' largest error: %.2f flip units" %
          (name, c.H, c.nh, c.n, c.mode, c.seed, b.order_flips))
    for n, em, er, r, bm in zip(b.names, b.e_max, b.e_rms, b.r, b.band_max):
        print("  %-28s E_max %.3e  E_rms %.3e  R %.3e  band_max %.3e (%.1e of the tensor's max)" %
              (n, em, er, r, bm, bm / (float(np.abs(b.ref[b.names.index(n)]).max()) + 1e-300)))
    # FLIPS is twice the orders' own largest count where flips are what separates them; in the grid-cap case (32 833 rows) E_t is the
    # ordinary float32 error of a 32 833-term sum (4.4 such units), which the first term of the band carries
    assert c.n > 2049 or b.order_flips <= B.FLIPS / 2, "the float32 orders differ by more flips than the allowance was derived from"
    # the reference is inside its own band, and so is every float32 order (by construction: E_t <= band / 3)
    assert all(m == 0.0 for _, m, _ in b.ratios(b.sums, b.grads))
    lo, hi = c.mutant_rows()
    rat = b.ratios(b.sums, b.without_rows(lo, hi))[3:]
    print("  rows [%d, %d) left out: max error / band per tensor: %s" % (lo, hi, " ".join("%.1f" % m for _, m, _ in rat)))
    outside = sum(1 for _, m, _ in rat if m > 1.0)
    med = float(np.median([m for _, m, _ in rat]))
    print("  outside the band: %d of %d tensors, median ratio %.1f" % (outside, len(rat), med))
    assert outside > len(rat) / 2 and med >= 5.0, (name, outside, med)
    mut = c.head_scale_mutant()
    if mut is not None:
        rat = dict((n, m) for n, m, _ in b.ratios(b.sums, mut))
        heads = ["var_layers.0.weight", "var_layers.0.bias", "var_layers.3.weight"]
        print("  head scaled by layer 0's dropout scale: " + " ".join("%s %.1f" % (n, rat[n]) for n in heads))
        assert all(rat[n] > 1.0 for n in heads), (name, [rat[n] for n in heads])


def test_band_of_the_injected_mask_cases_has_teeth():
    """The two injected-mask cases of the GPU test (recorded masks of g_net128.npz; 65 drawn rows): last row left out."""
    for label, b in (("g_net128", B.golden_band()), ("drawn65", B.drawn_mask_case()[5])):
        n = b.terms[0][0].shape[0]
        rat = b.ratios(b.sums, b.without_rows(n - 1, n))[3:]
        outside, med = sum(1 for _, m, _ in rat if m > 1.0), float(np.median([m for _, m, _ in rat]))
        print("%s: %d rows, float32 orders %.2f flip units; last row left out: %d of %d tensors outside, median ratio %.1f" %
              (label, n, b.order_flips, outside, len(rat), med))
        assert b.order_flips <= B.FLIPS / 2
        assert outside > len(rat) / 2 and med >= 5.0


# =======================================================================================
# The wide nets' policy (O.bf16_wide_train_step: fp32 stash, operands rounded where a product reads them) and the wide table
# =======================================================================================
WIDE_SHAPES = [(512, 2, 1), (512, 2, 129), (1024, 2, 145)]


@pytest.mark.parametrize("H,nh,n", WIDE_SHAPES)
@pytest.mark.parametrize("with_masks", [False, True])
def test_wide_manual_backward_is_autograd(H, nh, n, with_masks):
    """The wide statement with rounding off, float64: loss and all 2 nh + 8 gradients equal autograd on the oracle's forward to 1e-12 of
    each tensor's largest element -- the "kept" test read off the stash (h != 0) included."""
    P, x, y, pl, masks = _draw(H, nh, n, 7)
    pl, masks = (pl, masks) if with_masks else (None, None)
    sums, grads, _ = O.bf16_wide_train_step(P, x, y, pl, masks, torch.float64, rounding=False)
    lo, mse, want, _, _ = O.nll_loss_and_grads([p.double() for p in P], x.double(), y.double(), pl, masks)
    assert abs((sums[0] + 0.01 * sums[1]) / n - float(lo)) <= 1e-12 * abs(float(lo))
    assert abs(sums[2] / n - float(mse)) <= 1e-12 * abs(float(mse))
    worst = 0.0
    for name, g, w in zip(O.param_names(nh), grads, want):
        err = float((g.reshape(w.shape) - w).abs().max()) / float(w.abs().max())
        worst = max(worst, err)
        assert err <= 1e-12, (name, err)
    print("wide manual backward vs float64 autograd, H %d nh %d rows %d masks %s: worst %.1e of the tensor's max" % (H, nh, n, with_masks, worst))


@pytest.mark.parametrize("H,nh,n", WIDE_SHAPES)
@pytest.mark.parametrize("with_masks", [False, True])
def test_wide_forward_is_the_existing_statement(H, nh, n, with_masks):
    """The wide kernels round the forward where the fused ones do (every H x H, H -> H/2, H/2 -> H/4 product on bf(activation) . bf(W),
    layer 0 and both heads' dot products on fp32 values): rounding on, float32, unchunked, (u, logvar) of the wide statement are
    bit-equal to mlp_forward(bf16=True) -- no difference to state -- and the three loss sums are those of its outputs."""
    P, x, y, pl, masks = _draw(H, nh, n, 9)
    pl, masks = (pl, masks) if with_masks else (None, None)
    sums, _, det = O.bf16_wide_train_step(P, x, y, pl, masks, torch.float32)
    with torch.no_grad():
        u, lv = O.mlp_forward(P, x, pl, masks, bf16=True)
        lo = O.aleatoric_loss(y, u, lv).item()
    assert torch.equal(det["u"], u) and torch.equal(det["logvar"], lv)
    assert abs((sums[0] + 0.01 * sums[1]) / n - lo) <= 1e-5 * abs(lo)


def test_the_two_policies_differ_where_they_say():
    """Same rows, float64: the loss sums agree exactly (same forward); every gradient differs but the two scalar head biases
    (sums of du, dz) and dWv1 = bf(g2)^T bf(v1), whose operands are rounded once in either policy -- the fused policy rounds the stash
    and the stored d pre-activations, the wide one does not."""
    P, x, y, pl, masks = _draw(512, 2, 129, 11)
    sf, gf, _ = O.bf16_train_step(P, x, y, pl, masks)
    sw, gw, _ = O.bf16_wide_train_step(P, x, y, pl, masks)
    assert np.array_equal(sf, sw)
    same = [n for n, a, b in zip(O.param_names(2), gf, gw) if torch.equal(a, b)]
    assert same == ["predict.bias", "var_layers.3.weight", "var_layers.5.bias"]


@pytest.mark.parametrize("name", B.WIDE_IDS)
def test_wide_route_claims(name):
    """Every wide case lands on the weight-gradient route, slice count, tiles-per-slice pattern and grid that bf16_policy.py names for it
    (plan_workspace restated by wgrad_routes.plan from the constants of the source), and on the layer kernels' tile geometry."""
    import wgrad_routes as W
    c = B.case(name)
    got = W.plan(B.BF16, c.H, c.nh, c.n)
    want = B.WIDE_CLAIMS[name]
    assert {k: got[k] for k in want} == want, (name, got)
    assert got["walk"] == "contiguous"
    tiles = (c.n + B.WIDE_TILE - 1) // B.WIDE_TILE
    if name == "w_serial_cap":
        assert got["route"] == "serial" and got["t16"] >= W.constants()["fan_t16"] and tiles > B.HOST_CUS
        assert 0 in got["tiles"] and len(got["tiles"]) == 3           # full slices, a short one, empty ones behind it
        for cus in (256, 304):                                        # whatever the device: serial, 128 slices, a second tile per workgroup
            p = W.plan(B.BF16, c.H, c.nh, B.wide_cap_rows(cus))
            assert (p["route"], p["slices"], p["grid"]) == ("serial", 128, (128, 2, 2))
            assert (B.wide_cap_rows(cus) + B.WIDE_TILE - 1) // B.WIDE_TILE > cus + 1
    else:
        assert got["route"] == "fan" and tiles <= B.HOST_CUS
    if name in ("w_1024", "w_fan512"):
        assert 0 in got["tiles"] and len(got["tiles"]) == 3
    if name in ("w_wg-1", "w_wg", "w_wg+1"):
        assert c.H // 4 == 128 and (c.H // 4) % 256 != 0 and (c.H // 2) % 256 == 0      # last variance layer: kNT = 8; Wv1: 128 x 256
    if name == "w_nodrop":
        assert c.mode == 0 and (c.H // 4) % 256 == 0


def _wide_teeth(label, c_or_band, n, mutants, head_mutant, nh):
    b = c_or_band
    for n_, em, er, r, bm in zip(b.names, b.e_max, b.e_rms, b.r, b.band_max):
        print("  %-28s E_max %.3e  E_rms %.3e  R %.3e  band_max %.3e (%.1e of the tensor's max)" %
              (n_, em, er, r, bm, bm / (float(np.abs(b.ref[b.names.index(n_)]).max()) + 1e-300)))
    assert all(m == 0.0 for _, m, _ in b.ratios(b.sums, b.grads))
    for what, lo, hi in mutants:
        rat = b.ratios(b.sums, b.without_rows(lo, hi))[3:]
        outside = sum(1 for _, m, _ in rat if m > 1.0)
        med = float(np.median([m for _, m, _ in rat]))
        print("  %s, rows [%d, %d) left out: max error / band per tensor: %s" % (what, lo, hi, " ".join("%.1f" % m for _, m, _ in rat)))
        print("  %s: outside the band: %d of %d tensors, median ratio %.1f" % (what, outside, len(rat), med))
        assert outside > len(rat) / 2 and med >= 5.0, (label, what, outside, med)
    if nh >= 2:
        tensor, sw = b.blocks_swapped()
        m = dict((n_, m_) for n_, m_, _ in b.ratios(b.sums, sw))[tensor]
        print("  blocks (0,1) and (1,0) of %s exchanged: %.1f" % (tensor, m))
        assert m > 1.0, (label, "block swap", m)
    if head_mutant is not None:
        rat = dict((n_, m) for n_, m, _ in b.ratios(b.sums, head_mutant))
        heads = ["var_layers.0.weight", "var_layers.0.bias", "var_layers.3.weight"]
        print("  head scaled by layer 0's dropout scale: " + " ".join("%s %.1f" % (n_, rat[n_]) for n_ in heads))
        assert all(rat[n_] > 1.0 for n_ in heads), (label, [rat[n_] for n_ in heads])


@pytest.mark.parametrize("name", B.WIDE_IDS)
def test_wide_band_has_teeth(name):
    """For every wide case the GPU test runs, from the float64 reference of the WIDE policy alone: with the last row, the last full
    16-row tile, (from 256 rows) the last full 128-row tile or (w_serial_cap) the first second-pass workgroup tile left out of every row
    sum, the result lies outside band_t for more than half of the gradient tensors, by >= 5x in the median tensor; with the hidden
    layer's gradient blocks (0, 1) and (1, 0) exchanged that tensor lies outside; with the variance head's dropout scale taken from
    layer 0, Wv0, bv0 and Wv1 lie outside."""
    c = B.case(name)
    b = c.band
    print("\n%s: H %d, nh %d, %d rows, mode %d, seed %d; float32 orders' largest error: %.2f flip units" %
          (name, c.H, c.nh, c.n, c.mode, c.seed, b.order_flips))
    assert c.n > 2049 or b.order_flips <= B.FLIPS / 2, "the float32 orders differ by more flips than the allowance was derived from"
    _wide_teeth(name, b, c.n, c.row_mutants(), c.head_scale_mutant(), c.nh)


def test_wide_band_of_the_injected_mask_and_shard_cases_has_teeth():
    """The wide injected-mask case (129 drawn rows) and the shard case (333 rows) of the GPU test: last row and last full 16-row tile."""
    P, x, y, pl, masks, b = B.wide_drawn_mask_case()
    print("\nwide drawn129: float32 orders %.2f flip units" % b.order_flips)
    assert b.order_flips <= B.FLIPS / 2
    _wide_teeth("wide drawn129", b, 129, [("last row", 128, 129), ("last full 16-row tile", 112, 128)], None, 2)
    c = B.wide_shard_case()
    print("\nw_shard: float32 orders %.2f flip units" % c.band.order_flips)
    assert c.band.order_flips <= B.FLIPS / 2
    _wide_teeth("w_shard", c.band, c.n, c.row_mutants(), c.head_scale_mutant(), c.nh)


@pytest.mark.parametrize("name", ["w_wg+1", "w_fan512"])
def test_print_fused_policy_against_the_wide_band(name):
    """No gate: how far the FUSED policy's float64 result lies from the wide reference, in wide bands -- whether the band can tell the two
    statements apart."""
    c = B.case(name)
    s, g, _ = O.bf16_train_step(c.P, c.x, c.y, c.pl, c.masks)
    rat = c.band.ratios(s, [t.numpy() for t in g])
    print("\n%s: fused policy / wide band (max, rms)  " % name + "  ".join("%s %.2f %.2f" % r for r in rat))
    print("%s: fused policy against the wide band: worst %.2f, %d of %d tensors outside" %
          (name, max(max(m, r) for _, m, r in rat), sum(1 for _, m, r in rat if max(m, r) > 1.0), len(rat)))
