"""GPU parity of the opt-in bf16/fp32-mixed kernels (pinn_net_t.precision = PINN_PREC_BF16).

Two checks per kernel: (1) against the oracle run with the SAME rounding policy (bf16 MFMA inputs,
fp32 everything else) -- tight, only accumulation order differs; (2) against the fp32 oracle (= the
reference's arithmetic) at the mixed-precision tolerance rtol 2e-2 of SURVEY.md 8(c).  For the training
step (1) is the second half of this file: every loss sum and gradient tensor against a float64 run of
the kernels' own rounding policy -- O.bf16_train_step for the fused nets (H = 128, 256), O.bf16_wide_train_step
for the wide ones (H = 512, 1024, 2048: layer-by-layer kernels in scheme B1, weight gradients with one bf16
part per operand) --, inside a band derived on the CPU (tests/bf16_policy.py, test_bf16_policy_host.py)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16_policy as B
import pinn_oracle as O


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("H,nh,N,mode", [(256, 3, 1000, 0), (256, 3, 777, 1), (128, 3, 333, 1), (128, 1, 64, 1), (256, 5, 130, 1),
                                         (512, 2, 300, 1), (1024, 4, 200, 1)])          # the last two: wide nets (pinn_wide.hip, scheme B1)
def test_forward_bf16(lib, H, nh, N, mode):
    import hip_helpers as hh
    from pinn_amd import synth
    P = O.init_params([8] + [H] * nh + [1], seed=H + nh)
    x = synth.make_dataset(max(N, 2), (), seed=N)[0][:N].contiguous()
    fp, xd = hh.flat_params(P, H, nh).to(hh.dev()), x.to(hh.dev())
    pl = [0.2] * (nh + 1)
    seed, stream, row0 = 424242, 9, 1000
    drop = hh.dropout_struct(mode, pl, seed=seed, stream_id=stream, row_offset=row0)
    u, lv = hh.forward(lib, H, nh, fp, xd, drop, precision=1)
    masks = O.philox_masks_for_net(seed, stream, row0, N, H, nh, pl) if mode else None
    with torch.no_grad():
        ub, lvb = O.mlp_forward(P, x, pl, masks, bf16=True)
        uf, lvf = O.mlp_forward(P, x, pl, masks)
    # same rounding policy: tight (a bf16 rounding of an activation can flip on a 1-ulp fp32 difference, hence 2e-3)
    np.testing.assert_allclose(u.cpu().numpy(), ub.numpy().reshape(-1), rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(lv.cpu().numpy(), lvb.numpy().reshape(-1), rtol=2e-3, atol=2e-3)
    # against the fp32 reference arithmetic: mixed-precision tolerance
    scale = float(uf.abs().max())
    assert float((u.cpu() - uf.reshape(-1)).abs().max()) <= 2e-2 * max(scale, 1.0)
    assert float((lv.cpu() - lvf.reshape(-1)).abs().max()) <= 5e-2


def test_mc_dropout_bf16(lib):
    import hip_helpers as hh
    from pinn_amd import _lib, synth
    H, nh, N, T, p = 256, 3, 300, 16, 0.4
    P = O.init_params([8, H, H, H, 1], seed=1)
    x = synth.make_dataset(N, (), seed=2)[0]
    out = torch.empty(3, N, device=hh.dev())
    net = hh.make_net(lib, H, nh, 1)
    d = hh.dropout_struct(1, [p] * 4, seed=99, stream_id=1000, row_offset=0)
    fp, xd = hh.flat_params(P, H, nh).to(hh.dev()), x.to(hh.dev())
    _lib.check(lib.pinn_mc_dropout(ctypes.byref(net), hh.ptr(fp), hh.ptr(xd), N, ctypes.byref(d), T, hh.ptr(out[0]), hh.ptr(out[1]),
                                   hh.ptr(out[2]), hh.stream()), "mc")
    o = out.cpu().numpy()
    mf = lambda t: O.philox_masks_for_net(99, 1000 + t, 0, N, H, nh, [p] * 4)
    # oracle with the same rounding policy
    with torch.no_grad():
        ue, _ = O.mlp_forward(P, x, bf16=True)
        us, lvs = zip(*[O.mlp_forward(P, x, [p] * 4, mf(t), bf16=True) for t in range(T)])
    us = np.array([u.numpy() for u in us]); lvs = np.array([l.numpy() for l in lvs])
    np.testing.assert_allclose(o[0], ue.numpy().reshape(-1), rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(o[1], np.sqrt(np.exp(lvs.mean(0))).reshape(-1), rtol=5e-3)
    np.testing.assert_allclose(o[2], np.sqrt(us.var(0)).reshape(-1), rtol=2e-2, atol=2e-3)
    # and the fp32 reference statistics within the mixed-precision band
    pm, au, eu = O.mc_dropout(P, x, p, T, mf)
    assert abs(np.mean(o[2]) / np.mean(eu) - 1) < 2e-2 and abs(np.mean(o[1]) / np.mean(au) - 1) < 2e-2


@pytest.mark.parametrize("H,nh,N,mode", [(256, 3, 1000, 1), (128, 3, 333, 1), (256, 2, 129, 0), (128, 1, 64, 1), (512, 2, 300, 1), (1024, 4, 200, 1)])
def test_train_grads_bf16(lib, H, nh, N, mode):
    """bf16-mixed training step: loss against the same-policy oracle (tight), gradients against the fp32
    reference arithmetic at the mixed-precision tolerance (5e-2 of each tensor's max: d pre-activations are rounded to bf16 before the K = rows contraction)."""
    import hip_helpers as hh
    from pinn_amd import synth
    P = O.init_params([8] + [H] * nh + [1], seed=H + nh)
    ds = synth.make_dataset(N, (), seed=5)
    x, y = ds[0], ds[1].reshape(-1)
    pl = [0.2] * (nh + 1)
    seed, stream, row0 = 987654321987, 42, 12345
    drop = hh.dropout_struct(mode, pl, seed=seed, stream_id=stream, row_offset=row0)
    fp, xd, yd = hh.flat_params(P, H, nh).to(hh.dev()), x.to(hh.dev()).contiguous(), y.to(hh.dev()).contiguous()
    grads, loss = hh.train_grads(lib, H, nh, fp, xd, yd, drop, precision=1)
    masks = O.philox_masks_for_net(seed, stream, row0, N, H, nh, pl) if mode == 1 else None
    l = loss.cpu().numpy()
    with torch.no_grad():
        ub, lvb = O.mlp_forward(P, x, pl, masks, bf16=True)
        lb = O.aleatoric_loss(ds[1], ub, lvb).item()
    assert abs((l[0] + 0.01 * l[1]) / N - lb) <= 2e-3 * abs(lb) + 2e-4
    lo, mse, go, _, _ = O.nll_loss_and_grads(P, x, ds[1], pl, masks)
    assert abs((l[0] + 0.01 * l[1]) / N - lo.item()) <= 2e-2 * abs(lo.item()) + 2e-3
    got = hh.unflat(grads.cpu(), H, nh)
    for n, g, w in zip(O.param_names(nh), got, go):
        scale = float(w.abs().max()) + 1e-30
        err = float((g - w).abs().max())
        assert err <= 5e-2 * scale, (n, err, scale)
        # and the direction agrees closely
        cos = float((g * w).sum() / (g.norm() * w.norm() + 1e-30))
        assert cos > 0.998, (n, cos)


def test_model_surface_bf16_end_to_end():
    """precision="bf16" through the reference-shaped Python surface: trains, MC-samples, assembles results,
    and stays close to the fp32 path on the same seeds."""
    import pinn_amd
    from pinn_amd import synth
    ds = synth.make_dataset(3000, (300,), seed=0)
    outs = {}
    for prec in ("fp32", "bf16"):
        torch.manual_seed(0)
        m = pinn_amd.PhysicsInformedNN(ds[0], ds[1], [8, 256, 256, 256, 1], ds[4], ds[5], p=0.2, logvar=True, seed=3, precision=prec)
        m.verbose = False
        m.train_dnn(1); l0 = m.last_loss
        m.train_dnn(40); l1 = m.last_loss
        assert l1 < l0
        m.train_lambda(10, False); m.train_thermal(10)
        arr = pinn_amd.create_comprehensive_results_array_v2(m, ds, mc_times=16, dropout=0.4)
        assert arr.shape == (3300, 22) and np.all(np.isfinite(arr))
        outs[prec] = (l1, arr)
    # same seeds, same masks: the two precisions follow the same trajectory closely
    assert abs(outs["bf16"][0] - outs["fp32"][0]) < 0.05 * abs(outs["fp32"][0]) + 0.02
    yp32, yp16 = outs["fp32"][1][:, 9], outs["bf16"][1][:, 9]
    assert np.abs(yp32 - yp16).max() < 0.05 * np.abs(yp32).max()
    with pytest.raises(ValueError):
        pinn_amd.PhysicsInformedNN(ds[0], ds[1], [8, 256, 256, 256, 1], ds[4], ds[5], p=0.2, logvar=True, precision="fp8")


# =======================================================================================
# The kernels against a float64 reference of their OWN rounding policy (O.bf16_train_step, O.bf16_wide_train_step), inside a band that
# test_bf16_policy_host.py derives from that reference and float32 restatements alone (tests/bf16_policy.py).  The gates
# above, against the reference's fp32 arithmetic, state the 2e-2 mixed-precision contract and have to swallow the whole
# bf16 rounding error; the ones below do not, so a dropped ragged row, a skipped weight-gradient tile or a wrong keep bit
# shows.
# =======================================================================================
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev_inputs(P, x, y, H, nh):
    import hip_helpers as hh
    return hh.flat_params(P, H, nh).to(hh.dev()), x.to(hh.dev()).contiguous(), y.reshape(-1).to(hh.dev()).contiguous()


def _assert_in_band(label, band, loss, grads, H, nh, ref=None):
    """Prints every tensor's error / band (max and rms gate), then asserts both <= 1."""
    import hip_helpers as hh
    rat = band.ratios(loss.cpu().numpy()[:3], [g.numpy() for g in hh.unflat(grads.cpu(), H, nh)], ref)
    print("\n%s: error / band (max, rms)  " % label + "  ".join("%s %.3f %.3f" % (n, m, r) for n, m, r in rat))
    print("%s: worst ratio %.3f" % (label, max(max(m, r) for _, m, r in rat)))
    bad = [(n, m, r) for n, m, r in rat if not (m <= 1.0 and r <= 1.0)]
    assert not bad, (label, bad)


def _mc(lib, H, nh, fp, x, drop, T):
    import hip_helpers as hh
    from pinn_amd import _lib
    out = torch.empty(3, x.shape[0], device=hh.dev())
    net = hh.make_net(lib, H, nh, 1)
    _lib.check(lib.pinn_mc_dropout(ctypes.byref(net), hh.ptr(fp), hh.ptr(x), x.shape[0], ctypes.byref(drop), T, hh.ptr(out[0]),
                                   hh.ptr(out[1]), hh.ptr(out[2]), hh.stream()), "mc")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", B.CASE_IDS)
def test_train_grads_bf16_in_policy_band(lib, name):
    """Loss sums l[0..2] and all 2 nh + 8 gradient tensors of a bf16-mixed training step against the float64 policy reference,
    inside band_t = 3 E_t + 4 * 2^-8 * R_t for the largest and for the rms error (bf16_policy.py; one p per module, row offset
    and stream non-zero, poisoned workspace).  The cases: one row; the wave tile (15 / 16 / 17) and workgroup tile (63 / 64 / 65)
    boundaries; no dropout; 2049 rows (20 empty weight-gradient slices); and 2 CUs 64 + 65 rows, where a workgroup runs a
    second tile with the weight-slab pipeline carried over and the weight gradients take the serial route with 256 slices."""
    import hip_helpers as hh
    c = B.case(name, _cus())
    fp, xd, yd = _dev_inputs(c.P, c.x, c.y, c.H, c.nh)
    drop = hh.dropout_struct(c.mode, c.pl, seed=B.SEED, stream_id=B.STREAM, row_offset=B.ROW0)
    grads, loss = hh.train_grads(lib, c.H, c.nh, fp, xd, yd, drop, precision=1)
    _assert_in_band("%s (H %d, nh %d, %d rows)" % (name, c.H, c.nh, c.n), c.band, loss, grads, c.H, c.nh)


@pytest.mark.parametrize("name", B.WIDE_IDS)
def test_train_grads_bf16_wide_in_policy_band(lib, name):
    """The wide nets' bf16-mixed training step (wide_layer_x6_kernel<x6::B1, ..>, wgrad_d_kernel<.., 1>, wgrad_x_kernel<.., 1>): loss
    sums and all 2 nh + 8 gradient tensors against the float64 reference of the WIDE policy (O.bf16_wide_train_step), inside the same
    band_t = 3 E_t + 4 * 2^-8 * R_t with E_t from the wide policy's float32 orders.  The cases (bf16_policy.WIDE_CASES): one row; the
    wave tile (15 / 16 / 17) and the 128-row workgroup tile (127 / 128 / 129); no dropout at H = 1024; three hidden layers; the
    fan-out route with short and empty slices at H = 1024 and H = 512; 8 x 8 gradient blocks at H = 2048; and the serial route with
    more workgroup tiles than CUs (a second tile per workgroup)."""
    import hip_helpers as hh
    c = B.case(name, _cus())
    fp, xd, yd = _dev_inputs(c.P, c.x, c.y, c.H, c.nh)
    drop = hh.dropout_struct(c.mode, c.pl, seed=B.SEED, stream_id=B.STREAM, row_offset=B.ROW0)
    grads, loss = hh.train_grads(lib, c.H, c.nh, fp, xd, yd, drop, precision=1)
    _assert_in_band("%s (H %d, nh %d, %d rows)" % (name, c.H, c.nh, c.n), c.band, loss, grads, c.H, c.nh)


def test_bf16_wide_injected_masks(lib):
    """PINN_DROP_BITS through the wide kernels' activate_pair_rt: 129 torch-drawn rows of [8, 512, 512, 1], one p per module.  One row
    behind a 128-row workgroup tile: the padding rows of the second tile read the last real row's mask words (the local-row clamp of
    wide_input_kernel and wide_layer_x6_kernel).  Forward at the forward test's gate, the training step inside the wide band."""
    import hip_helpers as hh
    P, x, y, pl, masks, band = B.wide_drawn_mask_case()
    H, nh = 512, 2
    bits = hh.pack_mask_bits([masks]).to(hh.dev())
    drop = hh.dropout_struct(2, pl, bits=bits)
    fp, xd, yd = _dev_inputs(P, x, y, H, nh)
    u, lv = hh.forward(lib, H, nh, fp, xd, drop, precision=1)
    with torch.no_grad():
        ub, lvb = O.mlp_forward(P, x, pl, masks, bf16=True)
    np.testing.assert_allclose(u.cpu().numpy(), ub.numpy().reshape(-1), rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(lv.cpu().numpy(), lvb.numpy().reshape(-1), rtol=2e-3, atol=2e-3)
    grads, loss = hh.train_grads(lib, H, nh, fp, xd, yd, drop, precision=1)
    _assert_in_band("wide injected masks, 129 drawn rows", band, loss, grads, H, nh)


@pytest.mark.parametrize("which", ["g_net128", "drawn65"])
def test_bf16_injected_masks(lib, which):
    """PINN_DROP_BITS through mlp_bf16_kernel<.., kBits = true> and train_chain_bf16_kernel<H, true>: the recorded torch masks of
    g_net128.npz, and 65 drawn rows with one p per module (one row past a workgroup tile: the padding rows read the last mask
    row).  Forward against mlp_forward(bf16=True) at the forward test's gate, the training step against the policy reference
    under those masks, inside the band."""
    import hip_helpers as hh
    if which == "g_net128":
        (P, x, y, pl, masks), band = B.golden_case(), B.golden_band()
    else:
        P, x, y, pl, masks, band = B.drawn_mask_case()
    nh = (len(P) - 8) // 2
    H = P[0].shape[0]
    bits = hh.pack_mask_bits([masks]).to(hh.dev())
    drop = hh.dropout_struct(2, pl, bits=bits)
    fp, xd, yd = _dev_inputs(P, x, y, H, nh)
    u, lv = hh.forward(lib, H, nh, fp, xd, drop, precision=1)
    with torch.no_grad():
        ub, lvb = O.mlp_forward(P, x, pl, masks, bf16=True)
    np.testing.assert_allclose(u.cpu().numpy(), ub.numpy().reshape(-1), rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(lv.cpu().numpy(), lvb.numpy().reshape(-1), rtol=2e-3, atol=2e-3)
    grads, loss = hh.train_grads(lib, H, nh, fp, xd, yd, drop, precision=1)
    _assert_in_band("injected masks, " + which, band, loss, grads, H, nh)


def test_forward_and_mc_bf16_above_the_grid_cap(lib):
    """2 CUs 64 + 65 rows of [8, 128, 1]: launch_forward_bf16 caps its grid at 2 CUs workgroups, so one workgroup runs a second
    (and the ragged last) tile with the slab pipeline carried over.  Forward u / logvar and MC-dropout with T = 4 against the
    same-policy oracle at the gates of test_forward_bf16 / test_mc_dropout_bf16."""
    import hip_helpers as hh
    import regimes as R
    c = B.case("grid_cap", _cus())
    T = 4
    fp, xd, _ = _dev_inputs(c.P, c.x, c.y, c.H, c.nh)
    drop = hh.dropout_struct(1, c.pl, seed=B.SEED, stream_id=B.STREAM, row_offset=B.ROW0)
    u, lv = hh.forward(lib, c.H, c.nh, fp, xd, drop, precision=1)
    o = _mc(lib, c.H, c.nh, fp, xd, drop, T).cpu().numpy()
    passes = R.philox_masks_passes(c.layers, c.n, c.pl, [B.STREAM + t for t in range(T)], seed=B.SEED, row0=B.ROW0)
    with torch.no_grad():
        ue, _ = O.mlp_forward(c.P, c.x, bf16=True)
        us, lvs = zip(*[O.mlp_forward(c.P, c.x, c.pl, m, bf16=True) for m in passes])
    us = np.array([t.numpy().reshape(-1) for t in us]); lvs = np.array([t.numpy().reshape(-1) for t in lvs])
    np.testing.assert_allclose(u.cpu().numpy(), us[0], rtol=2e-3, atol=2e-3)          # pass 0 = the training stream's masks
    np.testing.assert_allclose(lv.cpu().numpy(), lvs[0], rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(o[0], ue.numpy().reshape(-1), rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(o[1], np.sqrt(np.exp(lvs.mean(0))), rtol=5e-3)
    np.testing.assert_allclose(o[2], np.sqrt(us.var(0)), rtol=2e-2, atol=2e-3)


def test_bf16_repeatable_and_shard_additive(lib):
    """Two identical bf16 training calls are bitwise equal; two row shards with n_global = N and their row offsets sum to the full
    call's gradient and loss sums within band_t (sharding only reorders the slab sums: no wider band is due).  A fused net
    ([8, 128 x 3, 1], 333 rows cut at 130) and a wide one ([8, 512, 512, 1], 333 rows cut at 129: one row behind a workgroup tile)."""
    import hip_helpers as hh
    for c, cut in ((B.case("mid128"), 130), (B.wide_shard_case(), 129)):
        fp, xd, yd = _dev_inputs(c.P, c.x, c.y, c.H, c.nh)
        mk = lambda off: hh.dropout_struct(1, c.pl, seed=B.SEED, stream_id=B.STREAM, row_offset=B.ROW0 + off)
        g1, l1 = hh.train_grads(lib, c.H, c.nh, fp, xd, yd, mk(0), precision=1)
        g2, l2 = hh.train_grads(lib, c.H, c.nh, fp, xd, yd, mk(0), precision=1)
        assert torch.equal(g1, g2) and torch.equal(l1, l2), c.name
        ga, la = hh.train_grads(lib, c.H, c.nh, fp, xd[:cut].contiguous(), yd[:cut].contiguous(), mk(0), n_global=c.n, precision=1)
        gb, lb = hh.train_grads(lib, c.H, c.nh, fp, xd[cut:].contiguous(), yd[cut:].contiguous(), mk(cut), n_global=c.n, precision=1)
        full = (l1.cpu().numpy()[:3], [g.numpy() for g in hh.unflat(g1.cpu(), c.H, c.nh)])
        tag = "%s: shards %d + %d" % (c.name, cut, c.n - cut)
        _assert_in_band(tag + " against the full call", c.band, la + lb, ga + gb, c.H, c.nh, ref=full)
        _assert_in_band(tag + " against the reference", c.band, la + lb, ga + gb, c.H, c.nh)


def test_mc_dropout_bf16_row_shards_and_eval_forward(lib):
    """Bitwise: an MC-dropout call equals the concatenation of two row shards with their row offsets, and its o0 equals the eval
    forward's u."""
    import hip_helpers as hh
    c = B.case("mid128")
    T, cut = 4, 130
    fp, xd, _ = _dev_inputs(c.P, c.x, c.y, c.H, c.nh)
    mk = lambda off: hh.dropout_struct(1, c.pl, seed=B.SEED, stream_id=100, row_offset=B.ROW0 + off)
    full = _mc(lib, c.H, c.nh, fp, xd, mk(0), T)
    a, b = _mc(lib, c.H, c.nh, fp, xd[:cut].contiguous(), mk(0), T), _mc(lib, c.H, c.nh, fp, xd[cut:].contiguous(), mk(cut), T)
    assert torch.equal(torch.cat([a, b], dim=1), full)
    u, _ = hh.forward(lib, c.H, c.nh, fp, xd, None, precision=1)
    torch.cuda.synchronize()
    assert torch.equal(full[0], u)
