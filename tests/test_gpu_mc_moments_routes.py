"""MC-dropout moments of every accumulation code (tests/mc_moments.py) at odd pass counts, on both x6 variants and across the chunk
edges of the wide and the general path, held to float64 moments of the library's OWN passes.

The passes of a call come one by one from pinn_mlp_forward / pinn_gnet_forward (same kernels, Philox stream s0 + t, or the injected
words of pass t alone), so forward error is no part of the comparison and the gates are a few ulps (mc_moments.Reference): pred_mean
bitwise, a_u and e_u per row.  On the wide and the general path the T = 1 (a_u = exp(0.5 lv_0)) and T = 2 (e_u = |du_0 - du_1| / 2)
cases establish that relation before the odd counts rely on it.  Outputs are pre-filled with NaN, every case runs once, and every
comparison prints its worst ratio to the gate before it asserts (run with -s).

    F1-F6  PINN_PREC_F32X6 / _G6, fused: two Welford states by parity, `split` and `waves8`, spare pass at odd T
    E1 B1  exact fp32 and bf16-mixed, fused: one state
    W0-W3  wide nets: accum[4][65 536] reused by the second row chunk, outputs and injected words offset by the chunk start
    G1 G2  general path: (pass, row) virtual rows, cut inside a pass at T = 121"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gnet_helpers as G
import hip_helpers as hh
import mc_moments as M
import pinn_oracle as O
import regimes as R

SEED, S0, P = M.SEED, M.STREAM, M.P_MC


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rows(n, seed):
    return (torch.rand(n, 8, generator=torch.Generator().manual_seed(seed)) * 2 - 1).contiguous()


def _net(H, nh, n, seed):
    """(parameters, flat parameters on the device, rows, rows on the device)."""
    Pm = O.init_params([8] + [H] * nh + [1], seed=seed)
    x = _rows(n, seed + 1)
    return Pm, hh.flat_params(Pm, H, nh).to(hh.dev()), x, x.to(hh.dev())


def _philox(nh, t=0, row_offset=0):
    return hh.dropout_struct(1, [P] * (nh + 1), seed=SEED, stream_id=S0 + t, row_offset=row_offset)


def _mc(lib, H, nh, prec, fp, xd, drop, T):
    from pinn_amd import _lib
    n = xd.shape[0]
    out = torch.full((3, n), float("nan"), device=hh.dev())
    net = hh.make_net(lib, H, nh, prec)
    _lib.check(lib.pinn_mc_dropout(ctypes.byref(net), hh.ptr(fp), hh.ptr(xd), n, ctypes.byref(drop), T, hh.ptr(out[0]), hh.ptr(out[1]),
                                   hh.ptr(out[2]), hh.stream()), "pinn_mc_dropout")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _passes(fwd, T, drop_of):
    """Reference of the library's own passes: fwd(drop or None) -> (u, lv) tensors; drop_of(t) the dropout of pass t alone."""
    u_eval = fwd(None)[0].cpu().numpy()
    got = [fwd(drop_of(t)) for t in range(T)]
    return M.Reference(u_eval, np.stack([u.cpu().numpy() for u, _ in got]), np.stack([lv.cpu().numpy() for _, lv in got]))


def _fused_ref(lib, H, nh, prec, fp, xd, T, drop_of):
    return _passes(lambda d: hh.forward(lib, H, nh, fp, xd, d, precision=prec), T, drop_of)


def _hold(tag, o, ref):
    """All three outputs of a call against the gates; prints the worst ratios first."""
    assert np.isfinite(o).all(), (tag, "rows left unwritten or not finite", int((~np.isfinite(o)).any(axis=0).sum()))
    ra, re_ = ref.a_ratio(o[1]), ref.e_ratio(o[2])
    same = np.array_equal(o[0], ref.pred_mean)
    print("%-44s T %-3d rows %-6d pred_mean %s  a_u %.3f of the gate (row %d)  e_u %.3f of the gate (row %d)"
          % (tag, ref.T, ref.n, "bitwise" if same else "DIFFERS", ra.max(), int(ra.argmax()), re_.max(), int(re_.argmax())))
    assert same, (tag, "pred_mean is not the forward without dropout", int((o[0] != ref.pred_mean).sum()))
    assert ra.max() <= 1.0, (tag, "a_u", float(ra.max()), int(ra.argmax()))
    assert re_.max() <= 1.0, (tag, "e_u", float(re_.max()), int(re_.argmax()))
    if ref.T == 1:
        assert np.array_equal(o[2], np.zeros(ref.n, dtype=np.float32)), (tag, "one pass has no spread")
    if ref.T == 2:
        want = np.abs(ref.du[0].astype(np.float64) - ref.du[1].astype(np.float64)) / 2
        r = M.Reference._over(np.abs(o[2].astype(np.float64) - want), ref.gate_e)
        print("%-44s T 2   e_u against |du0 - du1| / 2: %.3f of the gate" % (tag, r.max()))
        assert r.max() <= 1.0, (tag, float(r.max()))


def _done(*arrays):
    torch.cuda.synchronize()
    assert all(np.isfinite(a).all() for a in arrays)


def _oracle_gates(tag, o, want):
    """The tolerances of test_mc_dropout_x6 / test_wide_injected_masks against the fp32 oracle."""
    pm, au, eu = [np.asarray(w).reshape(-1) for w in want]
    r = [float((np.abs(o[0] - pm) / (1e-5 + 1e-5 * np.abs(pm))).max()), float((np.abs(o[1] - au) / (1e-4 * np.abs(au))).max()),
         float((np.abs(o[2] - eu) / (2e-6 + 1e-3 * np.abs(eu))).max())]
    print("%-44s against the oracle: pred_mean %.3f  a_u %.3f  e_u %.3f of its bound" % (tag, r[0], r[1], r[2]))
    assert max(r) <= 1.0, (tag, r)


# ---------------------------------------------------------------------------------------------------------------------------
# fused nets
def _fused_philox_case(lib, tag, prec, H, nh, n, T, seed):
    Pm, fp, x, xd = _net(H, nh, n, seed)
    o = _mc(lib, H, nh, prec, fp, xd, _philox(nh), T)
    ref = _fused_ref(lib, H, nh, prec, fp, xd, T, lambda t: _philox(nh, t))
    _hold(tag, o, ref)
    _done(o)
    return Pm, x, o


@pytest.mark.parametrize("T", [1, 3])
def test_f1_one_row_split(lib, cus, T):
    """`split`: one valid row, 63 padded; the spare pass at both counts."""
    assert M.variant(1, cus) == dict(variant="split", tile_rows=64, tiles=1, workgroups=1)
    _fused_philox_case(lib, "F1 x6 [8,256x3,1] split", 2, 256, 3, 1, T, 11)


@pytest.mark.parametrize("T", [1, 2, 3, 5, 7, 33])
def test_f2_ragged_second_tile_every_odd_branch(lib, cus, T):
    """`split`: 64 + 1 rows; T = 33 is 17 + 16 passes.  At T = 3 also against the oracle's own passes."""
    assert M.variant(65, cus)["variant"] == "split" and M.variant(65, cus)["tiles"] == 2
    Pm, x, o = _fused_philox_case(lib, "F2 x6 [8,128,1] split", 2, 128, 1, 65, T, 12)
    if T == 3:
        _oracle_gates("F2 x6 [8,128,1] split T 3", o,
                      O.mc_dropout(Pm, x, P, T, lambda t: O.philox_masks_for_net(SEED, S0 + t, 0, 65, 128, 1, [P] * 2)))


def test_f3_last_split_and_first_waves8_launch_agree_bitwise(lib, cus):
    """128 floor(cus / 2) rows and one more: the same rows at the same offsets through the two variants, odd T."""
    lo, hi = M.f3_rows(cus)
    assert M.variant(lo, cus)["variant"] == "split" and M.variant(hi, cus)["variant"] == "waves8"
    H, nh, T = 256, 3, 5
    Pm, fp, x, xd = _net(H, nh, hi, 13)
    o_hi = _mc(lib, H, nh, 2, fp, xd, _philox(nh), T)
    o_lo = _mc(lib, H, nh, 2, fp, xd[:lo].contiguous(), _philox(nh), T)
    ref = _fused_ref(lib, H, nh, 2, fp, xd, T, lambda t: _philox(nh, t))
    _hold("F3 x6 [8,256x3,1] waves8 %d rows" % hi, o_hi, ref)
    diff = int((o_lo != o_hi[:, :lo]).sum())
    print("F3 split %d rows against waves8 %d rows: %d of %d values differ" % (lo, hi, diff, o_lo.size))
    assert np.isfinite(o_lo).all() and diff == 0
    _done(o_lo, o_hi)


def test_f4_more_tiles_than_workgroups_and_the_tail_alone(lib, cus):
    """`waves8`, 128 (cus + 1) + 129 rows: a workgroup's second tile starts from zeroed states; the last 129 rows alone, with
    row_offset, run as `split` and are bitwise the full call's."""
    n, tail = M.f4_rows(cus), 129
    w = M.variant(n, cus)
    assert w["variant"] == "waves8" and w["tiles"] > w["workgroups"] and M.variant(tail, cus)["variant"] == "split"
    H, nh, T = 128, 2, 3
    Pm, fp, x, xd = _net(H, nh, n, 14)
    o = _mc(lib, H, nh, 2, fp, xd, _philox(nh), T)
    ref = _fused_ref(lib, H, nh, 2, fp, xd, T, lambda t: _philox(nh, t))
    _hold("F4 x6 [8,128x2,1] waves8", o, ref)
    o_t = _mc(lib, H, nh, 2, fp, xd[n - tail:].contiguous(), _philox(nh, 0, n - tail), T)
    diff = int((o_t != o[:, n - tail:]).sum())
    print("F4 the last %d rows alone (split): %d of %d values differ" % (tail, diff, o_t.size))
    assert np.isfinite(o_t).all() and diff == 0
    _done(o, o_t)


@pytest.mark.parametrize("T", [1, 3])
def test_f5_injected_masks_spare_pass_reads_pass_0(lib, cus, T):
    """PINN_DROP_BITS, `split`, a bits tensor of exactly T passes: the spare pass of the odd half has only pass 0's words to read."""
    H, nh, n = 128, 3, 130
    assert M.variant(n, cus)["variant"] == "split"
    Pm, fp, x, xd = _net(H, nh, n, 15)
    g = torch.Generator().manual_seed(16)
    per_pass = [[(torch.rand(n, w, generator=g) >= P).numpy() for w in [H] * nh + [H // 2]] for _ in range(T)]
    bits = hh.pack_mask_bits(per_pass).to(hh.dev())
    assert tuple(bits.shape) == (T, n, nh * H // 32 + H // 64)
    pl = [P] * (nh + 1)
    o = _mc(lib, H, nh, 2, fp, xd, hh.dropout_struct(2, pl, bits=bits), T)
    one = [bits[t:t + 1].contiguous() for t in range(T)]
    ref = _fused_ref(lib, H, nh, 2, fp, xd, T, lambda t: hh.dropout_struct(2, pl, bits=one[t]))
    _hold("F5 x6 [8,128x3,1] split, injected masks", o, ref)
    _done(o)


def test_f6_g6_precision_takes_the_same_forward(lib, cus):
    assert M.variant(200, cus)["variant"] == "split"
    _fused_philox_case(lib, "F6 g6 [8,256x2,1] split", 3, 256, 2, 200, 3, 17)


@pytest.mark.parametrize("T", [1, 3, 7])
@pytest.mark.parametrize("prec,name", [(0, "E1 fp32"), (1, "B1 bf16")])
def test_e1_b1_sequential_order(lib, prec, name, T):
    _fused_philox_case(lib, "%s [8,256x3,1]" % name, prec, 256, 3, 129, T, 18)


# ---------------------------------------------------------------------------------------------------------------------------
# wide nets
@pytest.mark.parametrize("T", [1, 2])
def test_w0_wide_forward_pass_is_the_mc_pass(lib, T):
    assert M.wide_chunks(300) == [(0, 300)]
    _fused_philox_case(lib, "W0 x6 [8,512,1] wide", 2, 512, 1, 300, T, 21)


def test_w3_wide_bf16(lib):
    _fused_philox_case(lib, "W3 bf16 [8,512,1] wide", 1, 512, 1, 300, 3, 22)


def test_w1_wide_second_chunk_in_a_reused_accum(lib):
    """65 536 + 129 rows, Philox, T = 3: every row against the per-pass reference; the 128 rows across row 65 536 and the second
    chunk's 129 rows, each run alone with row_offset, bitwise the full call's."""
    H, nh, n, T = 512, 1, M.W_ROWS, 3
    assert M.wide_chunks(n) == [(0, 65536), (65536, 129)]
    Pm, fp, x, xd = _net(H, nh, n, 23)
    o = _mc(lib, H, nh, 2, fp, xd, _philox(nh), T)
    ref = _fused_ref(lib, H, nh, 2, fp, xd, T, lambda t: _philox(nh, t))
    _hold("W1 x6 [8,512,1] wide, two chunks", o, ref)
    for w0, w in M.W_WINDOWS:
        o_w = _mc(lib, H, nh, 2, fp, xd[w0:w0 + w].contiguous(), _philox(nh, 0, w0), T)
        diff = int((o_w != o[:, w0:w0 + w]).sum())
        print("W1 rows [%d, %d) alone: %d of %d values differ" % (w0, w0 + w, diff, o_w.size))
        assert np.isfinite(o_w).all() and diff == 0
    _done(o)


def test_w2_wide_injected_masks_across_the_chunk_edge(lib):
    """PINN_DROP_BITS on 65 536 + 129 rows, p = 0.5 (words drawn on the device, every bit a fair coin): MC with T = 2 and a stochastic
    forward.  The full calls against the per-pass reference; the two windows, given the contiguous slice of the words, bitwise the full
    calls' rows and within the oracle's tolerances under the unpacked masks."""
    H, nh, n, T, p = 512, 1, M.W_ROWS, 2, 0.5
    words = nh * H // 32 + H // 64
    assert words == 24
    Pm, fp, x, xd = _net(H, nh, n, 24)
    bits = torch.randint(-2 ** 31, 2 ** 31, (T, n, words), dtype=torch.int32, device=hh.dev(), generator=torch.Generator(hh.dev()).manual_seed(25))
    pl = [p] * (nh + 1)
    bd = lambda b: hh.dropout_struct(2, pl, bits=b)
    o = _mc(lib, H, nh, 2, fp, xd, bd(bits), T)
    one = [bits[t:t + 1].contiguous() for t in range(T)]
    ref = _fused_ref(lib, H, nh, 2, fp, xd, T, lambda t: bd(one[t]))
    _hold("W2 x6 [8,512,1] wide, injected masks", o, ref)
    u_full, lv_full = [v.cpu().numpy() for v in hh.forward(lib, H, nh, fp, xd, bd(bits), precision=2)]      # the words of pass 0
    assert np.array_equal(u_full, ref.u_t[0]) and np.array_equal(lv_full, ref.lv_t[0])
    for w0, w in M.W_WINDOWS:
        bw = bits[:, w0:w0 + w].contiguous()
        xw = xd[w0:w0 + w].contiguous()
        o_w = _mc(lib, H, nh, 2, fp, xw, bd(bw), T)
        u_w, lv_w = [v.cpu().numpy() for v in hh.forward(lib, H, nh, fp, xw, bd(bw), precision=2)]
        diff = int((o_w != o[:, w0:w0 + w]).sum()) + int((u_w != u_full[w0:w0 + w]).sum()) + int((lv_w != lv_full[w0:w0 + w]).sum())
        print("W2 rows [%d, %d) alone: %d of %d values differ" % (w0, w0 + w, diff, o_w.size + 2 * w))
        assert np.isfinite(o_w).all() and diff == 0
        raw = np.unpackbits(bw.cpu().numpy().view(np.uint8).reshape(T, w, 4 * words), axis=-1, bitorder="little").astype(bool)
        masks = lambda t: [raw[t][:, :H], raw[t][:, H:H + H // 2]]
        _oracle_gates("W2 rows [%d, %d)" % (w0, w0 + w), o_w, O.mc_dropout(Pm, x[w0:w0 + w], p, T, masks))
        with torch.no_grad():
            uf, lvf = O.mlp_forward(Pm, x[w0:w0 + w], pl, masks(0))
        np.testing.assert_allclose(u_w, uf.numpy().reshape(-1), rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(lv_w, lvf.numpy().reshape(-1), rtol=1e-5, atol=1e-5)
    _done(o, u_full, lv_full)


# ---------------------------------------------------------------------------------------------------------------------------
# general path
def _general_case(lib, tag, layers, n, T, seed):
    Pm = O.init_params(layers, seed=seed)
    fp, xd = G.flat(layers, Pm), _rows(n, seed + 1).to(hh.dev())
    drop = lambda t: G.drop(1, layers, P, SEED, S0 + t, M.ROW0)
    o = G.mc(lib, layers, fp, xd, drop(0), T)
    ref = _passes(lambda d: G.forward(lib, layers, fp, xd, d), T, drop)
    _hold(tag, o, ref)
    _done(o)


@pytest.mark.parametrize("T", [1, 2, 3, 7])
def test_g1_general_virtual_rows_one_chunk(lib, T):
    """T = 1 and T = 2 establish that pinn_gnet_forward's pass is pinn_gnet_mc_dropout's."""
    _general_case(lib, "G1 general [8,100,100,1]", [8, 100, 100, 1], 200, T, 31)


def test_g2_general_chunk_cut_inside_a_pass_odd_count(lib):
    """[8,2048,8,1], 97 rows, T = 121: 97 * 122 = 11 834 virtual rows in chunks of 10 880 (test_general_mc_exact_across_a_chunk_boundary
    derives the figure); the odd twin of that test's T = 120."""
    layers, n, T = R.CHUNK_NET, R.CHUNK_ROWS, R.CHUNK_T + 1
    cap = ((256 << 20) // (4 * (3 * 2048 + 2))) // 64 * 64
    assert T == 121 and cap < n * (T + 1) <= 2 * cap and cap % n != 0
    _general_case(lib, "G2 general [8,2048,8,1] two chunks", layers, n, T, 32)
