"""CPU: the float64 referee of the residual passes (tests/residual_referee.py).  It reproduces the reference's recorded tuples, losses
and gradients at both parameter sets of the fixture and torch autograd's derivative sums at every set, so it is a restatement of its own
and not csrc/pinn_physics.h typed again; its rows reach every branch a set is named for, every marked row weighs at least 100 gates,
every gate from 255 rows on is at most 1e-5 of the sum of the terms' magnitudes, and float32 torch's own sums pass the gates."""
import numpy as np
import pytest
import torch

import pinn_oracle as O
import residual_referee as rr

ALL_SETS = rr.MAIN_SETS + rr.EDGE_SETS


def test_tables_agree_with_the_binding():
    from pinn_amd import _lib
    assert {n: i for i, n in enumerate(rr.COL_NAMES)} == _lib.C and {n: i for i, n in enumerate(rr.SUM_NAMES)} == _lib.S
    assert rr.NSUMS == _lib.NSUMS and len(rr.COL_NAMES) == _lib.NCOLS and set(rr.COL_SRC) == set(rr.COL_NAMES)
    assert rr.FLAG == {"V": _lib.RES_V, "T": _lib.RES_T, "H": _lib.RES_H, "O": _lib.RES_O}
    assert max(rr.PERSISTENT_COUNTS) == _lib.STAGE_RUN_MAX_ROWS
    assert np.array_equal(rr.param_sets()["init"], rr.fixture()[0]["s0.lambdas"].astype(np.float32))


@pytest.mark.parametrize("si", [0, 1])
def test_referee_reproduces_the_recorded_tuples_losses_and_gradients(si):
    g, sx, sy = rr.fixture()
    N = g["x"].shape[0]
    real = O.denorm(g["x"], *O.scaler_affine(sx))
    lamv = g["s%d.lambdas" % si].astype(np.float32)
    un, yn = g["u_eval"].reshape(-1), g["y"].reshape(-1)
    c32, t32, _, branches = rr.evaluate(real, un, yn, lamv, torch.float32)
    c64, t64, _, _ = rr.evaluate(real, un, yn, lamv, torch.float64, branches=branches)
    for c, (m, j) in rr.COL_SRC.items():
        want = g["s%d.%s.%d" % (si, m, j)].reshape(-1).astype(np.float64)
        if m == "V":                                         # transcendentals: the libm of the recording host
            np.testing.assert_allclose(c32[c], want, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(want).max()), err_msg=c)
        else:
            assert np.array_equal(c32[c], want), c
        np.testing.assert_allclose(c64[c], want, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(want).max()), err_msg=c)
    L = O.LAMBDA_NAMES.index
    vn_scale = float(O.target_affine(sy)[0])
    table = [("V", "FV2", [("FV_D1", "lambda_1"), ("FV_D2", "lambda_2"), ("FV_D3", "lambda_3")], 2.0),
             ("T", "FT2", [("FT_D1", "lambda_T1"), ("FT_D3", "lambda_T3"), ("FT_D5", "lambda_T5")], 2.0),
             ("H", "FH2", [("FH_D1", "lambda_H1"), ("FH_D2", "lambda_H2"), ("FH_D3", "lambda_H3")], 2.0),
             ("O", "FO2", [("FO_D1", "lambda_O1"), ("FO_D2", "lambda_O2"), ("FO_D3", "lambda_O3")], 2.0),
             ("Vn", "YV2", [("YV_D1", "lambda_1"), ("YV_D2", "lambda_2"), ("YV_D3", "lambda_3")], -2.0 * 5.0 * vn_scale)]
    # the tolerances of test_residuals_golden, for r32 and for r64 on r32's side of the thresholds (the recording is float32, and row 3
    # has It = |lambda_O3| to the ulp: in float64 it takes the other branch, which moves sum f d_3 by that row's whole term)
    for tag, lossn, grads, factor in table:
        for t in (t64, t32):
            loss = t[lossn].sum() / N
            want = float(g["s%d.%s.loss" % (si, tag)])
            assert abs(loss - want) <= 1e-5 * abs(want), (tag, loss, want)
            for sn, ln in grads:
                want = g["s%d.%s.grad" % (si, tag)][L(ln)]
                got = factor * t[sn].sum() / N
                assert abs(got - want) <= 1e-4 * abs(want) + 1e-9, (tag, sn, got, want)


def _autograd_sums(rw, lamv, models):
    """Sum of f d_k over the rows from torch autograd of the oracle in float64: d/dlambda_k of sum f^2 / 2 (and of sum (y - Vn)^2 / 2)."""
    _, _, sy = rr.fixture()
    ymn, ysc = O.scaler_affine(sy)
    lam = {k: v.requires_grad_(True) for k, v in rr._lam(lamv, torch.float64).items()}
    real = torch.tensor(rw.real, dtype=torch.float64)
    out = {}

    def grads(loss, pairs, factor=1.0):
        gs = torch.autograd.grad(loss, [lam[n] for _, n in pairs], allow_unused=True)
        for (s, _), gk in zip(pairs, gs):
            out[s] = 0.0 if gk is None else float(gk) * factor
    if "V" in models:
        r = O.net_f_V(real, torch.tensor(rw.un).reshape(-1, 1), ymn, ysc, lam)
        pairs = [("FV_D1", "lambda_1"), ("FV_D2", "lambda_2"), ("FV_D3", "lambda_3")]
        grads((r[0] ** 2).sum() / 2, pairs)
        vs, vm = (t.double() for t in O.target_affine(sy))
        y = torch.tensor(rw.yn, dtype=torch.float64).reshape(-1, 1)
        r = O.net_f_V(real, torch.tensor(rw.un).reshape(-1, 1), ymn, ysc, lam)
        grads(((y - (r[5] * vs + vm)) ** 2).sum() / 2, [("YV" + s[2:], n) for s, n in pairs], -1.0 / (5.0 * float(vs)))
    if "T" in models:
        grads((O.net_f_T_simple(real, lam)[0] ** 2).sum() / 2, [("FT_D1", "lambda_T1"), ("FT_D3", "lambda_T3"), ("FT_D5", "lambda_T5")])
    if "H" in models:
        grads((O.net_f_H(real, lam)[0] ** 2).sum() / 2, [("FH_D1", "lambda_H1"), ("FH_D2", "lambda_H2"), ("FH_D3", "lambda_H3")])
    if "O" in models:
        grads((O.net_f_O(real, lam)[0] ** 2).sum() / 2, [("FO_D1", "lambda_O1"), ("FO_D2", "lambda_O2"), ("FO_D3", "lambda_O3")])
    return out


@pytest.mark.parametrize("set_name,idle", [(s, False) for s in ALL_SETS] + [("init", True), ("B", True)])
def test_derivative_terms_are_torch_autograd(set_name, idle):
    """The where branches, the inclusive clamp mask and sgn(lambda_O3) of the terms are autograd's, in float64 with the indicators
    float64 gives: at 257 rows, where the sets A, B, D have the mask at 0 and C the sign at 0."""
    rw = rr.rows(257, idle)
    models = "HO" if idle else "VTHO"
    t64 = rr.evaluate(rw.real, rw.un, rw.yn, rr.param_sets()[set_name], torch.float64, models)[1]      # its own indicators
    want = _autograd_sums(rw, rr.param_sets()[set_name], models)
    for s, w in want.items():
        got = t64[s].sum()
        scale = np.abs(t64[s]).sum()
        print("%-8s %-6s terms %.15g autograd %.15g" % (set_name, s, got, w))
        assert abs(got - w) <= 1e-12 * scale, (set_name, s, got, w)


def test_sets_reach_their_branches_on_the_edge_rows():
    """The counts on the fixture's 256 edge rows, in float32.  The fixture's own two sets never reach the oxygen clamp."""
    for s in ALL_SETS:
        st = rr.edge_stats(s)
        print(s, st)
        for b in rr.NAMED_BRANCHES[s]:
            assert st[b] > 0, (s, b, st)
    for s in ("init", "s1"):
        st = rr.edge_stats(s)
        assert st["o_low"] == 0 and st["o_high"] == 0 and st["o_inside"] == 256
    assert rr.edge_stats("C")["o_sgn"] == 0.0 and rr.edge_stats("C")["o_lin"] == 0 and rr.edge_stats("B")["o_sgn"] == -1.0
    d = rr.edge_stats("D")
    assert d["o_low"] + d["o_high"] > 0 and d["o_lin"] > 0
    for s in ("edge15", "edge105"):
        st = rr.edge_stats(s)
        assert st["o_on_edge"] == 256 and st["o_inside"] == 256            # on the edge, and the inclusive mask is 1 there
    # the float64 restatement of float32(1.05) is on the other side of the edge: why r32 is the authority there
    g = rr.fixture()[0]
    real = O.denorm(g["x"], *O.scaler_affine(rr.fixture()[1]))
    other = rr.evaluate(real, g["u_eval"].reshape(-1), g["y"].reshape(-1), rr.param_sets()["edge105"], torch.float64, "O")[2]
    assert other["o_inside"] == 0 and other["o_low"] == 256


@pytest.mark.parametrize("N,set_name,idle", rr.cases())
def test_conditions_hold_for_every_case(N, set_name, idle):
    ref = rr.referee(N, set_name, idle)
    rw = ref.rows
    assert rw.marked == rr.marked_positions(N) and len(set(rw.marked)) == len(rw.marked)
    if N >= 258:
        for b in rr.NAMED_BRANCHES[set_name]:
            assert ref.stats[b] > 0, (N, set_name, b, ref.stats)
    if idle:
        assert ref.stats["h_flow_clamped"] > 0 and ref.stats["o_flow_clamped"] > 0 and ref.models == "HO"
        assert ref.stats["h_flow_clamped"] < len(rw.idle)                  # an idle row above the clamp too
    figures = rr.check_conditions(ref)
    print(N, set_name, idle, {k: "%.3g" % v for k, v in figures.items()})
    # float32 torch's own sums, added in float64, pass the tightest gate of the case
    gate = ref.gate(1)
    for k, name in enumerate(rr.SUM_NAMES):
        if ref.live[k]:
            assert abs(ref.t32[name].sum() - ref.center[k]) <= gate[k], (N, set_name, name)
            assert abs(ref.t64[name].sum() - ref.center[k]) <= gate[k], (N, set_name, name)


def test_launch_shapes():
    assert [rr.rows_per_thread(N, "rows") for N in rr.ROW_COUNTS] == [1, 1, 1, 1, 1, 1, 2, 3]
    assert [rr.rows_per_thread(N, "cached") for N in rr.ROW_COUNTS] == [1, 1, 1, 2, 2, 2, 2, 3]
    assert [rr.rows_per_thread(N, "persistent") for N in rr.PERSISTENT_COUNTS] == [1, 1, 2, 5, 64]
    assert rr.marked_positions(1) == [0] and rr.marked_positions(257) == [0, 256]
    assert rr.marked_positions(rr.GRID_ROWS + 1) == [0, rr.GRID_ROWS - 1, rr.GRID_ROWS]
    n = 2 * rr.GRID_ROWS + 3
    assert rr.marked_positions(n) == [0, rr.GRID_ROWS - 1, rr.GRID_ROWS, 2 * rr.GRID_ROWS - 1, 2 * rr.GRID_ROWS, n - 1]
