"""CPU: every (layers, regime) case of test_gpu_regimes.py is proved here, so that a GPU failure cannot be blamed on the case.

1. Branch shares, on the case's own Philox masks: `sign` / `sat_sign` put at least 25 % of the rows on each side of logvar = 0, `linear`
   at least 25 % on each side of z = 20, `floor` every row below z = -7 (var < 1e-3, so precision above 1e3 on every row; the median row, z = -14, has
   var = 1.8e-6, more than half of it the floor), `saturated` at least 10 % of the first layer's activations beyond 0.99.
2. The referee stays inside the gates: torch's float32 arithmetic (the oracle as every other test runs it) against the float64 oracle
   is within HALF of rtol = atol = 1e-5 in u and logvar (eval and under the masks), half of 2e-5 in loss and mse, a tenth of
   2e-4 * max |ref| in every gradient tensor, and half of the MC gates in pred_mean / a_u / e_u.  Float32 itself can therefore meet
   every gate test_gpu_regimes.py applies, and a device failure there is the device's.

Measured here (float32 against float64, in units of the gate): u at most 0.12, logvar at most 0.44 ([8,64,200,48,1] sat_sign), gradients
at most 5.1e-6 of the tensor's largest element (bound 2e-5); cases that needed a lower gz or gain to get there are listed, with the
figures, at regimes.OVERRIDES."""
import numpy as np
import pytest
import torch

import pinn_oracle as O
import regimes as R

CASES = R.all_cases()
IDS = ["%s-%s%s" % ("x".join(map(str, l)), r, "-bf16" if b else "") for l, r, n, b in CASES]


def _gate(a, b, tol):
    return float((np.abs(np.asarray(a, np.float64) - b) / (tol + tol * np.abs(b))).max())


def test_regime_params_touch_only_what_they_name():
    layers, n = [8, 64, 200, 48, 1], 100
    c0 = R.Case(layers, "init", n)
    P = O.init_params(layers, seed=sum(layers))
    assert all(torch.equal(a, b) for a, b in zip(c0.P, P))
    c = R.Case(layers, "sat_sign", n)
    names = O.param_names(3)
    for name, a, b in zip(names, c.P, P):
        if name.endswith(".bias") and name != "var_layers.5.bias" or name == "predict.weight":
            assert torch.equal(a, b), name
        elif name == "var_layers.5.weight":
            assert torch.equal(a, b * 8.0), name
        elif name != "var_layers.5.bias":
            assert torch.equal(a, b * 4.0), name
    _, z = R.head_z(c.P, c.x, c.pl, c.masks)
    assert abs(float(z.median()) - 0.5413) < 1e-6
    assert all(abs(p - q) < 1e-12 for p, q in zip(R.p_list([8] + [16] * 6 + [1]), [0.1, 0.2, 0.3, 0.4, 0.1, 0.2, 0.3]))
    assert R.SEED >= 1 << 32 and R.STREAM != 0 and R.ROW0 != 0


def test_philox_masks_passes_equal_the_oracle_masks():
    layers, n = [8, 33, 65, 7, 70, 1], 37           # widths off the 32-feature call groups, five modules
    pl = R.p_list(layers)
    streams = [R.MC_STREAM, R.MC_STREAM + 5, 0xFFFFFFFF]
    got = R.philox_masks_passes(layers, n, pl, streams)
    for s, per_module in zip(streams, got):
        want = R.philox_masks(layers, n, pl, stream=s)
        assert len(per_module) == len(want) == 5
        assert all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(per_module, want))


@pytest.mark.parametrize("layers,regime,n,bf16", CASES, ids=IDS)
def test_branch_shares(layers, regime, n, bf16):
    c = R.case(layers, regime, n, bf16)
    a0, z = R.head_z(c.P, c.x, c.pl, c.masks)
    z = z.numpy()
    lv = c.train64[1]
    # head_z restates the oracle: the same logvar from its z
    assert np.abs(np.log(np.logaddexp(0.0, z) + 1e-6) - lv).max() < 1e-9
    pos, neg, hi, lo = (lv > 0).mean(), (lv < 0).mean(), (z > 20).mean(), (z < 20).mean()
    sat = float((a0.abs() > 0.99).double().mean())
    print("%s %s: z %.2f..%.2f  logvar > 0 %.2f < 0 %.2f  z > 20 %.2f  first-layer |a| > 0.99 %.3f" % (layers, regime, z.min(), z.max(), pos, neg, hi, sat))
    if regime in ("sign", "sat_sign"):
        assert pos >= 0.25 and neg >= 0.25, (pos, neg)
    if regime == "linear":
        assert hi >= 0.25 and lo >= 0.25, (hi, lo)
    if regime == "floor":
        assert z.max() < -7.0, z.max()
    if regime == "saturated":
        assert sat >= 0.10, sat
    if regime == "init":
        assert sat == 0.0


@pytest.mark.parametrize("layers,regime,n,bf16", CASES, ids=IDS)
def test_float32_referee_within_half_a_gate(layers, regime, n, bf16):
    c = R.case(layers, regime, n, bf16)
    for train, ref in ((False, c.eval64), (True, c.train64)):
        u32, lv32 = c.forward(train, torch.float32)
        gu, glv = _gate(u32, ref[0], 1e-5), _gate(lv32, ref[1], 1e-5)
        print("%s %s %s: u %.3f logvar %.3f of the gate" % (layers, regime, "masks" if train else "eval", gu, glv))
        assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
        assert gu <= 0.5 and glv <= 0.5, (gu, glv)
    l64, m64, g64 = c.nll64
    l32, m32, g32 = c.nll32
    print("loss %.3e (rel err %.2e)  mse rel err %.2e" % (l64, abs(l32 - l64) / abs(l64), abs(m32 - m64) / abs(m64)))
    assert abs(l32 - l64) <= 0.5 * 2e-5 * abs(l64) and abs(m32 - m64) <= 0.5 * 2e-5 * abs(m64)
    for name, a, b in zip(O.param_names(c.k), g32, g64):
        scale = float(b.abs().max())
        err = float((a.double() - b).abs().max())
        assert np.isfinite(err) and scale > 0 and err <= 0.1 * 2e-4 * scale, (name, err / scale)


MC_CASES = [t for t in CASES if not t[3] and t[2] != 129 and t[2] != R.CHUNK_ROWS]


@pytest.mark.parametrize("layers,regime,n,bf16", MC_CASES, ids=[i for i, t in zip(IDS, CASES) if t in MC_CASES])
def test_float32_mc_referee_within_half_a_gate(layers, regime, n, bf16):
    c = R.case(layers, regime, n, bf16)
    pm, au, eu = c.mc64
    pm32, au32, eu32 = R.mc_reference(c.P, c.x, c.pl, R.MC_T, c.mc_masks, torch.float32)
    assert _gate(pm32, pm, 1e-5) <= 0.5
    assert float((np.abs(au32 - au) / (1e-4 * np.abs(au))).max()) <= 0.5
    assert float((np.abs(eu32 - eu) / (2e-6 + 1e-3 * np.abs(eu))).max()) <= 0.5
    assert np.all(eu > 0) and np.all(au > 0)
