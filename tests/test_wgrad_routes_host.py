"""CPU proof of tests/wgrad_routes.py: every case lands on the route, slice count and tiles-per-slice pattern it was chosen for (derived
from the constants of csrc/pinn_train.hip), and the gate that test_gpu_wgrad_routes.py applies tells every mutant from the float64
reference by MARGIN = 4 gates in every tensor the mutant touches, under the rms and the max form.

Where the K band alone does not reach 4 (one row of 163 857 is smaller than torch-fp32's own summation error in several tensors), the
module tightens that tensor's gate to a quarter of the mutant's distance; TIGHTENED records each such (case, tensor) with its margin in
K bands, measured here on the reference alone.  A (case, tensor) below 4 that is not recorded fails: redraw the case's seed, or record it."""
import numpy as np
import pytest

import pinn_oracle as O
import regimes as R
import wgrad_routes as W

# (case, H, tensor): smallest mutant distance in K bands (rms form, max form; K of the widest precision the case runs), all of mutant (a)
TIGHTENED = {
    ("serial_x3", 256, "predict.weight"): (2.57, 1.71),
    ("serial_x3", 256, "var_layers.0.weight"): (2.11, 1.15),
    ("serial_x3", 256, "var_layers.0.bias"): (3.60, 1.96),
    ("serial_x3", 256, "var_layers.3.weight"): (1.75, 0.58),
    ("serial_x3", 256, "var_layers.3.bias"): (3.00, 1.70),
    ("serial_x3", 256, "var_layers.5.weight"): (0.14, 0.09),
    ("serial_x3", 256, "var_layers.5.bias"): (None, 0.75),
}


def _k(name, H):
    """The widest K among the precisions a case runs on the net of width H: what TIGHTENED is recorded at (a lower K only narrows the band)."""
    return max(W.K_OF[p] for c, p, h, _ in W.RUNS if (c, h) == (name, H))


@pytest.mark.parametrize("run", W.RUNS, ids=W.run_id)
def test_route_claims(run):
    name, prec, H, nh = run
    rows = W.case_of(name)[2]
    got = W.plan(prec, H, nh, rows)
    want = W.CLAIMS[(name, prec, H)]
    assert {k: got[k] for k in want} == want, (W.run_id(run), got)
    assert rows % 128 == 17
    # several tiles per slice somewhere, and the walk's own edge: uneven counts (interleaved), a short and an empty slice (contiguous)
    assert max(got["tiles"]) >= 2
    if name in ("fan", "serial"):
        assert (len(got["tiles"]) == 2) if got["walk"] == "interleaved" else (0 in got["tiles"] and len(got["tiles"]) == 3)
    if name == "serial_x3":
        assert got["per_slice"][:9] == [41] * 8 + [40]


def test_plan_matches_the_small_oracle_cases():
    """The slice counts the parity tests of the wide nets run at (300, 200, 129 and 70 rows: 12, 8, 8, 4), from the same restatement."""
    assert [W.plan(W.X6, 512, 2, n)["slices"] for n in (300, 200, 129, 70)] == [12, 8, 8, 4]
    assert W.plan(W.X6, 256, 3, 4096)["route"] == "multi" and W.plan(W.X6, 256, 3, 4096)["tiles"] == {8: 32}
    assert W.plan(W.X6, 256, 3, 1_000_000)["route"] == "serial"


def test_philox_masks_bitwise():
    layers, pl = [8, 256, 128, 1], [0.2, 0.35, 0.5]
    seed, stream, row0, n = (3 << 32) + 17, 5, (1 << 32) - 300, 777          # rows on both sides of 2^32
    got = W.philox_masks(layers, n, pl, stream=stream, seed=seed, row0=row0)
    for l, (w, p) in enumerate(zip(R.widths(layers), pl)):
        assert np.array_equal(got[l], O.philox_keep_mask(seed, stream, row0, n, l, w, p)), l


def test_mutants_are_what_they_say():
    """On the smallest case: the mutants' rows; mutant (b) built by linearity equals the oracle's float64 gradient of the batch WITHOUT
    those 16 rows (rescaled from its own mean over 257 rows to the mean over 273); mutant (d) differs from g64 in the two blocks only."""
    ref = W.reference("wide2048", 2048, 2)
    n = ref.n
    lo, hi = ref.mutant_rows["b"]
    assert (lo, hi) == (256, 272) and ref.mutant_rows["a"] == (272, 273) and ref.mutant_rows["c"] == (128, 144, 160)
    keep = np.r_[0:lo, hi:n]
    masks = [m[keep] for m in W.philox_masks(ref.layers, n, ref.pl)]
    g = O.nll_loss_and_grads([p.double() for p in ref.P], ref.x.double()[keep], ref.y.double().reshape(-1, 1)[keep], ref.pl, masks)[2]
    for name, direct, mutant, full in zip(ref.names, g, ref.mutants["b"], ref.g64):
        direct = direct.numpy() * (len(keep) / n)
        assert np.abs(direct - mutant).max() <= 1e-12 * np.abs(full).max(), name
    i = ref.names.index("layers.layer_1.weight")
    d = ref.mutants["d"][i]
    assert np.array_equal(d[0:256, 256:512], ref.g64[i][256:512, 0:256]) and np.array_equal(d[256:512, 0:256], ref.g64[i][0:256, 256:512])
    assert np.array_equal(d[512:], ref.g64[i][512:]) and np.array_equal(d[:512, 512:], ref.g64[i][:512, 512:])
    assert np.array_equal(d[0:256, 0:256], ref.g64[i][0:256, 0:256]) and np.array_equal(d[256:512, 256:512], ref.g64[i][256:512, 256:512])
    assert all(np.array_equal(a, b) for k, (a, b) in enumerate(zip(ref.mutants["d"], ref.g64)) if k != i)


REFS = sorted({(name, H, nh) for name, _, H, nh in W.RUNS}, key=lambda r: W.CASE_IDS.index(r[0]))


@pytest.mark.parametrize("name,H,nh", REFS, ids=["%s-H%d" % r[:2] for r in REFS])
def test_every_mutant_four_gates_away(name, H, nh):
    ref = W.reference(name, H, nh)
    assert set(ref.mutants) == ({"a", "b", "c", "d"} if H > 256 else {"a", "b", "c"})
    for K in sorted({W.K_OF[p] for c, p, h, _ in W.RUNS if (c, h) == (name, H)}, reverse=True):
        low = {}
        for m, tensor, r, x in ref.mutant_margins(K):
            print("%-16s H%-5d K %g %s %-24s rms %10s  max %10.2f   (K bands)" % (name, H, K, m, tensor, "-" if r is None else "%.2f" % r, x))
            assert x > 0 and (r is None or r > 0)
            if min(x, x if r is None else r) < W.MARGIN:
                low.setdefault(tensor, []).append(m)
        if K == _k(name, H):
            unrecorded = sorted(t for t in low if (name, H, t) not in TIGHTENED)
            assert not unrecorded, ("mutants closer than %g K bands, not in TIGHTENED" % W.MARGIN, name, H, {t: low[t] for t in unrecorded})
        # the gate actually applied: every mutant MARGIN gates away in every tensor it touches, both forms
        for i, tensor in enumerate(ref.names):
            sr, sm = ref.gate_scale(tensor, K)
            assert 0 < sm <= 1.0 and (sr is None or 0 < sr <= 1.0)
            assert (sm == 1.0 and sr in (None, 1.0)) or (name, H, tensor) in TIGHTENED or K != _k(name, H)
            for m, g in ref.mutants.items():
                if np.array_equal(g[i], ref.g64[i]):
                    continue
                r, x = ref.in_bands(i, g, K)
                assert x / sm >= W.MARGIN * (1 - 1e-12) and (r is None or r / sr >= W.MARGIN * (1 - 1e-12)), (name, H, m, tensor)


def test_exceptions_are_real_runs_and_fit_their_gate():
    """Every EXCEPTIONS entry names a run and a tensor, records an excess over the K band, and that excess fits the gate it is given: a
    quarter of the tensor's smallest mutant distance -- which the proof above shows to be wider than the band only because every mutant
    is far more than 4 bands away there."""
    ids = {W.run_id(r): r for r in W.RUNS}
    for (rid, tensor), measured in W.EXCEPTIONS.items():
        assert rid in ids, rid
        name, prec, H, nh = ids[rid]
        ref = W.reference(name, H, nh)
        assert tensor in ref.names and tensor in W.excepted(ids[rid])
        assert (name, H, tensor) not in TIGHTENED
        sr, sm = ref.gate_scale(tensor, W.K_OF[prec], True)
        print("%-24s %-24s measured %.3f K bands, gate %s / %.1f K bands" % (rid, tensor, measured, "-" if sr is None else "%.1f" % sr, sm))
        assert 1.0 < measured <= min(sm, sm if sr is None else sr)
