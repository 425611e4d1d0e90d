"""CPU proof of tests/mc_moments.py: the fp32 twin of both accumulation orders against float64 on passes of the fp32 oracle (the
measurement behind G), the a_u bound on the twin, every claimed mutant beyond MARGIN = 4 gates on at least half of the rows, the two
closed forms (T = 1: e_u == 0 exactly; T = 2: |du_0 - du_1| / 2), and the route plan against the constants of the source.  Run with -s
to read the twin maxima and the mutant distances."""
import os
import re

import numpy as np
import pytest

import mc_moments as M

ORDERS = ("sequential", "parity")
CASES = [(s, T) for s in M.HOST_NET_SEEDS for T in M.HOST_T]
CASE_IDS = ["net%d-T%d" % c for c in CASES]


def _src(name):
    return open(os.path.join(M.CSRC, name)).read()


def test_twin_against_float64_is_the_measurement_behind_G():
    """The largest |twin - e64| / (2^-24 max_t |du_t|) over every host case and both orders: G is four times it."""
    worst = {}
    for s, T in CASES:
        ref = M.host_case(s, T)
        assert ref.n == M.HOST_ROWS and ref.T == T and float(ref.du_max.min()) > 0.0
        for order in ORDERS:
            a_u, e_u = M.twin(ref.du, ref.lv_t, order)
            units, ra, re_ = float(ref.e_units(e_u).max()), float(ref.a_ratio(a_u).max()), float(ref.e_ratio(e_u).max())
            print("net %d T %-3d %-10s e_u: %.3f units of 2^-24 max|du|, %.3f of the gate   a_u: %.3f of the gate" % (s, T, order, units, re_, ra))
            worst[order] = max(worst.get(order, 0.0), units)
            assert ra <= 1.0, (s, T, order, ra)
            assert re_ <= 1.0, (s, T, order, re_)
    twin_max = max(worst.values())
    print("twin maxima: %s   G = %g = 4 x %g" % ("  ".join("%s %.3f" % kv for kv in sorted(worst.items())), M.G, M.TWIN_MAX))
    assert twin_max <= M.G / 4.0 and M.G == 4.0 * M.TWIN_MAX
    assert twin_max > M.TWIN_MAX / 2.0, "TWIN_MAX is not the measurement any more: %.3f" % twin_max


@pytest.mark.parametrize("s,T", CASES, ids=CASE_IDS)
def test_claimed_mutants_are_four_gates_away_on_half_the_rows(s, T):
    ref = M.host_case(s, T)
    seen = 0
    for mutant in (1, 2, 3, 4):
        for order in (ORDERS if mutant == 4 else ("parity",)):
            if mutant == 4 and T < 2:
                continue
            a_u, e_u = M.twin(ref.du, ref.lv_t, order, mutant)
            ra, re_ = ref.a_ratio(a_u), ref.e_ratio(e_u)
            print("net %d T %-3d mutant %d %-10s e_u median %10.1f gates, beyond 4 on %5.1f %% of rows   a_u median %10.1f gates, beyond 4 on %5.1f %%"
                  % (s, T, mutant, order, np.median(re_), 100 * (re_ > M.MARGIN).mean(), np.median(ra), 100 * (ra > M.MARGIN).mean()))
            if (mutant, T) in M.CLAIMED_E:
                seen += 1
                assert (re_ > M.MARGIN).mean() >= 0.5, (mutant, T, order, float(np.median(re_)))
            if (mutant, T) in M.CLAIMED_A:
                seen += 1
                assert (ra > M.MARGIN).mean() >= 0.5, (mutant, T, order, float(np.median(ra)))
    assert seen == sum(2 if m == 4 else 1 for m, t in M.CLAIMED_E if t == T) + sum(1 for m, t in M.CLAIMED_A if t == T)


def test_claims_are_the_issue_s():
    odd = [T for T in M.HOST_T if T % 2]
    assert sorted(M.CLAIMED_A) == [(1, T) for T in odd]
    assert sorted(M.CLAIMED_E) == sorted([(1, T) for T in odd if T >= 3] + [(2, T) for T in (3, 5, 7)]
                                         + [(m, T) for m in (3, 4) for T in M.HOST_T if T >= 2])


@pytest.mark.parametrize("s", M.HOST_NET_SEEDS)
def test_one_pass_has_no_spread_and_two_passes_half_their_distance(s):
    ref = M.host_case(s, 1)
    for order in ORDERS:
        a_u, e_u = M.twin(ref.du, ref.lv_t, order)
        assert np.array_equal(e_u, np.zeros(ref.n, dtype=np.float32)), order
        assert float(ref.a_ratio(a_u).max()) <= 1.0
    ref = M.host_case(s, 2)
    want = np.abs(ref.du[0].astype(np.float64) - ref.du[1].astype(np.float64)) / 2
    assert np.abs(want - ref.e64).max() <= 2.0 ** -50 * ref.du_max.max()          # the float64 reference itself
    _, e_u = M.twin(ref.du, ref.lv_t, "parity")
    r = np.abs(e_u.astype(np.float64) - want) / ref.gate_e
    print("net %d T 2 parity against |du0 - du1| / 2: %.3f of the gate" % (s, r.max()))
    assert r.max() <= 1.0


def test_mutants_differ_only_where_they_say():
    """Mutant 1 is the twin itself at even T; mutant 2 at T = 2 (n0 = n1 = 1 either way); no mutant but 1 moves a_u."""
    ref = M.host_case(M.HOST_NET_SEEDS[0], 2)
    base = M.twin(ref.du, ref.lv_t, "parity")
    for mutant in (1, 2):
        got = M.twin(ref.du, ref.lv_t, "parity", mutant)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), mutant
    ref = M.host_case(M.HOST_NET_SEEDS[0], 5)
    base = M.twin(ref.du, ref.lv_t, "parity")
    for mutant in (2, 3, 4):
        got = M.twin(ref.du, ref.lv_t, "parity", mutant)
        assert np.array_equal(got[0], base[0]) and not np.array_equal(got[1], base[1]), mutant
    assert not np.array_equal(M.twin(ref.du, ref.lv_t, "parity", 1)[0], base[0])


def test_reference_is_numpy_s_own_statement():
    ref = M.host_case(M.HOST_NET_SEEDS[0], 7)
    du = (ref.u_t - ref.u_eval[None, :]).astype(np.float64)
    assert np.array_equal(ref.e64, np.sqrt(np.var(du, axis=0))) or np.abs(ref.e64 - np.sqrt(np.var(du, axis=0))).max() <= 1e-15
    assert np.allclose(ref.a64, np.sqrt(np.exp(np.mean(ref.lv_t.astype(np.float64), axis=0))), rtol=1e-14, atol=0)
    assert ref.pred_mean is ref.u_eval


# ---------------------------------------------------------------------------------------------------------------------------
# source drift
def test_plan_restates_the_source():
    x6, wide = _src("pinn_x6.hip"), _src("pinn_wide.hip")
    assert M.wide_chunk() == int(re.search(r"constexpr int kWideChunk = (\d+);", wide).group(1)) == 65536
    assert re.search(r"for \(long long r0 = 0; r0 < fa\.n_rows; r0 \+= kWideChunk\)", wide)
    assert re.search(r"const long long t128 = \(a\.n_rows \+ 127\) / 128;", x6)
    assert re.search(r"const bool small_n = !force8 && 2 \* t128 <= cus;", x6)
    assert re.search(r"const long long n_tiles = small_n \? \(a\.n_rows \+ 63\) / 64 : t128;", x6)
    assert re.search(r"const int grid = \(int\)\(n_tiles < cus \? n_tiles : cus\);", x6)
    # the parity states and the merge the twin restates
    assert re.search(r"const float inv_k = 1\.0f / \(float\)\(t / 2 \+ 1\)", x6)
    assert re.search(r"const float n0 = \(float\)\(\(n_passes \+ 1\) / 2\), n1 = \(float\)\(n_passes / 2\), inv_n = 1\.0f / \(float\)n_passes;", x6)
    assert re.search(r"a\.m2 = \(a\.m2 \+ b\.m2\) \+ \(d \* d\) \* \(n0 \* n1 \* inv_n\);", x6)
    assert re.search(r"t_end = kSplit \? 2 \* \(\(a\.n_passes \+ 1\) / 2\) : a\.n_passes;", x6)
    assert re.search(r"c\.pass = \(unsigned\)\(t < 0 \|\| spare \? 0 : t\);", x6)


def test_plan_at_the_row_counts_of_the_gpu_cases():
    cus = 256
    v = lambda n: M.variant(n, cus)
    assert v(1) == dict(variant="split", tile_rows=64, tiles=1, workgroups=1)                       # F1
    assert v(65) == dict(variant="split", tile_rows=64, tiles=2, workgroups=2)                      # F2
    lo, hi = M.f3_rows(cus)                                                                         # F3
    assert (lo, hi) == (16384, 16385)
    assert v(lo) == dict(variant="split", tile_rows=64, tiles=256, workgroups=256)
    assert v(hi) == dict(variant="waves8", tile_rows=128, tiles=129, workgroups=129)
    n4 = M.f4_rows(cus)                                                                             # F4
    assert n4 == 33025 and v(n4) == dict(variant="waves8", tile_rows=128, tiles=259, workgroups=256)
    assert v(129)["variant"] == "split" and v(129)["tiles"] == 3
    assert v(130)["variant"] == "split" and v(200)["variant"] == "split"                             # F5, F6
    # the switch and the tail hold for every CU count a device of this family reports
    for c in (64, 80, 104, 228, 256, 304):
        lo, hi = M.f3_rows(c)
        assert M.variant(lo, c)["variant"] == "split" and M.variant(hi, c)["variant"] == "waves8"
        w = M.variant(M.f4_rows(c), c)
        assert w["variant"] == "waves8" and w["tiles"] > w["workgroups"] == c and M.variant(129, c)["variant"] == "split"
    assert M.wide_chunks(300) == [(0, 300)]                                                          # W0, W3
    assert M.wide_chunks(M.W_ROWS) == [(0, 65536), (65536, 129)]                                     # W1, W2
    for w0, w in M.W_WINDOWS:
        assert w0 + w <= M.W_ROWS
    assert M.W_WINDOWS[0][0] < 65536 < sum(M.W_WINDOWS[0]) and M.W_WINDOWS[1] == (65536, 129)
