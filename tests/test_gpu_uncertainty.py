"""GPU: csrc/pinn_uncertainty.hip against the float64 numpy backend of pinn_amd.uncertainty.

Exact (bytes): every integer count, z per row, every quantile and rank, n and n_skipped, the monitor's lo / hi / flags and its
whole state after every chunk.  The cases are the ones a select or a tiled pass can get wrong (row counts around the tile
and at the block cap, ties, rank edges, every bit of the key, the limits), not workload sizes.

Float sums (moments, nll, crps): the referee is the host backend's per-row terms added with math.fsum, the gate
(u + d + 2) 2^-53 sum|t_i|, d the depth of the device's summation from the exported tile and block constants
(uncertainty_cases.sum_depth), u the per-term allowance for log, erfc and exp.  u was measured, not assumed: on the 1500 rows
of `measured` (standard normal z, v in 1.28 .. 8) the largest distance from an mpmath referee at 50 digits, in float64
spacings, was
    device (MI355X, ROCm's device library)   Phi 12.451   nll 1.518   crps 6.844
    host (numpy, math.erfc)                  Phi 12.451   nll 1.518   crps 5.792
and u = 2 x the largest of them = 24.9, taken as 25.  (Phi leads on both sides alike: its argument -z / sqrt 2 is rounded
twice and erfc's condition number in the lower tail is z^2 + 1; the libraries themselves are within a few spacings.)  The
per-row float outputs are gated by the same u, device against host; the largest such distance seen over every case of this
file was 9 spacings (crps, 2.1e6 rows).
"""
import math

import numpy as np
import pytest
import torch

import uncertainty_cases as C
from pinn_amd import _lib, risk, uncertainty as U

pytestmark = pytest.mark.gpu

U_ULP = 25.0                                # the measured allowance of the docstring

GROUPS = dict(normal=[0], **{k: list(v) for k, v in risk.FAULT_RANGE_MAP.items()})
TILE, CAP = _lib.UNC_TILE, _lib.UNC_MAX_BLOCKS


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def same_bytes(a, b):
    a, b = host(a), host(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_score(A, row_index=None, **kw):
    """Device and host on the same rows: counts and z to the byte, float sums and per-row terms inside the gate."""
    rh, ph = U.score_uncertainty(A, row_index=row_index, backend="host", per_row=True, **kw)
    rd, pd = U.score_uncertainty(dev(A), row_index=dev(row_index), backend="device", per_row=True, **kw)
    assert list(rh) == list(rd)
    n_pos = A.shape[0] if row_index is None else len(row_index)
    d = C.sum_depth(n_pos, TILE, CAP)
    assert same_bytes(pd["z"], ph["z"])
    valid = ~np.isnan(ph["z"])
    for key in ("pit", "nll", "crps"):
        x = host(pd[key])
        assert np.array_equal(np.isnan(x), ~valid), key
        dist = C.ulp_distance(x[valid], ph[key][valid])
        print("per-row %s: largest device-host distance %.2f spacings" % (key, dist.max() if dist.size else 0.0))
        assert (dist <= U_ULP).all(), (key, dist.max())
    for name in rh:
        H, D = rh[name], rd[name]
        assert (D.n, D.n_skipped) == (H.n, H.n_skipped)
        assert same_bytes(D.hits, H.hits) and same_bytes(D.pit, H.pit)
    # the sums, group by group, against fsum of the host's own terms
    Hrows = U._HostRows(A, *U._columns(kw.get("columns"), kw.get("groups") is not None), U._group_table(kw.get("groups"))[1],
                        list(kw.get("var_model", (1.0, 1.0, 0.0))), row_index)
    terms = dict(zip(U.SUM_NAMES, [np.ones(Hrows.n), Hrows.r, Hrows.r * Hrows.r, Hrows.s, Hrows.v, Hrows.z, Hrows.z * Hrows.z, ph["nll"], ph["crps"]]))
    for g, name in enumerate(rh):
        m = Hrows.g == g
        for key, t in terms.items():
            ref = math.fsum(t[m].tolist())
            gate = (U_ULP + d + 2) * 2.0 ** -53 * math.fsum(np.abs(t[m]).tolist())
            got = rd[name].sums[key]
            print("%s / %s: |device - fsum| = %.3g, gate %.3g" % (name, key, abs(got - ref), gate))
            assert abs(got - ref) <= gate or (not math.isfinite(ref) and (got == ref or (got != got and ref != ref))), (name, key, got, ref)
    return rd


def check_quantiles(A, row_index=None, **kw):
    qh = U.conformal_quantiles(A, row_index=row_index, backend="host", **kw)
    qd = U.conformal_quantiles(dev(A), row_index=dev(row_index), backend="device", **kw)
    assert same_bytes(qd.q, qh.q), (qd.q, qh.q)
    assert same_bytes(qd.rank, qh.rank) and same_bytes(qd.n, qh.n) and qd.n_skipped == qh.n_skipped
    return qd


@pytest.fixture(scope="module")
def measured():
    A = C.results_array(1500, 11)
    _, ph = U.score_uncertainty(A, backend="host", per_row=True)
    H = U._HostRows(A, [C.Y_TRUE, C.Y_PRED, C.ALE, C.EPI], -1, None, [1.0, 1.0, 0.0])
    return A, ph, C.mp_terms(H.z, H.v, H.s)


def test_the_measured_allowance_still_holds(measured):
    """The figures of the module docstring: distance of the per-row Phi, nll and crps from mpmath at 50 digits."""
    A, ph, ref = measured
    _, pd = U.score_uncertainty(dev(A), backend="device", per_row=True)
    worst = 0.0
    for key, r in zip(("pit", "nll", "crps"), ref):
        dd, dh = C.mp_ulp_distance(host(pd[key]), r).max(), C.mp_ulp_distance(ph[key], r).max()
        print("MEASURED %s: device %.3f host %.3f spacings from mpmath" % (key, dd, dh))
        worst = max(worst, dd, dh)
    print("MEASURED u = 2 x %.3f" % worst)
    assert 2.0 * worst <= U_ULP


@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1])
def test_score_around_the_tile(n):
    A = C.results_array(n, 20 + n % 7)
    if n > 100:
        A = C.spoil(A, 21)
    check_score(A, groups=GROUPS)
    one = check_score(A)["all"]
    assert one.n + one.n_skipped == n


@pytest.fixture(scope="module")
def capped():
    """More tiles than workgroups: 5 narrow columns so that the array stays small."""
    n = TILE * CAP + 5
    rng = np.random.default_rng(30)
    A = np.empty((n, 5))
    A[:, 1] = rng.normal(3.0, 0.5, n)
    A[:, 2] = rng.uniform(0.8, 2.0, n)
    A[:, 3] = rng.uniform(0.8, 2.0, n)
    A[:, 0] = A[:, 1] + np.sqrt(A[:, 2] ** 2 + A[:, 3] ** 2) * rng.normal(size=n)
    A[:, 4] = rng.integers(0, 4, n)
    A[::1001, 2] = np.nan
    return A


def test_score_at_the_block_cap(capped):
    assert -(-capped.shape[0] // TILE) > CAP
    check_score(capped, groups={"a": [0], "b": [1, 2]}, columns=(0, 1, 2, 3, 4), levels=(0.5, 0.9), bins=8)


def test_quantiles_at_the_block_cap(capped):
    check_quantiles(capped, groups={"a": [0], "b": [1, 2]}, columns=(0, 1, 2, 3, 4), levels=(1e-6, 0.5, 0.9, 0.999999))
    check_quantiles(capped, kind="z", conformal=False, columns=(0, 1, 2, 3), levels=(0.25,))


@pytest.mark.parametrize("kind", ["abs_z", "z"])
@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1])
def test_quantiles_around_the_tile(n, kind):
    A = C.results_array(n, 40 + n % 5)
    if n > 100:
        A = C.spoil(A, 41)
    check_quantiles(A, kind=kind, groups=GROUPS, levels=(0.1, 0.5, 0.9, 0.99))
    check_quantiles(A, kind=kind, conformal=False, levels=(0.5,))


def test_ties_and_rank_edges():
    A = C.results_array(600, 50)
    A[:, C.LABEL] = 0
    A[:200, C.ALE], A[:200, C.EPI], A[:200, C.Y_PRED], A[:200, C.Y_TRUE] = 3.0, 4.0, 1.0, 11.0              # a run of 200 ties: z = 2 exactly
    A[200:300, C.LABEL] = 1
    A[200:300, C.ALE], A[200:300, C.EPI], A[200:300, C.Y_PRED], A[200:300, C.Y_TRUE] = 3.0, 4.0, 1.0, 6.0      # all scores equal: z = 1
    A[300:310, C.LABEL] = 2
    A[300:310, C.ALE] = np.nan                                       # a group whose rows are all invalid; group "nobody" has no row
    groups = {"ties": [0], "equal": [1], "invalid": [2], "nobody": [3]}
    m = A[:, C.LABEL] == 0
    sc = np.sort(np.abs((A[m, C.Y_TRUE] - A[m, C.Y_PRED]) / np.sqrt(A[m, C.ALE] * A[m, C.ALE] + A[m, C.EPI] * A[m, C.EPI])))
    first = int(np.searchsorted(sc, 2.0, "left"))
    assert (sc[first:first + 200] == 2.0).all() and 0 < first and first + 200 < sc.size
    n0 = sc.size
    # ranks (conformal=False: k = ceil(n level)): 1, the first, an inner and the last of the run of ties, n
    levels = tuple((k - 0.5) / n0 for k in (1, first + 1, first + 100, first + 200, n0))
    Q = check_quantiles(A, groups=groups, levels=levels, conformal=False)
    assert Q.rank[0].tolist() == [1, first + 1, first + 100, first + 200, n0]
    assert Q.q[0, 1] == Q.q[0, 2] == Q.q[0, 3] and Q.q[0, 0] == sc[0] and Q.q[0, 4] == sc[-1]
    assert (Q.q[1] == 1.0).all() and np.isnan(Q.q[2]).all() and np.isnan(Q.q[3]).all() and Q.n.tolist() == [n0, 100, 0, 0]
    Q = check_quantiles(A, groups=groups, levels=(0.5, 1.0), conformal=True)
    assert np.isinf(Q.q[0, 1]) and Q.rank[0, 1] == n0 + 1 and np.isinf(Q.q[1, 1]) and Q.rank[2].tolist() == [0, 0]
    # more equal scores than the select gathers: every byte pass runs, and the rank stays inside one bin to the end
    B = np.repeat(A[200:201], 3 * _lib.UNC_COLLECT + 7, axis=0)
    B[::5, C.Y_TRUE] = 1.0                                            # and a second value, z = 0, below it
    Q = check_quantiles(B, levels=(0.1, 0.2, 0.2 + 1e-9, 0.9, 1.0), conformal=False)
    assert Q.q[0].tolist() == [0.0, 0.0, 1.0, 1.0, 1.0]


@pytest.mark.parametrize("part", range(4))
def test_every_bit_of_the_key_discriminates(part):
    """For each of 16 bit positions a group of 300 values whose keys agree above the bit and differ from it down, with ranks on
    both sides of the split: G = 16 with Q = 4."""
    bits = list(range(part * 16, part * 16 + 16))
    assert 300 > _lib.UNC_COLLECT                                     # more values than the select gathers: the byte passes have to split them
    A = C.bit_split_array(bits, 300, 60 + part)
    Q = check_quantiles(A, kind="column", column=0, conformal=False, groups={"bit%d" % b: [i] for i, b in enumerate(bits)},
                        columns=(0, 0, 0, 0, 1), levels=(0.02, 0.35, 0.65, 0.98))
    for g, b in enumerate(bits):
        k = [C.double_to_key(x) for x in Q.q[g]]
        assert (k[0] >> b) & 1 == 0 and (k[3] >> b) & 1 == 1, b


def test_key_map_special_values():
    vals = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, 1.0, -1.0, 1.7e308, -1.7e308, np.inf, -np.inf, np.nan] * 3)
    A = np.zeros((vals.size, 3))
    A[:, 0] = vals
    lv = tuple((k + 0.5) / 33.0 for k in range(0, 33, 5)) + (1.0,)
    Q = check_quantiles(A, kind="column", column=0, conformal=False, columns=(0, 0, 0, 0), levels=lv)
    assert Q.n[0] == 33 and Q.n_skipped == 9                          # +-inf and NaN are not valid
    # huge |z| from a tiny v, z = +-inf from an overflowing difference, negative z
    B = C.results_array(300, 70)
    B[:50, C.ALE], B[:50, C.EPI] = 1e-160, 0.0
    B[50:60, C.ALE], B[50:60, C.EPI] = 1e-170, 0.0                    # v underflows to 0: not valid
    B[60, C.Y_TRUE], B[60, C.Y_PRED] = 1.5e308, -1.5e308
    B[61, C.Y_TRUE], B[61, C.Y_PRED] = -1.5e308, 1.5e308
    for kind in ("abs_z", "z"):
        Q = check_quantiles(B, kind=kind, conformal=False, levels=(0.01, 0.1, 0.5, 0.9, 0.99, 1.0))
        assert Q.n_skipped == 10 and np.isinf(Q.q[0, -1])
    rh, ph = U.score_uncertainty(B, bins=5, backend="host", per_row=True)
    rd, pd = U.score_uncertainty(dev(B), bins=5, backend="device", per_row=True)
    assert same_bytes(pd["z"], ph["z"]) and same_bytes(rd["all"].hits, rh["all"].hits) and same_bytes(rd["all"].pit, rh["all"].pit)
    assert (rd["all"].n, rd["all"].n_skipped) == (rh["all"].n, rh["all"].n_skipped) == (290, 10)


def test_limits_and_inputs():
    A = C.spoil(C.results_array(3000, 80, ld=30, n_labels=64), 81)
    A[:, 25] = A[:, C.LABEL]
    A[:, 21:25] = A[:, [C.Y_TRUE, C.Y_PRED, C.ALE, C.EPI]]
    cols = (21, 22, 23, 24, 25)
    g8 = {"g%d" % i: [i, i + 8, 63 - i] for i in range(8)}
    lv8 = (0.05, 0.2, 0.4, 0.5, 0.6, 0.8, 0.95, 0.999)
    Q = check_quantiles(A, groups=g8, levels=lv8, columns=cols)        # G = 8 with Q = 8; most labels lie outside the table's groups
    assert Q.n_skipped > 1500
    g16 = {"g%d" % i: [4 * i, 4 * i + 1] for i in range(16)}
    check_quantiles(A, groups=g16, levels=(0.1, 0.5, 0.9, 0.99), columns=cols, kind="z")
    check_score(A, groups=g16, columns=cols, var_model=(0.5, 2.0, 0.01))
    ridx = np.concatenate([np.arange(0, 3000, 2), [7, 7, 7, -1, 3000, 10 ** 12, 2999], np.arange(2999, 0, -3)]).astype(np.int64)
    Q = check_quantiles(A, row_index=ridx, groups=g8, levels=lv8, columns=cols)
    check_score(A, row_index=ridx, groups=g8, columns=cols)
    # the same rows with and without a gather list
    full = np.arange(3000, dtype=np.int64)
    a = U.conformal_quantiles(dev(A), groups=g8, levels=lv8, columns=cols, backend="device")
    b = U.conformal_quantiles(dev(A), row_index=dev(full), groups=g8, levels=lv8, columns=cols, backend="device")
    assert same_bytes(a.q, b.q) and same_bytes(a.rank, b.rank) and same_bytes(a.n, b.n)
    ra, pa = U.score_uncertainty(dev(A), groups=g8, columns=cols, backend="device", per_row=True)
    rb, pb = U.score_uncertainty(dev(A), row_index=dev(full), groups=g8, columns=cols, backend="device", per_row=True)
    for name in ra:
        assert ra[name].sums == rb[name].sums and same_bytes(ra[name].pit, rb[name].pit)
    assert all(same_bytes(pa[k], pb[k]) for k in pa)
    # a strided view: ld > the columns of the view
    V = dev(A)[:, :26]
    c = U.conformal_quantiles(V, groups=g8, levels=lv8, columns=cols, backend="device")
    assert same_bytes(a.q, c.q)


def test_the_same_call_twice_gives_the_same_bytes(capped):
    Ad = dev(capped)
    kw = dict(groups={"a": [0], "b": [1, 2]}, columns=(0, 1, 2, 3, 4))
    r1, p1 = U.score_uncertainty(Ad, backend="device", per_row=True, **kw)
    r2, p2 = U.score_uncertainty(Ad, backend="device", per_row=True, **kw)
    for name in r1:
        assert r1[name].sums == r2[name].sums and same_bytes(r1[name].hits, r2[name].hits) and same_bytes(r1[name].pit, r2[name].pit)
    assert all(same_bytes(p1[k], p2[k]) for k in p1)
    q1 = U.conformal_quantiles(Ad, levels=(0.1, 0.9), backend="device", **kw)
    q2 = U.conformal_quantiles(Ad, levels=(0.1, 0.9), backend="device", **kw)
    assert same_bytes(q1.q, q2.q) and same_bytes(q1.rank, q2.rank)


def run_monitors(chunks, learn, **kw):
    mh = U.UncertaintyMonitor(backend="host", **kw)
    md = U.UncertaintyMonitor(backend="device", **kw)
    for ch, lr in zip(chunks, learn):
        uh, ud = mh.update(ch, learn=lr), md.update(dev(ch), learn=lr)
        assert same_bytes(ud.lo, uh.lo) and same_bytes(ud.hi, uh.hi) and same_bytes(ud.z, uh.z) and same_bytes(ud.miss, uh.miss)
        assert md.state_words().tobytes() == mh.state_words().tobytes()
    return mh, md


@pytest.mark.parametrize("gamma", [0.0, 0.5])
def test_monitor_small_window(gamma):
    """Window 16: the ring before it is full, wrap-around, ties, a chunk with no valid row, learn=False, chunk sizes 1 and 7,
    and with gamma > 0 alpha at both clips."""
    A = C.spoil(C.results_array(300, 7, understate=1.5), 8, share=0.1)
    A[100:130, C.Y_TRUE] += 1000.0
    A[200:300, C.ALE] *= 10.0 ** (1 + np.arange(100) // 10)
    A[40:44] = A[39]
    A[60:67, C.Y_TRUE] = np.nan
    cuts = [0, 1, 8, 15, 50, 60, 67, 100, 130, 150] + list(range(200, 301, 10))
    chunks = [A[a:b] for a, b in zip(cuts, cuts[1:])]
    learn = [True] * 6 + [False] + [True] * (len(chunks) - 7)
    mh, md = run_monitors(chunks, learn, level=0.9, window=16, gamma=gamma, alpha_min=0.02, alpha_max=0.3)
    assert mh.n_valid > 200 and md.q == mh.q and md.alpha == mh.alpha


def test_monitor_full_chunks_and_init():
    A = C.spoil(C.results_array(3 * 2048 + 100, 90, understate=2.0), 91)
    init = U.conformal_quantiles(A[:500], levels=(0.9,), backend="host")
    chunks = [A[:2048], A[2048:4096], A[4096:], A[:5000]]             # the last is taken 2048 rows at a time by both backends
    run_monitors(chunks, [True, True, False, True], level=0.9, window=4096, init=init)
    run_monitors(chunks[:2], [True, True], level=0.8, window=1000, gamma=0.05)
    lo_h, hi_h = U.conformal_band(A, init.q[0, 0], backend="host")
    lo_d, hi_d = U.conformal_band(dev(A), init.q[0, 0], backend="device")
    assert same_bytes(lo_d, lo_h) and same_bytes(hi_d, hi_h)
