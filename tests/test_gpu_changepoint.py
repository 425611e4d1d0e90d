"""GPU: the device backend of pinn_amd.changepoint (csrc/pinn_changepoint.hip) against the numpy backend and the brute force.

Kind "mean": F, change points, statuses and evaluation counts equal the numpy backend's to the bit (only + - * / and
comparisons are in play, in a fixed order, contraction off).  Kind "meanvar": change points equal on the margin-filtered
cases; F within an allowance for `log` that was measured: over the cases of test_meanvar_against_numpy the largest distance
of either backend's F from an np.longdouble evaluation of the same partition (direct two-pass sums) was 3.52e-13 of the
partition's scale, the sum of the absolute terms len |log v| + SS / v + penalty (device 3.52e-13, numpy 3.52e-13: the prefix
sums' rounding divided by a variance near var_floor, shared by both); the test grants twice that between the two backends,
which were 1.45e-17 of the scale apart at most.  The prefix tile is 256 rows and the step block 64: the sizes below sit on both
seams."""
import numpy as np
import pytest
import torch

import changepoint_cases as C
from pinn_amd import changepoint as cp

pytestmark = pytest.mark.gpu

MEANVAR_MEASURED = 3.52e-13             # see the docstring; printed again by test_meanvar_against_numpy


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stepped(seed, n, D, every=None, level=3.0):
    """Gaussian rows with a change of mean every `every` rows (default: three pieces)."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, D)) + level
    every = max(n // 3, 1) if every is None else every
    for k, lo in enumerate(range(every, n, every)):
        X[lo:] += (2.5 if k % 2 == 0 else -2.0) * (1.0 + 0.1 * np.arange(D))
    return X


def both(A, d_A, **kw):
    return cp.segment(d_A, backend="device", **kw), cp.segment(A, backend="numpy", **kw)


def same(d, h, evals=True):
    assert np.array_equal(d.status, h.status)
    assert np.array_equal(d.F, h.F, equal_nan=True), (d.F, h.F)
    assert len(d.change_points) == len(h.change_points)
    for a, b in zip(d.change_points, h.change_points):
        assert np.array_equal(a, b), (a, b)
    if evals:
        assert np.array_equal(d.evaluations, h.evaluations), (d.evaluations, h.evaluations)


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 129, 255, 256, 257, 513, 1023, 1024, 1025, 2049))
def test_mean_is_the_numpy_backend_to_the_bit(n):
    for D, min_len in ((1, 1), (4, 2), (8, 7)):
        A, cols = C.results_like(stepped(n + D, n, D), ld=20, first=3)
        d_A = dev(A)
        for prune, max_len, block in ((True, None, None), (False, None, None), (True, 20, None), (True, 150, None), (False, 150, 16),
                                      (True, None, 16)):
            if max_len is not None and max_len < min_len:
                continue
            d, h = both(A, d_A, features=cols, penalty=3.0 * (D + 1), min_len=min_len, max_len=max_len, prune=prune, _block_steps=block)
            same(d, h)
            if n >= 129 and max_len is None:
                assert d.n_change_points >= 2
    assert cp.segment(d_A, features=cols, backend="device").penalty == cp.default_penalty(n, 8, "mean")


def test_penalties_segments_gather_and_scaling_in_one_call():
    """Five penalties, three segments of unequal length (one shorter than 2 min_len), a gather list with an index outside
    the array in a fourth, mu and sigma given: each (segment, penalty) pair equals the numpy backend and the single calls."""
    X = np.concatenate([stepped(1, 700, 4), stepped(2, 9, 4), stepped(3, 300, 4), stepped(4, 200, 4)])
    A, cols = C.results_like(X, ld=20, first=8)
    d_A = dev(A)
    starts = [0, 700, 709, 1009]
    idx = np.arange(X.shape[0])[::-1].copy()
    idx = np.concatenate([np.arange(1009), idx[:200]])
    idx[1100] = X.shape[0] + 5
    mu, sigma = X[:200].mean(axis=0), X[:200].std(axis=0)
    pens = [0.0, 4.0, 15.0, 60.0, 1e4]
    kw = dict(features=cols, min_len=5, mu=mu, sigma=sigma, row_index=idx, seg_starts=starts)
    d_path = cp.penalty_path(d_A, pens, backend="device", **kw)
    h_path = cp.penalty_path(A, pens, backend="numpy", **kw)
    assert np.array_equal(d_path.n_change_points, h_path.n_change_points) and np.array_equal(d_path.F, h_path.F)
    assert np.array_equal(d_path.evaluations, h_path.evaluations)
    for i, p in enumerate(pens):
        d, h = both(A, d_A, penalty=p, **kw)
        same(d, h)
        assert list(d.status) == [0, 0, 0, cp.BAD_ROW] and d.change_points[1].size == 0
        assert np.array_equal(np.sort(np.concatenate(d.change_points)), d_path.change_points[i])
    assert d_path.n_change_points[0] > d_path.n_change_points[2] >= 4 and d_path.n_change_points[-1] == 0


def raw_call(d_A, cols, pens, starts=None, **kw):
    """The outputs of one device call as they come from the kernels."""
    pb = cp._Problem(cols, kw.pop("kind", "mean"), kw.pop("min_len", 2), None, None, None, True, cp.DEFAULT_VAR_FLOOR)
    n = d_A.shape[0]
    s, b = cp._bounds(starts, n)
    return cp._device_segment(d_A, pb, pens, None, s, b, cp_cap=16)


def test_a_pairs_bytes_do_not_depend_on_the_rest_of_the_call():
    X = np.concatenate([stepped(5, 520, 3), stepped(6, 300, 3)])
    A, cols = C.results_like(X)
    d_A, d_B = dev(A), dev(A[:520])
    one = raw_call(d_B, cols, [9.0])
    again = raw_call(d_B, cols, [9.0])
    many = raw_call(d_A, cols, [1.0, 9.0, 30.0], starts=[0, 520])
    for k in range(3):
        assert np.array_equal(one[k], again[k]) and np.array_equal(one[k][0, 0], many[k][0, 1])
    assert np.array_equal(one[3][0][0], again[3][0][0]) and np.array_equal(one[3][0][0], many[3][0][1])
    for kind in ("mean", "meanvar"):
        a = raw_call(d_A, cols, [2.0, 9.0], starts=[0, 520], kind=kind)
        b = raw_call(d_A, cols, [2.0, 9.0], starts=[0, 520], kind=kind)
        assert all(np.array_equal(a[k], b[k]) for k in range(3)) and all(np.array_equal(x, y) for s in range(2) for x, y in zip(a[3][s], b[3][s]))


def scale_of(Z, taus, beta, kind, var_floor):
    """(the partition's penalised cost, the sum of its absolute terms), both in np.longdouble from the rows themselves."""
    edges = [0] + [int(t) for t in taus] + [Z.shape[0]]
    total, scale = np.longdouble(beta) * len(taus), np.longdouble(beta) * len(taus)
    for a, b in zip(edges, edges[1:]):
        x = np.asarray(Z[a:b], dtype=np.longdouble)
        ss = ((x - x.mean(axis=0)) ** 2).sum(axis=0)
        if kind == "mean":
            total, scale = total + ss.sum(), scale + ss.sum()
        else:
            ln = np.longdouble(b - a)
            v = np.maximum(ss / ln, np.longdouble(var_floor))
            total, scale = total + (ln * np.log(v) + ss / v).sum(), scale + (np.abs(ln * np.log(v)) + ss / v).sum()
    return total, scale


def test_meanvar_against_numpy():
    cases = [(c["Z"], c["beta"], c["min_len"], c["max_len"], C.VAR_FLOOR) for c in C.cached_host_cases()[0] if c["kind"] == "meanvar"]
    for n, D, min_len in ((300, 3, 2), (513, 8, 5), (1100, 4, 20)):
        cases.append((stepped(n, n, D), cp.default_penalty(n, D, "meanvar"), min_len, None, cp.DEFAULT_VAR_FLOOR))
    far_dev = far_np = 0.0
    checks = []
    for Z, beta, min_len, max_len, floor in cases:
        kw = dict(features=list(range(Z.shape[1])), penalty=beta, kind="meanvar", min_len=min_len, max_len=max_len, var_floor=floor)
        d, h = both(Z, dev(Z), **kw)
        assert np.array_equal(d.change_points[0], h.change_points[0]) and np.array_equal(d.status, h.status)
        exact, scale = scale_of(Z, h.change_points[0], beta, "meanvar", floor)
        far_dev = max(far_dev, float(abs(np.longdouble(d.F[0]) - exact) / scale))
        far_np = max(far_np, float(abs(np.longdouble(h.F[0]) - exact) / scale))
        checks.append((abs(d.F[0] - h.F[0]), float(scale)))
    worst = max(gap / s for gap, s in checks)
    print("distance to np.longdouble / scale: device %.3g, numpy %.3g; |device - numpy| / scale at most %.3g; granted %.3g"
          % (far_dev, far_np, worst, 2 * MEANVAR_MEASURED))
    for gap, s in checks:
        assert gap <= 2 * MEANVAR_MEASURED * s


@pytest.mark.parametrize("block", (1, None), ids=("block1", "block64"))
def test_against_the_brute_force(block):
    for c in C.cached_host_cases()[0]:
        d = cp.segment(dev(c["Z"]), features=list(range(c["D"])), penalty=c["beta"], kind=c["kind"], min_len=c["min_len"], max_len=c["max_len"],
                       var_floor=C.VAR_FLOOR, backend="device", _block_steps=block)
        assert tuple(d.change_points[0]) == c["taus"], (c["n"], c["D"], c["kind"], c["min_len"], c["max_len"])
        assert abs(d.F[0] - c["best"]) <= C.rounding_bound(c["Z"], c["beta"], c["kind"]) and d.status[0] == 0
    g = C.golden_case()
    d = cp.segment(dev(g["Z"]), features=[0], penalty=g["penalty"], kind=g["kind"], min_len=g["min_len"], var_floor=g["var_floor"],
                   backend="device", _block_steps=block)
    assert list(d.change_points[0]) == g["change_points"]


@pytest.mark.parametrize("prune", (True, False))
def test_a_segment_that_needs_further_queued_launches_equals_the_host(prune):
    A, cols = C.results_like(stepped(9, 600, 2, every=170))
    d_A = dev(A)
    kw = dict(features=cols, min_len=3, prune=prune)              # the BIC penalty: the three true changes
    h = cp.segment(A, backend="numpy", **kw)
    whole = cp.segment(d_A, backend="device", **kw)
    for cap in (1, 2000, 30000):                                # a launch per block, a few launches, two or three
        same(cp.segment(d_A, backend="device", _launch_evals=cap, **kw), h)
    same(whole, h)
    assert h.evaluations[0] > 30000 and h.n_change_points == 3


def test_more_change_points_than_the_first_capacity():
    X = np.zeros((400, 1))
    X[(np.arange(400) // 4) % 2 == 1] = 5.0
    d, h = both(X, dev(X), features=[0], penalty=1.0, min_len=2)
    same(d, h)
    assert d.n_change_points == 99 and d.status[0] == 0


@pytest.mark.parametrize("chunk", (32, 50))
def test_the_monitor_follows_segment_on_its_window(chunk):
    rng = np.random.default_rng(2)
    X = rng.normal(size=(500, 2))
    X[140:] += 3.0
    X[333:] -= 4.0
    A, cols = C.results_like(X, ld=6, first=1)
    d_A = dev(A)
    mon = cp.ChangeMonitor(128, features=cols, penalty=9.0, min_len=3, backend="device")
    reported = []
    for lo in range(0, 500, chunk):
        found, new = mon.update(d_A[lo:lo + chunk])
        hi = min(lo + chunk, 500)
        w0 = max(hi - 128, 0)
        ref = cp.segment(A[w0:hi], features=cols, penalty=9.0, min_len=3, backend="numpy")
        assert np.array_equal(found, ref.change_points[0] + w0) and mon.F == ref.F[0] and mon.evaluations == ref.evaluations[0]
        assert np.array_equal(mon.window_rows(), X[w0:hi])
        reported += list(new)
    assert reported == [140, 333]
    wide = cp.ChangeMonitor(4096, features=[0, 1], penalty=12.0, min_len=2, backend="device")      # the longest window, filled at once
    Y = stepped(8, 4096, 2)
    found, _ = wide.update(dev(Y))
    ref = cp.segment(Y, features=[0, 1], penalty=12.0, min_len=2, backend="numpy")
    assert np.array_equal(found, ref.change_points[0]) and wide.F == ref.F[0]
