"""CPU: the numpy backend of pinn_amd.changepoint against a brute force over every admissible partition (changepoint_cases.py),
the delayed pruning rule, recording segments, short segments and bad rows."""
import numpy as np
import pytest

import changepoint_cases as C
from pinn_amd import changepoint as cp


def solve(Z, beta, kind, min_len, max_len=None, prune=True, block=None, **kw):
    return cp.segment(Z, features=list(range(Z.shape[1])), penalty=beta, kind=kind, min_len=min_len, max_len=max_len, prune=prune,
                      var_floor=C.VAR_FLOOR, backend="numpy", _block_steps=block, **kw)


def test_at_most_a_tenth_of_the_cases_is_dropped_for_a_near_tie():
    kept, generated, dropped = C.cached_host_cases()
    print("generated %d, dropped %d" % (generated, dropped))
    assert generated == 9 * 3 * (3 + 2) * 2 and dropped <= generated // 10
    assert {c["kind"] for c in kept} == {"mean", "meanvar"} and {c["min_len"] for c in kept} == {1, 2, 3}
    assert any(len(c["taus"]) >= 2 for c in kept) and any(c["max_len"] for c in kept)


@pytest.mark.parametrize("prune", (True, False))
@pytest.mark.parametrize("block", (1, 3, None), ids=("block1", "block3", "block64"))
def test_numpy_backend_equals_the_brute_force(prune, block):
    """Change points equal; F within the rounding bound of the case.  block1 is the per-step recursion: with prune the
    delayed rule acts at every step, with the default block these sizes are one block and nothing leaves the list."""
    worst = 0.0
    for c in C.cached_host_cases()[0]:
        s = solve(c["Z"], c["beta"], c["kind"], c["min_len"], c["max_len"], prune, block)
        assert tuple(s.change_points[0]) == c["taus"], (c["n"], c["D"], c["kind"], c["min_len"], c["max_len"])
        assert s.status[0] == 0
        bound = C.rounding_bound(c["Z"], c["beta"], c["kind"])
        worst = max(worst, abs(s.F[0] - c["best"]) / bound)
        assert abs(s.F[0] - c["best"]) <= bound
    print("worst |F - brute force| / bound: %.3g" % worst)


def test_immediate_pruning_loses_the_optimum_and_the_delayed_rule_does_not():
    """tests/golden/changepoint_immediate_pruning.json: min_len = 2, kind "meanvar"; dropping a candidate at the step of
    its test returns a worse partition, dropping it min_len steps later the brute force's."""
    g = C.golden_case()
    Z, beta = g["Z"], g["penalty"]
    best, taus, second, _ = C.brute_force(Z, beta, g["kind"], g["min_len"], None, g["var_floor"])
    assert list(taus) == g["change_points"] and second - best > 1e-3
    P = cp._host_prefix(Z)
    F_now, last_now, _ = cp._host_solve(P, beta, g["kind"], g["min_len"], 0, g["var_floor"], True, 1, immediate=True)
    assert F_now[-1] - best > 1e-3 and cp._walk(last_now, Z.shape[0]) != g["change_points"]
    for block in (1, 2, 5, None):
        s = cp.segment(Z, features=[0], penalty=beta, kind=g["kind"], min_len=g["min_len"], var_floor=g["var_floor"], backend="numpy",
                       _block_steps=block)
        assert list(s.change_points[0]) == g["change_points"] and abs(s.F[0] - best) <= C.rounding_bound(Z, beta, g["kind"], g["var_floor"])


@pytest.mark.parametrize("kind,min_len", (("mean", 1), ("mean", 7), ("meanvar", 2), ("meanvar", 5)))
def test_pruning_changes_the_work_and_nothing_else(kind, min_len):
    rng = np.random.default_rng(5)
    X = rng.normal(size=(700, 3))
    for a, b in ((150, 1.5), (320, -2.0), (480, 1.0)):
        X[a:] += b
    saved = []
    for block in (1, 16, None):
        on = solve(X, cp.default_penalty(700, 3, kind), kind, min_len, prune=True, block=block)
        off = solve(X, cp.default_penalty(700, 3, kind), kind, min_len, prune=False, block=block)
        assert np.array_equal(on.change_points[0], off.change_points[0]) and on.F[0] == off.F[0]
        assert on.evaluations[0] <= off.evaluations[0]
        saved.append(off.evaluations[0] / on.evaluations[0])
        assert np.all(np.abs(on.change_points[0][:, None] - np.array([150, 320, 480])).min(axis=0) <= 3)
    print("evaluations saved by pruning, blocks of 1, 16, 64 steps: %s" % np.round(saved, 2))
    assert saved[0] > 2.0 and saved[2] > 1.5                    # three changes in 700 rows: the candidates before a change leave


def test_a_recording_cut_by_seg_starts_equals_the_separate_calls():
    X = np.concatenate([C.shifted_rows(s, n, 2, level=5.0 * s) for s, n in ((1, 90), (2, 300), (3, 5), (4, 70))])
    starts = [0, 90, 390, 395]
    for kind, min_len in (("mean", 3), ("meanvar", 4)):
        whole = solve(X, 6.0, kind, min_len, seg_starts=starts)
        for i, (lo, hi) in enumerate(zip(starts, starts[1:] + [X.shape[0]])):
            part = solve(X[lo:hi], 6.0, kind, min_len)
            assert np.array_equal(whole.change_points[i], part.change_points[0] + lo)
            assert whole.F[i] == part.F[0] and whole.evaluations[i] == part.evaluations[0]
        assert whole.change_points[2].size == 0                 # 5 rows < 2 min_len
        assert np.array_equal(whole.seg_starts, np.unique(np.concatenate([starts] + whole.change_points)))
        labels = cp.labels_from_segments(whole)
        assert labels.shape == (X.shape[0],) and labels[0] == 0 and labels[-1] == whole.seg_starts.size - 1


@pytest.mark.parametrize("min_len", (2, 3, 9))
def test_a_segment_shorter_than_two_min_len_has_no_change_point(min_len):
    X = C.shifted_rows(7, 2 * min_len - 1, 2)
    X[min_len:] += 50.0
    for kind in ("mean", "meanvar"):
        s = solve(X, 0.0, kind, min_len)
        assert s.change_points[0].size == 0 and s.status[0] == 0 and np.isfinite(s.F[0])
    s = solve(X[:min_len - 1], 0.0, "mean", min_len)            # shorter than min_len itself: no admissible partition
    assert s.change_points[0].size == 0 and s.status[0] == cp.INFEASIBLE and s.F[0] == np.inf


def test_a_bad_row_flags_its_segment_only():
    X = np.concatenate([C.shifted_rows(s, 60, 2) for s in (1, 2, 3)])
    starts = [0, 60, 120]
    clean = solve(X, 5.0, "mean", 2, seg_starts=starts)
    for value in (np.nan, np.inf):
        Y = X.copy()
        Y[75, 1] = value
        s = solve(Y, 5.0, "mean", 2, seg_starts=starts)
        assert list(s.status) == [0, cp.BAD_ROW, 0] and np.isnan(s.F[1]) and s.change_points[1].size == 0 and s.evaluations[1] == 0
        for i in (0, 2):
            assert np.array_equal(s.change_points[i], clean.change_points[i]) and s.F[i] == clean.F[i]
    idx = np.arange(180)
    idx[130] = 10 ** 6                                          # a gather index outside the array reads nothing
    s = solve(X, 5.0, "mean", 2, seg_starts=starts, row_index=idx)
    assert list(s.status) == [0, 0, cp.BAD_ROW]


def test_standardising_and_a_far_level_do_not_move_the_answer():
    X = C.shifted_rows(11, 400, 2)
    mu, sigma = np.array([0.3, -0.2]), np.array([2.0, 0.5])
    a = solve(X, 8.0, "mean", 2)
    b = solve(X * sigma + mu, 8.0, "mean", 2, mu=mu, sigma=sigma)
    far = solve(X + 1e6, 8.0, "mean", 2)                        # rows are centred on the first: no cancellation in Q - S^2 / m
    assert np.array_equal(a.change_points[0], b.change_points[0]) and abs(a.F[0] - b.F[0]) < 1e-9 * abs(a.F[0])
    assert np.array_equal(a.change_points[0], far.change_points[0]) and abs(a.F[0] - far.F[0]) < 1e-6 * abs(a.F[0])
    assert list(a.change_points[0]) == [200]


def test_penalty_path_selection_and_tables():
    X = C.shifted_rows(3, 600, 4)
    A, cols = C.results_like(X, ld=20, first=8)
    pens = [0.5, 2.0, cp.default_penalty(600, 4, "mean"), 200.0, 1e5]
    path = cp.penalty_path(A, pens, features=cols, min_len=2, backend="numpy")
    assert np.all(np.diff(path.n_change_points) <= 0) and path.n_change_points[-1] == 0 and path.n_change_points[2] == 1
    assert np.all(np.diff(path.cost) >= 0)                      # fewer change points never fit better
    for i, p in enumerate(pens):
        s = cp.segment(A, features=cols, penalty=p, min_len=2, backend="numpy")
        assert s.n_change_points == path.n_change_points[i] and s.F[0] == path.F[i]
    assert cp.select_penalty(path, "bic") in (2, 3) and path.n_change_points[cp.select_penalty(path, "elbow")] >= 1
    s = cp.segment(A, features=cols, min_len=2, backend="numpy")
    table = cp.segment_table(A, s, features=cols)
    assert list(table["start"]) == [0, 300] and list(table["length"]) == [300, 300] and table["mean"].shape == (2, 4)
    assert np.allclose(table["mean"][1], X[300:].mean(axis=0)) and np.allclose(table["var"][0], X[:300].var(axis=0))
    y_prob = np.zeros((600, 3))
    y_prob[:300, 0], y_prob[300:, 2] = 1.0, 1.0
    mean, cls = cp.diagnose_segments(s, y_prob)
    assert list(cls) == [0, 2] and mean.shape == (2, 3)
    assert cp.default_penalty(100, 4, "mean") == 5 * np.log(100) and cp.default_penalty(100, 4, "meanvar") == 9 * np.log(100)


def test_arguments_are_checked():
    X = np.zeros((20, 3))
    for bad in (dict(kind="median"), dict(kind="meanvar", min_len=1), dict(min_len=0), dict(min_len=4, max_len=3), dict(penalty=-1.0),
                dict(penalty=np.nan), dict(var_floor=-1.0), dict(mu=[0, 0, 0]), dict(mu=[0, 0, 0], sigma=[1, 0, 1]),
                dict(seg_starts=[0, 9, 9]), dict(seg_starts=[1, 5]), dict(seg_starts=[0, 20]), dict(backend="cpu")):
        with pytest.raises(ValueError):
            cp.segment(X, **{"features": [0, 1, 2], "backend": "numpy", **bad})
    with pytest.raises(NotImplementedError):
        cp.segment(np.zeros((20, 9)), features=list(range(9)), backend="numpy")


@pytest.mark.parametrize("chunk", (32, 50))
def test_the_monitor_follows_segment_on_its_window(chunk):
    """Chunks that do and do not divide the window of 128, before the ring has filled and across its wrap."""
    rng = np.random.default_rng(2)
    X = rng.normal(size=(500, 2))
    X[140:] += 3.0
    X[333:] -= 4.0
    A, cols = C.results_like(X, ld=6, first=1)
    mon = cp.ChangeMonitor(128, features=cols, penalty=9.0, min_len=3, backend="numpy")
    reported = []
    for lo in range(0, 500, chunk):
        found, new = mon.update(A[lo:lo + chunk])
        hi = min(lo + chunk, 500)
        w0 = max(hi - 128, 0)
        ref = cp.segment(A[w0:hi], features=cols, penalty=9.0, min_len=3, backend="numpy")
        assert np.array_equal(found, ref.change_points[0] + w0) and mon.F == ref.F[0] and mon.n_seen == hi
        assert np.array_equal(mon.window_rows(), X[w0:hi])
        reported += list(new)
    assert reported == [140, 333]                               # each once, after two updates in a row
