"""GPU: the residual passes' columns and sums against the float64 referee of tests/residual_referee.py -- pinn_residuals (all flags
with columns, each single flag without, d_y = NULL), pinn_residuals_prepare + pinn_residuals_cached, one iteration of
pinn_lambda_stage_run, and pinn_net_f_t.  Every pass is assembled from csrc/pinn_physics.h, so the other suites' pass-against-pass
comparisons move together with an error in that text; the referee does not read it.

Row counts are the smallest at which a launch changes shape (one row, one workgroup and its neighbours, the last size of the
persistent kernel, the grid cap and the second grid-stride trip, the third row of a cached thread); the parameter sets reach both
clamps of the oxygen target, the sign 0, the exact clamp edges and parameters far from the start; marked rows sit at the seams.
Gates and conditions: residual_referee.py.  Every comparison prints its worst error / gate per sum before it asserts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import residual_referee as rr

ROW_CASES = [(N, s) for N in rr.ROW_COUNTS for s in rr.MAIN_SETS] + [(N, s) for N in rr.EDGE_COUNTS for s in rr.EDGE_SETS]
STAGES = [("LAMBDA_PM", "V"), ("LAMBDA_F", "V"), ("THERMAL", "T"), ("HYDROGEN", "H"), ("OXYGEN", "O")]


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=2)
def _device_rows(N, idle=False):
    import hip_helpers as hh
    rw = rr.rows(N, idle)
    _, sx, sy = rr.fixture()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hh.dev())
    return d(rw.xn), d(rw.un), d(rw.yn), hh.affine_struct(sx, sy)


def _lam(set_name):
    import hip_helpers as hh
    return torch.from_numpy(rr.param_sets()[set_name].copy()).to(hh.dev())


def _flags(models):
    return sum(rr.FLAG[m] for m in models)


def _residuals(lib, N, idle, lam, models, with_cols, with_y=True):
    """One pinn_residuals call -> (d_sums [32] float64, {column: [N]} or None).  Outputs are pre-filled with NaN: what the call has to
    write, it has to write."""
    import hip_helpers as hh
    from pinn_amd import _lib
    x, u, y, aff = _device_rows(N, idle)
    wb = lib.pinn_residuals_workspace_bytes()
    work = torch.full((wb,), 0xFF, dtype=torch.uint8, device=hh.dev())
    cols = torch.full((_lib.NCOLS, N), float("nan"), device=hh.dev()) if with_cols else None
    sums = torch.full((_lib.NSUMS,), float("nan"), dtype=torch.float64, device=hh.dev())
    _lib.check(lib.pinn_residuals(hh.ptr(x), hh.ptr(u) if "V" in models else None, hh.ptr(y) if with_y else None, ctypes.byref(aff), hh.ptr(lam),
                                  _flags(models), N, hh.ptr(cols), N if with_cols else 0, hh.ptr(sums), hh.ptr(work), wb, hh.stream()),
               "pinn_residuals")
    c = cols.cpu().numpy() if with_cols else None
    return sums.cpu().numpy(), (None if c is None else {n: c[i] for i, n in enumerate(rr.COL_NAMES) if rr.COL_SRC[n][0] in models})


def _cached(lib, N, idle, kind, lam0, lam):
    """The cache prepared at lam0, read at lam."""
    import hip_helpers as hh
    from pinn_amd import _lib
    x, u, y, aff = _device_rows(N, idle)
    wb = lib.pinn_residuals_workspace_bytes()
    work = torch.full((wb,), 0xFF, dtype=torch.uint8, device=hh.dev())
    cache = torch.full((6 * N,), float("nan"), device=hh.dev())
    _lib.check(lib.pinn_residuals_prepare(hh.ptr(x), hh.ptr(u), hh.ptr(y), ctypes.byref(aff), hh.ptr(lam0), rr.FLAG[kind], N, hh.ptr(cache),
                                          hh.stream()), "pinn_residuals_prepare")
    sums = torch.full((_lib.NSUMS,), float("nan"), dtype=torch.float64, device=hh.dev())
    _lib.check(lib.pinn_residuals_cached(hh.ptr(cache), ctypes.byref(aff), hh.ptr(lam), rr.FLAG[kind], N, hh.ptr(sums), hh.ptr(work), wb,
                                         hh.stream()), "pinn_residuals_cached")
    return sums.cpu().numpy()


def _show(kernel, N, set_name, ratios):
    print("RATIO %s N=%d set=%s %s" % (kernel, N, set_name, " ".join("%s=%.3g" % kv for kv in ratios.items())))


@pytest.mark.parametrize("N,set_name", ROW_CASES)
def test_row_passes_against_the_referee(lib, N, set_name):
    ref = rr.referee(N, set_name)
    rr.check_conditions(ref, ("rows", "cached"))
    lam, lam0 = _lam(set_name), _lam("init")
    r = rr.rows_per_thread(N, "rows")
    # all four models, columns and sums
    sums, cols = _residuals(lib, N, False, lam, "VTHO", True)
    _show("columns", N, set_name, rr.check_columns(cols, ref, rr.COL_NAMES, (N, set_name)))
    _show("rows/all", N, set_name, rr.check_sums(sums, ref, r, rr.SUM_NAMES, (N, set_name, "all")))
    # without the measured voltage: its sums are 0, everything else keeps its bytes
    s0, c0 = _residuals(lib, N, False, lam, "VTHO", True, with_y=False)
    for name in rr.COL_NAMES:
        assert c0[name].tobytes() == cols[name].tobytes(), name
    for k in range(rr.NSUMS):
        name = rr.SUM_NAMES[k] if k < len(rr.SUM_NAMES) else None
        if name in rr.Y_SUMS:
            assert s0[k] == 0.0, (name, s0[k])
        else:
            assert s0[k:k + 1].tobytes() == sums[k:k + 1].tobytes(), (name, s0[k], sums[k])
    # each stage's specialised pass, and its cached form: the cache from the initial parameters, read at the set's
    for kind in "VTHO":
        live = rr.model_sums(kind)
        s1, _ = _residuals(lib, N, False, lam, kind, False)
        _show("rows/" + kind, N, set_name, rr.check_sums(s1, ref, r, live, (N, set_name, kind)))
        s2 = _cached(lib, N, False, kind, lam0, lam)
        _show("cached/" + kind, N, set_name, rr.check_sums(s2, ref, rr.rows_per_thread(N, "cached"), live, (N, set_name, kind, "cached")))


@pytest.mark.parametrize("set_name", ["init", "B"])
def test_idle_rows_hydrogen_and_oxygen(lib, set_name):
    """I = 0, -0.0027 and -1 A without gas flow: the 1e-8 clamp of the stoichiometric flow, which no other row reaches."""
    N = 257
    ref = rr.referee(N, set_name, True)
    rr.check_conditions(ref, ("rows", "cached"))
    assert ref.stats["h_flow_clamped"] > 0 and ref.stats["o_flow_clamped"] > 0
    lam = _lam(set_name)
    sums, cols = _residuals(lib, N, True, lam, "HO", True)
    names = [c for c in rr.COL_NAMES if rr.COL_SRC[c][0] in "HO"]
    _show("idle columns", N, set_name, rr.check_columns(cols, ref, names, ("idle", set_name)))
    _show("idle rows/HO", N, set_name, rr.check_sums(sums, ref, rr.rows_per_thread(N, "rows"), rr.model_sums("HO"), ("idle", set_name)))
    s1, _ = _residuals(lib, N, True, lam, "HO", False)
    assert s1.tobytes() == sums.tobytes()
    for kind in "HO":
        s2 = _cached(lib, N, True, kind, _lam("init"), lam)
        _show("idle cached/" + kind, N, set_name,
              rr.check_sums(s2, ref, rr.rows_per_thread(N, "cached"), rr.model_sums(kind), ("idle", set_name, kind)))


@pytest.mark.parametrize("set_name", ["init", "moved", "B"])
@pytest.mark.parametrize("N", rr.PERSISTENT_COUNTS)
def test_persistent_kernel_sums_against_the_referee(lib, N, set_name):
    """One iteration of pinn_lambda_stage_run per stage: d_sums are the sums at the parameters the call was given (the step comes after
    them), every thread has added up to ceil(N / 1024) rows in float, and the log row carries the same sums rounded to float."""
    import hip_helpers as hh
    from pinn_amd import _lib
    ref = rr.referee(N, set_name)
    rr.check_conditions(ref, ("persistent",))
    x, u, y, aff = _device_rows(N)
    swb = lib.pinn_lambda_stage_workspace_bytes(N)
    for stage, kind in STAGES:
        lam = _lam(set_name)
        adam, loss = torch.zeros(2 * _lib.NLAMBDA, device=hh.dev()), torch.zeros(2, device=hh.dev())
        work = torch.full((swb,), 0xFF, dtype=torch.uint8, device=hh.dev())
        sums = torch.full((_lib.NSUMS,), float("nan"), dtype=torch.float64, device=hh.dev())
        log = torch.full((_lib.STAGE_LOG_FLOATS,), float("nan"), device=hh.dev())
        _lib.check(lib.pinn_lambda_stage_run(getattr(_lib, "STAGE_" + stage), rr.FLAG[kind], hh.ptr(x), hh.ptr(u), hh.ptr(y), ctypes.byref(aff), N,
                                             1e-3, 0.8, 1000, 0, 1, hh.ptr(lam), hh.ptr(adam), hh.ptr(loss), hh.ptr(log), 1, hh.ptr(sums),
                                             hh.ptr(work), swb, hh.stream()), "pinn_lambda_stage_run")
        got, row = sums.cpu().numpy(), log.cpu().numpy()
        _show("persistent/" + stage, N, set_name, rr.check_sums(got, ref, rr.rows_per_thread(N, "persistent"), rr.model_sums(kind), (N, stage)))
        assert row[20:20 + rr.NSUMS].tobytes() == got.astype(np.float32).tobytes(), (stage, row[20:52], got)


def _net_f_t(lib, x, u, aff, lam, halo=None):
    import hip_helpers as hh
    from pinn_amd import _lib
    n = x.shape[0]
    out = torch.full((3, max(n, 1)), float("nan"), device=hh.dev())
    xh, uh = (None, None) if halo is None else halo
    _lib.check(lib.pinn_net_f_t(hh.ptr(x), hh.ptr(u), hh.ptr(xh), hh.ptr(uh), ctypes.byref(aff), hh.ptr(lam), n, hh.ptr(out[0]), hh.ptr(out[1]),
                                hh.ptr(out[2]), hh.stream()), "pinn_net_f_t")
    return out[:, :n].cpu().numpy()


@pytest.mark.parametrize("set_name", ["init", "moved"])
@pytest.mark.parametrize("N", rr.EULER_COUNTS)
def test_net_f_t_against_the_referee(lib, N, set_name):
    rw, r64, r32 = rr.euler(N, set_name)
    x, u, y, aff = _device_rows(N)
    lam = _lam(set_name)
    got = _net_f_t(lib, x, u, aff, lam)
    ratios = {}
    for j, k in enumerate(("f", "t_pred", "t_real")):
        ratios[k] = rr.check_series(got[j], r64[k], r32[k], (N, set_name, k), exact=(k == "t_real"))
    _show("net_f_t", N, set_name, ratios)
    if N >= 2:
        # two shards, the second with the row before it as halo: the whole series to the byte
        cut = max(1, N // 2)
        a = _net_f_t(lib, x[:cut], u[:cut], aff, lam)
        b = _net_f_t(lib, x[cut:], u[cut:], aff, lam, halo=(x[cut - 1], u[cut - 1:cut]))
        assert np.concatenate([a, b], axis=1).tobytes() == got.tobytes()
