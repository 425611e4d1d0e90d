"""The cached physics-stage pass, one kernel instantiation per stage kind (pinn_residuals_prepare + pinn_residuals_cached):
only the stage's own range of the sums is reduced, every other entry of d_sums is exactly 0, the live ones are
pinn_residuals' for the same flag, and a call repeats to the byte.  Row counts: a single row, the odd second row of a
two-row trip (255, 257), many workgroups below the grid cap (65 537) and the cap reached with a second trip (524 291).

Where the reduction trees of two passes coincide (one workgroup, one row per thread) their sums are compared to the byte, and so
are the cache slots and the row pass's columns: the passes are assembled from one text of each model (csrc/pinn_physics.h), and
these tests are what holds them to it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pinn_oracle as O

ROWS = [1, 255, 257, 65537, 2 * 256 * 1024 + 3]
# stage flag -> (first, last) sum of its range (the enum of include/pinn_hip.h)
RANGES = {"V": ("FV2", "YU2"), "T": ("FT2", "FT_ABS"), "H": ("FH2", "TGTH"), "O": ("FO2", "TGTO")}


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


def _flag(kind):
    from pinn_amd import _lib
    return getattr(_lib, "RES_" + kind)


def _live(kind):
    from pinn_amd import _lib
    lo, hi = RANGES[kind]
    live = np.zeros(_lib.NSUMS, dtype=bool)
    live[_lib.S[lo]:_lib.S[hi] + 1] = True
    return live


def _lam0():
    return torch.tensor([O.LAMBDA_INIT[n] for n in O.LAMBDA_NAMES], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _rows(N):
    """Synthetic rows of one size on the device, shared by every case of that size."""
    import hip_helpers as hh
    from pinn_amd import synth
    ds = synth.make_dataset(N, (), seed=6)
    x, y = ds[0].to(hh.dev()), ds[1].reshape(-1).to(hh.dev())
    u = (y + 0.01).contiguous()
    return x, u, y, hh.affine_struct(ds[4], ds[5])


def _work(lib):
    import hip_helpers as hh
    wb = lib.pinn_residuals_workspace_bytes()
    return torch.empty(wb, dtype=torch.uint8, device=hh.dev()), wb


def _prepare(lib, N, kind, lam):
    import hip_helpers as hh
    from pinn_amd import _lib
    x, u, y, aff = _rows(N)
    cache = torch.empty(6 * N, dtype=torch.float32, device=hh.dev())
    _lib.check(lib.pinn_residuals_prepare(hh.ptr(x), hh.ptr(u), hh.ptr(y), ctypes.byref(aff), hh.ptr(lam), _flag(kind), N, hh.ptr(cache),
                                          hh.stream()), "prepare")
    return cache


def _cached(lib, N, kind, cache, lam, work, wb):
    """d_sums of one pinn_residuals_cached call, pre-filled with NaN: every entry has to be written."""
    import hip_helpers as hh
    from pinn_amd import _lib
    sums = torch.full((_lib.NSUMS,), float("nan"), dtype=torch.float64, device=hh.dev())
    _lib.check(lib.pinn_residuals_cached(hh.ptr(cache), ctypes.byref(_rows(N)[3]), hh.ptr(lam), _flag(kind), N, hh.ptr(sums), hh.ptr(work), wb,
                                         hh.stream()), "cached")
    return sums.cpu().numpy()


@pytest.mark.parametrize("kind", ["V", "T", "H", "O"])
@pytest.mark.parametrize("N", ROWS)
def test_stage_pass_live_and_dead_sums(lib, N, kind):
    import hip_helpers as hh
    from pinn_amd import _lib
    x, u, y, aff = _rows(N)
    lam = _lam0().to(hh.dev())
    work, wb = _work(lib)
    ref = torch.full((_lib.NSUMS,), float("nan"), dtype=torch.float64, device=hh.dev())
    _lib.check(lib.pinn_residuals(hh.ptr(x), hh.ptr(u), hh.ptr(y), ctypes.byref(aff), hh.ptr(lam), _flag(kind), N, None, 0, hh.ptr(ref),
                                  hh.ptr(work), wb, hh.stream()), "residuals")
    ref = ref.cpu().numpy()
    # the same sums through the kernel with run-time flags (a columns buffer selects it) and the full-range finalize: a reference that
    # shares neither the specialised instantiations nor the ranged reduction with the code under test
    cols = torch.empty(_lib.NCOLS, N, device=hh.dev())
    gen = torch.full((_lib.NSUMS,), float("nan"), dtype=torch.float64, device=hh.dev())
    _lib.check(lib.pinn_residuals(hh.ptr(x), hh.ptr(u), hh.ptr(y), ctypes.byref(aff), hh.ptr(lam), _flag(kind), N, hh.ptr(cols), N, hh.ptr(gen),
                                  hh.ptr(work), wb, hh.stream()), "residuals + columns")
    gen = gen.cpu().numpy()
    cache = _prepare(lib, N, kind, lam)
    a = _cached(lib, N, kind, cache, lam, work, wb)
    b = _cached(lib, N, kind, cache, lam, work, wb)
    live = _live(kind)
    print("N %d %s cached %s\n  residuals %s" % (N, kind, a[live].tolist(), ref[live].tolist()))
    assert a.tobytes() == b.tobytes()                                   # repeatable to the byte
    assert np.all(a[~live] == 0.0) and np.all(ref[~live] == 0.0)        # dead sums: exactly 0, in both forms of the pass
    # same rows per thread, same order of every sum, -ffp-contract=off: the specialised pass from the rows only drops dead work
    assert ref.tobytes() == gen.tobytes(), (ref, gen)
    assert np.all(np.isfinite(ref[live])) and ref[live][0] > 0.0        # (the first of a range is the stage's sum of squares)
    # the tolerance of test_residuals_cached_matches_residuals (DESIGN K1c): the two passes differ in the order of the row sums
    np.testing.assert_allclose(a[live], gen[live], rtol=2e-6, atol=1e-6 * max(1.0, np.abs(ref).max()) * 1e-3, err_msg="%s N=%d" % (kind, N))
    np.testing.assert_allclose(a[live], ref[live], rtol=2e-6, atol=1e-6 * max(1.0, np.abs(ref).max()) * 1e-3, err_msg="%s N=%d" % (kind, N))


def _residuals(lib, N, kind, lam, with_cols):
    """d_sums (pre-filled with NaN) and, with_cols, the columns of one pinn_residuals call for the one stage flag."""
    import hip_helpers as hh
    from pinn_amd import _lib
    x, u, y, aff = _rows(N)
    work, wb = _work(lib)
    cols = torch.full((_lib.NCOLS, N), float("nan"), device=hh.dev()) if with_cols else None
    sums = torch.full((_lib.NSUMS,), float("nan"), dtype=torch.float64, device=hh.dev())
    _lib.check(lib.pinn_residuals(hh.ptr(x), hh.ptr(u), hh.ptr(y), ctypes.byref(aff), hh.ptr(lam), _flag(kind), N,
                                  hh.ptr(cols) if with_cols else None, N if with_cols else 0, hh.ptr(sums), hh.ptr(work), wb, hh.stream()),
               "residuals")
    return sums.cpu().numpy(), (cols.cpu().numpy() if with_cols else None)


@pytest.mark.parametrize("kind", ["V", "T", "H", "O"])
@pytest.mark.parametrize("N", [1, 64, 255, 256])
def test_stage_pass_one_workgroup_equals_row_pass_to_the_byte(lib, N, kind):
    """Up to 256 rows the cached pass, the row pass specialised for the stage and the row pass with run-time flags (columns) are
    each one workgroup in which thread t holds row t alone: the reduction trees coincide, so any difference in a sum is a
    difference in a formula."""
    import hip_helpers as hh
    lam = _lam0().to(hh.dev())
    work, wb = _work(lib)
    cached = _cached(lib, N, kind, _prepare(lib, N, kind, lam), lam, work, wb)
    spec, _ = _residuals(lib, N, kind, lam, False)
    gen, _ = _residuals(lib, N, kind, lam, True)
    live = _live(kind)
    print("N %d %s\n  cached    %s\n  residuals %s\n  + columns %s" % (N, kind, cached[live].tolist(), spec[live].tolist(), gen[live].tolist()))
    assert np.all(np.isfinite(spec[live])) and spec[live][0] > 0.0
    assert cached.tobytes() == spec.tobytes(), (kind, N, np.flatnonzero(cached != spec))
    assert gen.tobytes() == spec.tobytes(), (kind, N, np.flatnonzero(gen != spec))


@pytest.mark.parametrize("stage,kind", [("LAMBDA_PM", "V"), ("LAMBDA_F", "V"), ("THERMAL", "T"), ("HYDROGEN", "H"), ("OXYGEN", "O")])
@pytest.mark.parametrize("N", [1, 64])
def test_persistent_kernel_sums_equal_row_pass_to_the_byte(lib, N, stage, kind):
    """One iteration of the persistent stage kernel from the initial parameters: up to 64 rows only wave 0 holds rows (one each)
    and the other waves add +0.0, so its d_sums are pinn_residuals' for the stage's flag, byte for byte."""
    import hip_helpers as hh
    from pinn_amd import _lib
    x, u, y, aff = _rows(N)
    lam = _lam0().to(hh.dev())
    ref, _ = _residuals(lib, N, kind, lam, False)
    swb = lib.pinn_lambda_stage_workspace_bytes(N)
    swork = torch.empty(swb, dtype=torch.uint8, device=hh.dev())
    lam_p, adam_p, loss_p = _lam0().to(hh.dev()), torch.zeros(2 * _lib.NLAMBDA, device=hh.dev()), torch.zeros(2, device=hh.dev())
    sums = torch.full((_lib.NSUMS,), float("nan"), dtype=torch.float64, device=hh.dev())
    _lib.check(lib.pinn_lambda_stage_run(getattr(_lib, "STAGE_" + stage), _flag(kind), hh.ptr(x), hh.ptr(u), hh.ptr(y), ctypes.byref(aff), N,
                                         1e-3, 0.8, 1000, 0, 1, hh.ptr(lam_p), hh.ptr(adam_p), hh.ptr(loss_p), None, 1000, hh.ptr(sums),
                                         hh.ptr(swork), swb, hh.stream()), "stage_run")
    got = sums.cpu().numpy()
    live = _live(kind)
    print("N %d %s persistent %s\n  residuals %s" % (N, stage, got[live].tolist(), ref[live].tolist()))
    assert np.all(np.isfinite(ref[live])) and ref[live][0] > 0.0
    assert got.tobytes() == ref.tobytes(), (stage, N, np.flatnonzero(got != ref))


def test_stage_cache_slots_equal_columns_to_the_byte(lib):
    """What stage_prepare stores is what the row pass writes as columns: i5, E and V_out of the voltage model (VOUT5 is 5 V_out,
    one float32 product) and T_out of the thermal model, at 257 rows (two workgroups)."""
    import hip_helpers as hh
    from pinn_amd import _lib
    N = 257
    lam = _lam0().to(hh.dev())
    cv = _prepare(lib, N, "V", lam).view(6, N).cpu().numpy()
    _, cols = _residuals(lib, N, "V", lam, True)
    assert np.all(np.isfinite(cv[:4])) and np.all(np.isfinite(cols[_lib.C["VOUT5"]]))
    for slot, col, scale in ((0, "I", None), (2, "ENERNST", None), (3, "VOUT5", np.float32(5.0))):
        want = cv[slot] if scale is None else (cv[slot] * scale).astype(np.float32)
        bad = np.flatnonzero(want.view(np.uint32) != cols[_lib.C[col]].view(np.uint32))
        print("V slot %d against column %s: %d of %d rows differ" % (slot, col, bad.size, N))
        assert bad.size == 0, (col, bad[:8], want[bad[:8]], cols[_lib.C[col]][bad[:8]])
    ct = _prepare(lib, N, "T", lam).view(6, N).cpu().numpy()
    _, cols = _residuals(lib, N, "T", lam, True)
    bad = np.flatnonzero(ct[3].view(np.uint32) != cols[_lib.C["TOUT"]].view(np.uint32))
    print("T slot 3 against column TOUT: %d of %d rows differ" % (bad.size, N))
    assert np.all(np.isfinite(ct[3])) and bad.size == 0, (bad[:8], ct[3][bad[:8]])


def test_stage_pass_matches_persistent_kernel(lib):
    """One iteration of the persistent stage kernel against one pinn_residuals_cached + pinn_lambda_step, all five stages at 4096
    rows: the same stage loss and parameters (only the order of the row sums differs), at the bounds of
    test_stage_run_persistent_matches_iterated_kernels."""
    import hip_helpers as hh
    from pinn_amd import _lib
    N = 4096
    x, u, y, aff = _rows(N)
    work, wb = _work(lib)
    swb = lib.pinn_lambda_stage_workspace_bytes(N)
    swork = torch.empty(swb, dtype=torch.uint8, device=hh.dev())
    stages = [(_lib.STAGE_LAMBDA_PM, "V", 1e-3), (_lib.STAGE_LAMBDA_F, "V", 1e-3), (_lib.STAGE_THERMAL, "T", 1.0),
              (_lib.STAGE_HYDROGEN, "H", 1e-1), (_lib.STAGE_OXYGEN, "O", 1e-2)]
    for stage, kind, lr in stages:
        lam_p, adam_p, loss_p = _lam0().to(hh.dev()), torch.zeros(2 * _lib.NLAMBDA, device=hh.dev()), torch.zeros(2, device=hh.dev())
        _lib.check(lib.pinn_lambda_stage_run(stage, _flag(kind), hh.ptr(x), hh.ptr(u), hh.ptr(y), ctypes.byref(aff), N, lr, 0.8, 1000, 0, 1,
                                             hh.ptr(lam_p), hh.ptr(adam_p), hh.ptr(loss_p), None, 1000, None, hh.ptr(swork), swb, hh.stream()),
                   "stage_run")
        lam_i, adam_i, loss_i = _lam0().to(hh.dev()), torch.zeros(2 * _lib.NLAMBDA, device=hh.dev()), torch.zeros(2, device=hh.dev())
        cache = _prepare(lib, N, kind, lam_i)
        sums = torch.full((_lib.NSUMS,), float("nan"), dtype=torch.float64, device=hh.dev())
        _lib.check(lib.pinn_residuals_cached(hh.ptr(cache), ctypes.byref(aff), hh.ptr(lam_i), _flag(kind), N, hh.ptr(sums), hh.ptr(work), wb,
                                             hh.stream()), "cached")
        _lib.check(lib.pinn_lambda_step(stage, hh.ptr(sums), N, aff.vn_scale, lr, 1, hh.ptr(lam_i), hh.ptr(adam_i), hh.ptr(loss_i),
                                        hh.stream()), "lambda_step")
        lp, li = loss_p.cpu().numpy(), loss_i.cpu().numpy()
        print("stage %d loss persistent %s iterated %s" % (stage, lp.tolist(), li.tolist()))
        assert np.all(np.isfinite(li)) and np.all(li > 0.0)
        assert np.all(np.abs(lp - li) <= 1e-5 * np.abs(li)), (stage, lp, li)
        np.testing.assert_allclose(lam_p.cpu().numpy(), lam_i.cpu().numpy(), rtol=2e-5, atol=1e-9, err_msg="stage %d" % stage)
        assert not np.array_equal(lam_i.cpu().numpy(), _lam0().numpy())          # the step moved the stage's parameters


def test_stage_pass_nan_row_reaches_live_sums_only(lib):
    """A NaN in one cached row makes every live sum of the stage NaN (never swallowed) and leaves the dead ones at 0."""
    import hip_helpers as hh
    N, kind, bad = 257, "T", 100
    lam = _lam0().to(hh.dev())
    work, wb = _work(lib)
    cache = _prepare(lib, N, kind, lam)
    clean = _cached(lib, N, kind, cache, lam, work, wb)
    cache.view(6, N)[:4, bad] = float("nan")            # the four cached floats of the thermal model, one row
    s = _cached(lib, N, kind, cache, lam, work, wb)
    live = _live(kind)
    assert np.all(np.isfinite(clean[live]))
    assert np.all(np.isnan(s[live])), s[live]
    assert np.all(s[~live] == 0.0)
