"""CPU: the host-side checks of the pinn_fs_* entry points (csrc/pinn_faultsets.hip).  Every call below returns before any
launch, with addresses that are never dereferenced, as test_uncertainty_abi.py does."""
import ctypes

import pytest

E_ARG, E_WS, OK = -1, -3, 0
A = 0x1000                                  # an aligned non-NULL address, never dereferenced
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    return _lib.load(build_if_missing=False)


def ints(v):
    return (ctypes.c_int * max(len(v), 1))(*v)


def lls(v):
    return (ctypes.c_longlong * max(len(v), 1))(*v)


def tail(C, L, state, n_cal, kmin, kind, randomized, seed, draw, first, regime, y, count, mask, size, novel, missing, scores, tally, null_ncal,
         null_kmin):
    n_cal = [100] * C + [0] if n_cal is None else n_cal
    kmin = [1] * (C * max(L, 1)) if kmin is None else kmin
    return (state, None if null_ncal else lls(n_cal), None if null_kmin else lls(kmin), L, kind, randomized, seed, draw, first, regime, y, count, mask,
            size, novel, missing, scores, tally)


def rank(lib, yp=A, n=10, C=4, L=2, state=A, n_cal=None, kmin=None, kind=0, randomized=0, seed=1, draw=4, first=0, regime=0, y=None, count=A,
         mask=A, size=A, novel=A, missing=A, scores=A, tally=None, null_ncal=False, null_kmin=False):
    return lib.pinn_fs_rank(yp, n, C, *tail(C, L, state, n_cal, kmin, kind, randomized, seed, draw, first, regime, y, count, mask, size, novel,
                                            missing, scores, tally, null_ncal, null_kmin), None)


def gmm(lib, arr=A, ld=22, n=10, n_arr=None, cols=(13, 14, 15, 16), ridx=None, K=8, gst=A, cmap=A, C=4, logmap=None, L=2, state=A, n_cal=None,
        kmin=None, kind=0, randomized=0, seed=1, draw=4, first=0, regime=0, y=None, count=A, mask=A, size=A, novel=A, missing=A, scores=A,
        tally=None, y_prob=A, y_pred=A, lpn=A, any_score=None, any_count=None, null_ncal=False, null_kmin=False):
    return lib.pinn_fs_gmm(arr, ld, n if n_arr is None else n_arr, ints(cols), len(cols), ridx, n, K, gst, cmap, C, logmap,
                           *tail(C, L, state, n_cal, kmin, kind, randomized, seed, draw, first, regime, y, count, mask, size, novel, missing,
                                 scores, tally, null_ncal, null_kmin), y_prob, y_pred, lpn, any_score, any_count, None)


def build(lib, scores=A, any_=None, cls=A, n=10, C=4, kind=0, seed=1, randomized=0, state=A, ws=A, wb=BIG):
    return lib.pinn_fs_build(scores, any_, cls, n, C, kind, seed, randomized, state, ws, wb, None)


SHARED_ERRORS = (
    dict(C=0), dict(C=17), dict(L=0), dict(L=9), dict(kind=-1), dict(kind=4), dict(regime=-1), dict(regime=4), dict(draw=0), dict(draw=5),
    dict(first=-1), dict(state=A + 4), dict(null_ncal=True), dict(null_kmin=True), dict(n_cal=[100, 100, 100, -1, 0]),
    dict(n_cal=[100, 100, 100, (1 << 20) + 1, 0]), dict(kmin=[1, 1, 1, 1, 1, 1, 1, -1]), dict(kmin=[1, 1, 1, 1, 1, 1, 1, 102]),
    dict(y=A + 4, tally=A), dict(y=A), dict(tally=A + 4), dict(count=A + 2), dict(mask=A + 1), dict(scores=A + 4),
    dict(regime=1, n_cal=[4000, 4000, 0, 0, 0]),                      # forced regimes that do not fit the LDS budget
    dict(regime=2, n_cal=[1 << 20, 1 << 20, 0, 0, 0]),
    dict(state=None), dict(state=None, L=0, count=None, mask=None, size=None, novel=None, tally=A),          # scores only: no rank output
)


def test_rank_checks_its_arguments_on_the_host(lib):
    for bad in SHARED_ERRORS + (dict(yp=None), dict(yp=A + 4), dict(n=-1), dict(n=(1 << 40) + 1), dict(kind=3)):
        assert rank(lib, **bad) == E_ARG, bad
    assert rank(lib, n=0) == OK and rank(lib, n=0, C=16, L=8, n_cal=[1 << 20] * 16 + [0], kmin=[(1 << 20) + 1] * 128, regime=3) == OK
    assert rank(lib, n=0, count=None, mask=None, size=None, novel=None, missing=None, scores=None, y=A, tally=A) == OK
    assert rank(lib, n=0, state=None, L=0, count=None, mask=None, size=None, novel=None) == OK                # scores only
    assert rank(lib, n=0, regime=1, n_cal=[1920] * 4 + [0]) == OK and rank(lib, n=0, regime=1, n_cal=[1920] * 3 + [1921, 0]) == E_ARG
    assert rank(lib, n=0, regime=2, n_cal=[30720] * 4 + [0]) == OK and rank(lib, n=0, regime=2, n_cal=[30720] * 3 + [30721, 0]) == E_ARG


def test_gmm_checks_its_arguments_on_the_host(lib):
    rows = (dict(arr=None), dict(arr=A + 4), dict(ridx=A + 4), dict(n=-1, n_arr=10), dict(n=11, n_arr=10), dict(ld=0), dict(cols=()),
            dict(cols=tuple(range(9))), dict(cols=(13, 14, 15, 22)), dict(cols=(-1, 14, 15, 16)), dict(K=0), dict(K=33))
    own = (dict(gst=None), dict(gst=A + 4), dict(cmap=None), dict(cmap=A + 4), dict(logmap=A), dict(kind=3), dict(kind=3, logmap=A + 4),
           dict(y_prob=A + 4), dict(y_pred=A + 4), dict(lpn=A + 4), dict(any_score=A), dict(any_count=A), dict(kind=3, logmap=A, any_score=A + 4),
           dict(kind=3, logmap=A, any_count=A + 2),
           dict(regime=1, n_cal=[1000, 1000, 1000, 73, 0]))           # the fused kernel's own, smaller budget
    for bad in rows + own + tuple(b for b in SHARED_ERRORS if "regime" not in b or b["regime"] not in (1, 2)):
        assert gmm(lib, **bad) == E_ARG, bad
    assert gmm(lib, n=0) == OK and gmm(lib, n=0, kind=3, logmap=A, any_score=A, any_count=A, n_cal=[100] * 4 + [400]) == OK
    assert gmm(lib, n=0, y_prob=None, y_pred=None, lpn=None, count=None, mask=None, size=None, novel=None, missing=None, scores=None, y=A, tally=A) == OK
    assert gmm(lib, n=0, state=None, L=0, count=None, mask=None, size=None, novel=None) == OK
    assert gmm(lib, n=0, regime=1, n_cal=[768] * 4 + [0]) == OK


def test_build_checks_its_arguments_on_the_host(lib):
    for bad in (dict(scores=None), dict(scores=A + 4), dict(any_=A + 4), dict(cls=None), dict(cls=A + 4), dict(n=-1), dict(C=0), dict(C=17),
                dict(kind=-1), dict(kind=4), dict(state=None), dict(state=A + 4), dict(ws=None), dict(ws=A + 4),
                dict(n=4 * (1 << 20) + 1), dict(C=1, n=(1 << 20) + 1)):
        assert build(lib, **bad) == E_ARG, bad
    for n, C in ((1, 1), (10, 4), (5000, 16), (1 << 20, 1), (16 << 20, 16)):
        assert build(lib, n=n, C=C, wb=lib.pinn_fs_workspace_bytes(n, C) - 1) == E_WS, (n, C)


def test_state_and_workspace_bytes_are_monotone_and_aligned(lib):
    from pinn_amd import _lib, faultsets as F
    assert (_lib.FS_MAX_CLASSES, _lib.FS_MAX_LEVELS, _lib.FS_MAX_CAL, _lib.FS_TILE, _lib.FS_MAX_BLOCKS, _lib.FS_LINE, _lib.FS_HEADER) == (
        F.MAX_CLASSES, F.MAX_LEVELS, F.MAX_CAL, F.TILE, F.MAX_BLOCKS, F.LINE, F.HEADER)
    assert (_lib.FS_LAC, _lib.FS_MARGIN, _lib.FS_APS, _lib.FS_DENSITY) == tuple(F.KINDS[k] for k in ("lac", "margin", "aps", "density"))
    assert (_lib.FS_DRAW_CAL, _lib.FS_DRAW_TEST) == (F.DRAW_CAL, F.DRAW_TEST) and len({0, 1, _lib.AUC_DRAW_BOOT, F.DRAW_CAL, F.DRAW_TEST}) == 5
    assert (_lib.FS_REGIME_AUTO, _lib.FS_REGIME_LDS, _lib.FS_REGIME_SAMPLED, _lib.FS_REGIME_GLOBAL) == tuple(
        F.REGIMES[k] for k in ("auto", "lds", "sampled", "global"))
    assert (_lib.FS_LDS_ENTRIES, _lib.FS_AUTO_LDS_ENTRIES, _lib.FS_STAGE_MIN_ROWS, _lib.FS_MAGIC, _lib.FS_H_NCAL, _lib.FS_H_OFFSET) == (
        F.LDS_ENTRIES, F.AUTO_LDS_ENTRIES, F.STAGE_MIN_ROWS, F.MAGIC, F.H_NCAL, F.H_OFFSET)
    assert _lib.FS_AUTO_LDS_ENTRIES <= _lib.FS_GMM_LDS_ENTRIES
    assert (_lib.FS_T_N, _lib.FS_T_COVERED, _lib.FS_T_HIST, _lib.FS_T_SINGLE, _lib.FS_T_OUT_N, _lib.FS_T_OUT_NOVEL, _lib.FS_TALLY_WORDS) == (
        F.T_N, F.T_COVERED, F.T_HIST, F.T_SINGLE, F.T_OUT_N, F.T_OUT_NOVEL, F.TALLY_WORDS)
    assert _lib.FS_GMM_LDS_ENTRIES < _lib.FS_LDS_ENTRIES and _lib.GMM_MAX_CLASSES == F.MAX_CLASSES
    sizes = [0, 1, 2, 15, 16, 17, 4096, 10 ** 5, 1 << 20]
    for fn in (lib.pinn_fs_state_bytes, lib.pinn_fs_workspace_bytes):
        for C in (1, 2, 5, 16):
            b = [fn(n, C) for n in sizes]
            assert all(x <= y for x, y in zip(b, b[1:])) and b[0] > 0 and all(x % 256 == 0 for x in b)
        for n in sizes:
            b = [fn(n, C) for C in range(1, 17)]
            assert all(x <= y for x, y in zip(b, b[1:]))
        assert fn(-1, 4) == 0 and fn(10, 0) == 0 and fn(10, 17) == 0 and fn(4 * (1 << 20) + 1, 4) == 0 and fn(4 << 20, 4) > 0
    # room for every table and the pooled one, each padded to a line, behind the header
    for n, C in ((0, 1), (7, 3), (1000, 16), (1 << 20, 4)):
        assert lib.pinn_fs_state_bytes(n, C) >= 8 * (F.HEADER + 2 * n + F.LINE * (C + 1))
