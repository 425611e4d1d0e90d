"""CPU: the host-side checks of the pinn_cp_* entry points (csrc/pinn_changepoint.hip).  Every call below returns before any
launch, with addresses that are never dereferenced, as test_hmm_abi.py does."""
import ctypes
import os
import re

import pytest

E_ARG, E_WS, OK = -1, -3, 0
A = 0x1000                                  # an aligned non-NULL address, never dereferenced
BIG = 1 << 40
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    return _lib.load(build_if_missing=False)


def doubles(v):
    return None if v is None else (ctypes.c_double * len(v))(*v)


def opts(kind=0, min_len=2, max_len=0, prune=1, block=0, floor=1e-8, launch=0):
    from pinn_amd import _lib
    return _lib.CpOpts(kind, min_len, max_len, prune, block, floor, launch)


def seg(lib, arr=A, D=3, n=100, n_arr=None, ridx=None, mu=None, sigma=None, starts=None, d_starts=A, o=None, pens=(1.0,), n_pen=None,
        F=A, ncp=A, cp=A, cap=8, evals=A, status=A, ws=A, wb=BIG, ld=8, no_opts=False, no_pens=False):
    cols = (ctypes.c_int * max(D, 1))(*range(max(D, 1)))
    ns = 0 if starts is None else len(starts)
    c_starts = None if starts is None else (ctypes.c_longlong * ns)(*starts)
    o = opts() if o is None else o
    return lib.pinn_cp_segment(arr, ld, n if n_arr is None else n_arr, cols, D, ridx, n, doubles(mu), doubles(sigma), c_starts,
                               d_starts if starts is not None else None, ns, None if no_opts else ctypes.byref(o),
                               None if no_pens else doubles(list(pens)), len(pens) if n_pen is None else n_pen, F, ncp, cp, cap, evals,
                               status, ws, wb, None)


def win(lib, arr=A, D=3, n=100, n_arr=None, ring_start=0, mu=None, sigma=None, o=None, pens=(1.0,), n_pen=None, F=A, ncp=A, cp=A, cap=8,
        evals=A, status=A, ws=A, wb=BIG, ld=8, no_opts=False, no_pens=False):
    cols = (ctypes.c_int * max(D, 1))(*range(max(D, 1)))
    o = opts() if o is None else o
    return lib.pinn_cp_window(arr, ld, n if n_arr is None else n_arr, cols, D, ring_start, n, doubles(mu), doubles(sigma),
                              None if no_opts else ctypes.byref(o), None if no_pens else doubles(list(pens)),
                              len(pens) if n_pen is None else n_pen, F, ncp, cp, cap, evals, status, ws, wb, None)


SHARED_BAD = (dict(arr=None), dict(arr=A + 4), dict(F=None), dict(F=A + 4), dict(ncp=None), dict(ncp=A + 4), dict(cp=None), dict(cp=A + 4),
              dict(evals=None), dict(evals=A + 4), dict(status=None), dict(status=A + 4), dict(ws=None), dict(ws=A + 4),
              dict(D=0), dict(D=9), dict(n=-1, n_arr=10), dict(n=11, n_arr=10), dict(ld=0), dict(no_opts=True), dict(no_pens=True),
              dict(n_pen=0), dict(pens=(1.0,) * 17), dict(cap=-1),
              dict(o=("kind", 2)), dict(o=("kind", -1)), dict(o=("min_len", 0)), dict(o=("kind", 1, "min_len", 1)), dict(o=("min_len", 5, "max_len", 4)),
              dict(o=("max_len", -1)), dict(o=("block", 65)), dict(o=("block", -1)), dict(o=("launch", -1)),
              dict(o=("floor", -1e-9)), dict(o=("floor", NAN)), dict(o=("floor", INF)),
              dict(pens=(NAN,)), dict(pens=(1.0, -0.5)), dict(pens=(INF,)),
              dict(mu=[0.0] * 3), dict(sigma=[1.0] * 3), dict(mu=[0.0] * 3, sigma=[1.0, 0.0, 1.0]), dict(mu=[0.0, NAN, 0.0], sigma=[1.0] * 3),
              dict(mu=[0.0] * 3, sigma=[1.0, INF, 1.0]))


def expand(bad):
    bad = dict(bad)
    if "o" in bad:
        kv = bad["o"]
        bad["o"] = opts(**{kv[i]: kv[i + 1] for i in range(0, len(kv), 2)})
    return bad


@pytest.mark.parametrize("call", [seg, win], ids=["segment", "window"])
def test_both_entry_points_check_their_arguments_on_the_host(lib, call):
    for bad in SHARED_BAD:
        assert call(lib, **expand(bad)) == E_ARG, bad
    assert call(lib, n=0) == OK and call(lib, n=0, ws=None, wb=0) == OK      # (a call that passes every check would launch: none is made)
    assert call(lib, n=0, o=opts(min_len=0)) == E_ARG              # the options are checked before n = 0 returns


def test_segment_starts_are_checked_on_the_host(lib):
    for starts in ([0, 50, 40], [0, 50, 50], [1, 50], [0, 100], [0, 50, 120], [-1, 50]):
        assert seg(lib, starts=starts) == E_ARG, starts
    assert seg(lib, starts=[0, 50], d_starts=None) == E_ARG and seg(lib, starts=[0, 50], d_starts=A + 4) == E_ARG
    assert seg(lib, ridx=A + 4) == E_ARG
    need = lib.pinn_cp_workspace_bytes(100, 3, 3, 1)
    assert seg(lib, starts=[0, 50, 70], wb=need - 1) == E_WS      # ascending starts pass the checks and reach the workspace's


def test_the_window_form_checks_its_ring(lib):
    assert win(lib, n=4097, n_arr=4097) == E_ARG and win(lib, ring_start=-1) == E_ARG and win(lib, ring_start=100) == E_ARG
    assert win(lib, n=50, n_arr=100, ring_start=99, wb=0) == E_WS


@pytest.mark.parametrize("call", [seg, win], ids=["segment", "window"])
def test_a_workspace_one_byte_short_is_refused(lib, call):
    for n, D, n_pen in ((1, 1, 1), (100, 3, 1), (255, 8, 5), (256, 4, 16), (257, 8, 2), (4096, 8, 16)):
        need = lib.pinn_cp_workspace_bytes(n, D, 0, n_pen)
        assert need > 0 and need % 256 == 0
        assert call(lib, n=n, D=D, pens=(1.0,) * n_pen, wb=need - 1) == E_WS, (n, D, n_pen)
    for n, D, starts, n_pen in ((100000, 5, [0, 7, 5000, 99999], 3), (1025, 2, [0, 1024], 1)):
        need = lib.pinn_cp_workspace_bytes(n, D, len(starts), n_pen)
        assert need > lib.pinn_cp_workspace_bytes(n, D, 0, n_pen) - 1
        assert seg(lib, n=n, D=D, starts=starts, pens=(1.0,) * n_pen, wb=need - 1) == E_WS, (n, D)


def test_workspace_is_monotone_and_the_constants_are_the_headers(lib):
    from pinn_amd import _lib, changepoint as cp
    assert (_lib.CP_MAX_FEAT, _lib.CP_MAX_PEN, _lib.CP_MAX_SEGMENTS, _lib.CP_MAX_WINDOW, _lib.CP_TILE, _lib.CP_BLOCK, _lib.CP_LAUNCH_EVALS) == \
        (cp.MAX_FEAT, cp.MAX_PEN, cp.MAX_SEGMENTS, cp.MAX_WINDOW, cp.TILE, cp.BLOCK, cp.LAUNCH_EVALS)
    assert (_lib.CP_MEAN, _lib.CP_MEANVAR) == (cp.KINDS["mean"], cp.KINDS["meanvar"])
    assert (_lib.CP_BAD_ROW, _lib.CP_OVERFLOW, _lib.CP_INFEASIBLE) == (cp.BAD_ROW, cp.OVERFLOW, cp.INFEASIBLE)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pinn_hip.h")).read()
    macros = {m.group(1): m.group(2) for m in re.finditer(r"#define PINN_CP_(\w+) (\(1LL << \d+\)|\d+)", header)}
    value = {k: (1 << int(re.search(r"<< (\d+)", v).group(1)) if "<<" in v else int(v)) for k, v in macros.items()}
    assert value == dict(MAX_FEAT=cp.MAX_FEAT, MAX_PEN=cp.MAX_PEN, MAX_SEGMENTS=cp.MAX_SEGMENTS, MAX_WINDOW=cp.MAX_WINDOW, TILE=cp.TILE,
                         BLOCK=cp.BLOCK, LAUNCH_EVALS=cp.LAUNCH_EVALS, MEAN=0, MEANVAR=1, BAD_ROW=cp.BAD_ROW, OVERFLOW=cp.OVERFLOW,
                         INFEASIBLE=cp.INFEASIBLE)
    assert ctypes.sizeof(_lib.CpOpts) == 40
    sizes = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2049, 5123, 10 ** 6, 10 ** 7]
    for D in range(1, 9):
        b = [lib.pinn_cp_workspace_bytes(n, D, 0, 1) for n in sizes]
        assert all(x <= y for x, y in zip(b, b[1:])) and b[0] > 0
    for n in sizes:
        for f in (lambda v: lib.pinn_cp_workspace_bytes(n, v, 0, 3), lambda v: lib.pinn_cp_workspace_bytes(n, 4, 0, v)):
            b = [f(v) for v in range(1, 9)]
            assert all(x <= y for x, y in zip(b, b[1:]))
        b = [lib.pinn_cp_workspace_bytes(n, 4, s, 2) for s in (0, 1, 2, 3, 100, 65535)]
        assert b[0] == b[1] and all(x <= y for x, y in zip(b, b[1:]))
    for bad in ((0, 3, 0, 1), (10, 0, 0, 1), (10, 9, 0, 1), (10, 3, 0, 0), (10, 3, 0, 17), (10, 3, 65536, 1), (10, 3, -1, 1), (1 << 31, 3, 0, 1)):
        assert lib.pinn_cp_workspace_bytes(*bad) == 0, bad
