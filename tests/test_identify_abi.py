"""CPU: the host-side checks of pinn_id_fit (csrc/pinn_identify.hip).  Every call below returns before any launch, with addresses
that are never dereferenced, as test_hmm_abi.py does; header, exports, ctypes and the module's constants agree."""
import ctypes
import os
import re

import pytest

E_ARG, OK = -1, 0
A = 0x1000                                  # an aligned non-NULL address, never dereferenced
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    return _lib.load(build_if_missing=False)


def opts(tol=1e-8, xtol=1e-14, mu0=1e-3, max_passes=100, reserved=0):
    from pinn_amd import _lib
    return ctypes.byref(_lib.IdOpts(tol, xtol, mu0, max_passes, reserved))


def fit(lib, arr=A, ld=4, n_arr=100, cols=(0, 1, 2, 3), model=0, ridx=None, n=100, ws=A, wl=A, nw=5, th0=A, stride=0, o=None, out=A, normal=A):
    c = None if cols is None else (ctypes.c_int * 4)(*cols)
    return lib.pinn_id_fit(arr, ld, n_arr, c, model, ridx, n, ws, wl, nw, th0, stride, o, out, normal, None)


def test_pinn_id_fit_checks_its_arguments_on_the_host(lib):
    nan, inf = float("nan"), float("inf")
    for bad in (dict(arr=None), dict(ws=None), dict(wl=None), dict(th0=None), dict(out=None), dict(cols=None),
                dict(arr=A + 4), dict(ridx=A + 4), dict(ws=A + 4), dict(wl=A + 4), dict(th0=A + 4), dict(out=A + 4), dict(normal=A + 4),
                dict(model=2), dict(model=-1), dict(stride=1), dict(stride=-3), dict(stride=6), dict(nw=-1), dict(n=-1), dict(n_arr=-1),
                dict(n=101), dict(ld=0), dict(cols=(0, 1, 2, 4)), dict(cols=(-1, 1, 2, 3)),
                dict(o=opts(tol=0.0)), dict(o=opts(tol=nan)), dict(o=opts(tol=inf)), dict(o=opts(tol=-1e-8)), dict(o=opts(xtol=0.0)),
                dict(o=opts(xtol=nan)), dict(o=opts(mu0=0.0)), dict(o=opts(mu0=inf)), dict(o=opts(mu0=-1.0)), dict(o=opts(max_passes=-1)),
                dict(o=opts(reserved=1))):
        assert fit(lib, **bad) == E_ARG, bad
    # no windows: nothing to do, whatever the window pointers are
    assert fit(lib, nw=0) == OK and fit(lib, nw=0, ws=None, wl=None, th0=None, out=None, normal=None) == OK
    assert fit(lib, nw=0, o=opts()) == OK and fit(lib, nw=0, stride=3, model=1, ridx=A, n=1000) == OK
    assert fit(lib, nw=0, o=opts(tol=nan)) == E_ARG                     # the options are checked before the early return


def test_header_exports_ctypes_and_constants_agree(lib):
    from pinn_amd import _lib, identify
    src = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PINN_ID_[A-Z_]+) (\d+)", src)}
    assert defs == {"PINN_ID_VOLTAGE": _lib.ID_VOLTAGE, "PINN_ID_THERMAL": _lib.ID_THERMAL, "PINN_ID_MAX_WINDOW": _lib.ID_MAX_WINDOW,
                    "PINN_ID_ONCHIP_ROWS": _lib.ID_ONCHIP_ROWS, "PINN_ID_FIT_WORDS": _lib.ID_FIT_WORDS, "PINN_ID_NORMAL_WORDS": _lib.ID_NORMAL_WORDS}
    assert (_lib.ID_MAX_WINDOW, _lib.ID_ONCHIP_ROWS, _lib.ID_FIT_WORDS, _lib.ID_NORMAL_WORDS) == (
        identify.MAX_WINDOW, identify.ONCHIP_ROWS, identify.FIT_WORDS, identify.NORMAL_WORDS)
    assert identify.MODELS == {"voltage": _lib.ID_VOLTAGE, "thermal": _lib.ID_THERMAL}
    assert "pinn_id_fit" in _lib.declared_symbols() and hasattr(lib, "pinn_id_fit")
    assert re.search(r"typedef struct pinn_id_opts \{ double tol, xtol, mu0; int max_passes; int reserved; \} pinn_id_opts_t;", src)
    assert ctypes.sizeof(_lib.IdOpts) == 32 and lib.pinn_abi_version() == 2
    import pinn_amd
    for name in ("voltage_table", "thermal_table", "sliding_windows", "fit_windows", "fit_baseline", "drift", "WindowFit", "ParameterTracker"):
        assert getattr(pinn_amd, name) is getattr(identify, name)
