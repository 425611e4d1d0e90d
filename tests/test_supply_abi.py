"""CPU: the host-side checks of pinn_bp_fit (csrc/pinn_breakpoint.hip).  Every call below returns before any launch, with addresses
that are never dereferenced, as test_identify_abi.py does; header, exports, ctypes and the module's constants agree."""
import ctypes
import os
import re

import pytest

import supply_cases  # noqa: F401  (the shared cases import the module under test)

E_ARG, OK = -1, 0
A = 0x1000                                  # an aligned non-NULL address, never dereferenced
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    return _lib.load(build_if_missing=False)


def opts(q=3.841458820694124, reserved=0, reserved2=0):
    from pinn_amd import _lib
    return ctypes.byref(_lib.BpOpts(q, reserved, reserved2))


def fit(lib, arr=A, ld=2, n_arr=100, cols=(0, 1), ridx=None, n=100, ws=A, wl=A, nw=5, longest=64, o=None, out=A):
    c = None if cols is None else (ctypes.c_int * 2)(*cols)
    return lib.pinn_bp_fit(arr, ld, n_arr, c, ridx, n, ws, wl, nw, longest, o, out, None)


def test_pinn_bp_fit_checks_its_arguments_on_the_host(lib):
    nan, inf = float("nan"), float("inf")
    for bad in (dict(arr=None), dict(ws=None), dict(wl=None), dict(out=None), dict(cols=None),
                dict(arr=A + 4), dict(ridx=A + 4), dict(ws=A + 4), dict(wl=A + 4), dict(out=A + 4),
                dict(nw=-1), dict(n=-1), dict(n_arr=-1), dict(longest=-1), dict(n=101), dict(ld=0), dict(ld=-2),
                dict(cols=(0, 2)), dict(cols=(-1, 1)), dict(ld=1),
                dict(o=opts(q=0.0)), dict(o=opts(q=nan)), dict(o=opts(q=inf)), dict(o=opts(q=-3.84)),
                dict(o=opts(reserved=1)), dict(o=opts(reserved2=1))):
        assert fit(lib, **bad) == E_ARG, bad
    # no windows: nothing to do, whatever the window pointers are
    assert fit(lib, nw=0) == OK and fit(lib, nw=0, ws=None, wl=None, out=None) == OK
    assert fit(lib, nw=0, o=opts()) == OK and fit(lib, nw=0, ridx=A, n=1000, longest=10 ** 9) == OK
    assert fit(lib, nw=0, o=opts(q=nan)) == E_ARG and fit(lib, nw=0, o=opts(reserved=2)) == E_ARG       # the options are checked before the early return


def test_header_exports_ctypes_and_constants_agree(lib):
    from pinn_amd import _lib, supply
    src = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PINN_BP_[A-Z_]+) (\d+)", src)}
    assert defs == {"PINN_BP_MAX_WINDOW": _lib.BP_MAX_WINDOW, "PINN_BP_FIT_WORDS": _lib.BP_FIT_WORDS} == {"PINN_BP_MAX_WINDOW": 4096, "PINN_BP_FIT_WORDS": 24}
    assert (_lib.BP_MAX_WINDOW, _lib.BP_FIT_WORDS) == (supply.MAX_WINDOW, supply.FIT_WORDS)
    assert "pinn_bp_fit" in _lib.declared_symbols() and hasattr(lib, "pinn_bp_fit")
    assert re.search(r"typedef struct pinn_bp_opts \{ double q; int reserved; int reserved2; \} pinn_bp_opts_t;", src)
    assert ctypes.sizeof(_lib.BpOpts) == 16 and lib.pinn_abi_version() == 2
    assert supply.Q95 == 3.841458820694124 and supply.THETA_NAMES == ("l1", "l2", "l3")
    # the identification entry point and its names stay as they were
    assert {k for k in re.findall(r"#define (PINN_ID_[A-Z_]+) ", src)} == {"PINN_ID_VOLTAGE", "PINN_ID_THERMAL", "PINN_ID_MAX_WINDOW", "PINN_ID_ONCHIP_ROWS",
                                                                        "PINN_ID_FIT_WORDS", "PINN_ID_NORMAL_WORDS"}
