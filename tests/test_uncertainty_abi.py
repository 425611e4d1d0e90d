"""CPU: the host-side checks of the pinn_unc_* entry points (csrc/pinn_uncertainty.hip).  Every call below returns before any
launch, with addresses that are never dereferenced, as test_hmm_abi.py does."""
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


def dbls(v):
    return (ctypes.c_double * max(len(v), 1))(*v)


def head(arr, ld, n_arr, cols, ridx, n):
    return (arr, ld, n if n_arr is None else n_arr, ints(cols), len(cols), ridx, n)


def groups_of(G, n_labels, label_col, table):
    if table is None:
        table = [i % max(G, 1) for i in range(max(n_labels, 1))]
    return (label_col, ints(table), n_labels, G)


def score(lib, arr=A, ld=22, n=10, n_arr=None, cols=(8, 9, 10, 11), ridx=None, G=3, n_labels=13, label_col=17, table=None, vm=(1.0, 1.0, 0.0),
          levels=(0.67, 1.64), edges=(-1.0, 0.0, 1.0), L=None, B=None, sums=A, cnt=A, hits=A, pit=A, skipped=A, z=None, phi=None, crps=None,
          nll=None, ws=A, wb=BIG, null_vm=False, null_table=False):
    g = groups_of(G, n_labels, label_col, table)
    if null_table:
        g = (g[0], None, g[2], g[3])
    return lib.pinn_unc_score(*head(arr, ld, n_arr, cols, ridx, n), *g, None if null_vm else dbls(vm), dbls(levels),
                              len(levels) if L is None else L, dbls(edges), len(edges) + 1 if B is None else B, sums, cnt, hits, pit, skipped,
                              z, phi, crps, nll, ws, wb, None)


def quant(lib, arr=A, ld=22, n=10, n_arr=None, cols=(8, 9, 10, 11), ridx=None, G=3, n_labels=13, label_col=17, table=None, vm=(1.0, 1.0, 0.0),
          kind=0, score_col=0, levels=(0.9,), Q=None, conformal=1, q=A, rank=A, cnt=A, skipped=A, ws=A, wb=BIG, null_vm=False):
    return lib.pinn_unc_quantiles(*head(arr, ld, n_arr, cols, ridx, n), *groups_of(G, n_labels, label_col, table), None if null_vm else dbls(vm),
                                  kind, score_col, dbls(levels), len(levels) if Q is None else Q, conformal, q, rank, cnt, skipped, ws, wb, None)


def update(lib, arr=A, ld=22, n=10, n_arr=None, cols=(8, 9, 10, 11), ridx=None, vm=(1.0, 1.0, 0.0), level=0.9, gamma=0.0, amin=0.0, amax=1.0,
           W=64, learn=1, state=A, lo=A, hi=A, z=A, flag=A, null_vm=False):
    return lib.pinn_unc_update(*head(arr, ld, n_arr, cols, ridx, n), None if null_vm else dbls(vm), level, gamma, amin, amax, W, learn, state,
                               lo, hi, z, flag, None)


ROW_ERRORS = (dict(arr=None), dict(arr=A + 4), dict(ridx=A + 4), dict(n=-1, n_arr=10), dict(n=11, n_arr=10), dict(ld=0), dict(cols=(8, 9, 10)),
              dict(cols=(8, 9, 10, 11, 12)), dict(cols=(8, 9, 10, 22)), dict(cols=(-1, 9, 10, 11)), dict(null_vm=True), dict(vm=(1.0, -1.0, 0.0)),
              dict(vm=(float("nan"), 1.0, 0.0)), dict(vm=(float("inf"), 1.0, 0.0)))
GROUP_ERRORS = (dict(G=0), dict(G=17), dict(n_labels=0), dict(n_labels=65), dict(label_col=22), dict(label_col=-2), dict(table=[0, 1, 3] + [0] * 10),
                dict(table=[0, -2, 1] + [0] * 10), dict(label_col=-1, G=2))


def test_score_checks_its_arguments_on_the_host(lib):
    for bad in ROW_ERRORS + GROUP_ERRORS + (
            dict(null_table=True), dict(L=0), dict(L=17), dict(B=0), dict(B=65), dict(edges=(0.0, 0.0)), dict(edges=(1.0, 0.0)),
            dict(edges=(0.0, float("nan"))), dict(levels=(-1.0,)), dict(levels=(float("nan"),)), dict(sums=None), dict(cnt=None), dict(hits=None),
            dict(pit=None), dict(skipped=None), dict(sums=A + 4), dict(cnt=A + 4), dict(hits=A + 4), dict(pit=A + 4), dict(skipped=A + 4),
            dict(z=A + 4), dict(phi=A + 4), dict(crps=A + 4), dict(nll=A + 4), dict(ws=None), dict(ws=A + 4)):
        assert score(lib, **bad) == E_ARG, bad
    assert score(lib, levels=tuple([1.0] * 16), edges=tuple(float(i) for i in range(63)), n=0) == OK      # the limits themselves are inside
    assert score(lib, G=16, n_labels=64, n=0) == OK and score(lib, label_col=-1, G=1, n=0) == OK
    assert score(lib, n=0) == OK and score(lib, n=0, ws=None, wb=0) == OK


def test_quantiles_check_their_arguments_on_the_host(lib):
    for bad in ROW_ERRORS + GROUP_ERRORS + (
            dict(Q=0), dict(Q=9), dict(levels=tuple([0.5] * 9)), dict(G=13, levels=tuple([0.5] * 5)), dict(G=9, levels=tuple([0.5] * 8)),
            dict(levels=(0.0,)), dict(levels=(1.5,)), dict(levels=(float("nan"),)), dict(kind=3), dict(kind=-1), dict(kind=2, score_col=22),
            dict(kind=2, score_col=-1), dict(q=None), dict(rank=None), dict(cnt=None), dict(skipped=None), dict(q=A + 4), dict(rank=A + 4),
            dict(cnt=A + 4), dict(skipped=A + 4), dict(ws=None), dict(ws=A + 4), dict(n=(1 << 40) + 1, n_arr=1 << 41)):
        assert quant(lib, **bad) == E_ARG, bad
    assert quant(lib, G=16, n_labels=64, levels=(0.1, 0.5, 0.9, 1.0), n=0) == OK and quant(lib, G=8, levels=tuple([0.5] * 8), n=0) == OK
    assert quant(lib, n=0) == OK and quant(lib, n=0, ws=None, wb=0) == OK


def test_update_checks_its_arguments_on_the_host(lib):
    for bad in ROW_ERRORS + (
            dict(W=0), dict(W=4097), dict(n=2049, n_arr=5000), dict(level=0.0), dict(level=1.0), dict(level=float("nan")), dict(gamma=-0.1),
            dict(gamma=float("inf")), dict(gamma=float("nan")), dict(amin=-0.1), dict(amax=1.1), dict(amin=0.5, amax=0.4), dict(amin=float("nan")),
            dict(state=None), dict(state=A + 4), dict(lo=A + 4), dict(hi=A + 4), dict(z=A + 4), dict(flag=A + 2)):
        assert update(lib, **bad) == E_ARG, bad
    assert update(lib, n=0) == OK and update(lib, n=0, W=4096) == OK and update(lib, n=0, lo=None, hi=None, z=None, flag=None) == OK
    assert lib.pinn_unc_state_bytes(0) == 0 and lib.pinn_unc_state_bytes(4097) == 0
    assert lib.pinn_unc_state_bytes(1) == 9 * 8 and lib.pinn_unc_state_bytes(4096) == (8 + 4096) * 8


def test_workspace_is_monotone_aligned_and_enforced(lib):
    from pinn_amd import _lib, uncertainty as U
    assert (_lib.UNC_TILE, _lib.UNC_MAX_BLOCKS, _lib.UNC_MAX_GROUPS, _lib.UNC_MAX_LABELS, _lib.UNC_MAX_LEVELS, _lib.UNC_MAX_BINS,
            _lib.UNC_MAX_QUANTILES, _lib.UNC_MAX_TARGETS, _lib.UNC_MAX_WINDOW, _lib.UNC_MAX_CHUNK, _lib.UNC_STATE_HEADER) == (
        U.TILE, U.MAX_BLOCKS, U.MAX_GROUPS, U.MAX_LABELS, U.MAX_LEVELS, U.MAX_BINS, U.MAX_QUANTILES, U.MAX_TARGETS, U.MAX_WINDOW, U.MAX_CHUNK,
        U.STATE_HEADER)
    assert (_lib.UNC_ABS_Z, _lib.UNC_Z, _lib.UNC_COLUMN) == (U.KINDS["abs_z"], U.KINDS["z"], U.KINDS["column"]) and _lib.UNC_SUMS == len(U.SUM_NAMES)
    sizes = [0, 1, 2, 2047, 2048, 2049, 10 ** 5, 2048 * 1024 - 1, 2048 * 1024, 2048 * 1024 + 1, 10 ** 7]
    for G, Q in ((1, 1), (1, 8), (5, 1), (8, 8), (16, 4)):
        b = [lib.pinn_unc_workspace_bytes(n, G, Q) for n in sizes]
        assert all(x <= y for x, y in zip(b, b[1:])) and b[0] > 0 and all(x % 256 == 0 for x in b)
    for n in sizes:
        b = [lib.pinn_unc_workspace_bytes(n, G, 4) for G in range(1, 17)]
        assert all(x <= y for x, y in zip(b, b[1:]))
        b = [lib.pinn_unc_workspace_bytes(n, 8, Q) for Q in range(1, 9)]
        assert all(x <= y for x, y in zip(b, b[1:]))
    for G, Q in ((0, 1), (17, 1), (1, 0), (1, 9), (13, 5), (9, 8)):
        assert lib.pinn_unc_workspace_bytes(10, G, Q) == 0, (G, Q)
    assert lib.pinn_unc_workspace_bytes(-1, 1, 1) == 0
    for n, G, Q in ((1, 1, 1), (10, 3, 1), (5000, 16, 4), (10 ** 7, 8, 8)):
        assert quant(lib, n=n, G=G, n_labels=16, levels=tuple([0.5] * Q), wb=lib.pinn_unc_workspace_bytes(n, G, Q) - 1) == E_WS, (n, G, Q)
        assert score(lib, n=n, G=G, n_labels=16, wb=lib.pinn_unc_workspace_bytes(n, G, 1) - 1) == E_WS, (n, G)
