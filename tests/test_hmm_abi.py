"""CPU: the host-side checks of the pinn_hmm_* entry points (csrc/pinn_hmm.hip).  Every call below returns before any launch,
with addresses that are never dereferenced, as test_abi.py's NULL-pointer test does."""
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


def cols(S):
    return (ctypes.c_int * max(S, 1))(*range(max(S, 1)))


def fb(lib, arr=A, S=3, n=10, model=A, seg=None, n_seg=0, cin=None, alpha=A, gamma=A, loglik=A, xi=A, gsum=A, cout=A, ws=A, wb=BIG,
       ridx=None, n_arr=None):
    return lib.pinn_hmm_forward_backward(arr, 8, n if n_arr is None else n_arr, cols(S), S, ridx, n, model, seg, n_seg, cin, 0, alpha, gamma,
                                         loglik, xi, gsum, cout, ws, wb, None)


def vit(lib, arr=A, S=3, n=10, model=A, seg=None, n_seg=0, cin=None, path=A, logprob=A, cout=A, ws=A, wb=BIG, ridx=None, n_arr=None):
    return lib.pinn_hmm_viterbi(arr, 8, n if n_arr is None else n_arr, cols(S), S, ridx, n, model, seg, n_seg, cin, path, logprob, cout, ws, wb,
                                None)


def mstep(lib, model=A, S=3, xi=A, loglik=A, n_seg=1, pseudo=None, tol=1e-6, max_hist=10):
    return lib.pinn_hmm_mstep(model, S, xi, loglik, n_seg, pseudo, tol, max_hist, None)


@pytest.mark.parametrize("call", [fb, vit], ids=["forward_backward", "viterbi"])
def test_scan_entry_points_check_their_arguments_on_the_host(lib, call):
    for bad in (dict(arr=None), dict(model=None), dict(ws=None), dict(arr=A + 4), dict(model=A + 4), dict(ws=A + 4), dict(cin=A + 4),
                dict(cout=A + 4), dict(ridx=A + 4), dict(seg=A + 4, n_seg=2), dict(seg=None, n_seg=2), dict(n_seg=-1),
                dict(S=0), dict(S=9), dict(n=-1, n_arr=10), dict(n=11, n_arr=10)):
        assert call(lib, **bad) == E_ARG, bad
    for n, S in ((1, 1), (10, 3), (1024, 8), (1025, 8), (100000, 5)):
        need = lib.pinn_hmm_workspace_bytes(n, S)
        assert need > 0 and need % 256 == 0
        assert call(lib, n=n, S=S, wb=need - 1) == E_WS, (n, S)
    assert call(lib, n=0) == OK and call(lib, n=0, ws=None, wb=0) == OK


def test_outputs_of_each_entry_point(lib):
    assert fb(lib, alpha=A + 4) == E_ARG and fb(lib, gamma=A + 4) == E_ARG and fb(lib, xi=A + 4) == E_ARG
    assert fb(lib, loglik=A + 4) == E_ARG and fb(lib, gsum=A + 4) == E_ARG
    assert vit(lib, path=None) == E_ARG and vit(lib, path=A + 4) == E_ARG and vit(lib, logprob=A + 4) == E_ARG


def test_mstep_checks_its_arguments_on_the_host(lib):
    """pinn_hmm_mstep has no workspace and no row count: its sizes are S and the number of segments."""
    for bad in (dict(model=None), dict(xi=None), dict(loglik=None), dict(model=A + 4), dict(xi=A + 4), dict(loglik=A + 4),
                dict(pseudo=A + 4), dict(S=0), dict(S=9), dict(n_seg=-1), dict(max_hist=-1), dict(tol=float("nan"))):
        assert mstep(lib, **bad) == E_ARG, bad
    assert mstep(lib, n_seg=0) == OK


def test_workspace_is_monotone(lib):
    from pinn_amd import _lib, temporal
    assert (_lib.HMM_MAX_STATES, _lib.HMM_TILE, _lib.HMM_ROWS_PER_THREAD) == (temporal.MAX_STATES, temporal.TILE, temporal.ROWS_PER_THREAD)
    sizes = [1, 2, 15, 16, 17, 1023, 1024, 1025, 2049, 5123, 10 ** 6, 10 ** 7]
    for S in range(1, 9):
        b = [lib.pinn_hmm_workspace_bytes(n, S) for n in sizes]
        assert all(x <= y for x, y in zip(b, b[1:])) and b[0] > 0
    for n in sizes:
        b = [lib.pinn_hmm_workspace_bytes(n, S) for S in range(1, 9)]
        assert all(x <= y for x, y in zip(b, b[1:]))
    assert lib.pinn_hmm_workspace_bytes(0, 3) == 0 and lib.pinn_hmm_workspace_bytes(10, 0) == 0 and lib.pinn_hmm_workspace_bytes(10, 9) == 0
