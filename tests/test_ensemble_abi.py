"""CPU: the host-side contract of the deep-ensemble entry points (pinn_gens_*): every bad call is refused before any launch, with
addresses that are never dereferenced, and the workspace is E copies of one network's."""
import ctypes

import pytest

import ensemble_cases as EC

OK, E_ARG, E_ARCH, E_WORKSPACE = 0, -1, -2, -3
AL = ctypes.c_void_p(0x1000)            # 16-byte aligned, never dereferenced
MIS = ctypes.c_void_p(0x1004)           # 4-byte aligned only
BIG = 1 << 50                           # "large enough" for every workspace check
LAYERS = [8, 64, 200, 48, 1]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    return _lib.load(build_if_missing=False)


def _drop(mode=None, d_bits=None, counter=None, p=0.2):
    from pinn_amd import _lib
    d = _lib.Dropout()
    d.mode = _lib.DROP_PHILOX if mode is None else mode
    for l in range(len(LAYERS) - 1):
        d.p[l] = p
    d.d_bits = d_bits
    d.d_step_counter = counter
    return ctypes.byref(d)


def _calls(lib, net=None, e=4, par=AL, x=AL, y=AL, n=10, drop=None, u=AL, lv=AL, g=AL, loss=AL, work=AL, wb=BIG, m=AL, v=AL, step=1):
    net = EC.gnet(LAYERS) if net is None else net
    return {
        "forward": lib.pinn_gens_forward(net, e, par, x, n, drop, u, lv, work, wb, None),
        "train_grads": lib.pinn_gens_train_grads(net, e, par, x, y, n, n if n > 0 else 1, drop, g, loss, work, wb, None),
        "train_step": lib.pinn_gens_train_step(net, e, par, x, y, n, n if n > 0 else 1, drop, g, loss, work, wb, m, v, 0.01, step, None),
    }


def _all(lib, rc, **kw):
    got = _calls(lib, **kw)
    assert got == {k: rc for k in got}, (kw, got)


def test_member_count_is_1_to_32(lib):
    for e in (0, 33, -1):
        _all(lib, E_ARG, e=e)
        assert lib.pinn_gens_workspace_bytes(EC.gnet(LAYERS), e, 100) == 0
        assert lib.pinn_gens_combine(AL, AL, e, 10, 0, AL, AL, AL, None) == E_ARG
    # the limits themselves pass the check (and fail the next one: a workspace of 16 bytes)
    for e in (1, 32):
        _all(lib, E_WORKSPACE, e=e, wb=16)
        assert lib.pinn_gens_workspace_bytes(EC.gnet(LAYERS), e, 100) > 0


def test_null_and_misaligned_pointers(lib):
    for bad in (None, MIS):
        _all(lib, E_ARG, par=bad)
        _all(lib, E_ARG, x=bad)
        _all(lib, E_ARG, work=bad)
        got = _calls(lib, g=bad)
        assert got["train_grads"] == E_ARG and got["train_step"] == E_ARG, got
    got = _calls(lib, y=None)
    assert got["train_grads"] == E_ARG and got["train_step"] == E_ARG, got
    got = _calls(lib, loss=None)
    assert got["train_grads"] == E_ARG and got["train_step"] == E_ARG, got
    assert _calls(lib, u=None)["forward"] == E_ARG
    assert _calls(lib, lv=None)["forward"] == E_ARG
    assert _calls(lib, m=None)["train_step"] == E_ARG
    assert _calls(lib, v=None)["train_step"] == E_ARG
    assert _calls(lib, step=0)["train_step"] == E_ARG
    for k in range(5):
        args = [AL, AL, 4, 10, 0, AL, AL, AL, None]
        args[(0, 1, 5, 6, 7)[k]] = None
        assert lib.pinn_gens_combine(*args) == E_ARG, k
    for rule in (-1, 2):
        assert lib.pinn_gens_combine(AL, AL, 4, 10, rule, AL, AL, AL, None) == E_ARG


def test_dropout_modes(lib):
    from pinn_amd import _lib
    # injected bit masks and the device step counter belong to the single-network calls
    _all(lib, E_ARG, drop=_drop(mode=_lib.DROP_BITS, d_bits=0x2000))
    _all(lib, E_ARG, drop=_drop(mode=_lib.DROP_BITS))
    _all(lib, E_ARG, drop=_drop(counter=0x3000))
    _all(lib, E_ARG, drop=_drop(mode=_lib.DROP_NONE, counter=0x3000))
    # the rest of the struct is validated as everywhere
    _all(lib, E_ARG, drop=_drop(mode=3))
    _all(lib, E_ARG, drop=_drop(p=1.0))
    # Philox, eval and no struct pass the check (and fail the next one)
    for d in (_drop(), _drop(mode=_lib.DROP_NONE), None):
        _all(lib, E_WORKSPACE, drop=d, wb=16)


def test_bad_architecture(lib):
    from pinn_amd import _lib
    for layers in ([7, 64, 1], [8, 64, 2], [8, 1], [8, 64, 3, 1], [8, 4096, 1], [8] + [16] * 9 + [1]):
        net = ctypes.byref(_lib.GNet(layers))
        _all(lib, E_ARCH, net=net)
        assert lib.pinn_gens_workspace_bytes(net, 4, 100) == 0
        rows, slices = ctypes.c_longlong(), ctypes.c_int()
        assert lib.pinn_gens_train_plan(net, 100, ctypes.byref(rows), ctypes.byref(slices)) == E_ARCH


def test_short_workspace_and_no_rows(lib):
    net = EC.gnet(LAYERS)
    for e in (1, 3, 32):
        need = lib.pinn_gens_workspace_bytes(net, e, 1000)
        # one member short: the training calls need every byte of the query (the forward needs fewer, and runs in what it needs)
        got = _calls(lib, e=e, n=1000, wb=need // e * (e - 1) + 16)
        assert got["train_grads"] == E_WORKSPACE and got["train_step"] == E_WORKSPACE, (e, got)
        got = _calls(lib, e=e, n=1000, wb=need - 1)
        assert got["train_grads"] == E_WORKSPACE and got["train_step"] == E_WORKSPACE, (e, got)
        _all(lib, E_WORKSPACE, e=e, n=1000, wb=16)
        _all(lib, E_WORKSPACE, e=e, n=1000, wb=0)
    # n_rows == 0: nothing to do, whatever the row pointers and the workspace are
    _all(lib, OK, n=0, x=None, y=None, u=None, lv=None, work=None, wb=0)
    assert lib.pinn_gens_combine(None, None, 4, 0, 0, None, None, None, None) == OK
    _all(lib, E_ARG, n=-1)
    assert lib.pinn_gens_workspace_bytes(net, 4, -1) == 0


def test_workspace_is_members_times_one_network(lib):
    """One member needs no more than the single-network calls; E members need E times one member's, up to alignment (the
    per-member regions are whole 256-byte blocks, so here it is exact)."""
    for layers in EC.LAYERS + [LAYERS, EC.WIDE]:
        net = EC.gnet(layers)
        for n in EC.ROWS + [0, 20000]:
            one = lib.pinn_gens_workspace_bytes(net, 1, n)
            assert 0 < one <= lib.pinn_gnet_workspace_bytes(net, n, 0), (layers, n)
            assert one % 256 == 0
            for e in EC.MEMBERS:
                got = lib.pinn_gens_workspace_bytes(net, e, n)
                assert e * one <= got <= e * (one + 256), (layers, n, e)


def test_train_plan_does_not_depend_on_members(lib):
    """A member's chunk rows and slices come from the row count and the net alone (the query takes no member count), chunks are whole
    64-row tiles, and the largest grid extent a weight-gradient launch can ask for stays inside the limit: a chunk has at most
    131 072 rows and a slice at least 128, so at most 1024 slices in the grid's z, and the member rides in the grid's x."""
    for layers in EC.LAYERS + [LAYERS, EC.WIDE]:
        for n in (1, 200, 4200, 131072, 1 << 20):
            rows, slices = EC.train_plan(lib, layers, n)
            assert rows % 64 == 0 and 64 <= rows <= 131072
            assert 1 <= slices <= 1024
            assert slices * 32 <= 65535
    rows, slices = ctypes.c_longlong(), ctypes.c_int()
    assert lib.pinn_gens_train_plan(EC.gnet(LAYERS), 100, None, ctypes.byref(slices)) == E_ARG
    assert lib.pinn_gens_train_plan(EC.gnet(LAYERS), -1, ctypes.byref(rows), ctypes.byref(slices)) == E_ARG
