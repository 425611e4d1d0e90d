"""CPU: argument checks of pinn_gnet_backward (the autograd backward, csrc/pinn_general.hip) and the ctypes binding."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    return _lib.load(build_if_missing=False)


def _call(lib, net, params, x, n, gu, grads, gx, work, wbytes, glv=None, drop=None):
    from pinn_amd import _lib
    return lib.pinn_gnet_backward(ctypes.byref(_lib.GNet(net)), params, x, n, drop, gu, glv, grads, gx, work, wbytes, None)


def test_backward_bound_and_declared(lib):
    from pinn_amd import _lib
    assert "pinn_gnet_backward" in _lib.declared_symbols()
    assert lib.pinn_gnet_backward.argtypes[0] is ctypes.POINTER(_lib.GNet)
    assert len(lib.pinn_gnet_backward.argtypes) == 12


def test_backward_rejects_bad_arguments_without_a_gpu(lib):
    """Argument checks run before anything touches the device."""
    net = [8, 100, 100, 1]
    fake = ctypes.c_void_p(1 << 20)
    mis = ctypes.c_void_p((1 << 20) + 4)
    big = 1 << 30
    # NULL params, x, g_u, grads
    assert _call(lib, net, None, fake, 10, fake, fake, fake, fake, big) == -1
    assert _call(lib, net, fake, None, 10, fake, fake, fake, fake, big) == -1
    assert _call(lib, net, fake, fake, 10, None, fake, fake, fake, big) == -1
    assert _call(lib, net, fake, fake, 10, fake, None, fake, fake, big) == -1
    # misaligned params, x, grads, dx, workspace
    assert _call(lib, net, mis, fake, 10, fake, fake, fake, fake, big) == -1
    assert _call(lib, net, fake, mis, 10, fake, fake, fake, fake, big) == -1
    assert _call(lib, net, fake, fake, 10, fake, mis, fake, fake, big) == -1
    assert _call(lib, net, fake, fake, 10, fake, fake, mis, fake, big) == -1
    assert _call(lib, net, fake, fake, 10, fake, fake, fake, mis, big) == -1
    # negative rows, NULL workspace
    assert _call(lib, net, fake, fake, -1, fake, fake, fake, fake, big) == -1
    assert _call(lib, net, fake, fake, 10, fake, fake, fake, None, big) == -1
    # too-small workspace, unsupported net
    assert _call(lib, net, fake, fake, 10, fake, fake, fake, fake, 16) == -3
    assert _call(lib, [8, 100, 3, 1], fake, fake, 10, fake, fake, fake, fake, big) == -2
    assert _call(lib, [8, 2049, 32, 1], fake, fake, 10, fake, fake, fake, fake, big) == -2


def test_backward_rejects_bad_dropout_without_a_gpu(lib):
    from pinn_amd import _lib
    net = [8, 32, 32, 32, 1]
    fake = ctypes.c_void_p(1 << 20)
    d = _lib.Dropout()
    d.mode = 2                        # BITS without a bit buffer
    for l in range(4):
        d.p[l] = 0.2
    assert _call(lib, net, fake, fake, 10, fake, fake, fake, fake, 1 << 30, drop=ctypes.byref(d)) == -1
    d.mode = 1
    d.p[0] = 1.0                      # p outside [0, 1)
    assert _call(lib, net, fake, fake, 10, fake, fake, fake, fake, 1 << 30, drop=ctypes.byref(d)) == -1
    d.p[0] = 0.2
    d.d_step_counter = 1 << 20        # general nets run launch by launch
    assert _call(lib, net, fake, fake, 10, fake, fake, fake, fake, 1 << 30, drop=ctypes.byref(d)) == -1


def test_backward_zero_rows_is_a_no_op(lib):
    fake = ctypes.c_void_p(1 << 20)
    assert _call(lib, [8, 64, 200, 48, 1], fake, None, 0, None, fake, None, None, 0) == 0
    assert _call(lib, [8, 256, 256, 256, 1], fake, fake, 0, fake, fake, fake, fake, 0) == 0
