"""CPU: argument checks of pinn_gnet_backward2 (the autograd double backward, csrc/pinn_general.hip), its ctypes binding and
header declaration, and the `autograd` mode values of pinn_amd.DNN."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    return _lib.load(build_if_missing=False)


def _call(lib, net, params, x, n, gu, vx, grads, gx, ggu, gglv, work, wbytes, glv=None, drop=None):
    from pinn_amd import _lib
    return lib.pinn_gnet_backward2(ctypes.byref(_lib.GNet(net)), params, x, n, drop, gu, glv, vx, grads, gx, ggu, gglv, work, wbytes,
                                   None)


def test_backward2_exported_declared_and_bound(lib):
    from pinn_amd import _lib
    header = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    for name in ("pinn_gnet_backward2_workspace_bytes", "pinn_gnet_backward2"):
        assert name in _lib.declared_symbols()
        assert getattr(lib, name) is not None
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.pinn_gnet_backward2.argtypes[0] is ctypes.POINTER(_lib.GNet)
    assert len(lib.pinn_gnet_backward2.argtypes) == 15
    assert lib.pinn_gnet_backward2_workspace_bytes.restype is ctypes.c_size_t
    assert lib.pinn_abi_version() == 2


def test_backward2_workspace_bytes(lib):
    from pinn_amd import _lib
    ws = lambda net, n: lib.pinn_gnet_backward2_workspace_bytes(ctypes.byref(_lib.GNet(net)), n)
    assert ws([8, 100, 3, 1], 10) == 0 and ws([8, 2049, 32, 1], 10) == 0 and ws([8, 32, 32, 1], -1) == 0
    small, big = ws([8, 64, 200, 48, 1], 100), ws([8, 64, 200, 48, 1], 10000)
    assert 0 < small < big
    # a primal and a tangent activation per layer: more than the first backward's workspace at the same rows, bounded for any row count
    first = lib.pinn_gnet_workspace_bytes(ctypes.byref(_lib.GNet([8, 64, 200, 48, 1])), 10000, 0)
    assert big > first
    assert ws([8, 2000, 300, 1], 10 ** 9) < (2 << 30)


def test_backward2_rejects_bad_arguments_without_a_gpu(lib):
    """Argument checks run before anything touches the device; the codes are pinn_gnet_backward's."""
    net = [8, 100, 100, 1]
    fake = ctypes.c_void_p(1 << 20)
    mis = ctypes.c_void_p((1 << 20) + 4)
    big = 1 << 30
    ok = dict(params=fake, x=fake, n=10, gu=fake, vx=fake, grads=fake, gx=fake, ggu=fake, gglv=fake, work=fake, wbytes=big)
    call = lambda **kw: _call(lib, kw.pop("net", net), **dict(ok, **kw))
    # NULL params, x, g_u, v
    for k in ("params", "x", "gu", "vx"):
        assert call(**{k: None}) == -1, k
    # misaligned params, x, v, grads, dx, workspace
    for k in ("params", "x", "vx", "grads", "gx", "work"):
        assert call(**{k: mis}) == -1, k
    # negative rows, NULL workspace
    assert call(n=-1) == -1
    assert call(work=None) == -1
    # too-small workspace (also with every optional output absent), unsupported net
    assert call(wbytes=16) == -3
    assert call(wbytes=16, grads=None, gx=None, ggu=None, gglv=None) == -3
    from pinn_amd import _lib
    need = lib.pinn_gnet_backward2_workspace_bytes(ctypes.byref(_lib.GNet(net)), 10)
    assert call(wbytes=need - 1) == -3
    assert call(net=[8, 100, 3, 1]) == -2
    assert call(net=[8, 2049, 32, 1]) == -2


def test_backward2_rejects_bad_dropout_without_a_gpu(lib):
    from pinn_amd import _lib
    net = [8, 32, 32, 32, 1]
    fake = ctypes.c_void_p(1 << 20)
    call = lambda d: _call(lib, net, fake, fake, 10, fake, fake, fake, fake, fake, fake, fake, 1 << 30, drop=ctypes.byref(d))
    d = _lib.Dropout()
    d.mode = 2                        # BITS without a bit buffer
    for l in range(4):
        d.p[l] = 0.2
    assert call(d) == -1
    d.mode = 1
    d.p[0] = 1.0                      # p outside [0, 1)
    assert call(d) == -1
    d.p[0] = 0.2
    d.d_step_counter = 1 << 20        # general nets run launch by launch
    assert call(d) == -1
    d.d_step_counter = None
    d.mode = 3
    assert call(d) == -1


def test_backward2_zero_rows_is_a_no_op(lib):
    """No rows and no d_grads to zero: nothing is launched, whatever the other pointers are."""
    fake = ctypes.c_void_p(1 << 20)
    assert _call(lib, [8, 64, 200, 48, 1], fake, None, 0, None, None, None, None, None, None, None, 0) == 0
    assert _call(lib, [8, 256, 256, 256, 1], fake, fake, 0, fake, fake, None, fake, fake, fake, fake, 0) == 0


def test_autograd_mode_values():
    """The setter's rules, on the property itself (a DNN needs a GPU to be built; its `autograd` property does not)."""
    from pinn_amd.model import DNN

    class Stub:
        precision = "fp32"
        _autograd = False
    prop = DNN.autograd
    s = Stub()
    for v in (False, True, "double"):
        prop.fset(s, v)
        assert prop.fget(s) == v and type(prop.fget(s)) is type(v)
    prop.fset(s, 1)
    assert prop.fget(s) is True
    for bad in ("twice", "Double", "", "true"):
        with pytest.raises(ValueError):
            prop.fset(s, bad)
    assert prop.fget(s) is True
    s.precision = "bf16"
    for on in (True, "double"):
        with pytest.raises(ValueError):
            prop.fset(s, on)
    prop.fset(s, False)
    assert prop.fget(s) is False
