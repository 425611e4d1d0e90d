"""CPU: the ctypes binding and argument checks of pinn_residuals_backward / pinn_net_f_t_backward (csrc/pinn_residuals.hip),
and the physics_autograd keyword's validation before anything touches a device."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    return _lib.load(build_if_missing=False)


FAKE = ctypes.c_void_p(1 << 20)
MIS = ctypes.c_void_p((1 << 20) + 4)
BIG = 1 << 30


def _res(lib, x=FAKE, u=FAKE, lam=FAKE, flags=15, n=10, g=FAKE, ld=10, gmask=1, gl=FAKE, gu=FAKE, gx=FAKE, work=FAKE, wb=BIG, aff=True):
    from pinn_amd import _lib
    a = ctypes.byref(_lib.Affine()) if aff else None
    return lib.pinn_residuals_backward(x, u, a, lam, flags, n, g, ld, gmask, gl, gu, gx, work, wb, None)


def _eul(lib, x=FAKE, u=FAKE, xh=None, uh=None, lam=FAKE, n=10, gf=FAKE, gp=None, gr=None, gl=FAKE, gu=FAKE, gx=FAKE, gxh=None,
         guh=None, work=FAKE, wb=BIG, aff=True):
    from pinn_amd import _lib
    a = ctypes.byref(_lib.Affine()) if aff else None
    return lib.pinn_net_f_t_backward(x, u, xh, uh, a, lam, n, gf, gp, gr, gl, gu, gx, gxh, guh, work, wb, None)


def test_new_entry_points_are_declared_and_bound(lib):
    from pinn_amd import _lib
    for name, nargs in (("pinn_residuals_backward", 15), ("pinn_net_f_t_backward", 18)):
        assert name in _lib.declared_symbols()
        assert len(getattr(lib, name).argtypes) == nargs
    assert lib.pinn_residuals_backward.argtypes[2] is ctypes.POINTER(_lib.Affine)
    assert lib.pinn_net_f_t_backward.argtypes[4] is ctypes.POINTER(_lib.Affine)
    assert lib.pinn_abi_version() == 2


def test_residuals_backward_rejects_bad_arguments_without_a_gpu(lib):
    assert _res(lib, aff=False) == -1
    assert _res(lib, lam=None) == -1
    assert _res(lib, gl=None) == -1                      # the parameter gradient is always written
    assert _res(lib, n=-1) == -1
    assert _res(lib, flags=16) == -1
    assert _res(lib, x=None) == -1
    assert _res(lib, x=MIS) == -1                        # rows are read as float4
    assert _res(lib, gx=MIS) == -1
    assert _res(lib, u=None) == -1                       # the voltage model reads u
    assert _res(lib, g=None) == -1                       # a column is present but no gradient buffer
    assert _res(lib, ld=9) == -1
    assert _res(lib, gmask=1 << 20) == -1                # not a column
    assert _res(lib, flags=2, gmask=1) == -1             # f_V upstream without the voltage model
    assert _res(lib, work=None) == -1
    assert _res(lib, wb=lib.pinn_residuals_workspace_bytes() - 8) == -3
    assert _res(lib, wb=16) == -3


def test_net_f_t_backward_rejects_bad_arguments_without_a_gpu(lib):
    assert _eul(lib, aff=False) == -1
    assert _eul(lib, lam=None) == -1
    assert _eul(lib, gl=None) == -1
    assert _eul(lib, n=-1) == -1
    assert _eul(lib, x=None) == -1
    assert _eul(lib, x=MIS) == -1
    assert _eul(lib, gx=MIS) == -1
    assert _eul(lib, u=None) == -1                       # rows t >= 1 read u[t - 1]
    assert _eul(lib, xh=FAKE) == -1                      # halo row without its u
    assert _eul(lib, uh=FAKE) == -1
    assert _eul(lib, xh=MIS, uh=FAKE) == -1
    assert _eul(lib, xh=FAKE, uh=FAKE, gxh=MIS) == -1
    assert _eul(lib, gxh=FAKE) == -1                     # halo gradient without a halo
    assert _eul(lib, guh=FAKE) == -1
    assert _eul(lib, work=None) == -1
    assert _eul(lib, wb=lib.pinn_residuals_workspace_bytes() - 8) == -3


def test_physics_autograd_modes_listed():
    from pinn_amd import model
    assert model.PHYSICS_AUTOGRAD_MODES == (False, "lambdas", "full")
    import inspect
    sig = inspect.signature(model.PhysicsInformedNN.__init__)
    assert sig.parameters["physics_autograd"].default is False
