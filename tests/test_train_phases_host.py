"""CPU: the host-side contracts the phase-split training calls and the optimizer routes rest on -- pinn_grad_split (where
the flat gradient splits into the HEAD and TAIL the data-parallel step reduces separately) and pinn_adam_coeffs (the
device coefficient table of pinn_adam_step_dev / pinn_mlp_train_step_dev).  No GPU: neither entry point launches anything."""
import ctypes
import math

import numpy as np
import pytest

import pinn_oracle as O


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    return _lib.load(build_if_missing=False)


DUMMY = 0x10000       # pinn_grad_split validates the struct only and never reads d_packed


@pytest.mark.parametrize("H", [128, 256, 512, 1024])
@pytest.mark.parametrize("nh", [1, 2, 3, 8])
def test_grad_split_layout(lib, H, nh):
    from pinn_amd import _lib, layout
    offs = {name: off for name, _, off in layout.param_offsets(8, H, nh)[0]}
    total = layout.param_offsets(8, H, nh)[1]
    wide = H > 256
    for prec in (0, 1, 2, 3):
        if wide and prec == 0:      # the layer-by-layer kernels have no exact-fp32 variant
            assert lib.pinn_grad_split(ctypes.byref(_lib.Net(8, H, nh, prec, None))) == -1
            continue
        if prec:                    # every precision but fp32 needs its packed scratch
            assert lib.pinn_grad_split(ctypes.byref(_lib.Net(8, H, nh, prec, None))) == -1
        split = lib.pinn_grad_split(ctypes.byref(_lib.Net(8, H, nh, prec, DUMMY if prec else None)))
        assert split % 4 == 0      # grad_finalize_kernel reduces groups of four floats
        if prec == 1 and not wide:
            assert split == 0       # the fused bf16 family launches its weight gradients as one block
            continue
        first_tail = "layers.layer_%d.weight" % (nh - 1) if nh >= 2 else "predict.weight"
        assert split == offs[first_tail], (prec, split, offs[first_tail])
        assert 0 < split < total
        # both scalar head biases, whose gradients the tail's reduction builds from the loss partials, lie in the tail
        assert offs["predict.bias"] >= split and offs["var_layers.5.bias"] >= split


def test_grad_split_invalid_nets(lib):
    from pinn_amd import _lib
    assert lib.pinn_grad_split(None) == -1
    for n_in, H, nh, prec in ((7, 256, 3, 0), (8, 64, 3, 0), (8, 384, 3, 2), (8, 256, 0, 0), (8, 256, 9, 0), (8, 256, 3, 4),
                              (8, 256, 3, -1), (8, 2048, 3, 0)):
        assert lib.pinn_grad_split(ctypes.byref(_lib.Net(n_in, H, nh, prec, DUMMY))) == -1, (n_in, H, nh, prec)


def test_adam_coeffs_against_float64(lib):
    """pinn_adam_coeffs(lr, t) == np.float32 of the float64 formula (step_size = lr / (1 - 0.9^t), bc2_sqrt =
    sqrt(1 - 0.999^t), lr as the float32 the C ABI takes) for t = 1 .. 60 000 at the reference's StepLR rates (train_dnn:
    lr 0.01, x0.8 every 1000 steps)."""
    ss, bs = ctypes.c_float(), ctypes.c_float()
    bad = []
    for t in range(1, 60001):
        lr = float(np.float32(O.steplr(0.01, 0.8, 1000, t - 1)))
        lib.pinn_adam_coeffs(lr, t, ctypes.byref(ss), ctypes.byref(bs))
        want_ss = np.float32(lr / (1.0 - math.pow(0.9, t)))
        want_bs = np.float32(math.sqrt(1.0 - math.pow(0.999, t)))
        if ss.value != float(want_ss) or bs.value != float(want_bs):
            bad.append((t, ss.value, float(want_ss), bs.value, float(want_bs)))
    assert not bad, bad[:5]
