"""CPU: the C-ABI library builds for gfx950, loads without a GPU and exports every symbol that
include/pinn_hip.h declares; host-only entry points behave (no compute calls here)."""
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


def _header_functions():
    src = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pinn_[a-z_0-9]+)\s*\(", src)))


def test_header_symbols_exported_and_bound(lib):
    from pinn_amd import _lib
    names = _header_functions()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), "library does not export %s" % n
    assert sorted(_lib.declared_symbols()) == names, "ctypes signatures out of sync with include/pinn_hip.h"


def test_host_only_entry_points(lib):
    from pinn_amd import _lib, layout
    assert lib.pinn_abi_version() == 2
    assert lib.pinn_residuals_workspace_bytes() == 1024 * 32 * 8
    for H, nh in ((256, 3), (128, 3), (256, 1), (128, 8)):
        net = _lib.Net(8, H, nh)
        offs, total = layout.param_offsets(8, H, nh)
        assert lib.pinn_param_count(ctypes.byref(net)) == total
        assert lib.pinn_train_workspace_bytes(ctypes.byref(net), 1000) > 0
    assert layout.param_offsets(8, 256, 3)[1] == 175362 + 6          # 175 362 parameters + two 3-float alignment pads
    assert lib.pinn_packed_bytes(ctypes.byref(_lib.Net(8, 256, 3, _lib.PREC_BF16))) == 688128
    assert lib.pinn_packed_bytes(ctypes.byref(_lib.Net(8, 256, 3))) == 0
    assert lib.pinn_train_workspace_bytes(ctypes.byref(_lib.Net(8, 256, 3, _lib.PREC_BF16, None)), 1000) == 0      # bf16 needs its scratch buffer
    # wide nets (layer-by-layer kernels): sized by shape alone; every precision but exact fp32 (which needs no scratch anywhere)
    assert lib.pinn_param_count(ctypes.byref(_lib.Net(8, 1024, 4))) == layout.param_offsets(8, 1024, 4)[1]
    wide_bytes = lib.pinn_packed_bytes(ctypes.byref(_lib.Net(8, 1024, 4, _lib.PREC_F32X6)))
    assert wide_bytes > 5 * 2 * 4 * 1024 * 1024                 # five 16-bit copies of the matrices + the activation scratch
    assert lib.pinn_packed_bytes(ctypes.byref(_lib.Net(8, 1024, 4, _lib.PREC_BF16))) == wide_bytes
    assert lib.pinn_packed_bytes(ctypes.byref(_lib.Net(8, 1024, 4, _lib.PREC_FP32))) == 0
    assert lib.pinn_param_count(ctypes.byref(_lib.Net(8, 384, 2))) < 0
    for bad in (_lib.Net(8, 96, 3), _lib.Net(7, 256, 3), _lib.Net(8, 256, 0), _lib.Net(8, 384, 3), _lib.Net(8, 256, 9)):
        assert lib.pinn_param_count(ctypes.byref(bad)) == -2
        assert lib.pinn_train_workspace_bytes(ctypes.byref(bad), 1000) == 0
    # struct layouts agree with the C side (sizes from the header's field lists)
    assert ctypes.sizeof(_lib.Affine) == 8 * 8 * 2 + 8 * 2 + 4 * 2
    assert ctypes.sizeof(_lib.Net) == 24          # 4 ints + 4 pad + device pointer
    assert ctypes.sizeof(_lib.Dropout) == 4 + 36 + 8 + 4 + 4 + 8 + 8 + 8   # incl. padding before row_offset


def test_null_workspace_and_buffer_pointers_are_argument_errors(lib):
    """Every entry point that takes a workspace / stash / output pointer returns PINN_E_ARG (-1) for NULL before it touches
    the GPU (the checks run on the host, so this needs no device), and PINN_E_WORKSPACE (-3) for a workspace that is too
    small: a kernel is never handed a pointer the entry point has not seen to be non-NULL and large enough.  (Round 2's
    scratch ablation builds faulted on address nil with a stash pointer their own edit had nulled, gpurun_out/ab2.txt.)"""
    from pinn_amd import _lib
    aff = _lib.Affine()
    one = ctypes.c_void_p(0x1000)          # a non-NULL address that is never dereferenced: every call below fails on the host
    E_ARG, E_WS = -1, -3
    # residual pass: sums requested without a workspace; workspace too small
    assert lib.pinn_residuals(one, one, one, ctypes.byref(aff), one, _lib.RES_ALL, 10, None, 0, one, None, 0, None) == E_ARG
    assert lib.pinn_residuals(one, one, one, ctypes.byref(aff), one, _lib.RES_ALL, 10, None, 0, one, one, 16, None) == E_WS
    assert lib.pinn_residuals(None, one, one, ctypes.byref(aff), one, _lib.RES_ALL, 10, None, 0, None, None, 0, None) == E_ARG
    assert lib.pinn_residuals_cached(one, ctypes.byref(aff), one, _lib.RES_T, 10, one, None, 0, None) == E_ARG
    assert lib.pinn_residuals_cached(one, ctypes.byref(aff), one, _lib.RES_T, 10, one, one, 16, None) == E_WS
    assert lib.pinn_residuals_cached(None, ctypes.byref(aff), one, _lib.RES_T, 10, one, one, 1 << 20, None) == E_ARG
    assert lib.pinn_residuals_prepare(one, None, None, ctypes.byref(aff), one, _lib.RES_T, 10, None, None) == E_ARG
    assert lib.pinn_lambda_stage_run(_lib.STAGE_THERMAL, _lib.RES_T, one, None, None, ctypes.byref(aff), 10, 1.0, 0.8, 1000, 0, 5, one, one, one,
                                     None, 1000, None, None, 0, None) == E_ARG
    assert lib.pinn_lambda_stage_run(_lib.STAGE_THERMAL, _lib.RES_T, one, None, None, ctypes.byref(aff), 10, 1.0, 0.8, 1000, 0, 5, one, one, one,
                                     None, 1000, None, one, 8, None) == E_WS
    assert lib.pinn_lambda_step(_lib.STAGE_THERMAL, None, 10, 1.0, 0.1, 1, one, one, one, None) == E_ARG
    assert lib.pinn_net_f_t(one, one, None, None, ctypes.byref(aff), one, 10, None, one, one, None) == E_ARG
    # network entry points: NULL parameter / row / output / workspace / packed-weight pointers
    net = _lib.Net(8, 256, 3)
    assert lib.pinn_mlp_forward(ctypes.byref(net), one, one, 10, None, None, one, None) == E_ARG
    assert lib.pinn_mlp_forward(ctypes.byref(net), one, None, 10, None, one, one, None) == E_ARG
    d = _lib.Dropout(); d.mode = _lib.DROP_PHILOX
    assert lib.pinn_mc_dropout(ctypes.byref(net), one, one, 10, ctypes.byref(d), 4, one, None, one, None) == E_ARG
    assert lib.pinn_mlp_train_grads(ctypes.byref(net), one, one, one, 10, 10, None, one, one, None, 1 << 30, None) == E_ARG
    assert lib.pinn_mlp_train_grads(ctypes.byref(net), one, one, one, 10, 10, None, ctypes.c_void_p(0x1000), one, ctypes.c_void_p(0x2000), 16, None) == E_WS
    assert lib.pinn_mlp_train_grads(ctypes.byref(net), one, one, one, 10, 10, None, ctypes.c_void_p(0x1004), one, ctypes.c_void_p(0x2000), 1 << 30, None) == E_ARG   # alignment
    for prec in (_lib.PREC_BF16, _lib.PREC_F32X6, _lib.PREC_F32X6_G6):
        split = _lib.Net(8, 256, 3, prec, None)           # a split-operand precision without its packed-weight scratch
        assert lib.pinn_mlp_forward(ctypes.byref(split), one, one, 10, None, one, one, None) == E_ARG
        assert lib.pinn_mlp_train_grads(ctypes.byref(split), one, one, one, 10, 10, None, one, one, one, 1 << 30, None) == E_ARG
    d.mode = _lib.DROP_BITS            # injected masks without the mask buffer
    assert lib.pinn_mlp_forward(ctypes.byref(net), one, one, 10, ctypes.byref(d), one, one, None) == E_ARG
    assert lib.pinn_adam_step(one, one, None, one, 10, 0.01, 1, None) == E_ARG
    # gradients + Adam as one launch sequence: NULL moments / coefficient table / step counter, a step count below 1, and the
    # device-counter form on a precision whose kernels do not leave the counter's snapshot
    al = ctypes.c_void_p(0x1000)
    assert lib.pinn_mlp_train_step(ctypes.byref(net), al, one, one, 10, 10, None, al, one, ctypes.c_void_p(0x2000), 1 << 30, None, al, 0.01, 1, None) == E_ARG
    assert lib.pinn_mlp_train_step(ctypes.byref(net), al, one, one, 10, 10, None, al, one, ctypes.c_void_p(0x2000), 1 << 30, al, al, 0.01, 0, None) == E_ARG
    assert lib.pinn_mlp_train_step(ctypes.byref(net), al, one, one, 10, 10, None, al, one, None, 1 << 30, al, al, 0.01, 1, None) == E_ARG
    dc = _lib.Dropout(); dc.mode = _lib.DROP_PHILOX
    assert lib.pinn_mlp_train_step_dev(ctypes.byref(net), al, one, one, 10, 10, ctypes.byref(dc), al, one, ctypes.c_void_p(0x2000), 1 << 30, al, al, al, None) == E_ARG  # no counter
    dc.d_step_counter = 0x3000
    assert lib.pinn_mlp_train_step_dev(ctypes.byref(net), al, one, one, 10, 10, ctypes.byref(dc), al, one, ctypes.c_void_p(0x2000), 1 << 30, al, al, None, None) == E_ARG
    assert lib.pinn_mlp_train_step_dev(ctypes.byref(net), al, one, one, 10, 10, ctypes.byref(dc), al, one, ctypes.c_void_p(0x2000), 1 << 30, al, al, al, None) == -2     # PINN_E_ARCH: exact fp32
    assert lib.pinn_results_assemble(one, one, ctypes.byref(aff), 0.0, 1.0, 200, None, 0, one, one, one, one, 10, None, 10, None, None) == E_ARG


def test_stage_run_refuses_a_stage_that_contradicts_its_flag(lib):
    """pinn_lambda_stage_run, all 5 x 4 pairs, on the host: with n_iters = 0 a valid call returns PINN_OK before any launch, so the
    addresses are never dereferenced.  The voltage stages go with PINN_RES_V, every other stage with its own flag."""
    from pinn_amd import _lib
    aff = _lib.Affine()
    one = ctypes.c_void_p(0x1000)
    own = {_lib.STAGE_LAMBDA_PM: _lib.RES_V, _lib.STAGE_LAMBDA_F: _lib.RES_V, _lib.STAGE_THERMAL: _lib.RES_T, _lib.STAGE_HYDROGEN: _lib.RES_H,
           _lib.STAGE_OXYGEN: _lib.RES_O}
    for stage, flag in own.items():
        for flags in (_lib.RES_V, _lib.RES_T, _lib.RES_H, _lib.RES_O):
            rc = lib.pinn_lambda_stage_run(stage, flags, one, one, one, ctypes.byref(aff), 10, 1.0, 0.8, 1000, 0, 0, one, one, one, None, 1000, None,
                                           one, 1 << 20, None)
            assert rc == (0 if flags == flag else -1), (stage, flags, rc)


def test_dropout_struct_is_validated_alike_at_every_entry_point(lib):
    """One pinn_dropout_t, one rule: every entry point that takes the struct rejects the same bad ones with PINN_E_ARG (-1),
    on the host.  Only failing calls, with addresses that are never dereferenced."""
    from pinn_amd import _lib
    E_ARG, E_ARCH = -1, -2
    al = ctypes.c_void_p(0x1000)           # 16-byte aligned, never dereferenced
    big = 1 << 40                          # "large enough" for every workspace check
    nh = 3
    net = ctypes.byref(_lib.Net(8, 256, nh))
    gnet = ctypes.byref(_lib.GNet([8, 64, 200, 48, 1]))

    def drop(mode=_lib.DROP_PHILOX, slot=None, p=0.2, d_bits=None, counter=None):
        d = _lib.Dropout()
        d.mode = mode
        for l in range(nh + 1):
            d.p[l] = 0.2
        if slot is not None:
            d.p[slot] = p
        d.d_bits = d_bits
        d.d_step_counter = counter
        return ctypes.byref(d)

    calls = {
        "pinn_mlp_forward": lambda d: lib.pinn_mlp_forward(net, al, al, 10, d, al, al, None),
        "pinn_mc_dropout": lambda d: lib.pinn_mc_dropout(net, al, al, 10, d, 4, al, al, al, None),
        "pinn_mlp_train_grads": lambda d: lib.pinn_mlp_train_grads(net, al, al, al, 10, 10, d, al, al, al, big, None),
        "pinn_mlp_train_step": lambda d: lib.pinn_mlp_train_step(net, al, al, al, 10, 10, d, al, al, al, big, al, al, 0.01, 1, None),
        "pinn_gnet_forward": lambda d: lib.pinn_gnet_forward(gnet, al, al, 10, d, al, al, al, big, None),
        "pinn_gnet_mc_dropout": lambda d: lib.pinn_gnet_mc_dropout(gnet, al, al, 10, d, 4, al, al, al, al, big, None),
        "pinn_gnet_train_grads": lambda d: lib.pinn_gnet_train_grads(gnet, al, al, al, 10, 10, d, al, al, al, big, None),
        "pinn_gnet_train_step": lambda d: lib.pinn_gnet_train_step(gnet, al, al, al, 10, 10, d, al, al, al, big, al, al, 0.01, 1, None),
        "pinn_gnet_backward": lambda d: lib.pinn_gnet_backward(gnet, al, al, 10, d, al, al, al, al, al, big, None),
        "pinn_gnet_backward2": lambda d: lib.pinn_gnet_backward2(gnet, al, al, 10, d, al, al, al, al, al, al, al, al, big, None),
    }
    bad = {
        "mode -1": drop(mode=-1),
        "mode 3": drop(mode=3),
        "p = 1.0": drop(slot=0, p=1.0),
        "p = -0.1": drop(slot=1, p=-0.1),
        "p = NaN": drop(slot=nh, p=float("nan")),
        "bits without d_bits": drop(mode=_lib.DROP_BITS),
    }
    for name, call in calls.items():
        for what, d in bad.items():
            assert call(d) == E_ARG, (name, what)
    # the device step counter: training calls of the fused nets only
    counted = drop(counter=0x3000)
    wide = ctypes.byref(_lib.Net(8, 512, 2, _lib.PREC_F32X6, 0x4000))
    assert lib.pinn_mlp_train_grads(wide, al, al, al, 10, 10, counted, al, al, al, big, None) == E_ARCH
    assert lib.pinn_mlp_train_step(wide, al, al, al, 10, 10, counted, al, al, al, big, al, al, 0.01, 1, None) == E_ARCH
    for name, call in calls.items():
        if name.startswith("pinn_gnet_"):
            assert call(counted) == E_ARG, name


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "physics-informed-neural-network-for-explainable-fault-diagnosis-in-fuel-cells_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "pinn_oracle" not in txt and "import oracle" not in txt, f


def test_model_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import pinn_amd
    from pinn_amd import synth
    ds = synth.make_dataset(64, (), seed=0)
    with pytest.raises(Exception) as e:
        pinn_amd.PhysicsInformedNN(ds[0], ds[1], [8, 256, 256, 256, 1], ds[4], ds[5], p=0.2, logvar=True)
    assert "GPU" in str(e.value)
