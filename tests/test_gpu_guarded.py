"""Canary guards round every buffer of the network and physics ABI (include/pinn_hip.h, pinn_residuals .. pinn_results_assemble):
no entry point writes outside the memory it was given, reads behind an input into a result, or needs a byte more than the library's
size functions state.

Every case builds its call twice from one description (a builder below: the takes, then the ctypes arguments) -- once on the
guarded arena of tests/guarded.py, once on ordinary tensors -- and asserts
  1. arena.check(): every guard byte is still 0xFF and every input buffer kept its bytes;
  2. every out / inout buffer of the guarded call is byte-equal to the ordinary call's (the ABI is bitwise deterministic, so a result
     that depends on what lies behind an input or around a workspace differs here);
  3. workspaces, packed weights, caches and optimizer state are taken at exactly the size the library states, and the call succeeds.
Refused calls (work_bytes one short: PINN_E_WORKSPACE; one NULL pointer: PINN_E_ARG) must leave every out and scratch byte 0xFF.
(pinn_gnet_forward, pinn_gnet_mc_dropout and pinn_gens_forward run in a smaller plan than the size function states, which covers
training too -- tests/test_ensemble_abi.py pins that -- so their short workspace is one byte below the forward's own plan.)
The one deliberate overrun is pinn_gens_combine told n + 1 rows on outputs of n floats: check() has to name exactly those three
buffers (test_device_teeth_one_float_too_many says why it is not pinn_adam_step).
Inputs, parameters and dropout structs come from hip_helpers, gnet_helpers, ensemble_cases and synth.  No tolerance anywhere.

Row counts (ROWS): 1; 15, 17 (the 16-row tile of the small forward kernel); 63, 65 (the 64-row tile); 127, 129 (the 128-row x6 /
wide tile); 257 (a third tile, one row long); and tile * CUs + tile + 1, a workgroup's second tile, once per family (tile 64 for the
fp32 / bf16 fused nets, 128 for x6 and wide)."""
import ctypes
import functools
import os
import re
import time

import numpy as np
import pytest
import torch

import guarded as G

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_ARG, E_ARCH, E_WORKSPACE, E_RANGE = 0, -1, -2, -3, -4
FP32, BF16, X6, G6 = 0, 1, 2, 3
PRECS = [FP32, BF16, X6, G6]
PREC_NAME = {FP32: "fp32", BF16: "bf16", X6: "x6", G6: "g6"}
ROWS = [1, 15, 17, 63, 65, 127, 129, 257]
LOSS_TAIL = [1.5, -2.5, 3.25, 4.0]            # the data-parallel loss tail that model.py keeps directly behind the flat gradient

# entry point -> the buffers its cases take from the arena (in / out / inout / scratch as in the builders below)
ENTRY_POINTS = {
    "pinn_residuals": "x u y lambda | cols [20 ld] sums [32] | work",
    "pinn_lambda_step": "sums | lambda [17] adam [34] loss [2]",
    "pinn_lambda_stage_run": "x u y | lambda [17] adam [34] loss [2] log [n_logged 64] sums [32] | work (6 n floats)",
    "pinn_residuals_prepare": "x u y lambda | cache [6 n]",
    "pinn_residuals_cached": "cache [6 n] lambda | sums | work",
    "pinn_net_f_t": "x u x_halo [8] u_halo [1] lambda | f t_pred t_real [n]",
    "pinn_residuals_backward": "x u lambda g [20 ld] | glambda [17] gu [n] gx [n 8] | work",
    "pinn_net_f_t_backward": "x u halos lambda gf gt_pred gt_real | glambda gu gx gx_halo [8] gu_halo [1] | work",
    "pinn_net_range_status": "packed",
    "pinn_mlp_forward": "params x bits [passes n words] | u lv [n] | packed",
    "pinn_mc_dropout": "params x bits | pred_mean a_u e_u [n] | packed",
    "pinn_mlp_train_grads": "params x y | grads [P] + loss tail [4], loss [4] | work packed",
    "pinn_mlp_train_grads_phases": "as pinn_mlp_train_grads, one arena over the calls of a sequence",
    "pinn_adam_step": "grads | params m v [n]",
    "pinn_adam_step_dev": "grads coeffs [2 steps] counter [1] | params m v [n]",
    "pinn_mlp_train_step_dev": "x y coeffs [2 steps] | params grads + tail loss m v counter [1] | work packed",
    "pinn_mlp_train_step": "x y | params grads + tail loss m v | work packed",
    "pinn_gnet_forward": "params x | u lv [n] | work",
    "pinn_gnet_mc_dropout": "params x | pred_mean a_u e_u [n] | work",
    "pinn_gnet_train_grads": "params x y | grads [P] + loss tail, loss [4] | work",
    "pinn_gnet_train_step": "x y | params grads + tail loss m v | work",
    "pinn_gnet_backward": "params x gu glv | grads [P] + tail, gx [n 8] | work",
    "pinn_gnet_backward2": "params x gu glv vx | grads [P] + tail, gx [n 8] ggu gglv [n] | work",
    "pinn_gens_forward": "params [E P] x | u lv [E n] | work",
    "pinn_gens_train_grads": "params [E P] x y | grads [E P] loss [E 4] | work",
    "pinn_gens_train_step": "x y | params grads m v [E P] loss [E 4] | work",
    "pinn_gens_combine": "u lv [E n] | pred_mean a_u e_u: rows of one [3 n] buffer, or three buffers",
    "pinn_results_assemble": "x y seg_end pred_mean a_u e_u cols [20 ld] labels | out [n 22] float64",
}
# declared in the same range of the header, but host-only: sizes, counts, plans (their values are what rule 3 uses)
HOST_QUERIES = ["pinn_lambda_stage_workspace_bytes", "pinn_packed_bytes", "pinn_param_count", "pinn_train_workspace_bytes", "pinn_grad_split",
                "pinn_adam_coeffs", "pinn_gnet_param_count", "pinn_gnet_workspace_bytes", "pinn_gnet_backward2_workspace_bytes",
                "pinn_gens_workspace_bytes", "pinn_gens_train_plan"]


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


def P(b):
    return ctypes.c_void_p(b.ptr) if b is not None else None


def _stream():
    import hip_helpers as hh
    return hh.stream()


def _dev():
    return torch.device("cuda:0")


class Call:
    """One ABI call: the function's name and its ctypes arguments; wb / null: the positions of work_bytes and of a required pointer
    (what the refused-call cases change); keep: host structs the arguments point into."""

    def __init__(self, fn, args, wb=None, null=None, keep=(), expect=OK, floor=None):
        self.fn, self.args, self.wb, self.null, self.keep, self.expect = fn, list(args), wb, null, keep, expect
        self.floor = floor          # what the call itself needs where that is less than the stated size (the any-width forwards)

    def run(self, lib):
        return getattr(lib, self.fn)(*self.args)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs (host tensors, shared by the guarded and the ordinary call)
@functools.lru_cache(maxsize=16)
def _dataset(n):
    from pinn_amd import synth
    import hip_helpers as hh
    ds = synth.make_dataset(max(n, 2), (), seed=n % 97 + 1)
    x, y = ds[0][:n].contiguous(), ds[1].reshape(-1)[:n].contiguous()
    gen = torch.Generator().manual_seed(n)
    u = (y + 0.05 * torch.randn(n, generator=gen)).contiguous()
    return x, y, u, hh.affine_struct(ds[4], ds[5])


def _lambda():
    import pinn_oracle as O
    return np.array([O.LAMBDA_INIT[k] for k in O.LAMBDA_NAMES], dtype=np.float32)


def _rand(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).contiguous()


@functools.lru_cache(maxsize=4)
def _fused_params(H, nh):
    import hip_helpers as hh
    import pinn_oracle as O
    return hh.flat_params(O.init_params([8] + [H] * nh + [1], seed=H + nh), H, nh)


def _grads_with_tail(A, n_params):
    """d_grads as exactly n_params floats with the 4-float loss tail directly behind it, in one buffer."""
    init = np.concatenate([np.full(n_params, 0xFFFFFFFF, np.uint32), np.asarray(LOSS_TAIL, np.float32).view(np.uint32)])
    return A.take("grads+tail", 4 * (n_params + 4), "inout", init)


def _tail_kept(A):
    return A["grads+tail"].bytes()[-16:] == np.asarray(LOSS_TAIL, np.float32).tobytes()


# ---------------------------------------------------------------------------------------------------------------------------
# the fused and the wide nets (pinn_mlp_*): shape = (H, n_hidden, precision)
def _net(A, lib, shape):
    from pinn_amd import _lib
    H, nh, prec = shape
    net = _lib.Net(8, H, nh, prec, None)
    nb = lib.pinn_packed_bytes(ctypes.byref(net))
    if prec != FP32:
        assert nb > 0
        net.d_packed = A.take("packed", nb, "scratch").ptr            # exactly pinn_packed_bytes
    else:
        assert nb == 0
    return net


def _arch(shape, fn):
    """What the header promises: the wide nets have no exact-fp32 kernels, the device-stepped step only the fused split-operand nets."""
    H, nh, prec = shape
    if fn == "pinn_mlp_train_step_dev" and not (prec >= X6 and H <= 256):
        return E_ARCH
    return E_ARCH if (H > 256 and prec == FP32) else OK


def _drop(A, shape, n, mode, passes=1, counter=None):
    import hip_helpers as hh
    H, nh, _ = shape
    if mode == "eval":
        return None
    d = hh.dropout_struct({"philox": 1, "bits": 2}[mode], [0.2] * (nh + 1), seed=2024, stream_id=5)
    if mode == "bits":
        words = nh * H // 32 + H // 64
        bits = torch.randint(-2 ** 31, 2 ** 31, (passes, n, words), generator=torch.Generator().manual_seed(7), dtype=torch.int64).to(torch.int32)
        d.d_bits = A.take("bits", 4 * passes * n * words, "in", bits).ptr      # exactly [passes][n][words]
    if counter is not None:
        d.d_step_counter = counter.ptr
    return d


def b_forward(A, lib, shape, n, mode="eval"):
    net = _net(A, lib, shape)
    H, nh, _ = shape
    fp, x = A.take("params", 4 * _fused_params(H, nh).numel(), "in", _fused_params(H, nh)), A.take("x", 32 * n, "in", _dataset(n)[0])
    d = _drop(A, shape, n, mode)
    u, lv = A.take("u", 4 * n, "out"), A.take("lv", 4 * n, "out")
    return [Call("pinn_mlp_forward", [ctypes.byref(net), P(fp), P(x), n, ctypes.byref(d) if d else None, P(u), P(lv), _stream()], null=5,
                 keep=(net, d), expect=_arch(shape, "pinn_mlp_forward"))]


def b_mc(A, lib, shape, n, T=3, mode="philox"):
    net = _net(A, lib, shape)
    H, nh, _ = shape
    fp, x = A.take("params", 4 * _fused_params(H, nh).numel(), "in", _fused_params(H, nh)), A.take("x", 32 * n, "in", _dataset(n)[0])
    d = _drop(A, shape, n, mode, passes=T)
    o = [A.take(k, 4 * n, "out") for k in ("pred_mean", "a_u", "e_u")]
    return [Call("pinn_mc_dropout", [ctypes.byref(net), P(fp), P(x), n, ctypes.byref(d), T, P(o[0]), P(o[1]), P(o[2]), _stream()], null=7,
                 keep=(net, d), expect=_arch(shape, "pinn_mc_dropout"))]


def b_range_status(A, lib, shape, n, after_forward=True):
    """pinn_net_range_status reads the record that the forward's pack kernel left at the end of d_packed."""
    calls = b_forward(A, lib, shape, n) if after_forward else []
    net = calls[0].keep[0] if calls else _net(A, lib, shape)
    return calls + [Call("pinn_net_range_status", [ctypes.byref(net), _stream()], null=0, keep=(net,),
                         expect=OK if shape[2] in (FP32, BF16) else _arch(shape, "pinn_net_range_status"))]


PHASES = {"all": [7], "split": [1, 32 | 128, 64 | 256]}          # PHASE_ALL; CHAIN, WGRAD_TAIL | REDUCE_TAIL, WGRAD_HEAD | REDUCE_HEAD


def b_train(A, lib, shape, n, variant="grads"):
    """variant: grads, all, split (pinn_mlp_train_grads_phases), step, step_dev."""
    net = _net(A, lib, shape)
    H, nh, _ = shape
    fp0 = _fused_params(H, nh)
    np_ = fp0.numel()
    stepping = variant in ("step", "step_dev")
    fp = A.take("params", 4 * np_, "inout" if stepping else "in", fp0)
    x, y = A.take("x", 32 * n, "in", _dataset(n)[0]), A.take("y", 4 * n, "in", _dataset(n)[1])
    counter = A.take("counter", 4, "inout", np.array([1], np.uint32)) if variant == "step_dev" else None      # the one-word counter
    d = _drop(A, shape, n, "philox", counter=counter)
    g, loss = _grads_with_tail(A, np_), A.take("loss", 32, "out")
    wb = lib.pinn_train_workspace_bytes(ctypes.byref(net), n)
    work = A.take("work", wb, "scratch")                          # exactly pinn_train_workspace_bytes
    head = [ctypes.byref(net), P(fp), P(x), P(y), n, n, ctypes.byref(d), P(g), P(loss), P(work), wb]
    kw = dict(wb=10, null=7, keep=(net, d))
    if variant == "grads":
        return [Call("pinn_mlp_train_grads", head + [_stream()], expect=_arch(shape, "pinn_mlp_train_grads"), **kw)]
    if variant in PHASES:
        return [Call("pinn_mlp_train_grads_phases", head + [_stream(), ph], expect=_arch(shape, "pinn_mlp_train_grads_phases"), **kw)
                for ph in PHASES[variant]]
    m, v = A.take("m", 4 * np_, "inout", _rand((np_,), 1, 1e-3)), A.take("v", 4 * np_, "inout", _rand((np_,), 2, 1e-3).abs())
    if variant == "step":
        return [Call("pinn_mlp_train_step", head + [P(m), P(v), 1e-3, 3, _stream()], expect=_arch(shape, "pinn_mlp_train_step"), **kw)]
    from pinn_amd import _lib
    n_steps, co = 2, []                                           # d_coeffs: exactly 2 n_steps floats; the counter reaches n_steps
    for k in range(n_steps):
        a, b = ctypes.c_float(), ctypes.c_float()
        lib.pinn_adam_coeffs(1e-3, k + 1, ctypes.byref(a), ctypes.byref(b))
        co += [a.value, b.value]
    coeffs = A.take("coeffs", 8 * n_steps, "in", np.asarray(co, np.float32))
    return [Call("pinn_mlp_train_step_dev", head + [P(m), P(v), P(coeffs), _stream()], expect=_arch(shape, "pinn_mlp_train_step_dev"), **kw)]


def b_adam(A, lib, n, dev=False):
    p, g = A.take("params", 4 * n, "inout", _rand((n,), 3)), A.take("grads", 4 * n, "in", _rand((n,), 4))
    m, v = A.take("m", 4 * n, "inout", _rand((n,), 5, 1e-2)), A.take("v", 4 * n, "inout", _rand((n,), 6, 1e-2).abs())
    if not dev:
        return [Call("pinn_adam_step", [P(p), P(g), P(m), P(v), n, 1e-3, 2, _stream()], null=2)]
    co, cnt = A.take("coeffs", 16, "in", np.asarray([1e-2, 0.03, 5.3e-3, 0.0447], np.float32)), A.take("counter", 4, "in", np.array([2], np.uint32))
    return [Call("pinn_adam_step_dev", [P(p), P(g), P(m), P(v), n, P(co), P(cnt), _stream()], null=2)]


# ---------------------------------------------------------------------------------------------------------------------------
# the any-width nets (pinn_gnet_*) and the ensembles (pinn_gens_*)
def _gnet(layers):
    import ensemble_cases as ec
    return ec.gnet(layers)


@functools.lru_cache(maxsize=8)
def _gparams(layers, e):
    import ensemble_cases as ec
    return ec.member_params(list(layers), e, seed=3)


def _gdrop(layers, mode):
    import gnet_helpers as gh
    return gh.drop(1, layers, seed=11, stream=2) if mode == "philox" else None


def b_gnet(A, lib, layers, n, call="forward", T=3, glv=True, gx=True, omit=None, e=None):
    """call: forward, mc, grads, step, backward, backward2 (omit: one of its outputs NULL); e: the pinn_gens_* form with e members."""
    import ensemble_cases as ec
    ens = e is not None
    E = e or 1
    fp0 = _gparams(tuple(layers), E)
    npar = fp0.shape[1]
    assert npar == lib.pinn_gnet_param_count(_gnet(layers))
    stepping = call == "step"
    fp = A.take("params", 4 * E * npar, "inout" if stepping else "in", fp0)          # exactly [E, P]
    x = A.take("x", 32 * n, "in", _dataset(n)[0])
    net, st = _gnet(layers), _stream()
    head = ([net, E] if ens else [net]) + [P(fp), P(x)]
    off = 1 if ens else 0
    pre = "pinn_gens_" if ens else "pinn_gnet_"
    if call == "backward2":
        wb = lib.pinn_gnet_backward2_workspace_bytes(net, n)
    elif ens:
        wb = lib.pinn_gens_workspace_bytes(net, E, n)
    else:
        wb = lib.pinn_gnet_workspace_bytes(net, n, T if call == "mc" else 0)
    assert wb > 0
    if call in ("forward", "mc"):
        d = _gdrop(layers, "philox" if call == "mc" else "eval")
        outs = [A.take(k, 4 * E * n, "out") for k in (("pred_mean", "a_u", "e_u") if call == "mc" else ("u", "lv"))]      # exactly [E, n]
        work = A.take("work", wb, "scratch")
        args = head + [n, ctypes.byref(d) if d else None] + ([T] if call == "mc" else []) + [P(o) for o in outs] + [P(work), wb, st]
        # the one size function covers training too; the forward runs in its own, smaller plan (gnet_referee restates it to the byte)
        import gnet_referee as gr
        floor = E * (gr.infer_layout(layers, n * (T + 1)) + G.round_up(16 * n) if call == "mc" else gr.infer_layout(layers, n))
        assert floor <= wb
        return [Call(pre + ("mc_dropout" if call == "mc" else "forward"), args, wb=len(args) - 2, null=off + (6 if call == "mc" else 5), keep=(d,),
                     floor=floor)]
    if call in ("grads", "step"):
        y = A.take("y", 4 * n, "in", _dataset(n)[1])
        d = _gdrop(layers, "philox")
        g = A.take("grads", 4 * E * npar, "out") if ens else _grads_with_tail(A, npar)
        loss = A.take("loss", 32 * E, "out")
        work = A.take("work", wb, "scratch")
        args = head + [P(y), n, n, ctypes.byref(d), P(g), P(loss), P(work), wb]
        if stepping:
            m = A.take("m", 4 * E * npar, "inout", _rand((E * npar,), 1, 1e-3))
            v = A.take("v", 4 * E * npar, "inout", _rand((E * npar,), 2, 1e-3).abs())
            args += [P(m), P(v), 1e-3, 2]
        return [Call(pre + ("train_step" if stepping else "train_grads"), args + [st], wb=off + 10, null=off + 7, keep=(d,))]
    gu, glv_t, vx = _rand((n,), 21), _rand((n,), 22), _rand((n, 8), 23)
    d = _gdrop(layers, "philox")
    bgu = A.take("gu", 4 * n, "in", gu)
    bglv = A.take("glv", 4 * n, "in", glv_t) if glv else None
    if call == "backward":
        g = _grads_with_tail(A, npar)
        bgx = A.take("gx", 32 * n, "out") if gx else None
        work = A.take("work", wb, "scratch")
        return [Call("pinn_gnet_backward", head + [n, ctypes.byref(d), P(bgu), P(bglv), P(g), P(bgx), P(work), wb, st], wb=10, null=7, keep=(d,))]
    assert call == "backward2"
    bvx = A.take("vx", 32 * n, "in", vx)
    g = _grads_with_tail(A, npar) if omit != "grads" else None
    bgx = A.take("gx", 32 * n, "out") if omit != "gx" else None
    ggu = A.take("ggu", 4 * n, "out") if omit != "ggu" else None
    gglv = A.take("gglv", 4 * n, "out") if omit != "gglv" else None
    work = A.take("work", wb, "scratch")
    return [Call("pinn_gnet_backward2", head + [n, ctypes.byref(d), P(bgu), P(bglv), P(bvx), P(g), P(bgx), P(ggu), P(gglv), P(work), wb, st],
                 wb=13, null=7, keep=(d,))]


def b_combine(A, lib, n, e=3, rows_of_one=True, rule=0, told=None):
    """told: the row count the library is told (the device-teeth case: n + 1 on outputs of n floats; the inputs are [e, told])."""
    told = n if told is None else told
    if told == n:
        u, lv = A.take("u", 4 * e * n, "in", _rand((e, n), 31)), A.take("lv", 4 * e * n, "in", _rand((e, n), 32))
    else:
        u, lv = A.take("u", 4 * e * told, "in", torch.ones(e, told)), A.take("lv", 4 * e * told, "in", torch.zeros(e, told))
    if rows_of_one:
        o = A.take("out3", 12 * n, "out")
        ptrs = [ctypes.c_void_p(o.ptr + 4 * n * k) for k in range(3)]            # rows of one [3, n] buffer
    else:
        ptrs = [P(A.take(k, 4 * n, "out")) for k in ("pred_mean", "a_u", "e_u")]
    return [Call("pinn_gens_combine", [P(u), P(lv), e, told, rule] + ptrs + [_stream()], null=6)]


# ---------------------------------------------------------------------------------------------------------------------------
# physics
def _phys(A, n, names="xuyl"):
    x, y, u, aff = _dataset(n)
    src = {"x": ("x", 32 * n, x), "u": ("u", 4 * n, u), "y": ("y", 4 * n, y), "l": ("lambda", 68, _lambda())}
    return [A.take(src[k][0], src[k][1], "in", src[k][2]) for k in names], aff


def b_residuals(A, lib, n, flags=15, pad=0, cols=True, sums=True):
    (x, u, y, lam), aff = _phys(A, n)
    ld = n + pad
    c = A.take("cols", 4 * 20 * ld, "out") if cols else None                    # exactly PINN_NCOLS * ld floats
    s = A.take("sums", 8 * 32, "out") if sums else None
    wb = lib.pinn_residuals_workspace_bytes()
    work = A.take("work", wb, "scratch")
    return [Call("pinn_residuals", [P(x), P(u), P(y), ctypes.byref(aff), P(lam), flags, n, P(c), ld if cols else 0, P(s), P(work), wb, _stream()],
                 wb=11, null=4, keep=(aff,))]


def b_prepare(A, lib, n, flags=1):
    (x, u, y, lam), aff = _phys(A, n)
    cache = A.take("cache", lib.pinn_lambda_stage_workspace_bytes(n), "out")            # exactly 6 n floats
    assert cache.nbytes == 24 * n
    return [Call("pinn_residuals_prepare", [P(x), P(u), P(y), ctypes.byref(aff), P(lam), flags, n, P(cache), _stream()], null=7, keep=(aff,))]


def b_cached(A, lib, n, flags=1, prepared=True):
    """prepared: the cache comes from pinn_residuals_prepare on the same arena; else it is an input of arbitrary floats."""
    calls = b_prepare(A, lib, n, flags) if prepared else []
    if prepared:
        cache, lam, aff = A["cache"], A["lambda"], calls[0].keep[0]
    else:
        (lam,), aff = _phys(A, n, "l")
        cache = A.take("cache", 24 * n, "in", _rand((6 * n,), 41).abs() + 0.5)
    s = A.take("sums", 8 * 32, "out")
    wb = lib.pinn_residuals_workspace_bytes()
    work = A.take("work", wb, "scratch")
    return calls + [Call("pinn_residuals_cached", [P(cache), ctypes.byref(aff), P(lam), flags, n, P(s), P(work), wb, _stream()], wb=7, null=5,
                         keep=(aff,))]


def b_lambda_step(A, lib, n, stage=1):
    sums = A.take("sums", 8 * 32, "in", (_rand((32,), 51).abs() * n).double())
    lam = A.take("lambda", 4 * 17, "inout", _lambda())
    adam = A.take("adam", 4 * 34, "inout", np.zeros(34, np.float32))
    loss = A.take("loss", 8, "out")
    return [Call("pinn_lambda_step", [stage, P(sums), n, 0.5, 1e-3, 1, P(lam), P(adam), P(loss), _stream()], null=6)]


STAGE_FLAG = {0: 1, 1: 1, 2: 2, 3: 4, 4: 8}


def b_stage_run(A, lib, n, stage=0, n_iters=3, log_every=2):
    from pinn_amd import _lib
    (x, u, y), aff = _phys(A, n, "xuy")
    lam = A.take("lambda", 4 * 17, "inout", _lambda())
    adam = A.take("adam", 4 * 34, "inout", np.zeros(34, np.float32))
    loss = A.take("loss", 8, "out")
    n_logged = len([k for k in range(n_iters) if k % log_every == 0])
    log = A.take("log", 4 * n_logged * _lib.STAGE_LOG_FLOATS, "out")            # exactly n_logged rows
    sums = A.take("sums", 8 * 32, "out")
    wb = lib.pinn_lambda_stage_workspace_bytes(n)
    work = A.take("work", wb, "scratch")
    return [Call("pinn_lambda_stage_run", [stage, STAGE_FLAG[stage], P(x), P(u), P(y), ctypes.byref(aff), n, 1e-3, 0.8, 1000, 0, n_iters, P(lam),
                                           P(adam), P(loss), P(log), log_every, P(sums), P(work), wb, _stream()], wb=19, null=12, keep=(aff,))]


def _halo(A, halo):
    if not halo:
        return None, None
    return A.take("x_halo", 32, "in", _rand((8,), 61, 0.3)), A.take("u_halo", 4, "in", _rand((1,), 62, 0.3))      # exactly [8] and [1]


def b_f_t(A, lib, n, halo=False):
    (x, u, lam), aff = _phys(A, n, "xul")
    xh, uh = _halo(A, halo)
    o = [A.take(k, 4 * n, "out") for k in ("f", "t_pred", "t_real")]
    return [Call("pinn_net_f_t", [P(x), P(u), P(xh), P(uh), ctypes.byref(aff), P(lam), n, P(o[0]), P(o[1]), P(o[2]), _stream()], null=7, keep=(aff,))]


GRAD_COLS = {1: 0xFF, 2: 0x700, 4: 0x7800, 8: 0xF8000}


def b_residuals_backward(A, lib, n, flags=15, pad=0, omit=None):
    (x, u, lam), aff = _phys(A, n, "xul")
    ld = n + pad
    g = A.take("g", 4 * 20 * ld, "in", _rand((20, ld), 71))
    gmask = sum(m for f, m in GRAD_COLS.items() if flags & f)
    gl = A.take("glambda", 4 * 17, "out")
    gu = A.take("gu", 4 * n, "out") if omit != "gu" else None
    gx = A.take("gx", 32 * n, "out") if omit != "gx" else None
    wb = lib.pinn_residuals_workspace_bytes()
    work = A.take("work", wb, "scratch")
    return [Call("pinn_residuals_backward", [P(x), P(u), ctypes.byref(aff), P(lam), flags, n, P(g), ld, gmask, P(gl), P(gu), P(gx), P(work), wb,
                                             _stream()], wb=13, null=9, keep=(aff,))]


def b_f_t_backward(A, lib, n, halo=False):
    (x, u, lam), aff = _phys(A, n, "xul")
    xh, uh = _halo(A, halo)
    ups = [A.take(k, 4 * n, "in", _rand((n,), 80 + j)) for j, k in enumerate(("gf", "gt_pred", "gt_real"))]
    gl, gu, gx = A.take("glambda", 4 * 17, "out"), A.take("gu", 4 * n, "out"), A.take("gx", 32 * n, "out")
    gxh = A.take("gx_halo", 32, "out") if halo else None
    guh = A.take("gu_halo", 4, "out") if halo else None
    wb = lib.pinn_residuals_workspace_bytes()
    work = A.take("work", wb, "scratch")
    return [Call("pinn_net_f_t_backward", [P(x), P(u), P(xh), P(uh), ctypes.byref(aff), P(lam), n] + [P(b) for b in ups] +
                 [P(gl), P(gu), P(gx), P(gxh), P(guh), P(work), wb, _stream()], wb=16, null=10, keep=(aff,))]


def b_results(A, lib, n, window=200, segs=None, pad=0, labels=True):
    (x, y), aff = _phys(A, n, "xy")
    ld = n + pad
    seg = A.take("seg_end", 8 * len(segs), "in", np.asarray(segs, np.int64)) if segs else None
    mc = [A.take(k, 4 * n, "in", _rand((n,), 90 + j).abs()) for j, k in enumerate(("pred_mean", "a_u", "e_u"))]
    cols = A.take("cols", 4 * 20 * ld, "in", _rand((20, ld), 95))
    lab = A.take("labels", 4 * n, "in", torch.arange(n, dtype=torch.float32) % 5) if labels else None
    out = A.take("out", 8 * 22 * n, "out")                                   # exactly n 22 doubles
    return [Call("pinn_results_assemble", [P(x), P(y), ctypes.byref(aff), -1.0, 2.0, window, P(seg), len(segs) if segs else 0, P(mc[0]), P(mc[1]),
                                           P(mc[2]), P(cols), ld, P(lab), n, P(out), _stream()], null=15, keep=(aff,))]


# ---------------------------------------------------------------------------------------------------------------------------
# the three rules
def guarded_pair(lib, what, build, *args, **kw):
    """Run the calls of build(A, lib, ...) on ordinary tensors and on an arena; rules 1-3.  Returns (arena, plain, return codes)."""
    t0 = time.time()
    dev = _dev()
    plain = G.Plain(dev)
    calls = build(plain, lib, *args, **kw)
    rc_p = [c.run(lib) for c in calls]
    torch.cuda.synchronize()
    arena = G.Arena(dev, G.capacity_for([b.nbytes for b in plain.bufs]))      # not a byte more than the takes need
    calls = build(arena, lib, *args, **kw)
    rc_a = [c.run(lib) for c in calls]
    torch.cuda.synchronize()
    expect = [c.expect for c in calls]
    refused = any(e != OK for e in expect)
    diff = G.differing_outputs(arena, plain)
    print("CASE %s: rc %s (expected %s), outputs that differ from the ordinary call: %s, %.3f s" % (what, rc_a, expect, diff or "none", time.time() - t0))
    arena.check(what, untouched=refused)                                      # rule 1 (a PINN_E_ARCH call wrote nothing at all)
    assert rc_a == expect and rc_p == expect, (what, rc_a, rc_p, expect)      # rule 3: the stated sizes are enough
    assert diff == [], (what, diff)                                           # rule 2
    if not refused:            # and the comparison is one of results: a call that ran left no output buffer wholly at the fill
        idle = [b.name for b in arena.bufs if b.role == "out" and b.nbytes and b.bytes() == b"\xff" * b.nbytes]
        assert idle == [], (what, "never written", idle)
    if not refused and any(b.name == "grads+tail" for b in arena.bufs):
        assert _tail_kept(arena) and _tail_kept(plain), (what, "the loss tail behind d_grads changed")
    return arena, plain, rc_a


def refused_calls(lib, what, build, *args, **kw):
    """work_bytes one short -> PINN_E_WORKSPACE, one NULL pointer -> PINN_E_ARG; after each nothing was written."""
    dev = _dev()
    for kind in ("workspace", "null"):
        arena = G.Arena(dev, 64 << 20)
        calls = build(arena, lib, *args, **kw)
        assert len(calls) == 1
        c = calls[0]
        if kind == "workspace":
            if c.wb is None:
                continue
            c.args[c.wb] = (c.floor or c.args[c.wb]) - 1
        else:
            c.args[c.null] = None
        rc = c.run(lib)
        torch.cuda.synchronize()
        print("REFUSED %s %s: rc %d" % (what, kind, rc))
        assert rc == (E_WORKSPACE if kind == "workspace" else E_ARG), (what, kind, rc)
        arena.check("%s refused (%s)" % (what, kind), untouched=True)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def second_tile_rows(tile):
    return tile * _cus() + tile + 1


# ---------------------------------------------------------------------------------------------------------------------------
# host: the table above against the header
def test_entry_point_table_matches_the_header():
    """Every function the header declares from pinn_residuals to pinn_results_assemble is a guarded entry point with a refused-call
    case (REFUSED below) or one of the host-only queries: a new entry point cannot be forgotten."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "pinn_hip.h")).read(), flags=re.S)
    names = re.findall(r"\b(pinn_[a-z0-9_]+)\s*\(", text)
    lo, hi = names.index("pinn_residuals"), names.index("pinn_results_assemble")
    declared = set(names[lo:hi + 1])
    assert names[lo - 1] == "pinn_residuals_workspace_bytes" and names[hi + 1].startswith("pinn_rf_")
    table = set(ENTRY_POINTS) | set(HOST_QUERIES)
    assert table == declared, sorted(table ^ declared)
    assert not set(ENTRY_POINTS) & set(HOST_QUERIES)
    assert set(REFUSED) == set(ENTRY_POINTS), sorted(set(REFUSED) ^ set(ENTRY_POINTS))


# ---------------------------------------------------------------------------------------------------------------------------
# fused and wide nets
FUSED = [(128, 1), (256, 3)]
WIDE = [(512, 1), (512, 2)]            # layers [8, 512, 1] and [8, 512, 512, 1]


def _net_id(v):
    return "H%d-nh%d" % v if isinstance(v, tuple) else (PREC_NAME[v] if v in PREC_NAME and not isinstance(v, bool) else str(v))


def _net_rows(hn, prec, n):
    if n != "second":
        return n
    return second_tile_rows(64 if (hn[0] <= 256 and prec in (FP32, BF16)) else 128)


def _forward_cases(lib, hn, prec, n):
    shape = hn + (prec,)
    tag = "%s-%s-n%d " % (_net_id(hn), PREC_NAME[prec], n)
    for mode in ("eval", "philox", "bits"):
        guarded_pair(lib, tag + "forward/" + mode, b_forward, shape, n, mode=mode)
    for T in (1, 3):
        guarded_pair(lib, tag + "mc/T%d" % T, b_mc, shape, n, T=T)
    guarded_pair(lib, tag + "mc/bits", b_mc, shape, n, T=3, mode="bits")
    guarded_pair(lib, tag + "range_status", b_range_status, shape, n)


def _train_cases(lib, hn, prec, n):
    shape = hn + (prec,)
    tag = "%s-%s-n%d " % (_net_id(hn), PREC_NAME[prec], n)
    for variant in ("grads", "all", "split", "step", "step_dev"):
        guarded_pair(lib, tag + "train/" + variant, b_train, shape, n, variant=variant)


@gpu
@pytest.mark.parametrize("n", ROWS + ["second"], ids=str)
@pytest.mark.parametrize("prec", PRECS, ids=_net_id)
@pytest.mark.parametrize("hn", FUSED + WIDE, ids=_net_id)
def test_net_forward(lib, hn, prec, n):
    _forward_cases(lib, hn, prec, _net_rows(hn, prec, n))


@gpu
@pytest.mark.parametrize("n", ROWS + ["second"], ids=str)
@pytest.mark.parametrize("prec", PRECS, ids=_net_id)
@pytest.mark.parametrize("hn", FUSED + WIDE, ids=_net_id)
def test_net_training(lib, hn, prec, n):
    _train_cases(lib, hn, prec, _net_rows(hn, prec, n))


@gpu
@pytest.mark.parametrize("dev", [False, True], ids=["host-scalars", "device-scalars"])
@pytest.mark.parametrize("n", [1, 3, 257, 2048 * 256 + 5])
def test_adam(lib, n, dev):
    guarded_pair(lib, "adam n=%d dev=%s" % (n, dev), b_adam, n, dev=dev)


# ---------------------------------------------------------------------------------------------------------------------------
# any-width nets and ensembles
GNET_LAYERS = [[8, 4, 1], [8, 33, 12, 1], [8, 65, 5, 1]]
GNET_ROWS = [1, 63, 65, 129, 289]


@gpu
@pytest.mark.parametrize("n", GNET_ROWS)
@pytest.mark.parametrize("layers", GNET_LAYERS, ids=lambda l: "x".join(map(str, l)))
def test_any_width_net(lib, layers, n):
    tag = "%s-n%d " % ("x".join(map(str, layers)), n)
    guarded_pair(lib, tag + "forward", b_gnet, layers, n, call="forward")
    for T in (1, 3):
        guarded_pair(lib, tag + "mc/T%d" % T, b_gnet, layers, n, call="mc", T=T)
    guarded_pair(lib, tag + "train_grads", b_gnet, layers, n, call="grads")
    guarded_pair(lib, tag + "train_step", b_gnet, layers, n, call="step")
    for glv in (True, False):
        for gx in (True, False):
            guarded_pair(lib, tag + "backward glv=%d gx=%d" % (glv, gx), b_gnet, layers, n, call="backward", glv=glv, gx=gx)
    for omit in (None, "grads", "gx", "ggu", "gglv"):
        guarded_pair(lib, tag + "backward2 without %s" % omit, b_gnet, layers, n, call="backward2", omit=omit)


@gpu
@pytest.mark.parametrize("n", [1, 65, 200])
@pytest.mark.parametrize("e", [1, 3])
def test_ensemble(lib, e, n):
    layers = [8, 33, 12, 1]
    for call in ("forward", "grads", "step"):
        guarded_pair(lib, "gens E=%d n=%d %s" % (e, n, call), b_gnet, layers, n, call=call, e=e)


@gpu
@pytest.mark.parametrize("rows_of_one", [True, False], ids=["one-3xn-buffer", "three-buffers"])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_ensemble_combine(lib, n, rows_of_one):
    for rule in (0, 1):
        guarded_pair(lib, "combine n=%d rule=%d" % (n, rule), b_combine, n, e=3, rows_of_one=rows_of_one, rule=rule)


# ---------------------------------------------------------------------------------------------------------------------------
# physics and results
PHYS_ROWS = [1, 255, 257, 1025]


@gpu
@pytest.mark.parametrize("n", PHYS_ROWS)
def test_residual_passes(lib, n):
    for flags in (1, 2, 4, 8, 15):
        for pad in (0, 3):
            guarded_pair(lib, "residuals n=%d flags=%d ld=n+%d" % (n, flags, pad), b_residuals, n, flags=flags, pad=pad)
        guarded_pair(lib, "residuals n=%d flags=%d no cols" % (n, flags), b_residuals, n, flags=flags, cols=False)
        guarded_pair(lib, "residuals n=%d flags=%d no sums" % (n, flags), b_residuals, n, flags=flags, sums=False)
    for flags in (1, 2, 4, 8):
        guarded_pair(lib, "prepare n=%d flags=%d" % (n, flags), b_prepare, n, flags=flags)
        guarded_pair(lib, "prepare + cached n=%d flags=%d" % (n, flags), b_cached, n, flags=flags)
    for stage in range(5):
        guarded_pair(lib, "lambda_step n=%d stage=%d" % (n, stage), b_lambda_step, n, stage=stage)


@gpu
@pytest.mark.parametrize("n", [1, 64, 257])
def test_stage_run(lib, n):
    for stage in range(5):
        guarded_pair(lib, "stage_run n=%d stage=%d" % (n, stage), b_stage_run, n, stage=stage)


@gpu
@pytest.mark.parametrize("n", PHYS_ROWS)
def test_thermal_series_and_backwards(lib, n):
    for halo in (False, True):
        guarded_pair(lib, "net_f_t n=%d halo=%d" % (n, halo), b_f_t, n, halo=halo)
        guarded_pair(lib, "net_f_t_backward n=%d halo=%d" % (n, halo), b_f_t_backward, n, halo=halo)
    for pad in (0, 3):
        for omit in (None, "gu", "gx"):
            guarded_pair(lib, "residuals_backward n=%d ld=n+%d without %s" % (n, pad, omit), b_residuals_backward, n, pad=pad, omit=omit)


@gpu
@pytest.mark.parametrize("n,window,segs", [(1, 200, None), (255, 7, [100, 255]), (257, 1024, [1, 2, 257]), (700, 200, [300, 450, 700])],
                         ids=["n1", "n255", "n257", "n700"])
def test_results_assemble(lib, n, window, segs):
    for pad in (0, 5):
        for labels in (True, False):
            guarded_pair(lib, "results n=%d ld=n+%d labels=%d" % (n, pad, labels), b_results, n, window=window, segs=segs, pad=pad, labels=labels)


# ---------------------------------------------------------------------------------------------------------------------------
# refused calls write nothing: one case per entry point, at the smallest row count
X6_SMALL = (128, 1, X6)
REFUSED = {
    "pinn_residuals": (b_residuals, (1,), {}),
    "pinn_lambda_step": (b_lambda_step, (1,), {}),
    "pinn_lambda_stage_run": (b_stage_run, (1,), {}),
    "pinn_residuals_prepare": (b_prepare, (1,), {}),
    "pinn_residuals_cached": (b_cached, (1,), {"prepared": False}),
    "pinn_net_f_t": (b_f_t, (1,), {}),
    "pinn_residuals_backward": (b_residuals_backward, (1,), {}),
    "pinn_net_f_t_backward": (b_f_t_backward, (1,), {}),
    "pinn_net_range_status": (b_range_status, (X6_SMALL, 1), {"after_forward": False}),
    "pinn_mlp_forward": (b_forward, (X6_SMALL, 1), {}),
    "pinn_mc_dropout": (b_mc, (X6_SMALL, 1), {}),
    "pinn_mlp_train_grads": (b_train, (X6_SMALL, 1), {"variant": "grads"}),
    "pinn_mlp_train_grads_phases": (b_train, (X6_SMALL, 1), {"variant": "all"}),
    "pinn_adam_step": (b_adam, (1,), {}),
    "pinn_adam_step_dev": (b_adam, (1,), {"dev": True}),
    "pinn_mlp_train_step_dev": (b_train, (X6_SMALL, 1), {"variant": "step_dev"}),
    "pinn_mlp_train_step": (b_train, (X6_SMALL, 1), {"variant": "step"}),
    "pinn_gnet_forward": (b_gnet, ([8, 4, 1], 1), {"call": "forward"}),
    "pinn_gnet_mc_dropout": (b_gnet, ([8, 4, 1], 1), {"call": "mc"}),
    "pinn_gnet_train_grads": (b_gnet, ([8, 4, 1], 1), {"call": "grads"}),
    "pinn_gnet_train_step": (b_gnet, ([8, 4, 1], 1), {"call": "step"}),
    "pinn_gnet_backward": (b_gnet, ([8, 4, 1], 1), {"call": "backward"}),
    "pinn_gnet_backward2": (b_gnet, ([8, 4, 1], 1), {"call": "backward2"}),
    "pinn_gens_forward": (b_gnet, ([8, 33, 12, 1], 1), {"call": "forward", "e": 3}),
    "pinn_gens_train_grads": (b_gnet, ([8, 33, 12, 1], 1), {"call": "grads", "e": 3}),
    "pinn_gens_train_step": (b_gnet, ([8, 33, 12, 1], 1), {"call": "step", "e": 3}),
    "pinn_gens_combine": (b_combine, (1,), {}),
    "pinn_results_assemble": (b_results, (1,), {}),
}


@gpu
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_calls_write_nothing(lib, name):
    build, args, kw = REFUSED[name]
    refused_calls(lib, name, build, *args, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# device teeth, without a faulty kernel
@gpu
def test_device_teeth_one_float_too_many(lib):
    """pinn_gens_combine told n + 1 rows on outputs taken for n = 257 floats (inputs exactly [3, n + 1], all u = 1 and logvar = 0, so
    the stray values are 1.0, 1.0 and 0.0) writes exactly one float behind pred_mean, a_u and e_u -- inside the arena's own guards,
    memory this test allocated -- and check() names those three buffers at offsets 0..3 past the end, nothing else.  The only
    deliberate overrun of the suite.

    Why not pinn_adam_step with n + 1: measured on the MI355X, that call leaves findings() == [].  Its stray element is a
    read-modify-write of guard words: p, g, m and v all read 0xFFFFFFFF, a NaN, the arithmetic propagates that NaN with its payload,
    and the three stores put back exactly the fill.  (No uniform fill shows the m store: g == m leaves m = m + 0.1 (g - m) as it
    was.)  An overrun of that kind is what rule 2 and the adjacent loss tail are for; the guards see stores of anything else."""
    n = 257
    arena = G.Arena(_dev(), G.capacity_for([12 * (n + 1)] * 2 + [4 * n] * 3))
    calls = b_combine(arena, lib, n, e=3, rows_of_one=False, told=n + 1)
    assert calls[0].run(lib) == OK
    torch.cuda.synchronize()
    found = arena.findings()
    print("TEETH", found)
    assert found == [("pred_mean", "after", 0, 3, 4), ("a_u", "after", 0, 3, 4), ("e_u", "after", 0, 3, 4)], found
    with pytest.raises(G.GuardError) as e:
        arena.check("teeth")
    for name in ("pred_mean", "a_u", "e_u"):
        assert "guard after %s: 4 bytes changed, offsets 0..3 past the end" % name in str(e.value)
    assert "guard after u:" not in str(e.value) and "input" not in str(e.value) and str(e.value).count("guard") == 3
    out = torch.cat([arena[k].view(torch.float32) for k in ("pred_mean", "a_u", "e_u")]).cpu()
    assert out.tolist() == [1.0] * (2 * n) + [0.0] * n
