"""`DNN` and `PhysicsInformedNN` -- the reference's model surface on the gfx950 HIP library.

Mirrors 01_train_pinn_multiphysics_model.py (cited 01:<line>): same constructor, attributes
(`.dnn`, `.lambda_*`, `.x`, `.u`, `.X`, `.x_scal`, `.u_scal`), methods (`net_u`, `net_f_V`,
`net_f_T_simple`, `net_f_T`, `net_f_H`, `net_f_O`, `aleatoric_loss`, `train_dnn`, `train_lambda`,
`train_thermal`, `train_hydrogen`, `train_oxygen`, `predict`) and tuple orders, so the
reference's `__main__` (01:2139-2158) and its scripts 02-05 run unchanged on top.

What is underneath is different: every numeric step is a call through the C ABI of
include/pinn_hip.h (ctypes, raw device pointers, the current HIP stream).  torch supplies
device memory, streams and `torch.distributed`; there is no CPU fallback.

Extensions (keyword-only, all optional): `precision` ("f32x6", default: fp32-accurate matrix math on the bf16
matrix cores, same parity tolerances as "fp32"; "fp32": exact fp32 MFMA; "bf16" = bf16 MFMA inputs with fp32
accumulation, rtol ~2e-2 -- see DNN.set_precision), `seed` (Philox dropout seed), `row_offset` /
`n_global` (this process holds rows [row_offset, row_offset+N) of an n_global-row series:
data-parallel training with one all-reduce(SUM) of the flat gradient per step),
`train_dnn(..., batch_size=)` for minibatches, and `kernels` ("auto", default: the shapes `layout.check_arch` accepts on the
fused / wide kernels; "general": ANY layers list `layout.check_general` accepts -- unequal widths, widths 1..2048 -- on the
exact-fp32 layer-by-layer kernels of csrc/pinn_general.hip, precision "fp32" only), and `autograd` (False, default: DNN
outputs carry no grad_fn; True: they are differentiable under torch autograd with respect to the inputs and the 14 weight and
bias tensors -- see DNN.forward; "double": also twice differentiable through dL/dx, so that a loss may contain
`torch.autograd.grad(u.sum(), x, create_graph=True)[0]` -- see DNN.autograd), and `physics_autograd` (False, default: the physics functions return plain tensors; "lambdas":
differentiable with respect to the physics parameters, the reference's own graph; "full": also with respect to X, halo rows and,
through the DNN output, the weights -- see PhysicsInformedNN.physics_autograd).
"""
import ctypes
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, layout
from . import dp as _dp

LAMBDA_NAMES = ["lambda_1", "lambda_2", "lambda_3", "lambda_4",
                "lambda_T1", "lambda_T2", "lambda_T3", "lambda_T4", "lambda_T5",
                "lambda_H1", "lambda_H2", "lambda_H3", "lambda_H4",
                "lambda_O1", "lambda_O2", "lambda_O3", "lambda_O4"]
# initial values: 01:453-456, 477-481, 497-500, 514-517
LAMBDA_INIT = [0.167897923477715, 2.36682075851268e-06, 2.43414469188443, 1.0,
               10.0, 10.0, 10.0, 10.0, 10.0,
               5.0, -1.559, 197.715, 1.20,
               2.0, 0.5, 200.0, 1.0]


def _device():
    if not torch.cuda.is_available():
        raise _lib.PinnError("pinn_amd needs a ROCm GPU (gfx950): torch.cuda.is_available() is False and there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _as_rows(g, n):
    """An upstream gradient [n, 1] (or None) as a contiguous float32 vector of n entries."""
    return None if g is None else g.detach().reshape(n).to(torch.float32).contiguous()


class _DNNFunction(torch.autograd.Function):
    """DNN.forward as one autograd node: the forward is the kernel call of DNN._run; the backward is pinn_gnet_backward (exact
    fp32, csrc/pinn_general.hip) with the dropout masks the forward drew, and returns the gradient of every parameter tensor (views of
    one fresh flat buffer) and, if x requires it, of x."""

    @staticmethod
    def forward(ctx, dnn, row_offset, x, *params):
        u, lv, drop, keep = dnn._run(x, row_offset)
        ctx.dnn = dnn
        ctx.drop = None if drop is None else _lib.Dropout.from_buffer_copy(drop)
        ctx.keep = keep                           # keeps the injected keep-mask tensor of the pass alive until the backward
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, *params)
        if not dnn.logvar:
            ctx.mark_non_differentiable(lv)
        return u, lv

    @staticmethod
    def backward(ctx, g_u, g_lv):
        if torch.is_grad_enabled():
            if ctx.dnn._autograd != "double":
                raise RuntimeError("pinn_amd.DNN is once-differentiable under autograd: create_graph=True (double backward) is not supported")
            x, *params = ctx.saved_tensors
            out = _DNNGradFunction.apply(ctx.dnn, ctx.drop, ctx.keep, ctx.needs_input_grad[2], g_u, g_lv, x, *params)
            return (None, None) + tuple(out)
        return _DNNFunction._vjp(ctx, g_u, g_lv)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def _vjp(ctx, g_u, g_lv):
        x, *params = ctx.saved_tensors               # torch's version check: an in-place change since the forward raises here
        return (None, None) + _dnn_vjp(ctx.dnn, ctx.drop, ctx.needs_input_grad[2], g_u, g_lv, x)


def _dnn_vjp(dnn, drop, want_gx, g_u, g_lv, x):
    """The pinn_gnet_backward call of the DNN node -> (dL/dx or None, every parameter's gradient as views of one fresh flat buffer)."""
    n = x.shape[0]
    total = dnn._flat.numel()
    grads = (torch.zeros if n == 0 else torch.empty)(total, dtype=torch.float32, device=x.device)
    gx = torch.zeros(n, 8, dtype=torch.float32, device=x.device) if want_gx else None
    if n > 0:
        gu = _as_rows(g_u, n) if g_u is not None else torch.zeros(n, dtype=torch.float32, device=x.device)
        glv = _as_rows(g_lv, n) if dnn.logvar else None
        gnet, work = dnn._backward_net(n)
        rc = dnn._lib.pinn_gnet_backward(ctypes.byref(gnet), _ptr(dnn._flat), _ptr(x), n,
                                         ctypes.byref(drop) if drop is not None else None, _ptr(gu), _ptr(glv),
                                         _ptr(grads), _ptr(gx), _ptr(work), work.numel(), _stream())
        _lib.check(rc, "pinn_gnet_backward")
    pg = [grads[off:off + nel].view(shape) for _, _, off, nel, shape in dnn._views]
    return (gx,) + tuple(pg)


class _DNNGradFunction(torch.autograd.Function):
    """The backward of _DNNFunction as an autograd node of its own (autograd="double", backward taken under create_graph=True):
    the forward is the same pinn_gnet_backward call; the backward is pinn_gnet_backward2 (csrc/pinn_general.hip), the gradient of
    <v, dL/dx> with respect to g_u, g_lv, x and the parameters for the cotangent v that arrives on dL/dx.  Second order goes
    through dL/dx only: a cotangent on a parameter gradient (a Hessian-vector product in the weights) raises."""

    @staticmethod
    def forward(ctx, dnn, drop, keep, want_gx, g_u, g_lv, x, *params):
        ctx.dnn, ctx.drop, ctx.keep = dnn, drop, keep
        ctx.have = (g_u is not None, g_lv is not None)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*([t for t in (g_u, g_lv) if t is not None] + [x] + list(params)))
        return _dnn_vjp(dnn, drop, want_gx, g_u, g_lv, x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v_x, *v_params):
        if any(v is not None for v in v_params):
            raise RuntimeError("pinn_amd.DNN autograd='double' differentiates twice through dL/dx only: a gradient flowing back into a "
                               "parameter gradient (a Hessian-vector product with respect to the weights) is not supported")
        saved = list(ctx.saved_tensors)              # torch's version check, as in the first backward
        g_u = saved.pop(0) if ctx.have[0] else None
        g_lv = saved.pop(0) if ctx.have[1] else None
        x, params = saved[0], saved[1:]
        none = (None,) * (7 + len(params))
        if v_x is None:
            return none
        dnn = ctx.dnn
        n = x.shape[0]
        dev = x.device
        need = ctx.needs_input_grad
        want_gu = g_u is not None and need[4]
        want_glv = g_lv is not None and dnn.logvar and need[5]
        want_w = any(need[7:])
        if n == 0:
            return (None,) * 4 + (torch.zeros_like(g_u) if want_gu else None, torch.zeros_like(g_lv) if want_glv else None,
                                  torch.zeros_like(x) if need[6] else None) + tuple(torch.zeros_like(p) if w else None
                                                                                    for p, w in zip(params, need[7:]))
        grads = torch.empty(dnn._flat.numel(), dtype=torch.float32, device=dev) if want_w else None
        gx = torch.empty(n, 8, dtype=torch.float32, device=dev) if need[6] else None
        ggu = torch.empty(n, dtype=torch.float32, device=dev) if want_gu else None
        gglv = torch.empty(n, dtype=torch.float32, device=dev) if want_glv else None
        gu = _as_rows(g_u, n) if g_u is not None else torch.zeros(n, dtype=torch.float32, device=dev)
        glv = _as_rows(g_lv, n) if dnn.logvar else None
        vx = v_x.detach().to(torch.float32).contiguous()
        gnet, work = dnn._backward2_net(n)
        rc = dnn._lib.pinn_gnet_backward2(ctypes.byref(gnet), _ptr(dnn._flat), _ptr(x), n,
                                          ctypes.byref(ctx.drop) if ctx.drop is not None else None, _ptr(gu), _ptr(glv), _ptr(vx),
                                          _ptr(grads), _ptr(gx), _ptr(ggu), _ptr(gglv), _ptr(work), work.numel(), _stream())
        _lib.check(rc, "pinn_gnet_backward2")
        pg = tuple(grads[off:off + nel].view(shape) if w else None
                   for (_, _, off, nel, shape), w in zip(dnn._views, need[7:]))
        return (None,) * 4 + (ggu.view_as(g_u) if want_gu else None, gglv.view_as(g_lv) if want_glv else None, gx) + pg


PHYSICS_AUTOGRAD_MODES = (False, "lambdas", "full")

# Tuple columns of the four pinn_residuals models: (column, physics parameters it reads, reads x, reads u)
_L = {n: i for i, n in enumerate(LAMBDA_NAMES)}
_RES_SPECS = {
    _lib.RES_V: (["lambda_1", "lambda_2", "lambda_3"],
                 [("FV", (0, 1, 2), True, True), ("VACT", (1,), True, False), ("VOHM", (0,), True, False), ("VCONC", (2,), True, False),
                  ("ENERNST", (), True, False), ("VEST5", (0, 1, 2), True, False), ("I", (), True, False), ("VOUT5", (), False, True)]),
    _lib.RES_T: (["lambda_T1", "lambda_T3", "lambda_T5"],
                 [("FT", (0, 1, 2), True, False), ("TPRED", (0, 1, 2), True, False), ("TOUT", (), True, False)]),
    _lib.RES_H: (["lambda_H1", "lambda_H2", "lambda_H3"],
                 [("FH", (0, 1, 2), True, False), ("ACTH", (), True, False), ("TGTH", (0, 1, 2), True, False), ("ITOT", (), True, False)]),
    _lib.RES_O: (["lambda_O1", "lambda_O2", "lambda_O3"],
                 [("FO", (0, 1, 2), True, False), ("ACTO", (), True, False), ("TGTO", (0, 1, 2), True, False), ("QO2", (), True, False),
                  ("O2FLOW", (), True, False)]),
}
_EULER_LAMBDAS = ["lambda_T1", "lambda_T2", "lambda_T3", "lambda_T4"]


def _no_double_backward(what):
    if torch.is_grad_enabled():
        raise RuntimeError("pinn_amd.%s is once-differentiable under autograd: create_graph=True (double backward) is not supported" % what)


def _differentiable(lams, x, u, deps, x_dep, u_dep):
    return (any(lams[j].requires_grad for j in deps) or (x_dep and x is not None and x.requires_grad)
            or (u_dep and u is not None and u.requires_grad))


class _ResidualsFunction(torch.autograd.Function):
    """One of net_f_V / net_f_T_simple / net_f_H / net_f_O as one autograd node: the forward is today's pinn_residuals call
    (bit-identical columns); the backward is pinn_residuals_backward, which recomputes the rows' terms from x, u and the
    parameters the forward used.  Inputs: the normalised rows, the DNN output u (voltage model) and the model's physics
    parameters; tuple elements that depend on nothing requiring grad are non-differentiable."""

    @staticmethod
    def forward(ctx, model, flags, x_scal, xd, u, *lams):
        c = model._residuals(xd, x_scal, flags, u=u)
        ctx.model, ctx.flags, ctx.aff = model, flags, model._affine(x_scal)
        ctx.lam = model._lambda.clone()          # the values this forward used, for the backward's recomputation
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xd, u, *lams)      # version counters: an in-place change before the backward raises there
        names, cols = _RES_SPECS[flags]
        outs = tuple(c[_lib.C[name]].unsqueeze(1) for name, _, _, _ in cols)
        nd = [o for o, (_, deps, xdp, udp) in zip(outs, cols) if not _differentiable(lams, xd, u, deps, xdp, udp)]
        if nd:
            ctx.mark_non_differentiable(*nd)
        return outs

    @staticmethod
    def backward(ctx, *gouts):
        _no_double_backward("PhysicsInformedNN residuals")
        return _ResidualsFunction._vjp(ctx, *gouts)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def _vjp(ctx, *gouts):
        xd, u, *lams = ctx.saved_tensors
        model, n = ctx.model, xd.shape[0]
        names, cols = _RES_SPECS[ctx.flags]
        dev = xd.device
        present = [(_lib.C[name], g) for (name, _, _, _), g in zip(cols, gouts) if g is not None]
        gmask, g = 0, None
        if present and n > 0:
            g = torch.zeros(max(k for k, _ in present) + 1, n, dtype=torch.float32, device=dev)
            for k, gk in present:
                g[k].copy_(gk.reshape(n))
                gmask |= 1 << k
        gx = torch.empty(n, 8, dtype=torch.float32, device=dev) if ctx.needs_input_grad[3] else None
        gu = torch.empty(n, dtype=torch.float32, device=dev) if ctx.needs_input_grad[4] else None
        gl = torch.empty(_lib.NLAMBDA, dtype=torch.float32, device=dev)
        rc = model._lib.pinn_residuals_backward(_ptr(xd.detach()), _ptr(u), ctypes.byref(ctx.aff), _ptr(ctx.lam), ctx.flags, n, _ptr(g), n,
                                                gmask, _ptr(gl), _ptr(gu), _ptr(gx), _ptr(model._res_work), model._res_work.numel(),
                                                _stream())
        _lib.check(rc, "pinn_residuals_backward")
        lg = tuple(gl[_L[nm]:_L[nm] + 1] if ctx.needs_input_grad[5 + j] else None for j, nm in enumerate(names))
        if gu is not None:
            gu = gu.view(u.shape)
        return (None, None, None, gx, gu) + lg


class _EulerFunction(torch.autograd.Function):
    """net_f_T (the Euler model, pinn_net_f_t) as one autograd node; backward: pinn_net_f_t_backward.  Inputs: the rows, the
    DNN output u, the optional halo row and its u, and lambda_T1..T4."""

    @staticmethod
    def forward(ctx, model, x_scal, xd, u, xh, uh, *lams):
        n = xd.shape[0]
        aff = model._affine(x_scal)
        out = torch.empty(3, n, device=xd.device, dtype=torch.float32)
        rc = model._lib.pinn_net_f_t(_ptr(xd), _ptr(u), _ptr(xh), _ptr(uh), ctypes.byref(aff), _ptr(model._lambdas()), n,
                                     _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream())
        _lib.check(rc, "pinn_net_f_t")
        ctx.model, ctx.aff = model, aff
        ctx.lam = model._lambda.clone()
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xd, u, xh, uh, *lams)
        f, pred, real = out[0].unsqueeze(1), out[1].unsqueeze(1), out[2].unsqueeze(1)
        step = (any(l.requires_grad for l in lams) or xd.requires_grad or any(t is not None and t.requires_grad for t in (u, xh, uh)))
        nd = ([] if step else [f, pred]) + ([] if xd.requires_grad else [real])
        if nd:
            ctx.mark_non_differentiable(*nd)
        return f, pred, real

    @staticmethod
    def backward(ctx, g_f, g_pred, g_real):
        _no_double_backward("PhysicsInformedNN.net_f_T")
        return _EulerFunction._vjp(ctx, g_f, g_pred, g_real)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def _vjp(ctx, g_f, g_pred, g_real):
        xd, u, xh, uh, *lams = ctx.saved_tensors
        model, n = ctx.model, xd.shape[0]
        dev = xd.device
        need = ctx.needs_input_grad
        gx = torch.empty(n, 8, dtype=torch.float32, device=dev) if need[2] else None
        gu = torch.empty(n, dtype=torch.float32, device=dev) if need[3] else None
        gxh = torch.empty(8, dtype=torch.float32, device=dev) if need[4] else None
        guh = torch.empty(1, dtype=torch.float32, device=dev) if need[5] else None
        gl = torch.empty(_lib.NLAMBDA, dtype=torch.float32, device=dev)
        rc = model._lib.pinn_net_f_t_backward(_ptr(xd.detach()), _ptr(u), _ptr(xh), _ptr(uh), ctypes.byref(ctx.aff), _ptr(ctx.lam), n,
                                              _ptr(_as_rows(g_f, n)), _ptr(_as_rows(g_pred, n)), _ptr(_as_rows(g_real, n)), _ptr(gl),
                                              _ptr(gu), _ptr(gx), _ptr(gxh), _ptr(guh), _ptr(model._res_work), model._res_work.numel(),
                                              _stream())
        _lib.check(rc, "pinn_net_f_t_backward")
        lg = tuple(gl[_L[nm]:_L[nm] + 1] if need[6 + j] else None for j, nm in enumerate(_EULER_LAMBDAS))
        return (None, None, gx, None if gu is None else gu.view(u.shape), gxh, guh) + lg


class DNN(torch.nn.Module):
    """01:389-438.  Same module tree / state_dict keys as the reference; the 14 weight and
    bias tensors are views into ONE flat float32 device buffer that the kernels read."""

    def __init__(self, p, logvar, layers, seed=0, precision=None, kernels="auto", autograd=False):
        """kernels="auto": the shapes layout.check_arch accepts, precision None = "f32x6".  kernels="general": any list
        layout.check_general accepts (exact-fp32 layer-by-layer kernels, csrc/pinn_general.hip); precision None or "fp32".
        autograd=True: outputs are differentiable under torch autograd (see forward); "double": twice, through dL/dx (see the
        `autograd` property); neither with precision "bf16"."""
        super().__init__()
        self._autograd = False
        self.depth = len(layers) - 1
        self.p = p
        self.logvar = logvar
        self.activation = torch.nn.Tanh
        if kernels not in ("auto", "general"):
            raise ValueError("kernels must be 'auto' or 'general'")
        self.kernels = kernels
        dev = _device()
        self._lib = _lib.load()
        self._packed = None
        self._gwork = None
        self._bwork = None
        self._b2work = None
        if kernels == "general":
            self.widths = layout.check_general(layers)
            if precision not in (None, "fp32"):
                raise ValueError("kernels='general' runs exact fp32 only (precision None or 'fp32', got %r)" % (precision,))
            self.n_in, self.hidden, self.n_hidden = int(layers[0]), None, len(self.widths)
            self._net = None
            self._gnet = _lib.GNet(layers)
            offs, total = layout.general_offsets(layers)
            assert self._lib.pinn_gnet_param_count(ctypes.byref(self._gnet)) == total
            self.precision = "fp32"
        else:
            self.n_in, self.hidden, self.n_hidden = layout.check_arch(layers)
            self.widths = [self.hidden] * self.n_hidden
            self._gnet = None
            self._net = _lib.Net(self.n_in, self.hidden, self.n_hidden)
            offs, total = layout.param_offsets(self.n_in, self.hidden, self.n_hidden)
            assert self._lib.pinn_param_count(ctypes.byref(self._net)) == total
            # the autograd backward of these nets runs on the general kernels: same flat layout, Philox stream and keep-bit words
            bl = [self.n_in] + [self.hidden] * self.n_hidden + [1]
            self._bwd_gnet = _lib.GNet(bl)
            assert layout.general_offsets(bl) == (offs, total)
            assert self._lib.pinn_gnet_param_count(ctypes.byref(self._bwd_gnet)) == total
            self.set_precision("f32x6" if precision is None else precision)
        self.layer_sizes = [self.n_in] + list(self.widths) + [1]
        self._offsets = offs
        self._flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self._flat_grad_full = torch.zeros(total + _dp.LOSS_TAIL, dtype=torch.float32, device=dev)
        self._flat_grad = self._flat_grad_full[:total]

        layer_list = []
        for i in range(self.depth - 1):
            layer_list.append(("layer_%d" % i, torch.nn.Linear(layers[i], layers[i + 1])))
            layer_list.append(("activation_%d" % i, self.activation()))
            layer_list.append(("dropout_%d" % i, torch.nn.Dropout(p=self.p)))
        self.layers = torch.nn.Sequential(OrderedDict(layer_list))
        self.predict = torch.nn.Linear(layers[-2], layers[-1])
        self.var_layers = torch.nn.Sequential(
            torch.nn.Linear(layers[-2], layers[-2] // 2), torch.nn.Tanh(), torch.nn.Dropout(p=self.p),
            torch.nn.Linear(layers[-2] // 2, layers[-2] // 4), torch.nn.Tanh(),
            torch.nn.Linear(layers[-2] // 4, layers[-1]))
        # move the torch-default initial values into the flat buffer and alias the Parameters onto it
        mods = dict(self.named_modules())
        self._views = []
        for name, shape, off in offs:
            mname, pname = name.rsplit(".", 1)
            mod = mods[mname]
            init = getattr(mod, pname).detach()
            n = init.numel()
            view = self._flat[off:off + n].view(shape)
            view.copy_(init)
            par = torch.nn.Parameter(view)
            par.grad = self._flat_grad[off:off + n].view(shape)
            setattr(mod, pname, par)
            self._views.append((mod, pname, off, n, shape))
        self.seed = int(seed)
        self._fwd_counter = 0
        # parity-test hook: int32 device tensor [n_passes, N, words] of bit-packed keep-masks;
        # when set, stochastic passes replay these masks instead of drawing Philox ones
        self._mask_bits = None
        self._mask_pass = 0
        self.autograd = autograd

    @property
    def autograd(self):
        """True: forward is differentiable under torch autograd (weights and inputs), once.  "double": also twice, through dL/dx: a
        backward taken under create_graph=True returns a dL/dx that losses can contain (pinn_gnet_backward2).  Returns what was
        set.  Settable; raises ValueError for "bf16" nets and for any other string."""
        return self._autograd

    @autograd.setter
    def autograd(self, on):
        if isinstance(on, str):
            if on != "double":
                raise ValueError("autograd must be False, True or 'double' (got %r)" % (on,))
        else:
            on = bool(on)
        if on and self.precision == "bf16":
            raise ValueError("autograd=%r needs an fp32-accurate forward: precision 'bf16' is not (use 'f32x6', 'f32x6g6' or 'fp32')"
                             % (on,))
        self._autograd = on

    def set_precision(self, precision):
        """"fp32": exact fp32 matrix math (v_mfma_f32_*_f32; hidden <= 256 only).  "f32x6" (default): fp32-ACCURATE matrix
        math on the 16-bit matrix cores from split operands (two fp16 parts, three products, fp32 accumulation; gradients
        under exact power-of-two scales) -- same parity tolerances as "fp32", 2-3x faster.  "f32x6g6": as "f32x6" with the
        gradients from three bf16 parts / six products (24-bit operands, fp32's exponent range per element; ~20 % slower).
        "bf16": bf16 MFMA inputs, fp32 accumulate / activations / loss / master weights; rtol ~2e-2.
        kernels="general" nets: "fp32" only."""
        if self.kernels == "general":
            if precision != "fp32":
                raise ValueError("kernels='general' runs exact fp32 only (got %r)" % (precision,))
            return
        codes = {"fp32": _lib.PREC_FP32, "bf16": _lib.PREC_BF16, "f32x6": _lib.PREC_F32X6, "f32x6g6": _lib.PREC_F32X6_G6}
        if precision not in codes:
            raise ValueError("precision must be 'fp32', 'f32x6', 'f32x6g6' or 'bf16'")
        if precision == "bf16" and self._autograd:
            raise ValueError("precision 'bf16' is not fp32-accurate: set dnn.autograd = False first")
        self.precision = precision
        if precision == "fp32":
            self._net = _lib.Net(self.n_in, self.hidden, self.n_hidden, _lib.PREC_FP32, None)
            return
        probe = _lib.Net(self.n_in, self.hidden, self.n_hidden, codes[precision], None)
        nbytes = self._lib.pinn_packed_bytes(ctypes.byref(probe))
        if self._packed is None or self._packed.numel() < nbytes:
            self._packed = torch.empty(nbytes, dtype=torch.uint8, device=_device())
        self._net = _lib.Net(self.n_in, self.hidden, self.n_hidden, codes[precision], self._packed.data_ptr())

    def check_range(self):
        """Raise PinnRangeError when the last launches met a weight (or, in training, a gradient) outside the domain of the
        split-operand precisions -- |w| >= 1023.5 in a hidden or variance-head matrix, which the fp32 reference (01:389-438)
        computes without trouble.  Synchronises the stream: called where the host waits anyway (log lines, results).
        A no-op on kernels="general" nets (exact fp32: no range limit)."""
        if self.kernels == "general":
            return
        rc = self._lib.pinn_net_range_status(ctypes.byref(self._net), _stream())
        if rc == _lib.E_RANGE:
            raise _lib.PinnRangeError(
                "a weight or gradient left the range of precision %r (|w| must stay below 1023.5 in the hidden and variance-head "
                "matrices); the outputs of the last calls are inf / NaN there.  dnn.set_precision('fp32') has no such limit%s"
                % (self.precision, "" if self.hidden <= 256 else " but does not support this width"))
        _lib.check(rc, "pinn_net_range_status")

    # -- flat buffer <-> Parameter aliasing ------------------------------------------------
    def flat_params(self):
        """The flat parameter buffer; re-gathers a Parameter that user code re-pointed elsewhere."""
        base = self._flat.data_ptr()
        for mod, pname, off, n, shape in self._views:
            par = getattr(mod, pname)
            if par.data_ptr() != base + 4 * off or not par.is_contiguous():
                view = self._flat[off:off + n].view(shape)
                view.copy_(par.detach().to(self._flat.device, torch.float32))
                par.data = view
        return self._flat

    def dropout_modules(self):
        return [m for _, m in self.named_modules() if isinstance(m, torch.nn.Dropout)]

    def dropout_struct(self, stream_id, row_offset=0, mode=None, p_override=None):
        d = _lib.Dropout()
        mods = self.dropout_modules()
        d.mode = _lib.DROP_PHILOX if mode is None else mode
        for l, m in enumerate(mods):
            d.p[l] = float(m.p if p_override is None else p_override)
        d.seed = self.seed
        d.stream = int(stream_id) & 0xFFFFFFFF
        d.row_offset = int(row_offset)
        d.d_bits = None
        if self._mask_bits is not None and mode is None:
            d.mode = _lib.DROP_BITS
            d.d_bits = self._mask_bits[self._mask_pass].data_ptr()
        return d

    def _grown(self, cache, query, gnet, *args):
        """The uint8 tensor cached in attribute `cache`, grown to the bytes that the library's `query`(gnet, *args) asks for."""
        nb = getattr(self._lib, query)(ctypes.byref(gnet), *args)
        if nb == 0:
            raise _lib.PinnError(query + " rejected the network")
        work = getattr(self, cache)
        if work is None or work.numel() < nb:
            setattr(self, cache, None)          # free the smaller one first
            work = torch.empty(nb, dtype=torch.uint8, device=self._flat.device)
            setattr(self, cache, work)
        return work

    def general_workspace(self, n_rows, n_passes=0):
        """Workspace of the general kernels for n_rows rows (and n_passes MC passes); cached, grown on demand."""
        return self._grown("_gwork", "pinn_gnet_workspace_bytes", self._gnet, int(n_rows), int(n_passes))

    def _backward_net(self, n_rows):
        """(pinn_gnet_t, workspace) that pinn_gnet_backward runs on for n_rows rows: general nets their own net and workspace,
        fused / wide nets the equal-width general net and a workspace cached for the backward."""
        if self.kernels == "general":
            return self._gnet, self.general_workspace(n_rows)
        return self._bwd_gnet, self._grown("_bwork", "pinn_gnet_workspace_bytes", self._bwd_gnet, int(n_rows), 0)

    def _backward2_net(self, n_rows):
        """(pinn_gnet_t, workspace) of pinn_gnet_backward2 for n_rows rows: the net of _backward_net, a workspace of its own."""
        gnet = self._gnet if self.kernels == "general" else self._bwd_gnet
        return gnet, self._grown("_b2work", "pinn_gnet_backward2_workspace_bytes", gnet, int(n_rows))

    def inject_masks(self, bits):
        """Replay recorded keep-masks (tests only). bits: int32 [n_passes, N, words] or None."""
        self._mask_bits = None if bits is None else bits.to(self._flat.device).contiguous()
        self._mask_pass = 0

    def forward(self, x, row_offset=0):
        """(out [N,1], logvar [N,1]) -- eval: dropout off; train: on-chip Philox masks (01:421-438).

        With `autograd` on, grad mode enabled and x or a parameter requiring grad, the call is one torch.autograd.Function: the
        same kernel call (bit-identical outputs), and a backward (pinn_gnet_backward) that recomputes the forward with the masks
        this call drew and returns dL/dx and every parameter's gradient.  The backward is exact fp32 for every kernel family; on
        "f32x6" / "f32x6g6" nets it is the gradient of the exact-fp32 function at the same parameters and masks, which agrees with
        the gradient of the split-operand forward to fp32 accuracy.  Once-differentiable (create_graph=True raises) unless `autograd` is "double": then a backward under create_graph=True is
        the same pinn_gnet_backward call recorded as a node whose backward is pinn_gnet_backward2 (exact fp32, same masks), for
        cotangents on dL/dx only; a third derivative, or a cotangent on a parameter gradient, raises.  logvar=False:
        the logvar output is a constant zero."""
        params = [getattr(mod, pname) for mod, pname, _, _, _ in self._views]
        if self._autograd and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            self.flat_params()                          # re-gather re-pointed Parameters before autograd records them
            params = [getattr(mod, pname) for mod, pname, _, _, _ in self._views]
            xd = x.to(self._flat.device, torch.float32).contiguous()      # differentiable: x.grad comes back in x's dtype / device
            u, lv = _DNNFunction.apply(self, int(row_offset), xd, *params)
        else:
            u, lv, _, _ = self._run(x.detach(), row_offset)
        if not self.logvar:
            lv = torch.zeros_like(u)
        return u, lv

    def _run(self, x, row_offset):
        """The kernel call of forward -> (u, logvar, the dropout struct it used or None, the injected mask tensor or None)."""
        x = x.detach().to(self._flat.device, torch.float32).contiguous()
        n = x.shape[0]
        u = torch.empty(n, 1, device=x.device, dtype=torch.float32)
        lv = torch.empty(n, 1, device=x.device, dtype=torch.float32)
        drop = None
        if self.training and any(m.p > 0 for m in self.dropout_modules()):
            self._fwd_counter += 1
            drop = self.dropout_struct(0x80000000 + self._fwd_counter, row_offset)
            if self._mask_bits is not None:
                self._mask_pass += 1
        if self.kernels == "general":
            work = self.general_workspace(n)
            rc = self._lib.pinn_gnet_forward(ctypes.byref(self._gnet), _ptr(self.flat_params()), _ptr(x), n,
                                             ctypes.byref(drop) if drop is not None else None, _ptr(u), _ptr(lv), _ptr(work),
                                             work.numel(), _stream())
            _lib.check(rc, "pinn_gnet_forward")
        else:
            rc = self._lib.pinn_mlp_forward(ctypes.byref(self._net), _ptr(self.flat_params()), _ptr(x), n,
                                            ctypes.byref(drop) if drop is not None else None, _ptr(u), _ptr(lv), _stream())
            _lib.check(rc, "pinn_mlp_forward")
        keep = self._mask_bits if drop is not None and drop.mode == _lib.DROP_BITS else None
        return u, lv, drop, keep


class PhysicsInformedNN():
    """01:441-1410."""

    def __init__(self, X, u, layers, x_scal, u_scal, p, logvar, *, seed=0, row_offset=0, n_global=None, process_group=None,
                 precision=None, kernels="auto", autograd=False, physics_autograd=False):
        """kernels="general" runs any layers list layout.check_general accepts on the exact-fp32 layer-by-layer kernels
        (precision None or "fp32"); such nets train launch by launch (use_graph is ignored) and, data-parallel, with one
        blocking all-reduce of the whole gradient per step (no two-part overlap).  autograd=True / "double": see DNN.forward (passed to
        the DNN; `model.dnn.autograd` is settable).  physics_autograd: see the `physics_autograd` property.  The library's
        trainers use neither."""
        dev = _device()
        self._lib = _lib.load()
        self.x = X[:, 0:].clone().detach().float().to(dev).contiguous().requires_grad_(True)
        self.u = u.clone().detach().float().to(dev).contiguous()
        self.u_scal = u_scal
        self.x_scal = x_scal
        self.X = X
        self.row_offset = int(row_offset)
        self.n_local = int(self.x.shape[0])
        self.n_global = int(n_global) if n_global is not None else self.n_local
        self._group = process_group
        # 17 physics parameters: one device vector, each nn.Parameter a 1-element view of it
        self._lambda = torch.tensor(LAMBDA_INIT, dtype=torch.float32, device=dev)
        for i, name in enumerate(LAMBDA_NAMES):
            setattr(self, name, torch.nn.Parameter(self._lambda[i:i + 1]))
        self.dnn = DNN(p, logvar, layers, seed=seed, precision=precision, kernels=kernels, autograd=autograd)
        # registration order and the `lambda_3` <- lambda_4 overwrite of 01:465-468 are kept for state_dict parity
        self.dnn.register_parameter("lambda_1", self.lambda_1)
        self.dnn.register_parameter("lambda_2", self.lambda_2)
        self.dnn.register_parameter("lambda_3", self.lambda_3)
        self.dnn.register_parameter("lambda_3", self.lambda_4)
        for name in LAMBDA_NAMES[4:]:
            self.dnn.register_parameter(name, getattr(self, name))
        self._step_counter = 0
        self._work = {}
        self._aff_cache = {}
        n = self.dnn._flat.numel()
        self._adam_m = torch.zeros(n, dtype=torch.float32, device=dev)
        self._adam_v = torch.zeros(n, dtype=torch.float32, device=dev)
        self._sums = torch.zeros(_lib.NSUMS, dtype=torch.float64, device=dev)
        self._res_work = torch.empty(self._lib.pinn_residuals_workspace_bytes(), dtype=torch.uint8, device=dev)
        self.verbose = True
        self._physics_autograd = False
        self.physics_autograd = physics_autograd

    @property
    def physics_autograd(self):
        """Whether net_f_V / net_f_T_simple / net_f_H / net_f_O / net_f_T are differentiable under torch autograd.

        False (default): plain tensors, no grad_fn.  "lambdas": the reference's graph -- each function is one autograd node
        (the same kernel call, bit-identical outputs) whose differentiable inputs are the physics parameters only; the rows
        and the DNN output enter as constants, as the reference's numpy round trip makes them.  "full": also differentiable
        with respect to X (when the tensor passed requires grad), to `halo` tensors that require grad and, through the DNN
        output inside net_f_V / net_f_T, to the network's weights; needs model.dnn.autograd = True.  Both modes: nothing is
        recorded under torch.no_grad(); once-differentiable (create_graph=True raises).  Parameter gradients are sums over
        the local rows: under data parallelism all-reduce them like the DNN's gradients.  Settable; ValueError for other
        values and for "full" without dnn.autograd."""
        return self._physics_autograd

    @physics_autograd.setter
    def physics_autograd(self, mode):
        if mode is None:
            mode = False
        if isinstance(mode, bool) and mode:
            raise ValueError("physics_autograd must be False, 'lambdas' or 'full' (got True)")
        if mode not in PHYSICS_AUTOGRAD_MODES:
            raise ValueError("physics_autograd must be False, 'lambdas' or 'full' (got %r)" % (mode,))
        if mode == "full" and not self.dnn.autograd:
            raise ValueError("physics_autograd='full' differentiates through the DNN: set model.dnn.autograd = True first")
        self._physics_autograd = mode or False

    def _physics_mode(self):
        """The mode of this call: False when off or under torch.no_grad()."""
        mode = self._physics_autograd
        if mode == "full" and not self.dnn.autograd:
            raise ValueError("physics_autograd='full' needs model.dnn.autograd = True (it has been turned off)")
        return mode if torch.is_grad_enabled() else False

    def _physics_rows(self, X, mode):
        """The rows of a physics function: in "full" mode a tensor that requires grad keeps its graph."""
        if mode == "full" and isinstance(X, torch.Tensor) and X.requires_grad:
            return X.to(self.x.device, torch.float32).contiguous()
        return self._dev_rows(X)

    def _physics_u(self, xd, mode):
        """The DNN output the physics functions read: in the caller's train / eval mode (same dropout masks in every mode);
        differentiable in "full" mode, a constant otherwise."""
        if mode == "lambdas":
            with torch.no_grad():
                return self.net_u(xd)[0].reshape(-1).contiguous()
        return self.net_u(xd)[0].reshape(-1).contiguous()

    def _residual_tuple(self, X, x_scal, flags, mode):
        """Columns of one residual model: through _ResidualsFunction when something requires grad, else today's call."""
        names, cols = _RES_SPECS[flags]
        xd = self._physics_rows(X, mode)
        u = self._physics_u(xd, mode) if flags == _lib.RES_V else None
        self._lambdas()                             # re-gather parameters re-pointed by `lambda_k.data = ...`
        lams = [getattr(self, n) for n in names]
        if xd.requires_grad or (u is not None and u.requires_grad) or any(l.requires_grad for l in lams):
            return _ResidualsFunction.apply(self, flags, x_scal, xd, u, *lams)
        c = self._residuals(xd, x_scal, flags, u=u)
        return tuple(self._col(c, name) for name, _, _, _ in cols)

    # ------------------------------------------------------------------ helpers
    def _lambdas(self):
        base = self._lambda.data_ptr()
        for i, name in enumerate(LAMBDA_NAMES):
            par = getattr(self, name)
            if par.data_ptr() != base + 4 * i:
                self._lambda[i:i + 1].copy_(par.detach().reshape(1).to(self._lambda.device, torch.float32))
                par.data = self._lambda[i:i + 1]
        return self._lambda

    def _affine(self, x_scal):
        key = id(x_scal)
        if key not in self._aff_cache:
            a = _lib.Affine()
            mn = np.asarray(x_scal.min_, dtype=np.float64).reshape(-1)
            sc = np.asarray(x_scal.scale_, dtype=np.float64).reshape(-1)
            if mn.size != 8:
                raise ValueError("x scaler must have 8 features")
            for c in range(8):
                a.x_min[c], a.x_scale[c] = mn[c], sc[c]
            a.y_min = float(np.asarray(self.u_scal.min_, dtype=np.float64).reshape(-1)[0])
            a.y_scale = float(np.asarray(self.u_scal.scale_, dtype=np.float64).reshape(-1)[0])
            # 01:1017-1022: float32 tensors
            lo, hi = float(self.u_scal.feature_range[0]), float(self.u_scal.feature_range[1])
            dmin = torch.tensor(np.asarray(self.u_scal.data_min_), dtype=torch.float32)
            dmax = torch.tensor(np.asarray(self.u_scal.data_max_), dtype=torch.float32)
            scale_y = (hi - lo) / (dmax - dmin + 1e-12)
            min_y = lo - dmin * scale_y
            a.vn_scale, a.vn_min = float(scale_y), float(min_y)
            self._aff_cache[key] = (a, x_scal)      # keep the scaler alive so id() stays unique
        return self._aff_cache[key][0]

    def _dev_rows(self, X):
        if X is self.X or X is self.x:
            return self.x.detach()
        return X.detach().to(self.x.device, torch.float32).contiguous()

    def _residuals(self, X, x_scal, flags, u=None, y=None, cols=True, sums=False):
        xd = self._dev_rows(X)
        n = xd.shape[0]
        c = torch.empty(_lib.NCOLS, n, device=xd.device, dtype=torch.float32) if cols else None
        rc = self._lib.pinn_residuals(_ptr(xd), _ptr(u), _ptr(y), ctypes.byref(self._affine(x_scal)), _ptr(self._lambdas()),
                                      flags, n, _ptr(c), n, _ptr(self._sums) if sums else None,
                                      _ptr(self._res_work), self._res_work.numel(), _stream())
        _lib.check(rc, "pinn_residuals")
        return c

    @staticmethod
    def _col(c, name):
        return c[_lib.C[name]].unsqueeze(1)

    # ------------------------------------------------------------------ model functions
    def net_u(self, x):
        prediction, log_var = self.dnn(x, self.row_offset if x.shape[0] == self.n_local else 0)
        return prediction, log_var

    def net_f_V(self, X, x_scal):
        """01:724-765 -> (f, V_act, V_ohmic, V_conc, E_nerst, V_out_est*5, i, il, V_out*5)."""
        mode = self._physics_mode()
        if mode:
            f, va, vo, vc, e, v5, i, vout5 = self._residual_tuple(X, x_scal, _lib.RES_V, mode)
            return f, va, vo, vc, e, v5, i, self.lambda_3, vout5
        xd = self._dev_rows(X)
        u, _ = self.net_u(xd)                       # in the caller's train/eval mode, detached (01:733-734)
        c = self._residuals(xd, x_scal, _lib.RES_V, u=u.reshape(-1))
        g = lambda n: self._col(c, n)
        return g("FV"), g("VACT"), g("VOHM"), g("VCONC"), g("ENERNST"), g("VEST5"), g("I"), self.lambda_3, g("VOUT5")

    def net_f_T_simple(self, X, x_scal):
        """01:869-914 -> (f_T, T_out_predicted, T_out_real).  (The reference's unused DNN forward is not run.)"""
        mode = self._physics_mode()
        if mode:
            return self._residual_tuple(X, x_scal, _lib.RES_T, mode)
        c = self._residuals(X, x_scal, _lib.RES_T)
        return self._col(c, "FT"), self._col(c, "TPRED"), self._col(c, "TOUT")

    def net_f_H(self, X, x_scal):
        """01:621-722 -> (f_H2, actual_excess_ratio, target_excess_ratio, I_total, I_threshold)."""
        mode = self._physics_mode()
        if mode:
            return self._residual_tuple(X, x_scal, _lib.RES_H, mode) + (self.lambda_H3,)
        c = self._residuals(X, x_scal, _lib.RES_H)
        return self._col(c, "FH"), self._col(c, "ACTH"), self._col(c, "TGTH"), self._col(c, "ITOT"), self.lambda_H3

    def net_f_O(self, X, x_scal):
        """01:535-619 -> (f_O2, actual_excess_ratio, target_excess_ratio, Q_O2_theoretical_slpm, o2_flow_actual)."""
        mode = self._physics_mode()
        if mode:
            return self._residual_tuple(X, x_scal, _lib.RES_O, mode)
        c = self._residuals(X, x_scal, _lib.RES_O)
        return self._col(c, "FO"), self._col(c, "ACTO"), self._col(c, "TGTO"), self._col(c, "QO2"), self._col(c, "O2FLOW")

    def net_f_T(self, X, x_scal, halo=None):
        """01:767-867: Euler energy balance row t-1 -> t -> (f_T, T_out_predicted_full, T_out_real_full), one fused
        kernel (pinn_net_f_t).  The DNN runs in the caller's train / eval mode on the rows, as the reference runs it on
        X[:-1] (01:826-830).  `halo` = (x_row [8], u) of the row before X[0] when X is a row shard that does not start
        the series (device or host tensors; not in the reference, which has no sharding).  Under physics_autograd
        (see there) one autograd node whose backward is pinn_net_f_t_backward; in "full" mode halo tensors that require
        grad receive the gradient of that row."""
        mode = self._physics_mode()
        xd = self._physics_rows(X, mode) if mode else self._dev_rows(X)
        n = xd.shape[0]
        dev = xd.device
        if n < 2 and halo is None:
            z = torch.zeros(n, 1, device=dev)
            return z, z.clone(), z.clone()
        u = self._physics_u(xd, mode) if n > 0 else None
        xh = uh = None
        if halo is not None:
            xh = torch.as_tensor(halo[0], dtype=torch.float32).reshape(8).to(dev).contiguous()
            uh = torch.as_tensor(halo[1], dtype=torch.float32).reshape(1).to(dev).contiguous()
            if mode != "full":
                xh, uh = xh.detach(), uh.detach()
        if mode:
            self._lambdas()
            lams = [getattr(self, nm) for nm in _EULER_LAMBDAS]
            if any(t is not None and t.requires_grad for t in [xd, u, xh, uh] + lams):
                return _EulerFunction.apply(self, x_scal, xd, u, xh, uh, *lams)
        out = torch.empty(3, n, device=dev, dtype=torch.float32)
        rc = self._lib.pinn_net_f_t(_ptr(xd), _ptr(u), _ptr(xh), _ptr(uh), ctypes.byref(self._affine(x_scal)), _ptr(self._lambdas()), n,
                                    _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream())
        _lib.check(rc, "pinn_net_f_t")
        return out[0].unsqueeze(1), out[1].unsqueeze(1), out[2].unsqueeze(1)

    def aleatoric_loss(self, gt, pred_y, logvar):
        """01:916-927."""
        precision = torch.exp(-logvar)
        loss = torch.mean(0.5 * precision * (gt - pred_y) ** 2 + 0.5 * logvar)
        return loss + 0.01 * torch.mean(torch.abs(logvar))

    # ------------------------------------------------------------------ trainers
    def _log(self, *a):
        if self.verbose and _dp.rank(self._group) == 0:
            print(*a)

    def _workspace(self, n_rows):
        if self.dnn.kernels == "general":
            return self.dnn.general_workspace(n_rows)
        key = (n_rows, self.dnn.precision)          # the tile padding of the stash depends on the kernels used
        if key not in self._work:
            self._work.clear()
            wb = self._lib.pinn_train_workspace_bytes(ctypes.byref(self.dnn._net), n_rows)
            if wb == 0:
                raise _lib.PinnError("pinn_train_workspace_bytes rejected the network")
            self._work[key] = torch.empty(wb, dtype=torch.uint8, device=self.x.device)
        return self._work[key]

    def train_step_grads(self, x, y, row_offset, n_global, between=None, adam=None):
        """One fused forward + aleatoric_loss + backward on rows (x, y): fills the flat gradient
        (already divided by n_global) and returns the raw loss sums double[4] on the device.
        `between` (data-parallel overlap): called once the TAIL of the gradient -- last hidden layer and heads,
        [pinn_grad_split, end) -- is final, before the head's weight-gradient kernels are launched."""
        n = x.shape[0]
        work = self._workspace(n)
        self._step_counter += 1
        training = self.dnn.training and any(m.p > 0 for m in self.dnn.dropout_modules())
        drop = self.dnn.dropout_struct(self._step_counter, row_offset) if training else None
        if drop is not None and self.dnn._mask_bits is not None:
            self.dnn._mask_pass += 1
        loss = torch.empty(4, dtype=torch.float64, device=x.device)

        if self.dnn.kernels == "general":          # one launch sequence; `between` runs once the whole gradient is final
            g = ctypes.byref(self.dnn._gnet)
            if adam is not None:
                rc = self._lib.pinn_gnet_train_step(g, _ptr(self.dnn.flat_params()), _ptr(x), _ptr(y), n, int(n_global),
                                                    ctypes.byref(drop) if drop else None, _ptr(self.dnn._flat_grad), _ptr(loss),
                                                    _ptr(work), work.numel(), _ptr(self._adam_m), _ptr(self._adam_v), adam[0], adam[1],
                                                    _stream())
                _lib.check(rc, "pinn_gnet_train_step")
            else:
                rc = self._lib.pinn_gnet_train_grads(g, _ptr(self.dnn.flat_params()), _ptr(x), _ptr(y), n, int(n_global),
                                                     ctypes.byref(drop) if drop else None, _ptr(self.dnn._flat_grad), _ptr(loss),
                                                     _ptr(work), work.numel(), _stream())
                _lib.check(rc, "pinn_gnet_train_grads")
                if between is not None:
                    between()
            return loss

        def run(phases):
            rc = self._lib.pinn_mlp_train_grads_phases(ctypes.byref(self.dnn._net), _ptr(self.dnn.flat_params()), _ptr(x), _ptr(y), n,
                                                       int(n_global), ctypes.byref(drop) if drop else None,
                                                       _ptr(self.dnn._flat_grad), _ptr(loss), _ptr(work), work.numel(), _stream(), phases)
            _lib.check(rc, "pinn_mlp_train_grads")
        if adam is not None:      # (lr, step): the optimizer step rides in the gradient reduction's launch (single process, no collective in between)
            rc = self._lib.pinn_mlp_train_step(ctypes.byref(self.dnn._net), _ptr(self.dnn.flat_params()), _ptr(x), _ptr(y), n, int(n_global),
                                               ctypes.byref(drop) if drop else None, _ptr(self.dnn._flat_grad), _ptr(loss), _ptr(work),
                                               work.numel(), _ptr(self._adam_m), _ptr(self._adam_v), adam[0], adam[1], _stream())
            _lib.check(rc, "pinn_mlp_train_step")
        elif between is None:
            run(_lib.PHASE_ALL)
        else:
            run(_lib.PHASE_CHAIN | _lib.PHASE_WGRAD_TAIL | _lib.PHASE_REDUCE_TAIL)
            between()
            run(_lib.PHASE_WGRAD_HEAD | _lib.PHASE_REDUCE_HEAD)
        return loss

    # Data-parallel step with the gradient all-reduce in two parts: the tail of the bucket (last hidden layer +
    # heads, 0.43 of 0.70 MB for the reference net) is summed on a side stream while the head's weight-gradient kernels run;
    # both parts are complete before Adam.  Two ranks sum the same pairs of floats either way: bit-identical to one blocking
    # all-reduce (tests/test_gpu_dp.py); overlap_allreduce = False keeps the single collective.
    overlap_allreduce = True

    def _dp_step(self, xb, yb, row_offset, n_norm, has_rows):
        full = self.dnn._flat_grad_full
        # general nets: the blocking single all-reduce (split = 0)
        split = int(self._lib.pinn_grad_split(ctypes.byref(self.dnn._net))) if self.overlap_allreduce and self.dnn.kernels == "auto" else 0
        if not (_dp._active(self._group) and split > 0):
            if has_rows:
                loss = self.train_step_grads(xb, yb, row_offset, n_norm)
            else:       # a rank without rows in this batch: zero gradient, same dropout-stream position, same collective
                self._step_counter += 1
                full.zero_()
                loss = torch.zeros(4, dtype=torch.float64, device=self.x.device)
            _dp.allreduce_grads(full, self._group)
            return loss
        if getattr(self, "_side_stream", None) is None:
            self._side_stream = torch.cuda.Stream(device=self.x.device)
        works = []

        def tail_ready():
            ev = torch.cuda.Event()
            ev.record()
            with torch.cuda.stream(self._side_stream):
                self._side_stream.wait_event(ev)
                works.append(_dp.allreduce_grads_begin(full[split:], self._group))
        if has_rows:
            loss = self.train_step_grads(xb, yb, row_offset, n_norm, between=tail_ready)
        else:
            self._step_counter += 1
            full.zero_()
            loss = torch.zeros(4, dtype=torch.float64, device=self.x.device)
            tail_ready()
        works.append(_dp.allreduce_grads_begin(full[:split], self._group))
        for w in works:
            if w is not None:
                w.wait()              # the current stream waits for the collective (NCCL); gloo: the host does
        return loss

    # train_dnn at the reference's data sizes (1e3-1e4 rows, 12 002 steps: 01:2143-2147) is a chain of short dependent launches
    # (five per step).  With one process and full batches the step can be captured ONCE as a hipGraph and replayed: step count,
    # Adam coefficients and dropout stream live on the device (pinn_dropout_t.d_step_counter, pinn_mlp_train_step_dev), so nothing
    # in the captured sequence changes from step to step.  Same kernels, same arguments otherwise: bit-identical to the
    # launch-by-launch path (tests/test_gpu_model.py).  Opt-in: since the step's launches all sit on one stream, a replayed
    # step is 3-8 us SLOWER than a launched one on this runtime (92-103 against 87-95 us at 500 .. 4200 rows); what the graph
    # buys is a free host thread.
    use_graph = False

    def _train_dnn_replay(self, epochs, x, y, n_norm, log):
        """Steps 2 .. epochs of a full-batch train_dnn call as replays of one captured step (step 1 ran launch by launch:
        it also settles every lazy launch attribute before the capture)."""
        dev = x.device
        n = x.shape[0]
        flat, grad = self.dnn.flat_params(), self.dnn._flat_grad
        coeffs = np.empty((epochs, 2), dtype=np.float32)
        ss, bs = ctypes.c_float(), ctypes.c_float()
        for k in range(epochs):             # entry k: optimizer step k + 1, lr of epoch k (StepLR(1000, 0.8), 01:939-940)
            self._lib.pinn_adam_coeffs(ctypes.c_float(0.01 * 0.8 ** (k // 1000)), k + 1, ctypes.byref(ss), ctypes.byref(bs))
            coeffs[k] = (ss.value, bs.value)
        d_coeffs = torch.from_numpy(coeffs).to(dev)
        counter = torch.ones(1, dtype=torch.int32, device=dev)          # one step done
        work = self._workspace(n)
        loss = torch.empty(4, dtype=torch.float64, device=dev)
        training = self.dnn.training and any(m.p > 0 for m in self.dnn.dropout_modules())
        # step k of the call draws stream S0 + k and mask pass M0 + k - 1 (S0, M0: the positions before the call, as train_step_grads
        # counts them); the kernels add the device counter = k - 1 to what the struct holds
        drop = self.dnn.dropout_struct(self._step_counter, self.row_offset, mode=None if training else _lib.DROP_NONE)
        if training and self.dnn._mask_bits is not None:
            drop.d_bits = self.dnn._mask_bits[self.dnn._mask_pass - 1].data_ptr()
        drop.d_step_counter = counter.data_ptr()
        net = self.dnn._net

        one_call = net.precision in (_lib.PREC_F32X6, _lib.PREC_F32X6_G6)       # the reduction's launch applies the Adam step too

        def step():
            if one_call:
                _lib.check(self._lib.pinn_mlp_train_step_dev(ctypes.byref(net), _ptr(flat), _ptr(x), _ptr(y), n, int(n_norm), ctypes.byref(drop),
                                                             _ptr(grad), _ptr(loss), _ptr(work), work.numel(), _ptr(self._adam_m),
                                                             _ptr(self._adam_v), _ptr(d_coeffs), _stream()), "pinn_mlp_train_step_dev")
                return
            _lib.check(self._lib.pinn_mlp_train_grads(ctypes.byref(net), _ptr(flat), _ptr(x), _ptr(y), n, int(n_norm), ctypes.byref(drop),
                                                      _ptr(grad), _ptr(loss), _ptr(work), work.numel(), _stream()), "pinn_mlp_train_grads")
            _lib.check(self._lib.pinn_adam_step_dev(_ptr(flat), _ptr(grad), _ptr(self._adam_m), _ptr(self._adam_v), flat.numel(),
                                                    _ptr(d_coeffs), _ptr(counter), _stream()), "pinn_adam_step_dev")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        # a graph launch costs ~8 us of idle GPU between two replays (a fifteenth of a step at 1e4 rows): long calls replay
        # kChunk steps per launch wherever no log line falls inside the chunk (a line reads the loss of ITS step)
        kChunk = self.graph_chunk
        chunk = None
        if epochs - 1 >= 4 * kChunk:
            chunk = torch.cuda.CUDAGraph()
            with torch.cuda.graph(chunk):
                for _ in range(kChunk):
                    step()
        epoch = 1
        while epoch < epochs:
            next_log = (epoch + 999) // 1000 * 1000          # the first epoch >= this one that prints a line
            if chunk is not None and epoch + kChunk <= epochs and next_log >= epoch + kChunk - 1:
                chunk.replay()
                epoch += kChunk
            else:
                graph.replay()
                epoch += 1
            if (epoch - 1) % 1000 == 0:
                log(epoch - 1, loss)
        torch.cuda.current_stream().synchronize()
        self._step_counter += epochs - 1
        if training and self.dnn._mask_bits is not None:
            self.dnn._mask_pass += epochs - 1
        self._keep_alive = (d_coeffs, counter, work, loss, graph, chunk)      # until the next call: the stream may still be replaying
        return loss

    def train_dnn(self, nIter, batch_size=None):
        """01:929-964: Adam(lr=0.01) + StepLR(1000, 0.8) over the 14 weight/bias tensors,
        full batch (or `batch_size`-row minibatches: one optimizer step each)."""
        for param in self.dnn.parameters():
            param.requires_grad = True
        for n in LAMBDA_NAMES[:4]:
            getattr(self, n).requires_grad = False
        self._adam_m.zero_(); self._adam_v.zero_()
        self._log('================== DNN training ==================')
        self._log('  Epoch |    Loss    |    MSE     |    LR    ')
        self.dnn.train()
        x, y = self.x.detach(), self.u.reshape(-1)
        n = self.n_local
        flat, grad = self.dnn.flat_params(), self.dnn._flat_grad
        step = 0
        loss_sums = None
        n_norm = max(1, self.n_global)
        # the schedule has the same length on every rank (empty batches included): one gradient all-reduce per entry
        batches = _dp.batch_schedule(n, batch_size, self.x.device, self._group)

        def log_line(epoch, sums):
            self.dnn.check_range()
            ls = _dp.allreduce_sums(sums.clone(), self._group).cpu().numpy()      # fp64, only when a line is printed
            lr_next = 0.01 * 0.8 ** ((epoch + 1) // 1000)
            self._log(f' {epoch:5d}  | {(ls[0] + 0.01 * ls[1]) / n_norm:10.3e} | {ls[2] / n_norm:10.3e} | {lr_next:8.1e}')
        replay = (self.use_graph and nIter >= max(2, self.graph_min_steps) and len(batches) == 1 and batches[0][:2] == (0, n) and n > 0 and not _dp._active(self._group)
                  and self.dnn.kernels == "auto" and self.dnn.hidden <= 256)
        for epoch in range(nIter):
            lr = 0.01 * 0.8 ** (epoch // 1000)
            for (s, e, n_norm) in batches:
                xb, yb = (x, y) if (s, e) == (0, n) else (x[s:e], y[s:e])
                step += 1
                if self.fuse_adam and not _dp._active(self._group) and e > s:      # one process: gradients and Adam in one launch sequence
                    loss_sums = self.train_step_grads(xb, yb, self.row_offset + s, n_norm, adam=(lr, step))
                    continue
                loss_sums = self._dp_step(xb, yb, self.row_offset + s, n_norm, e > s)
                rc = self._lib.pinn_adam_step(_ptr(flat), _ptr(grad), _ptr(self._adam_m), _ptr(self._adam_v), flat.numel(),
                                              lr, step, _stream())
                _lib.check(rc, "pinn_adam_step")
            if epoch % 1000 == 0 and loss_sums is not None:
                log_line(epoch, loss_sums)
            if replay:
                loss_sums = self._train_dnn_replay(nIter, x, y, n_norm, log_line)
                break
        if loss_sums is not None:
            self.dnn.check_range()
            ls = _dp.allreduce_sums(loss_sums.clone(), self._group).cpu().numpy()
            self.last_loss = (ls[0] + 0.01 * ls[1]) / n_norm
            self._log(f'DNN training done, final loss: {self.last_loss:.3e}')

    def _run_lambda_stage(self, stage, nIter, flags, lr0, gamma, need_u, log_fn):
        self.dnn.eval()
        dev = self.x.device
        x, y = self.x.detach(), self.u.reshape(-1)
        aff = self._affine(self.x_scal)
        u = None
        if need_u:      # DNN weights are frozen during the stage: one eval forward serves every iteration
            u = self.dnn(x)[0].reshape(-1)
        adam = torch.zeros(2 * _lib.NLAMBDA, dtype=torch.float32, device=dev)
        loss = torch.zeros(2, dtype=torch.float32, device=dev)
        lam = self._lambdas()
        if self._group is None and self.n_global == self.n_local and 0 < self.n_local <= self.stage_run_max_rows and nIter > 0:
            # the reference's data sizes: the whole stage in ONE launch (persistent workgroup)
            n_log = (nIter + 999) // 1000
            log = torch.zeros(n_log, _lib.STAGE_LOG_FLOATS, dtype=torch.float32, device=dev)
            wb = self._lib.pinn_lambda_stage_workspace_bytes(self.n_local)
            work = torch.empty(wb, dtype=torch.uint8, device=dev)
            rc = self._lib.pinn_lambda_stage_run(stage, flags, _ptr(x), _ptr(u), _ptr(y), ctypes.byref(aff), self.n_local, lr0, gamma, 1000, 0,
                                                 nIter, _ptr(lam), _ptr(adam), _ptr(loss), _ptr(log), 1000, _ptr(self._sums), _ptr(work), wb,
                                                 _stream())
            _lib.check(rc, "pinn_lambda_stage_run")
            rows = log.cpu().numpy()
            for k in range(n_log):
                self._lambda_log_view = rows[k, 3:20]
                log_fn(1000 * k, rows[k, 0:2], rows[k, 20:20 + 32].astype("float64"), float(rows[k, 2]))
            self._lambda_log_view = None
            self.last_loss = float(loss[0].item())
            return
        # large series / row shards: the parameter-independent half of every row once, then per iteration a pass over that
        # 8-24 B/row cache -> [all-reduce of 32 sums] -> Adam + clamp on the device
        cache = None
        if nIter > 0 and self.n_local > 0:
            cache = torch.empty(6 * self.n_local, dtype=torch.float32, device=dev)
            rc = self._lib.pinn_residuals_prepare(_ptr(x), _ptr(u), _ptr(y), ctypes.byref(aff), _ptr(lam), flags, self.n_local, _ptr(cache),
                                                  _stream())
            _lib.check(rc, "pinn_residuals_prepare")
        for epoch in range(nIter):
            lr = lr0 * gamma ** (epoch // 1000)
            if cache is not None:
                rc = self._lib.pinn_residuals_cached(_ptr(cache), ctypes.byref(aff), _ptr(lam), flags, self.n_local, _ptr(self._sums),
                                                     _ptr(self._res_work), self._res_work.numel(), _stream())
            else:       # a rank without rows still takes part in the all-reduce
                rc = self._lib.pinn_residuals(_ptr(x), _ptr(u), _ptr(y), ctypes.byref(aff), _ptr(lam), flags, self.n_local,
                                              None, 0, _ptr(self._sums), _ptr(self._res_work), self._res_work.numel(), _stream())
            _lib.check(rc, "pinn_residuals")
            _dp.allreduce_sums(self._sums, self._group)
            rc = self._lib.pinn_lambda_step(stage, _ptr(self._sums), self.n_global, aff.vn_scale, lr, epoch + 1, _ptr(lam),
                                            _ptr(adam), _ptr(loss), _stream())
            _lib.check(rc, "pinn_lambda_step")
            if epoch % 1000 == 0:
                log_fn(epoch, loss.cpu().numpy(), self._sums.cpu().numpy(), lr0 * gamma ** ((epoch + 1) // 1000))
        self.last_loss = float(loss[0].item()) if nIter > 0 else None

    graph_chunk = 8                 # train_dnn steps per graph launch in long replayed calls
    fuse_adam = True                # single process: the Adam step rides in the gradient reduction's launch (False: two calls, bit-identical)
    graph_min_steps = 200           # shorter calls launch their steps one by one: a capture costs ~0.5 ms, a replayed step is no faster
    stage_run_max_rows = 32768      # <= _lib.STAGE_RUN_MAX_ROWS; larger series iterate the multi-workgroup kernels
    _lambda_log_view = None

    def _freeze_all_but(self, live):
        for n in LAMBDA_NAMES:
            getattr(self, n).requires_grad = n in live

    def train_lambda(self, nIter, dnn_para=False):
        """01:966-1058."""
        for param in self.dnn.parameters():
            param.requires_grad = dnn_para
        self._freeze_all_but(LAMBDA_NAMES[:4])
        self._log('================ voltage parameter training ================')
        self._log('  Epoch | total loss | phys loss |   l1    |    l2     |   l3   |    LR    ')

        def log(epoch, loss, sums, lr):
            l = self._lambda_log_view if self._lambda_log_view is not None else self._lambda.cpu().numpy()
            self._log(f' {epoch:5d}  | {loss[0]:9.3e} | {loss[1]:10.3e} | {l[0]:7.4f} | {l[1]:9.2e} | {l[2]:6.3f} | {lr:8.1e}')
        self._run_lambda_stage(_lib.STAGE_LAMBDA_F if dnn_para else _lib.STAGE_LAMBDA_PM, nIter, _lib.RES_V, 1e-3, 0.8, True, log)

    def train_thermal(self, nIter):
        """01:1060-1151."""
        for param in self.dnn.parameters():
            param.requires_grad = False
        self._freeze_all_but(LAMBDA_NAMES[4:9])
        self._log('---------------- thermal parameter training ----------------')
        self._log(' Epoch |   Loss    |  MAE(C)  |   T1    |   T2   |   T3   |   T4   |    T5    |    LR   |')

        def log(epoch, loss, sums, lr):
            l = self._lambda_log_view if self._lambda_log_view is not None else self._lambda.cpu().numpy()
            mae = sums[_lib.S["FT_ABS"]] / self.n_global
            self._log(f' {epoch:3d}   | {loss[0]:9.3e} | {mae:8.2f} | {l[4]:7.4f} | {l[5]:6.3f} | {l[6]:6.3f} | {l[7]:6.2f} | {l[8]:6.2f} |{lr:8.1e}')
        self._run_lambda_stage(_lib.STAGE_THERMAL, nIter, _lib.RES_T, 1.0, 0.8, False, log)

    def train_hydrogen(self, nIter):
        """01:1305-1399."""
        for param in self.dnn.parameters():
            param.requires_grad = False
        self._freeze_all_but(LAMBDA_NAMES[9:13])
        self._log('================ hydrogen parameter training ================')
        self._log(' Epoch |   Loss    |   actual   |   target   |   H1    |   H2   |   H3   |   H4   |    LR    ')

        def log(epoch, loss, sums, lr):
            l = self._lambda_log_view if self._lambda_log_view is not None else self._lambda.cpu().numpy()
            self._log(f' {epoch:3d}   | {loss[0]:9.3e} | {sums[_lib.S["ACTH"]] / self.n_global:10.3f} | '
                      f'{sums[_lib.S["TGTH"]] / self.n_global:10.3f} | {l[9]:7.4f} | {l[10]:6.3f} | {l[11]:6.3f} | {l[12]:6.2f} | {lr:8.1e}')
        self._run_lambda_stage(_lib.STAGE_HYDROGEN, nIter, _lib.RES_H, 1e-1, 0.9, False, log)

    def train_oxygen(self, nIter):
        """01:1153-1303."""
        for param in self.dnn.parameters():
            param.requires_grad = False
        self._freeze_all_but(LAMBDA_NAMES[13:17])
        self._log('================ oxygen parameter training ================')
        self._log(' Epoch |   Loss    |   actual   |   target   |   O1    |   O2   |   O3   |   O4   |    LR    ')

        def log(epoch, loss, sums, lr):
            l = self._lambda_log_view if self._lambda_log_view is not None else self._lambda.cpu().numpy()
            self._log(f' {epoch:3d}   | {loss[0]:6.3e} | {sums[_lib.S["ACTO"]] / self.n_global:6.3f} | '
                      f'{sums[_lib.S["TGTO"]] / self.n_global:6.3f} | {l[13]:7.2f} | {l[14]:6.3f} | {abs(l[15]):6.1f}A | {l[16]:5.2f} | {lr:8.1e}')
        self._run_lambda_stage(_lib.STAGE_OXYGEN, nIter, _lib.RES_O, 1e-2, 0.9, False, log)

    def predict(self, X, x_scal):
        """01:1401-1410: (u [N,1], log_var [N,1]) numpy, in the caller's train/eval mode.
        (The reference's discarded `net_f_V` call, 01:1407, is not run.)"""
        x = self._dev_rows(X)
        u, log_var = self.net_u(x)
        self.dnn.check_range()
        return u.detach().cpu().numpy(), log_var.detach().cpu().numpy()

    # ------------------------------------------------------------------ MC-dropout (used by mc.get_MC_samples)
    def mc_dropout(self, X, mc_times, row_offset=0):
        """1 eval pass + mc_times stochastic passes in one persistent launch -> three [N] device tensors."""
        x = self._dev_rows(X)
        n = x.shape[0]
        out = torch.empty(3, n, device=x.device, dtype=torch.float32)
        self._mc_calls = getattr(self, "_mc_calls", 0) + 1
        drop = self.dnn.dropout_struct(0xC0000000 + (self._mc_calls << 16), row_offset)
        if self.dnn.kernels == "general":
            work = self.dnn.general_workspace(n, int(mc_times))
            rc = self._lib.pinn_gnet_mc_dropout(ctypes.byref(self.dnn._gnet), _ptr(self.dnn.flat_params()), _ptr(x), n, ctypes.byref(drop),
                                                int(mc_times), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(work), work.numel(), _stream())
            _lib.check(rc, "pinn_gnet_mc_dropout")
            return out[0], out[1], out[2]
        rc = self._lib.pinn_mc_dropout(ctypes.byref(self.dnn._net), _ptr(self.dnn.flat_params()), _ptr(x), n, ctypes.byref(drop),
                                       int(mc_times), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream())
        _lib.check(rc, "pinn_mc_dropout")
        return out[0], out[1], out[2]
