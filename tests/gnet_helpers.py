"""Helpers of the GPU tests of the general (any layers list) kernels, csrc/pinn_general.hip: flat parameters, dropout structs and masks,
inputs, the ctypes wrappers of the five entry points and the CPU oracles of the two backward passes.  Nothing here carries a tolerance:
every bound stays in the test file that asserts it."""
import ctypes

import numpy as np
import torch

import pinn_oracle as O
from hip_helpers import dev, ptr, stream

SHAPES = [[8, 32, 32, 32, 1], [8, 100, 100, 1], [8, 64, 200, 48, 1], [8, 7, 1, 4, 1], [8, 2000, 300, 1], [8, 256, 256, 256, 1]]


def flat(layers, params):
    from pinn_amd import layout
    offs, total = layout.general_offsets(layers)
    f = torch.zeros(total, dtype=torch.float32)
    for (_, shape, off), p in zip(offs, params):
        f[off:off + p.numel()] = p.detach().reshape(-1)
    return f.to(dev())


def unflat(layers, flat):
    from pinn_amd import layout
    offs, _ = layout.general_offsets(layers)
    flat = flat.cpu()
    return [flat[off:off + int(np.prod(shape))].reshape(shape) for _, shape, off in offs]


def padding(layers, flat):
    """The entries of the flat buffer that belong to no tensor."""
    from pinn_amd import layout
    offs, total = layout.general_offsets(layers)
    used = torch.zeros(total, dtype=torch.bool)
    for _, shape, off in offs:
        used[off:off + int(np.prod(shape))] = True
    return flat.cpu()[~used]


def widths(layers):
    return list(layers[1:-1]) + [layers[-2] // 2]


def drop(mode, layers, p=0.2, seed=0, stream=0, row_offset=0, bits=None):
    from pinn_amd import _lib
    d = _lib.Dropout()
    d.mode = mode
    for l in range(len(layers) - 1):
        d.p[l] = p
    d.seed, d.stream, d.row_offset = seed, stream, row_offset
    d.d_bits = bits.data_ptr() if bits is not None else None
    d.d_step_counter = None
    return d


_BIG_MASKS = {}      # (layers, seed, stream, row0, p) -> the masks of the most rows asked for so far, for calls of >= 1e7 elements


def philox_masks(layers, seed, stream, row0, n, p):
    """Keep masks of every dropout module.  The oracle draws them element by element (30 s for 50 000 rows of [8, 2000, 300, 1]), and a
    mask depends on its global row alone, so the several-chunk tests that agree on the stream share one draw, by row prefix."""
    make = lambda rows: [O.philox_keep_mask(seed, stream, row0, rows, l, w, p) for l, w in enumerate(widths(layers))]
    if n * sum(widths(layers)) < 10 ** 7:
        return make(n)
    key = (tuple(layers), seed, stream, row0, p)
    if key not in _BIG_MASKS or _BIG_MASKS[key][0].shape[0] < n:
        _BIG_MASKS[key] = make(n)
    return [m[:n] for m in _BIG_MASKS[key]]


def pack_bits(masks, passes=False):
    """list over modules of bool [N, w] (passes: a list over passes of such lists) -> int32 [T, N, words], T = 1 for one pass;
    module l starts at word sum ceil(w_j / 32)."""
    out = []
    for one in (masks if passes else [masks]):
        parts = []
        for m in one:
            m = np.asarray(m, dtype=np.uint8)
            m = np.concatenate([m, np.zeros((m.shape[0], (-m.shape[1]) % 32), np.uint8)], axis=1)
            parts.append(np.packbits(m, axis=-1, bitorder="little"))
        out.append(np.ascontiguousarray(np.concatenate(parts, axis=-1)).view(np.int32))
    return torch.from_numpy(np.stack(out, 0).copy())


def data(n, seed, with_y=False):
    """x [n, 8] of the synthetic dataset; with_y: (x, y [n])."""
    from pinn_amd import synth
    ds = synth.make_dataset(n, (), seed=seed)
    return (ds[0], ds[1].reshape(-1)) if with_y else ds[0]


def upstream(n, seed, with_v=False):
    """g_u, g_lv [n]; with_v: then v [n, 8] from the same generator."""
    gen = torch.Generator().manual_seed(seed)
    gu, glv = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    return (gu, glv, torch.randn(n, 8, generator=gen)) if with_v else (gu, glv)


def model(layers, n, seed=11, **kw):
    import pinn_amd
    from pinn_amd import synth
    ds = synth.make_dataset(n, (), seed=0)
    torch.manual_seed(0)
    m = pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=True, seed=seed, **kw)
    m.verbose = False
    return m, ds


def params(dnn):
    """The network's parameters in the oracle's order."""
    named = dict(dnn.named_parameters())
    return [named[n] for n in O.param_names(dnn.n_hidden)]


# ---------------------------------------------------------------------------------------------------------------------------
# the entry points; workspaces are poisoned (reads of unwritten words show as NaN) and so are the outputs
def _net(layers):
    from pinn_amd import _lib
    return ctypes.byref(_lib.GNet(layers))


def _work(nbytes):
    assert nbytes > 0
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev())


def _opt(d):
    return ctypes.byref(d) if d else None


def forward(lib, layers, fp, x, drop=None):
    from pinn_amd import _lib
    n = x.shape[0]
    u, lv = torch.empty(n, device=dev()), torch.empty(n, device=dev())
    w = _work(lib.pinn_gnet_workspace_bytes(_net(layers), n, 0))
    _lib.check(lib.pinn_gnet_forward(_net(layers), ptr(fp), ptr(x), n, _opt(drop), ptr(u), ptr(lv), ptr(w), w.numel(), stream()),
               "pinn_gnet_forward")
    torch.cuda.synchronize()
    return u.cpu(), lv.cpu()


def mc(lib, layers, fp, x, drop, T):
    from pinn_amd import _lib
    n = x.shape[0]
    out = torch.empty(3, n, device=dev())
    w = _work(lib.pinn_gnet_workspace_bytes(_net(layers), n, T))
    _lib.check(lib.pinn_gnet_mc_dropout(_net(layers), ptr(fp), ptr(x), n, ctypes.byref(drop), T, ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                        ptr(w), w.numel(), stream()), "pinn_gnet_mc_dropout")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def train_grads(lib, layers, fp, x, y, drop=None, n_global=None):
    from pinn_amd import _lib
    n = x.shape[0]
    w = _work(lib.pinn_gnet_workspace_bytes(_net(layers), n, 0))
    g = torch.full((fp.numel(),), float("nan"), device=dev())
    loss = torch.zeros(4, dtype=torch.float64, device=dev())
    _lib.check(lib.pinn_gnet_train_grads(_net(layers), ptr(fp), ptr(x), ptr(y), n, n_global or n, _opt(drop), ptr(g), ptr(loss), ptr(w),
                                         w.numel(), stream()), "pinn_gnet_train_grads")
    torch.cuda.synchronize()
    return g.cpu(), loss.cpu()


def backward(lib, layers, fp, x, gu, glv=None, drop=None, want_dx=True):
    """pinn_gnet_backward -> (flat grads, dx or None) on the host."""
    from pinn_amd import _lib
    n = x.shape[0]
    w = _work(lib.pinn_gnet_workspace_bytes(_net(layers), n, 0))
    g = torch.full((fp.numel(),), float("nan"), device=dev())
    dx = torch.full((n, 8), float("nan"), device=dev()) if want_dx else None
    _lib.check(lib.pinn_gnet_backward(_net(layers), ptr(fp), ptr(x), n, _opt(drop), ptr(gu), ptr(glv), ptr(g), ptr(dx), ptr(w), w.numel(),
                                      stream()), "pinn_gnet_backward")
    torch.cuda.synchronize()
    return g.cpu(), (dx.cpu() if dx is not None else None)


def backward2(lib, layers, fp, x, gu, glv, vx, drop=None, want=("grads", "gx", "ggu", "gglv")):
    """pinn_gnet_backward2 -> dict of the requested outputs on the host."""
    from pinn_amd import _lib
    n = x.shape[0]
    w = _work(lib.pinn_gnet_backward2_workspace_bytes(_net(layers), n))
    nan = lambda *s: torch.full(s, float("nan"), device=dev())
    out = {"grads": nan(fp.numel()) if "grads" in want else None, "gx": nan(n, 8) if "gx" in want else None,
           "ggu": nan(n) if "ggu" in want else None, "gglv": nan(n) if "gglv" in want else None}
    _lib.check(lib.pinn_gnet_backward2(_net(layers), ptr(fp), ptr(x), n, _opt(drop), ptr(gu), ptr(glv), ptr(vx), ptr(out["grads"]),
                                       ptr(out["gx"]), ptr(out["ggu"]), ptr(out["gglv"]), ptr(w), w.numel(), stream()),
               "pinn_gnet_backward2")
    torch.cuda.synchronize()
    return {k: (v.cpu() if v is not None else None) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# the oracles of the two backward passes (torch autograd on the CPU)
def oracle_vjp(P, x, gu, glv, p_list=None, masks=None):
    """torch.autograd.grad((u, lv), P + [x], (g_u, g_lv)) of O.mlp_forward, fp32 on the CPU."""
    P = [p.detach().clone().requires_grad_(True) for p in P]
    x = x.detach().clone().requires_grad_(True)
    u, lv = O.mlp_forward(P, x, p_list, masks)
    outs, gos = [u], [gu.reshape(-1, 1)]
    if glv is not None:
        outs.append(lv)
        gos.append(glv.reshape(-1, 1))
    g = torch.autograd.grad(outs, P + [x], gos, allow_unused=True)
    g = [torch.zeros_like(t) if gi is None else gi for gi, t in zip(g, P + [x])]
    return g[:-1], g[-1]


def oracle2(P, x, gu, glv, vx, p_list=None, masks=None):
    """float64: (dS/dparams, dS/dx, dS/dg_u, dS/dg_lv) of S = <v, d(g_u . u + g_lv . lv)/dx> by torch's double autograd."""
    P = [p.detach().double().clone().requires_grad_(True) for p in P]
    x = x.detach().double().clone().requires_grad_(True)
    gu = gu.detach().double().reshape(-1, 1).clone().requires_grad_(True)
    have_lv = glv is not None
    glv = (glv.detach().double().reshape(-1, 1).clone() if have_lv else torch.zeros_like(gu)).requires_grad_(True)
    u, lv = O.mlp_forward(P, x, p_list, masks)
    dx, = torch.autograd.grad([u, lv], x, [gu, glv], create_graph=True)
    ins = [gu, glv, x] + P
    g = torch.autograd.grad(dx, ins, vx.detach().double(), allow_unused=True)
    g = [torch.zeros_like(t) if gi is None else gi for gi, t in zip(g, ins)]
    return g[3:], g[2], g[0].reshape(-1), g[1].reshape(-1)
