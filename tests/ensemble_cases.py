"""Cases, the float64 referee of the combine rules and the call wrappers of the deep-ensemble tests (pinn_gens_*,
pinn_amd.ensemble).  The criterion of the batched kernels is exact: member m of a batched call equals the single-network call on
member m's slices with seed + m, bit for bit, so nothing here carries a tolerance; the one bound (the combine, one float32
spacing) stays in the test that asserts it.  Importable without a GPU: torch and the package are imported inside the wrappers."""
import ctypes

import numpy as np

# the smallest shapes at which each mechanism can go wrong:
#   [8, 4, 1]        the narrowest legal net: variance-head widths 2 and 1, every width padded to 32
#   [8, 33, 12, 1]   unequal widths that cross a 32 pad (two keep words for layer 0, one for layer 1)
#   [8, 64, 64, 1]   whole 64-wide tiles
LAYERS = [[8, 4, 1], [8, 33, 12, 1], [8, 64, 64, 1]]
# one row; one short of a 64-row tile and one past it; 200 = no multiple of 64 or of a weight-gradient slice; 4200 = the reference's
ROWS = [1, 63, 65, 200, 4200]
MEMBERS = [1, 2, 3, 5, 32]
CASES = [(layers, n, e) for layers in LAYERS for n in ROWS for e in MEMBERS]
WIDE = [8, 2048, 2048, 1]          # the multi-chunk case: its chunk capacity (from the library) is about 1.3e4 rows
SEED = 2 ** 64 - 2                 # members 0, 1, 2, ... draw seeds 2^64 - 2, 2^64 - 1, 0, ...: the 64-bit wrap is among the cases
MASK64 = 2 ** 64 - 1


def case_id(c):
    return "%s-n%d-E%d" % ("x".join(str(v) for v in c[0]), c[1], c[2])


# ---------------------------------------------------------------------------------------------------------------------------
# float64 referee of pinn_gens_combine: members in index order, every operation rounded on its own, one rounding to float32
def combine_referee(u, logvar, rule):
    """u, logvar [E, N] float32 -> (pred_mean, a_u, e_u) float64 [N] before the final rounding."""
    u = np.asarray(u, dtype=np.float32).astype(np.float64)
    lv = np.asarray(logvar, dtype=np.float32).astype(np.float64)
    e = u.shape[0]
    su, suu, sl = np.zeros(u.shape[1]), np.zeros(u.shape[1]), np.zeros(u.shape[1])
    for m in range(e):
        su = su + u[m]
        suu = suu + u[m] * u[m]
        sl = sl + (np.exp(lv[m]) if rule == 1 else lv[m])
    mean = su / e
    var = suu / e - mean * mean
    var = np.where(var > 0.0, var, 0.0)
    a_u = np.sqrt(sl / e) if rule == 1 else np.sqrt(np.exp(sl / e))
    return mean, a_u, np.sqrt(var)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and parameters (GPU tests)
def gnet(layers):
    from pinn_amd import _lib
    return ctypes.byref(_lib.GNet(layers))


def member_params(layers, n_members, seed=0, identical=False):
    """[E, P] float32 on the host: every tensor uniform in +-1 / sqrt(fan_in) like torch's default, padding zero; identical: E copies
    of member 0."""
    import torch
    from pinn_amd import layout
    offs, total = layout.general_offsets(layers)
    gen = torch.Generator().manual_seed(seed)
    fp = torch.zeros(n_members, total)
    for m in range(n_members):
        for _, shape, off in offs:
            k = int(np.prod(shape))
            bound = 1.0 / np.sqrt(shape[-1] if len(shape) > 1 else max(1, k))
            fp[m, off:off + k] = (torch.rand(k, generator=gen) * 2 - 1) * bound
    if identical:
        fp[:] = fp[0]
    return fp


def train_plan(lib, layers, n_rows):
    """(rows of a training chunk, weight-gradient slices of a chunk) of one member at n_rows rows, from the library."""
    rows, slices = ctypes.c_longlong(), ctypes.c_int()
    assert lib.pinn_gens_train_plan(gnet(layers), n_rows, ctypes.byref(rows), ctypes.byref(slices)) == 0
    return rows.value, slices.value


def member_drop(layers, m, stream, p=0.2, seed=SEED):
    """The struct of the single call that member m of a batched call with (seed, stream) must equal."""
    import gnet_helpers as G
    from pinn_amd import _lib
    return G.drop(_lib.DROP_PHILOX, layers, p=p, seed=(seed + m) & MASK64, stream=stream)


def _work(lib, layers, e, n):
    import torch
    from hip_helpers import dev
    nb = lib.pinn_gens_workspace_bytes(gnet(layers), e, n)
    assert nb > 0
    return torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev())          # poisoned: a read of an unwritten word shows as NaN


def _opt(d):
    return ctypes.byref(d) if d is not None else None


# ---------------------------------------------------------------------------------------------------------------------------
# the batched entry points; device tensors in, host tensors out (outputs poisoned before the call)
def gens_forward(lib, layers, fp, x, drop=None):
    import torch
    from hip_helpers import dev, ptr, stream
    from pinn_amd import _lib
    e, n = fp.shape[0], x.shape[0]
    u = torch.full((e, n), float("nan"), device=dev())
    lv = torch.full((e, n), float("nan"), device=dev())
    w = _work(lib, layers, e, n)
    _lib.check(lib.pinn_gens_forward(gnet(layers), e, ptr(fp), ptr(x), n, _opt(drop), ptr(u), ptr(lv), ptr(w), w.numel(), stream()),
               "pinn_gens_forward")
    torch.cuda.synchronize()
    return u.cpu(), lv.cpu()


def gens_train_grads(lib, layers, fp, x, y, drop=None):
    import torch
    from hip_helpers import dev, ptr, stream
    from pinn_amd import _lib
    e, n = fp.shape[0], x.shape[0]
    g = torch.full(tuple(fp.shape), float("nan"), device=dev())
    loss = torch.full((e, 4), float("nan"), dtype=torch.float64, device=dev())
    w = _work(lib, layers, e, n)
    _lib.check(lib.pinn_gens_train_grads(gnet(layers), e, ptr(fp), ptr(x), ptr(y), n, n, _opt(drop), ptr(g), ptr(loss), ptr(w), w.numel(),
                                         stream()), "pinn_gens_train_grads")
    torch.cuda.synchronize()
    return g.cpu(), loss.cpu()


def gens_train_steps(lib, layers, fp, x, y, drops, lr=0.01):
    """len(drops) consecutive pinn_gens_train_step calls from zero moments -> (params, m, v) [E, P] on the host; fp is not changed."""
    import torch
    from hip_helpers import dev, ptr, stream
    from pinn_amd import _lib
    e, n = fp.shape[0], x.shape[0]
    par, m, v = fp.clone(), torch.zeros_like(fp), torch.zeros_like(fp)
    g = torch.full(tuple(fp.shape), float("nan"), device=dev())
    loss = torch.zeros(e, 4, dtype=torch.float64, device=dev())
    w = _work(lib, layers, e, n)
    for k, d in enumerate(drops):
        _lib.check(lib.pinn_gens_train_step(gnet(layers), e, ptr(par), ptr(x), ptr(y), n, n, _opt(d), ptr(g), ptr(loss), ptr(w), w.numel(),
                                            ptr(m), ptr(v), lr, k + 1, stream()), "pinn_gens_train_step")
    torch.cuda.synchronize()
    return par.cpu(), m.cpu(), v.cpu()


def gnet_train_steps(lib, layers, fp_m, x, y, drops, lr=0.01):
    """The same steps of one network by pinn_gnet_train_step, on a copy of its slice."""
    import torch
    from hip_helpers import dev, ptr, stream
    from pinn_amd import _lib
    n = x.shape[0]
    par, m, v = fp_m.clone(), torch.zeros_like(fp_m), torch.zeros_like(fp_m)
    g = torch.full((fp_m.numel(),), float("nan"), device=dev())
    loss = torch.zeros(4, dtype=torch.float64, device=dev())
    nb = lib.pinn_gnet_workspace_bytes(gnet(layers), n, 0)
    w = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev())
    for k, d in enumerate(drops):
        _lib.check(lib.pinn_gnet_train_step(gnet(layers), ptr(par), ptr(x), ptr(y), n, n, _opt(d), ptr(g), ptr(loss), ptr(w), w.numel(),
                                            ptr(m), ptr(v), lr, k + 1, stream()), "pinn_gnet_train_step")
    torch.cuda.synchronize()
    return par.cpu(), m.cpu(), v.cpu()


def gens_combine(lib, u, lv, rule):
    import torch
    from hip_helpers import dev, ptr, stream
    from pinn_amd import _lib
    e, n = u.shape
    out = torch.full((3, n), float("nan"), device=dev())
    _lib.check(lib.pinn_gens_combine(ptr(u), ptr(lv), e, n, rule, ptr(out[0]), ptr(out[1]), ptr(out[2]), stream()), "pinn_gens_combine")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bytes(a, b):
    """torch.equal on the raw bytes (NaN payloads and the sign of zero included)."""
    import torch
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
