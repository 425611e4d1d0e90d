"""Cases, float64 referee and error band of the general (any layers list) exact-fp32 kernels, csrc/pinn_general.hip, shared by
test_gnet_referee_host.py (CPU: proves the referee, settles the floor, shows the band's teeth) and test_gpu_general_referee.py (GPU:
holds the four entry points to it).

Referee: `run`, a manual restatement of O.mlp_forward and of its first-order backward under given keep masks, in numpy.  In float64 it
is the referee (the host test holds it to torch's double autograd of O.mlp_forward at 1e-12); the same statements in float32 with every
K dimension summed in slabs of 32 in order, and the weight gradients' rows per slice and then across slices, are the independent float32
restatement that settles the floor.  It keeps its intermediates: every gradient tensor t is g_t^T a_t over the rows (g_t the d
pre-activation of matrix t, a_t its input activation, a ones column for the bias), dx = dpre_0 W_0, u = b_p + a_k . w_p, z likewise.

Normalisation: every output element e has its own absolute sum M_e, the same last product with every addend in absolute value
(`scales`): the error an exact-fp32 k-ordered chain can make in e is a few roundings of M_e, whatever the other elements of its tensor
are.  eps_e = |got_e - ref_e| / M_e; an element with M_e = 0 has no addend and must be exactly 0.  logvar = log(softplus(z) + 1e-6): a
relative error in the variance is an absolute one in its logarithm, so M_lv = f'(z) M_z + 1 + |lv|.  The double backward keeps torch's
float64 double autograd (gnet_helpers.oracle2) as its referee: its parameter gradients are scaled element by element by the first-order
M_e of the same tensor under (|g_u|, |g_lv|), a scale and not a bound; gx, ggu and gglv by their own row's largest |reference|.

Gate, per tensor, for the largest and for the rms eps_e alike:

    eps(device) <= FACTOR * eps(torch float32 autograd on the CPU, same masks) + floor

FACTOR = 2 is the project's factor for an exact-fp32 kernel against torch-fp32's distance from float64.  The floor
covers the cases where torch's own error is exactly 0 (one row of [8, 4, 1]); it started at 4 u, u = 2^-24, and was settled on the CPU by
the float32 restatements alone (they must lie inside half the band on every case; DESIGN 4d has the figures) -- never by a device's output.
Only the forward outputs and the loss sums stayed at 4 u.  M_e sees the last product alone: the error a gradient element inherits from
the cancellation inside its d pre-activation (layers above it) is a few roundings of THAT sum, and beside a small M_e it is large, most
of all in a one-row call, where M_e is a single product.  So the largest eps over a tensor has a heavy tail in every correct float32
program, and FLOORS keeps (largest, rms) floors per class of output (`klass`): forward, dx, gradient tensors (one-row calls apart), the
double backward's gradient tensors and each of its three per-row outputs, which are scaled by the row's largest |reference|, no absolute
sum at all.

Loss sums (pinn_gnet_train_grads' loss[0..2]): the kernels compute every row's terms in float32 and add them in float64, so the sum's
error is the sum of the rows' errors with no rounding of the addition and no cancellation to count on (nothing of the form u sqrt(n)):
    |S - S64| <= FACTOR * sum_r |t32_r - t64_r| + floor * sum_r M_r
t32 torch's float32 terms, M_r the term's own scale through u and logvar: nll 0.5 prec e^2 + 0.5 lv: prec |e| M_u + |0.5 prec e^2 - 0.5|
M_lv + 0.5 prec e^2 + 0.5 |lv|; |lv|: M_lv; e^2: 2 |e| M_u + e^2.
"""
import functools
import math

import numpy as np
import torch

import pinn_oracle as O

U = 2.0 ** -24
FACTOR = 2.0
FLOOR = 4 * U            # where the floor started, and where it stayed for the forward outputs and the loss sums
# (largest, rms) floors in units of u per class of output, settled on the CPU by test_float32_restatement_inside_half_the_band: where the
# float32 restatement was inside half the band at 4 u the floor stayed; elsewhere it is twice the floor that puts the restatement at
# exactly half the band on its worst case, rounded up to two digits (NEED has the measured figures, which the host test asserts again).
NEED = {"sums": (1.4, 1.4), "fwd": (2.9, 1.2), "dx": (99.0, 3.7), "grad": (114.8, 16.3), "grad_1row": (3680.2, 541.7),
        "grad2": (2629.1, 48.6), "grad2_1row": (20311.8, 948.7), "gx": (122.5, 6.9), "ggu": (21108.8, 1858.7), "gglv": (21868.9, 1285.5)}
FLOORS = {"sums": (4, 4), "fwd": (4, 4), "dx": (200, 4), "grad": (230, 33), "grad_1row": (7400, 1100), "grad2": (5300, 98),
          "grad2_1row": (41000, 1900), "gx": (250, 14), "ggu": (43000, 3800), "gglv": (44000, 2600)}
# The five double-backward classes were first measured with one order, K slabs of 32, which on widths up to 32 is torch's own product
# (needs of exactly 0 on [8, 4, 1] and [8, 31, 1]); (513.6, 9.1), (2962.7, 318.4), (34.8, 4.2), (8634.1, 543.2), (7427.9, 585.5) then.  The
# restatements of ORDERS2, none of them torch's run, leave half of those bands on the CPU, in the tensors a device left them too.
SEED, STREAM, ROW0 = (1 << 32) + 20251021, 9, 7777       # Philox: seed >= 2^32, stream != 0, row_offset != 0
P_PHILOX, P_BITS = 0.2, 0.3

EDGE_SHAPES = [
    [8, 4, 1],                                    # smallest legal net: hv1 = 2, hv2 = 1, k = 1
    [8, 31, 1],                                   # every width below one 32-pad
    [8, 33, 65, 1],                               # one over the pad, one over the 64 tile; hv1 = 32, hv2 = 16
    [8, 63, 64, 64, 1],                           # in = 63: the bias column is the last of its tile; in = 64 twice: it has a tile of its own
    [8, 65, 5, 1],                                # odd last width: hv1 = 2, hv2 = 1
    [8, 129, 127, 1],                             # in + 1 = 130 (three column tiles), in + 1 = 128 (exactly two); hv1 = 63, hv2 = 31
    [8, 16, 8, 40, 24, 72, 12, 36, 20, 1],        # k = 8 = kMaxHidden; word_off over nine dropout modules
    [8, 2048, 2048, 1],                           # kMaxWidth, 64 K slabs, 32 x 32 tiles; 65 rows only
]
ROWS = (1, 63, 64, 65, 127, 128, 129, 257, 289, 321)
ROWS2 = (1, 63, 65, 129, 289)                     # the double backward
MODES = ("eval", "philox", "bits")
# (chunk rows, weight-gradient slices, rows per slice) by train_layout / slice_plan: rows round up to 64; at most rows // 128 slices of
# rup(ceil(rows / slices), 32) rows.  257 and 289 -> 320 rows -> 2 slices of 160 (97 and 129 valid rows in the second); 321 -> 384 rows ->
# 3 slices of 128, the last with 65 valid rows.  The double backward's layout (ns = 2) has the same figures at these sizes.
SLICES = {1: (64, 1, 64), 63: (64, 1, 64), 64: (64, 1, 64), 65: (128, 1, 128), 127: (128, 1, 128), 128: (128, 1, 128),
          129: (192, 1, 192), 257: (320, 2, 160), 289: (320, 2, 160), 321: (384, 3, 128)}


def rows_of(layers):
    return (65,) if layers[1] == 2048 else ROWS


def rows2_of(layers):
    return (65,) if layers[1] == 2048 else ROWS2


def widths(layers):
    return list(layers[1:-1]) + [layers[-2] // 2]


# ---------------------------------------------------------------------------------------------------------------------------
# the workspace layout restated (csrc/pinn_general.hip: make_shape, slice_plan, train_layout, infer_layout)
def _rup(v, m):
    return (v + m - 1) // m * m


def _geometry(layers):
    w = list(layers[1:-1])
    k, hk = len(w), w[-1]
    outs = w + [1, hk // 2, hk // 4, 1]
    ins = [8] + w[:-1] + [hk, hk, hk // 2, hk // 4]
    gemm = [t < k or t in (k + 1, k + 2) for t in range(k + 4)]
    return k, outs, ins, gemm


def slice_plan(layers, rows):
    """(slice_rows, slices) of a chunk of `rows` rows."""
    k, outs, ins, gemm = _geometry(layers)
    tiles = max([1] + [_rup(o, 64) // 64 * (_rup(i + 1, 64) // 64) for o, i, g in zip(outs, ins, gemm) if g])
    gtotal = sum(_rup(o * (i + 1), 4) for o, i in zip(outs, ins))
    sl = min((2048 + tiles - 1) // tiles, max(rows // 128, 1), max((256 << 20) // (4 * gtotal), 1))
    slice_rows = _rup((rows + sl - 1) // sl, 32)
    return slice_rows, (rows + slice_rows - 1) // slice_rows


def train_layout(layers, n, ns=1):
    """(chunk rows, slices, slice_rows, workspace bytes) of pinn_gnet_train_grads / pinn_gnet_backward (ns = 1) and pinn_gnet_backward2
    (ns = 2) on n rows."""
    k, outs, ins, gemm = _geometry(layers)
    mp = [_rup(o, 32) for o in outs]
    kp = [_rup(i, 32) for i in ins]
    max_wp = max(m for m, g in zip(mp, gemm) if g)
    words = sum((w + 31) // 32 for w in widths(layers))
    gtotal = sum(_rup(o * (i + 1), 4) for o, i in zip(outs, ins))
    pack = sum(mp[t] * kp[t] * (1 if t == 0 else 2) for t in range(k + 4) if gemm[t])
    per_row = words + 2 * ns * max_wp + ns + 1 + ns * sum(m for m, g in zip(mp, gemm) if g)
    cap = min(max((512 << 20) // (4 * per_row) // 64 * 64, 64), 131072)
    rows = min(_rup(max(n, 1), 64), cap)
    slice_rows, slices = slice_plan(layers, rows)
    at = 0

    def take(nbytes):
        nonlocal at
        at = _rup(at + nbytes, 256)

    take(4 * pack)
    for t in range(k + 4):
        if gemm[t]:
            for _ in range(ns):
                take(4 * rows * mp[t])
    take(4 * rows * words)
    for _ in range(2 * ns):
        take(4 * rows * max_wp)
    for _ in range(2 if ns == 1 else 3):
        take(4 * rows)
    take(4 * slices * gtotal)
    take(4 * gtotal)
    if ns == 1:
        take(64 * ((n + rows - 1) // rows) * (rows // 16))
    return rows, slices, slice_rows, at


def infer_layout(layers, n):
    """Workspace bytes of pinn_gnet_forward on n rows."""
    k, outs, ins, gemm = _geometry(layers)
    mp = [_rup(o, 32) for o in outs]
    kp = [_rup(i, 32) for i in ins]
    max_wp = max(m for m, g in zip(mp, gemm) if g)
    pack = sum(mp[t] * kp[t] * (1 if t == 0 else 2) for t in range(k + 4) if gemm[t])
    cap = min(max((256 << 20) // (4 * (3 * max_wp + 2)) // 64 * 64, 64), 1 << 20)
    rows = min(_rup(max(n, 1), 64), cap)
    return sum(_rup(b, 256) for b in [4 * pack] + [4 * rows * max_wp] * 3 + [4 * rows] * 2)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
def _mm(a, b, slab, start=None):
    """a [N, K] @ b [K, M] (+ start); slab: the K dimension in slabs of that size, in order, on the accumulator (float32 restatement)."""
    if slab is None:
        r = a @ b
        return r if start is None else start + r
    acc = np.zeros((a.shape[0], b.shape[1]), a.dtype) if start is None else start.astype(a.dtype, copy=True)
    bt = np.ascontiguousarray(b.T)
    for s in range(0, a.shape[1], slab):
        acc = acc + _slab(a[:, s:s + slab], bt[:, s:s + slab])
    return acc


def kernel_tanh(x):
    """tanh_f32 of csrc/pinn_mlp_core.h in float32, 1 - 2 / (2^(2 x log2 e) + 1), which the general kernels' layer epilogue used for every
    argument until these tests: its error is absolute (about 1.5e-7), so an activation of size 0.01 carries a relative error
    near 1e-5, which a float32 tanh does not have.  Only test_absolute_error_tanh_leaves_half_the_band runs it."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore"):
        e = np.exp2(x * np.float32(2.8853900817779268))
    return np.float32(1.0) - np.float32(2.0) * (np.float32(1.0) / (e + np.float32(1.0)))


def _slab(a, bt):
    """a [N, s] . bt [M, s]^T -> [N, M] in a's dtype: every product rounded, then numpy's own sum over the s addends.  No BLAS call,
    so the float32 restatement does not depend on the host's GEMM kernels or thread count."""
    out = np.empty((a.shape[0], bt.shape[0]), a.dtype)
    step = max(1, (1 << 22) // max(1, bt.shape[0] * a.shape[1]))
    for i in range(0, a.shape[0], step):
        out[i:i + step] = (a[i:i + step, None, :] * bt[None, :, :]).sum(axis=2, dtype=a.dtype)
    return out


def _tn(g, a, slab, slice_rows):
    """g^T a over the rows; slab: rows in slabs of that size in order within a slice of slice_rows rows, then the slices in order."""
    if slab is None:
        return g.T @ a
    total, gt, at = None, np.ascontiguousarray(g.T), np.ascontiguousarray(a.T)
    for s0 in range(0, g.shape[0], slice_rows):
        acc = np.zeros((g.shape[1], a.shape[1]), g.dtype)
        for r in range(s0, min(s0 + slice_rows, g.shape[0]), slab):
            acc = acc + _slab(gt[:, r:r + slab], at[:, r:r + slab])
        total = acc if total is None else total + acc
    return total


def _softplus(z):
    with np.errstate(over="ignore"):
        return np.where(z > 20.0, z, np.log1p(np.exp(np.minimum(z, 20.0).astype(z.dtype))))


def _sigmoid(z):
    with np.errstate(over="ignore"):
        return np.where(z > 20.0, np.ones_like(z), 1.0 / (1.0 + np.exp(-z)))


def run(P, x, ps=None, masks=None, gu=None, glv=None, y=None, dtype=np.float64, slab=None, slice_rows=None, drop_rows=(),
        zero_act=None, bias_col=None, tanh=np.tanh):
    """O.mlp_forward and its first-order backward, statement by statement.  P: tensors in O.param_names order; x [N, 8]; masks / ps as
    O.mlp_forward (None: eval).  Upstream: y given: aleatoric_loss on (x, y), gradients of its mean over the N rows and the three loss
    sums; else g_u and g_lv (None: zero) per row; neither: forward only.  dtype float64, slab None: the referee.  dtype float32, slab 32,
    slice_rows: the float32 restatement.  Mutants of the referee (the host test's teeth): drop_rows: rows left out of every weight
    gradient; zero_act = (l, column): that column of hidden layer l's activation zeroed; bias_col = t: matrix t's bias gradient taken
    from column n_in - 1 of the weight-gradient product instead of n_in.

    Returns a dict: a (input activation of every matrix, in O.param_names' matrix order: k hidden, predict, var 0, 3, 5), u, z, lv [N],
    and with an upstream du, dz [N], dpre (d pre-activation per matrix, [N, out]), grads (O.param_names order), dx [N, 8], sums."""
    cast = lambda t: np.asarray(t.detach().numpy() if isinstance(t, torch.Tensor) else t).astype(dtype)
    P = [cast(p) for p in P]
    x = cast(x)
    N, k = x.shape[0], (len(P) - 8) // 2
    W = [P[2 * t] for t in range(k + 4)]
    b = [P[2 * t + 1] for t in range(k + 4)]
    c = [None] * (k + 1)                       # keep * scale per dropout module (None: identity)
    if masks is not None:
        c = [np.asarray(m).astype(dtype) * dtype(float(O.dropout_scale(ps[l]))) for l, m in enumerate(masks)]
    lin = lambda h, t: _mm(h, np.ascontiguousarray(W[t].T), slab, np.broadcast_to(b[t], (N, W[t].shape[0])))

    def module(pre, l):                        # tanh + dropout -> (tanh, output)
        h = tanh(pre)
        return h, (h if c[l] is None else h * c[l])

    a, th = [None] * (k + 4), [None] * (k + 3)             # inputs of every matrix; tanh outputs of the GEMM matrices
    a[0] = x
    for l in range(k):
        th[l], out = module(lin(a[l], l), l)
        if zero_act is not None and zero_act[0] == l:
            out = out.copy()
            out[:, zero_act[1]] = 0
        a[l + 1 if l + 1 < k else k] = out
    hk = a[k]
    a[k + 1] = hk
    u = lin(hk, k)[:, 0]
    th[k + 1], a[k + 2] = module(lin(hk, k + 1), k)
    th[k + 2] = tanh(lin(a[k + 2], k + 2))
    a[k + 3] = th[k + 2]
    z = lin(a[k + 3], k + 3)[:, 0]
    var = _softplus(z) + dtype(1e-6)
    lv = np.log(var)
    R = dict(a=a, u=u, z=z, lv=lv, W=W, b=b)
    if y is None and gu is None:
        return R
    f1 = _sigmoid(z) / var
    if y is not None:
        y = cast(y).reshape(-1)
        prec, e, inv_n = np.exp(-lv), y - u, dtype(1.0 / N)
        du = -(prec * e) * inv_n
        dz = (dtype(-0.5) * prec * e * e + dtype(0.5) + dtype(0.01) * np.sign(lv)) * inv_n * f1
        terms = np.stack([0.5 * prec * e * e + 0.5 * lv, np.abs(lv), e * e])
        R.update(terms=terms, sums=terms.astype(np.float64).sum(axis=1))
    else:
        du = cast(gu).reshape(-1)
        dz = np.zeros_like(du) if glv is None else cast(glv).reshape(-1) * f1
    dpre = [None] * (k + 4)
    dpre[k], dpre[k + 3] = du[:, None], dz[:, None]
    dpre[k + 2] = dz[:, None] * W[k + 3] * (1 - th[k + 2] ** 2)

    def dmodule(d, t, l):                      # through dropout module l and the tanh of matrix t
        d = d * (1 - th[t] ** 2)
        return d if c[l] is None else d * c[l]

    dpre[k + 1] = dmodule(_mm(dpre[k + 2], W[k + 2], slab), k + 1, k)
    da = _mm(dpre[k + 1], W[k + 1], slab, du[:, None] * W[k])
    for l in range(k - 1, -1, -1):
        dpre[l] = dmodule(da, l, l)
        da = _mm(dpre[l], W[l], slab)
    grads = []
    ones = np.ones((N, 1), dtype)
    for t in range(k + 4):
        g = dpre[t]
        if len(drop_rows):
            g = g.copy()
            g[list(drop_rows)] = 0
        full = _tn(g, np.concatenate([a[t], ones], axis=1), slab, slice_rows)
        n_in = a[t].shape[1]
        grads += [full[:, :n_in], full[:, n_in - 1 if bias_col == t else n_in]]
    R.update(du=du, dz=dz, dpre=dpre, grads=grads, dx=da)
    return R


def scales(R, gu=None, glv=None):
    """The absolute sums M_e of a referee run R: dict u, lv [N]; with a backward also grads (O.param_names order) and dx [N, 8]."""
    k = len(R["a"]) - 4
    a, W, b = R["a"], R["W"], R["b"]
    Mu = np.abs(b[k][0]) + np.abs(a[k]) @ np.abs(W[k][0])
    Mz = np.abs(b[k + 3][0]) + np.abs(a[k + 3]) @ np.abs(W[k + 3][0])
    z = R["z"]
    Mlv = _sigmoid(z) / (_softplus(z) + 1e-6) * Mz + 1.0 + np.abs(R["lv"])
    M = dict(u=Mu, lv=Mlv)
    if "dpre" in R:
        M["grads"] = []
        for t in range(k + 4):
            g = np.abs(R["dpre"][t])
            M["grads"] += [g.T @ np.abs(a[t]), g.sum(axis=0)]
        M["dx"] = np.abs(R["dpre"][0]) @ np.abs(W[0])
    if "terms" in R:
        prec, e2 = np.exp(-R["lv"]), R["terms"][2]
        e = np.sqrt(e2)
        M["terms"] = np.stack([prec * e * Mu + np.abs(0.5 * prec * e2 - 0.5) * Mlv + 0.5 * prec * e2 + 0.5 * np.abs(R["lv"]),
                               Mlv, 2 * e * Mu + e2])
    return M


def eps(got, ref, M):
    """(largest, rms) of |got - ref| / M over the elements with M > 0; inf if an element with M = 0 is not exactly 0 or anything is not
    finite."""
    got, ref, M = (np.asarray(t, dtype=np.float64) for t in (got, ref, M))
    got, ref, M = got.reshape(-1), ref.reshape(-1), M.reshape(-1)
    assert got.shape == ref.shape == M.shape, (got.shape, ref.shape, M.shape)
    if not np.all(np.isfinite(got)):
        return math.inf, math.inf
    nz = M > 0
    if np.any(got[~nz] != 0) or np.any(ref[~nz] != 0):
        return math.inf, math.inf
    if not nz.any():
        return 0.0, 0.0
    e = np.abs(got[nz] - ref[nz]) / M[nz]
    return float(e.max()), float(np.sqrt((e ** 2).mean()))


def row_scale(ref):
    """[N, c] (or [N]) -> every element's own row's largest |ref| (the double backward's gx, ggu, gglv)."""
    r = np.abs(np.asarray(ref, dtype=np.float64))
    return r if r.ndim == 1 else np.broadcast_to(r.max(axis=1, keepdims=True), r.shape)


def klass(name, n, second=False):
    """The class of output whose floors `name` takes (FLOORS): the forward outputs, dx, a gradient tensor (one-row calls apart: there M_e
    is a single product and the cancellation inside a d pre-activation shows undamped), and for the double backward its gradient tensors
    and each of its three per-row outputs."""
    if name in ("u", "lv"):
        return "fwd"
    if name in ("dx", "gx", "ggu", "gglv"):
        return name
    return ("grad2" if second else "grad") + ("_1row" if n == 1 else "")


def ratio(e_got, e_torch, cls):
    """The larger of the two (largest, rms) ratios of a tensor's eps to its band."""
    return max(g / (FACTOR * t + f * U) for g, t, f in zip(e_got, e_torch, FLOORS[cls]))


def need(e_got, e_torch):
    """(largest, rms) floors in u with which e_got is at exactly half the band."""
    return tuple((2 * g - FACTOR * t) / U for g, t in zip(e_got, e_torch))


def sum_ratio(got, t64, t32, Mt):
    """Loss sums [3] against the float64 terms [3, N]: the largest |S - S64| / (FACTOR sum |t32 - t64| + FLOOR sum M)."""
    got, t64, t32, Mt = (np.asarray(t, dtype=np.float64) for t in (got, t64, t32, Mt))
    floor = FLOORS["sums"][0] * U
    return float((np.abs(got - t64.sum(axis=1)) / (FACTOR * np.abs(t32 - t64).sum(axis=1) + floor * Mt.sum(axis=1))).max())


def sum_need(got, t64, t32, Mt):
    """The floor in u with which the loss sums `got` are at exactly half their band."""
    got, t64, t32, Mt = (np.asarray(t, dtype=np.float64) for t in (got, t64, t32, Mt))
    return float(((2 * np.abs(got - t64.sum(axis=1)) - FACTOR * np.abs(t32 - t64).sum(axis=1)) / Mt.sum(axis=1)).max() / U)


def old_rule(got, ref):
    """The gate the suite had: max |err| / (2e-4 max |ref| + 1e-6 max |ref|); <= 1 passes."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max()) + 1e-30
    return float(np.abs(got - ref).max()) / (2e-4 * scale + 1e-6 * scale)


# ---------------------------------------------------------------------------------------------------------------------------
# torch float32 on the CPU: what sizes the band
def torch_forward(P, x, ps=None, masks=None, lin=None):
    """O.mlp_forward's statements with the product given (lin(h, W, b)): a float32 run in another summation order that torch can
    differentiate twice.  lin None: O.mlp_forward itself."""
    if lin is None:
        return O.mlp_forward(P, x, ps, masks)
    k = (len(P) - 8) // 2
    h = x
    for l in range(k):
        h = torch.tanh(lin(h, P[2 * l], P[2 * l + 1]))
        if masks is not None:
            h = h * (torch.as_tensor(np.asarray(masks[l]), dtype=torch.float32).to(h.dtype) * float(O.dropout_scale(ps[l])))
    u = lin(h, P[2 * k], P[2 * k + 1])
    v = torch.tanh(lin(h, P[2 * k + 2], P[2 * k + 3]))
    if masks is not None:
        v = v * (torch.as_tensor(np.asarray(masks[k]), dtype=torch.float32).to(v.dtype) * float(O.dropout_scale(ps[k])))
    v = torch.tanh(lin(v, P[2 * k + 4], P[2 * k + 5]))
    z = lin(v, P[2 * k + 6], P[2 * k + 7])
    return u, torch.log(torch.nn.functional.softplus(z) + 1e-6)


ORDERS2 = (8, 16, 32, 64, 128)      # K slabs of the double backward's float32 restatements (the orders of tests/bf16_policy.py)


def slab_linear(h, W, b, slab=32):
    """h W^T + b with K in slabs of `slab`, in order.  A contraction no longer than one slab would be torch's own product again (the
    widths up to 32 of [8, 4, 1] and [8, 31, 1], layer 0 of every list): there every product is rounded and the addends are summed by
    torch's reduction instead, so that no list's restatement is torch's float32 run itself."""
    if W.shape[1] <= slab:
        return b + (h[:, None, :] * W[None, :, :]).sum(dim=2)
    acc = b.expand(h.shape[0], W.shape[0])
    for s in range(0, W.shape[1], slab):
        acc = acc + h[:, s:s + slab] @ W[:, s:s + slab].t()
    return acc


def double32(P, x, gu, glv, vx, ps=None, masks=None, lin=None):
    """gnet_helpers.oracle2 in float32: (dS/dparams, dS/dx, dS/dg_u, dS/dg_lv) as numpy arrays."""
    P = [p.detach().clone().requires_grad_(True) for p in P]
    x = x.detach().clone().requires_grad_(True)
    gu = gu.detach().reshape(-1, 1).clone().requires_grad_(True)
    glv = (glv.detach().reshape(-1, 1).clone() if glv is not None else torch.zeros_like(gu)).requires_grad_(True)
    u, lv = torch_forward(P, x, ps, masks, lin)
    dx, = torch.autograd.grad([u, lv], x, [gu, glv], create_graph=True)
    ins = [gu, glv, x] + P
    g = torch.autograd.grad(dx, ins, vx.detach(), allow_unused=True)
    g = [(torch.zeros_like(t) if gi is None else gi).detach().numpy() for gi, t in zip(g, ins)]
    return g[3:], g[2], g[0].reshape(-1), g[1].reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    """One (layers, rows, mode): inputs, and lazily the float64 referee runs, their scales and torch-float32's eps per output."""

    def __init__(self, layers, n, mode):
        from gnet_helpers import data, upstream
        self.layers, self.n, self.mode, self.k = list(layers), n, mode, len(layers) - 2
        self.names = O.param_names(self.k)
        self.P = O.init_params(layers, seed=sum(layers) + n)
        self.x, self.y = data(n, seed=n + 1, with_y=True)
        self.gu, self.glv, self.vx = upstream(n, n + 2, with_v=True)
        self.p = {"eval": None, "philox": P_PHILOX, "bits": P_BITS}[mode]
        self.ps = None if self.p is None else [self.p] * (self.k + 1)
        self.masks = None
        if mode == "philox":
            self.masks = [O.philox_keep_mask(SEED, STREAM, ROW0, n, l, w, self.p) for l, w in enumerate(widths(layers))]
        elif mode == "bits":
            gen = torch.Generator().manual_seed(n + 3)
            self.masks = [(torch.rand(n, w, generator=gen) >= self.p).numpy() for w in widths(layers)]
        self.rows, self.slices, self.slice_rows, _ = train_layout(layers, n)

    def drop(self, bits=None):
        """The pinn_dropout_t of the mode (bits: the packed masks on the device)."""
        from gnet_helpers import drop
        if self.mode == "eval":
            return None
        if self.mode == "philox":
            return drop(1, self.layers, self.p, SEED, STREAM, ROW0)
        return drop(2, self.layers, self.p, bits=bits)

    def upstream(self, kind):
        """kwargs of `run` for "train", "vjp" (g_u and g_lv) and "vjp_u" (g_lv = NULL)."""
        return dict(train=dict(y=self.y), vjp=dict(gu=self.gu, glv=self.glv), vjp_u=dict(gu=self.gu))[kind]

    @functools.lru_cache(maxsize=None)
    def ref(self, kind):
        """(referee run, its scales)."""
        R = run(self.P, self.x, self.ps, self.masks, **self.upstream(kind))
        return R, scales(R)

    @functools.lru_cache(maxsize=None)
    def restated(self, kind, tanh=np.tanh):
        """The float32 restatement: K slabs of 32, this case's weight-gradient slices."""
        return run(self.P, self.x, self.ps, self.masks, dtype=np.float32, slab=32, slice_rows=self.slice_rows, tanh=tanh,
                   **self.upstream(kind))

    @functools.lru_cache(maxsize=None)
    def torch32(self, kind):
        """torch float32 autograd of O.mlp_forward, same masks: dict like a run's (u, lv, grads, dx, terms)."""
        if kind == "train":
            _, _, g, u, lv = O.nll_loss_and_grads(self.P, self.x, self.y.reshape(-1, 1), self.ps, self.masks)
            u, lv = u.reshape(-1), lv.reshape(-1)
            e = self.y.reshape(-1) - u
            terms = torch.stack([0.5 * torch.exp(-lv) * e * e + 0.5 * lv, lv.abs(), e * e])
            return dict(u=u.numpy(), lv=lv.numpy(), grads=[t.numpy() for t in g], terms=terms.numpy())
        from gnet_helpers import oracle_vjp
        with torch.no_grad():
            u, lv = O.mlp_forward(self.P, self.x, self.ps, self.masks)
        g, dx = oracle_vjp(self.P, self.x, self.gu, self.glv if kind == "vjp" else None, self.ps, self.masks)
        return dict(u=u.reshape(-1).numpy(), lv=lv.reshape(-1).numpy(), grads=[t.numpy() for t in g], dx=dx.numpy())

    def outputs(self, kind):
        """Names of the outputs of `kind`, forward ones first."""
        return ["u", "lv"] + self.names + ([] if kind == "train" else ["dx"])

    def pick(self, res, name):
        return res["grads"][self.names.index(name)] if name in self.names else res[name]

    def eps_of(self, res, kind, name):
        """(largest, rms) eps of output `name` of a result dict against the referee."""
        R, M = self.ref(kind)
        return eps(self.pick(res, name), self.pick(R, name), self.pick(M, name))

    @functools.lru_cache(maxsize=None)
    def eps_torch(self, kind, name):
        return self.eps_of(self.torch32(kind), kind, name)

    def ratio(self, res, kind, name):
        return ratio(self.eps_of(res, kind, name), self.eps_torch(kind, name), klass(name, self.n))

    def sums_ratio(self, sums, fn=None):
        R, M = self.ref("train")
        return (fn or sum_ratio)(sums, R["terms"], self.torch32("train")["terms"], M["terms"])

    # the double backward: referee gnet_helpers.oracle2 (float64), scales from the first-order run under (|g_u|, |g_lv|)
    @functools.lru_cache(maxsize=None)
    def ref2(self, with_glv=True):
        from gnet_helpers import oracle2
        glv = self.glv if with_glv else None
        wp, wx, wgu, wglv = oracle2(self.P, self.x, self.gu, glv, self.vx, self.ps, self.masks)
        ref = dict(grads=[t.numpy() for t in wp], gx=wx.numpy(), ggu=wgu.numpy(), gglv=wglv.numpy())
        Ma = scales(run(self.P, self.x, self.ps, self.masks, gu=self.gu.abs(), glv=glv.abs() if with_glv else None))
        M = dict(grads=Ma["grads"], gx=row_scale(ref["gx"]), ggu=row_scale(ref["ggu"]), gglv=row_scale(ref["gglv"]))
        return ref, M

    @functools.lru_cache(maxsize=None)
    def torch2(self, with_glv=True, slab=False):
        """torch float32 double autograd (slab: with every product in K slabs of that size: another float32 order)."""
        wp, wx, wgu, wglv = double32(self.P, self.x, self.gu, self.glv if with_glv else None, self.vx, self.ps, self.masks,
                                     functools.partial(slab_linear, slab=int(slab)) if slab else None)
        return dict(grads=wp, gx=wx, ggu=wgu, gglv=wglv)

    def eps2_of(self, res, name, with_glv=True):
        ref, M = self.ref2(with_glv)
        return eps(self.pick(res, name), self.pick(ref, name), self.pick(M, name))

    def ratio2(self, res, name, with_glv=True):
        return ratio(self.eps2_of(res, name, with_glv), self.eps2_of(self.torch2(with_glv), name, with_glv), klass(name, self.n, True))


def mutants(c):
    """Wrong answers a band must reject: (kind, name, a `run`-like result of pinn_gnet_backward's outputs, the outputs the mutant touches)
    for every mutant that case c admits.  Each is the float64 referee with one mistake a tile, seam or layout error would make."""
    kw = dict(gu=c.gu, glv=c.glv)
    n, k, L, names = c.n, c.k, c.layers, c.names
    base = lambda **m: run(c.P, c.x, c.ps, c.masks, **kw, **m)
    yield "last_row", "last_row", base(drop_rows=(n - 1,)), names                      # the last valid row left out of the weight gradients
    if c.slices > 1:
        yield "slice_row", "slice_row", base(drop_rows=(c.slice_rows - 1,)), names      # the last row of the first slice
    for l in range(k):                                                     # the last feature of an odd width zeroed in one activation
        if L[l + 1] in (33, 65):
            nxt = [names[2 * (l + 1)]] if l + 1 < k else ["predict.weight", "var_layers.0.weight"]
            yield "zero_act", "zero_act_%d" % l, base(zero_act=(l, L[l + 1] - 1)), ["u"] + nxt
    for t in range(k + 4):                                                 # the bias gradient from column n_in - 1
        yield "bias_col", "bias_col_%d" % t, base(bias_col=t), [names[2 * t + 1]]
    if c.masks is not None:                                                # one keep bit at a word seam flipped in one row
        for l, w in enumerate(widths(L)):
            for f in (31, 32):
                if w > f:
                    m = [np.array(q, dtype=bool) for q in c.masks]
                    m[l][n // 2, f] ^= True
                    t = l if l < k else k + 1
                    yield "flip", "flip_%d_%d" % (l, f), run(c.P, c.x, c.ps, m, **kw), names[2 * t:2 * t + 2]
    if L[-2] % 2:                                                          # the variance head with ceil(h_k / 2) units: the last one twice
        P, j = list(c.P), 2 * (k + 1)
        P[j], P[j + 1] = torch.cat([P[j], P[j][-1:]]), torch.cat([P[j + 1], P[j + 1][-1:]])
        P[j + 2] = torch.cat([P[j + 2], P[j + 2][:, -1:]], dim=1)
        m = None if c.masks is None else list(c.masks[:k]) + [np.concatenate([c.masks[k], np.ones((n, 1), bool)], axis=1)]      # kept
        yield "ceil_head", "ceil_head", run(P, c.x, c.ps, m, **kw), ["lv", names[2 * (k - 1)]]
    if n >= 2:                                                             # dx of one row replaced by its neighbour's
        R = dict(c.ref("vjp")[0])
        dx, r = R["dx"].copy(), n // 2
        dx[r] = dx[r + 1 if r + 1 < n else r - 1]
        R["dx"] = dx
        yield "dx_row", "dx_row", R, ["dx"]


@functools.lru_cache(maxsize=None)
def case(layers, n, mode):
    return Case(layers, n, mode)


def cases(layers, rows=None):
    for n in rows or rows_of(layers):
        for mode in MODES:
            yield case(tuple(layers), n, mode)
