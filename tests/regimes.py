"""Weight regimes away from initialisation, shared by test_regimes_host.py (CPU) and test_gpu_regimes.py (GPU).

Every other parity test draws its weights from O.init_params: hidden pre-activations are O(1), no unit is saturated and the variance
head's pre-activation z sits in about [-0.6, 0.3], so logvar = log(softplus(z) + 1e-6) is negative on every row.  `regime_params` moves a
net of init_params to where the other branches of the kernels' heads and the flat end of tanh are reached:

    regime      gain  gz   z_med     what it reaches
    init        1     1    -         control
    saturated   6     1    -         about 19 % of the first layer's units with |a| > 0.99
    sign        1     8    0.5413    logvar crosses 0 (softplus(0.5413) = 1)
    floor       1     40   -14       var at the 1e-6 floor, precision up to 1e6
    linear      1     40   20        both sides of the z > 20 branch of softplus and its derivative
    sat_sign    4     8    0.5413    both at once

gain multiplies every hidden matrix, var_layers.0.weight and var_layers.3.weight (no bias); gz multiplies var_layers.5.weight; then
var_layers.5.bias is moved so that the median over the rows of z, from the float64 oracle on the case's own masks, is z_med: half the
rows on each side of the branch, whatever the net's width.  The bf16-mixed family keeps gz = 1 (its tolerances were set at init and a gz
of 40 would multiply its rounding of v2 by 40): there the bias alone moves z.

A `Case` holds one (layers, regime, rows) combination: weights, synth.make_dataset rows, per-module dropout probabilities
p[l] = 0.1 + 0.1 * (l % 4), Philox masks (seed >= 2^32, stream and row offset non-zero) and, computed once and shared by every test that
asks, the float64 references.  A reference is never modified by a test.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import pinn_oracle as O

#            gain gz  z_med
REGIMES = {
    "init": (1.0, 1.0, None),
    "saturated": (6.0, 1.0, None),
    "sign": (1.0, 8.0, 0.5413),
    "floor": (1.0, 40.0, -14.0),
    "linear": (1.0, 40.0, 20.0),
    "sat_sign": (4.0, 8.0, 0.5413),
}
BF16_REGIMES = ("init", "sign", "floor", "linear")

SEED, STREAM, ROW0 = (1 << 32) + 987654321, 7, 999
MC_STREAM, MC_T = 1000, 6

FUSED_NETS = [[8, 128, 1], [8, 256, 256, 256, 1]]
WIDE_NETS = [[8, 512, 512, 1]]
BF16_NETS = [[8, 256, 256, 256, 1], [8, 512, 512, 1]]
GENERAL_NETS = [[8, 64, 200, 48, 1], [8, 33, 65, 7, 1], [8, 130, 1], [8, 40, 24, 72, 8, 96, 31, 64, 36, 1]]
EDGE_NETS = [[8, 2048, 8, 1], [8, 4, 2048, 1]]          # kMaxWidth as an output and as an input width; h_k // 4 == 2, h_k // 2 == 2
EDGE_REGIMES = ("init", "saturated")
CHUNK_NET, CHUNK_ROWS, CHUNK_T = [8, 2048, 8, 1], 97, 120

# (layers, regime) -> (gain, gz[, gain_deep]) where the table's values miss a condition of test_regimes_host.py.  Every entry comes from
# the CPU measurement alone (torch float32 against float64, in units of the gate; share of rows), none from a device's output:
#   floor, [8,64,200,48,1] and [8,130,1]: at gz = 40 the largest z under the masks is -5.1 / -6.1, not below -7; gz = 28 / 30: -7.8 / -8.1
#   sat_sign, [8,33,65,7,1] and the 8-hidden-layer net: at gain 4 torch's float32 logvar is 0.79 / 0.99 of the gate; gain 3: 0.43 / 0.40
#   saturated, the 8-hidden-layer net: at gain 6 float32 is 0.76 (u) / 0.71 (logvar) of the gate and 3.9e-5 of the largest gradient; no
#     single gain keeps both 10 % of the first layer saturated (gain >= 5.5) and float32 inside half a gate (gain <= 4.5), so the first
#     layer keeps gain 6 (15 % saturated) and the eight matrices behind it take 3.5: 0.12 / 0.19 of the gate, 3.2e-6 of the gradient
OVERRIDES = {
    ((8, 64, 200, 48, 1), "floor"): (1.0, 28.0),
    ((8, 130, 1), "floor"): (1.0, 30.0),
    ((8, 33, 65, 7, 1), "sat_sign"): (3.0, 8.0),
    ((8, 40, 24, 72, 8, 96, 31, 64, 36, 1), "sat_sign"): (3.0, 8.0),
    ((8, 40, 24, 72, 8, 96, 31, 64, 36, 1), "saturated"): (6.0, 1.0, 3.5),
}


def rows_of(layers):
    return 300 if layers[1] == 512 else 777


def widths(layers):
    """Widths of the dropout modules in forward order: every hidden layer, then var_layers.2."""
    return list(layers[1:-1]) + [layers[-2] // 2]


def p_list(layers):
    return [0.1 + 0.1 * (l % 4) for l in range(len(layers) - 1)]


def philox_masks(layers, n, pl, stream=STREAM, seed=SEED, row0=ROW0):
    return [O.philox_keep_mask(seed, stream, row0, n, l, w, pl[l]) for l, w in enumerate(widths(layers))]


def philox_masks_passes(layers, n, pl, streams, seed=SEED, row0=ROW0):
    """philox_masks for several streams at once, one Philox call per eight features (the eight 16-bit draws of a call serve the eight
    features O.philox_keep_mask's docstring names): list over streams of lists over modules.  About ten times quicker than one
    O.philox_keep_mask per pass and module when a test needs 120 passes of a 2048-wide layer; test_regimes_host.py holds it to
    O.philox_keep_mask bit for bit."""
    streams = np.asarray(streams, dtype=np.uint64)
    g = np.arange(n, dtype=np.uint64) + np.uint64(row0)
    out = [[] for _ in streams]
    for l, w in enumerate(widths(layers)):
        thr = O.dropout_threshold16(pl[l])
        ncall = (w + 31) // 32 * 4
        c2 = (np.uint64(l) << np.uint64(16)) | np.arange(ncall, dtype=np.uint64)
        words = O.philox4x32_10((g & np.uint64(0xFFFFFFFF))[None, :, None], (g >> np.uint64(32))[None, :, None], c2[None, None, :],
                                (streams & np.uint64(0xFFFFFFFF))[:, None, None], seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        words = np.stack(words, axis=-1)                                                    # [S, n, ncall, 4]
        draws = np.stack([words & np.uint32(0xFFFF), words >> np.uint32(16)], axis=-1)        # [S, n, ncall, word, half]
        draws = draws.reshape(len(streams), n, ncall, 8)                                    # idx = 2 * word + half
        f = np.arange(w)
        keep = draws[:, :, ((f >> 5) << 2) | ((f >> 2) & 3), 4 * ((f >> 4) & 1) + (f & 3)] >= np.uint32(thr)
        if thr >= 65536:
            keep[:] = False
        for s in range(len(streams)):
            out[s].append(keep[s])
    return out


def head_z(P, x, pl=None, masks=None):
    """float64: (first-layer activation a0 [N, h_0], variance-head pre-activation z [N]) of O.mlp_forward, whose statements these are.
    test_regimes_host.py checks log(softplus(z) + 1e-6) against the oracle's own logvar."""
    P = [p.detach().double() for p in P]
    k = (len(P) - 8) // 2
    h = x.detach().double()
    a0 = None
    with torch.no_grad():
        for l in range(k):
            a = torch.tanh(F.linear(h, P[2 * l], P[2 * l + 1]))
            if l == 0:
                a0 = a
            if masks is not None:
                a = a * (torch.as_tensor(np.asarray(masks[l]), dtype=torch.float32) * float(O.dropout_scale(pl[l])))
            h = a
        v = torch.tanh(F.linear(h, P[2 * k + 2], P[2 * k + 3]))
        if masks is not None:
            v = v * (torch.as_tensor(np.asarray(masks[k]), dtype=torch.float32) * float(O.dropout_scale(pl[k])))
        v = torch.tanh(F.linear(v, P[2 * k + 4], P[2 * k + 5]))
        z = F.linear(v, P[2 * k + 6], P[2 * k + 7])
    return a0, z.reshape(-1)


def regime_params(P, name, p_list, masks, x, gain=None, gz=None, gain_deep=None):
    """A new float32 parameter list: P (O.init_params order) moved to regime `name`.  gain / gz override the table's values; gain_deep,
    if given, replaces gain on every matrix it applies to but the first layer's (whose saturation the regime is defined by)."""
    g0, z0, z_med = REGIMES[name]
    gain = g0 if gain is None else gain
    gz = z0 if gz is None else gz
    gain_deep = gain if gain_deep is None else gain_deep
    k = (len(P) - 8) // 2
    Q = [p.detach().clone() for p in P]
    for i in list(range(0, 2 * k, 2)) + [2 * k + 2, 2 * k + 4]:
        Q[i] = Q[i] * (gain if i == 0 else gain_deep)
    Q[2 * k + 6] = Q[2 * k + 6] * gz
    if z_med is not None:
        _, z = head_z(Q, x, p_list, masks)
        Q[2 * k + 7] = (Q[2 * k + 7].double() + (z_med - float(z.median()))).float()
    return Q


def mc_reference(P, x, pl, T, mask_fn, dtype=torch.float64):
    """O.mc_dropout with one p per module: pred_mean, a_u, e_u [N] as numpy arrays of `dtype`."""
    P = [p.to(dtype) for p in P]
    x = x.to(dtype)
    with torch.no_grad():
        u_eval, _ = O.mlp_forward(P, x)
        us, lvs = zip(*[O.mlp_forward(P, x, pl, mask_fn(t)) for t in range(T)])
    us, lvs = np.array([u.numpy() for u in us]), np.array([lv.numpy() for lv in lvs])
    return u_eval.numpy().reshape(-1), np.sqrt(np.exp(np.mean(lvs, axis=0))).reshape(-1), np.sqrt(np.var(us, axis=0)).reshape(-1)


def vjp64(P, x, gu, glv, pl=None, masks=None):
    """float64 torch.autograd.grad((u, lv), P + [x], (g_u, g_lv)) of O.mlp_forward -> (parameter gradients, dL/dx)."""
    P = [p.detach().double().clone().requires_grad_(True) for p in P]
    x = x.detach().double().clone().requires_grad_(True)
    u, lv = O.mlp_forward(P, x, pl, masks)
    outs, gos = [u], [gu.double().reshape(-1, 1)]
    if glv is not None:
        outs.append(lv)
        gos.append(glv.double().reshape(-1, 1))
    g = torch.autograd.grad(outs, P + [x], gos, allow_unused=True)
    g = [torch.zeros_like(t) if gi is None else gi for gi, t in zip(g, P + [x])]
    return g[:-1], g[-1]


class Case:
    def __init__(self, layers, regime, n, bf16=False):
        from pinn_amd import synth
        self.layers, self.regime, self.n, self.bf16 = list(layers), regime, n, bf16
        self.k = len(layers) - 2
        ds = synth.make_dataset(n, (), seed=n)
        self.x, self.y = ds[0].contiguous(), ds[1].reshape(-1, 1).contiguous()
        self.pl = p_list(self.layers)
        self.masks = philox_masks(self.layers, n, self.pl)
        gain, gz, deep = (tuple(OVERRIDES.get((tuple(layers), regime), REGIMES[regime][:2])) + (None,))[:3]
        self.gain, self.gz, self.gain_deep = gain, (1.0 if bf16 else gz), deep
        self.P = regime_params(O.init_params(self.layers, seed=sum(self.layers)), regime, self.pl, self.masks, self.x, self.gain, self.gz,
                               self.gain_deep)
        self.P64 = [p.double() for p in self.P]

    def mc_masks(self, t):
        return philox_masks(self.layers, self.n, self.pl, stream=MC_STREAM + t)

    def forward(self, train, dtype=torch.float64):
        """(u, logvar) [N] numpy of the oracle in `dtype`: eval, or under the case's Philox masks."""
        with torch.no_grad():
            u, lv = O.mlp_forward([p.to(dtype) for p in self.P], self.x.to(dtype), self.pl if train else None, self.masks if train else None)
        return u.numpy().reshape(-1), lv.numpy().reshape(-1)

    @functools.cached_property
    def eval64(self):
        return self.forward(False)

    @functools.cached_property
    def train64(self):
        return self.forward(True)

    def nll(self, dtype=torch.float64):
        """(loss, mse, gradients) of aleatoric_loss under the case's masks, oracle autograd in `dtype`."""
        lo, mse, g, _, _ = O.nll_loss_and_grads([p.to(dtype) for p in self.P], self.x.to(dtype), self.y.to(dtype), self.pl, self.masks)
        return float(lo), float(mse), g

    @functools.cached_property
    def nll64(self):
        return self.nll()

    @functools.cached_property
    def nll32(self):
        return self.nll(torch.float32)

    @functools.cached_property
    def mc64(self):
        return mc_reference(self.P, self.x, self.pl, MC_T, self.mc_masks)


@functools.lru_cache(maxsize=None)
def _case(layers, regime, n, bf16):
    return Case(layers, regime, n, bf16)


def case(layers, regime, n=None, bf16=False):
    return _case(tuple(layers), regime, rows_of(layers) if n is None else n, bf16)


def all_cases():
    """Every (layers, regime, rows, bf16) that test_gpu_regimes.py runs; test_regimes_host.py proves each one on the CPU."""
    out = []
    for layers in FUSED_NETS + WIDE_NETS + GENERAL_NETS:
        out += [(layers, r, rows_of(layers), False) for r in REGIMES]
    for layers in BF16_NETS:
        out += [(layers, r, rows_of(layers), True) for r in BF16_REGIMES]
    for layers in EDGE_NETS:
        out += [(layers, r, 129, False) for r in EDGE_REGIMES]
    out.append((CHUNK_NET, "sign", CHUNK_ROWS, False))
    return out
