"""Cases, float64 reference and error band of the bf16/fp32-mixed training kernels -- the fused nets (H = 128, 256: csrc/pinn_bf16.hip)
and the wide nets (H = 512, 1024, 2048: wide_layer_x6_kernel<x6::B1, ..>, wgrad_d_kernel<.., 1>, wgrad_x_kernel<.., 1>) --, shared by
test_bf16_policy_host.py (CPU: proves the references and the band) and test_gpu_bf16.py (GPU: holds the kernels to them).

Reference: the family's own rounding policy in float64, stated once in the oracle: O.bf16_train_step (fused), O.bf16_wide_train_step
(wide).  Band, Case and the mutants take that step function; everything else is one implementation.  The band of tensor t is

    band_t = 3 E_t + 4 * 2^-8 * R_t

E_t: the largest distance from the float64 result among six float32 runs of the same policy that differ only in summation order (K
     chunks of 8, 16, 32, 64, 128 and unchunked) -- the largest element error for the max gate, the rms error for the rms gate;
R_t: the largest single-row contribution to t in the float64 run, max_n (max_i |g[n, i]| max_j |in[n, j]|) for t = g^T in.
The factor 3 is the project's margin for a 16-bit MFMA against a float32 restatement (test_gradient_error_no_worse_than_torch_fp32).
The second term is a flip allowance: a 1-ulp float32 difference can flip a bf16 rounding, which moves one row's term by at most 2^-8 of
itself; flips are rare discrete events, so two correct implementations differ by a few of them (the float32 orders themselves: up to 1.9
such units, printed per case by the host test); 4 is twice that, rounded up.  Neither number comes from a device's output.

A case's seed is part of the table: test_bf16_policy_host.py proves for every row that a reference with the last row (grid-cap case:
the last full 64-row tile) left out lies outside the band, so the seed is what may be redrawn (at most three times), never the band.
Redrawn here: wave-1 (seed 0: median ratio 1.8), wave (seeds 0, 1: 1.9, 4.9), wg+1 (seed 0: 4.1) and mid256 (seed 0: 4.9; seed 1: 5.004,
too close to 5 to rest on one host's BLAS) -- in each the drawn last row happened to carry a small share of the variance head's gradient.

The wide table (WIDE_CASES).  Geometry: a workgroup tile of the layer kernels is 128 rows (8 waves x 16), one weight-gradient K-tile is 16
rows, the stash is padded to whole workgroup tiles (t16 = 8 ceil(rows / 128)); the weight-gradient route and slice count are
plan_workspace's (tests/wgrad_routes.py `plan`, which does not depend on the precision; the walk is the contiguous one) and WIDE_CLAIMS
states per case what its row count reaches -- the host test holds `plan` to it.  Every wide case met the host conditions at seed 0 (row
mutants: the last row, the last full 16-row tile, from 256 rows the last full 128-row tile, w_serial_cap's first second-pass tile; the
hidden layer's gradient blocks (0, 1) and (1, 0) exchanged; the head's dropout scale from layer 0): none was redrawn.

    id            net              rows    what it reaches
    w_one_row     [8,512,1]        1       seven wave tiles of the workgroup tile all padding; nh = 1: no H x H layer launch
    w_wave-1/0/+1 [8,512,1]        15/16/17 wave-tile boundary
    w_wg-1/0/+1   [8,512,512,1]    127/128/129 workgroup-tile boundary; H / 4 = 128: the kNT = 8 instantiation on the last variance layer;
                                           Wv1's gradient on the 128 x 256 tiling
    w_nodrop      [8,1024,1024,1]  145     no dropout; every layer kNT = 16; 4 x 4 gradient blocks
    w_deep        [8,512x3,1]      333     two transposed H x H backward launches in a row
    w_1024        [8,1024,1024,1]  2065    fan-out route, grid 64 x 4 x 4: 45 slices of 3 tiles, one of 1, 18 empty
    w_2048        [8,2048,2048,1]  273     12 slices of 2 tiles, 8 x 8 blocks
    w_fan512      [8,512,512,1]    8209    64 slices, 57 of 9 tiles, one of 7, 6 empty
    w_serial_cap  [8,512,512,1]    max(32913, 128 CUs + 145): the serial route (t16 >= 2048, 128 slices for H = 512) AND more workgroup
                                           tiles than CUs: a second tile per workgroup with the slab pipeline carried over
"""
import functools

import numpy as np
import torch

import pinn_oracle as O
import regimes as R

ORDERS = (8, 16, 32, 64, 128, None)
MARGIN, FLIPS, FLIP = 3.0, 4.0, 2.0 ** -8
SEED, STREAM, ROW0 = (1 << 32) + 20250607, 11, 4321
HOST_CUS = 256          # compute units of an MI355X: the row count of the grid-cap cases where no device can be asked
BF16 = 1                # pinn_net_t.precision = PINN_PREC_BF16

#        id            H    nh rows  mode seed
CASES = [("one_row", 128, 2, 1, 1, 0),              # three of four wave tiles all padding
         ("wave-1", 256, 1, 15, 1, 1),              # wave tile boundary
         ("wave", 256, 1, 16, 1, 2),
         ("wave+1", 256, 1, 17, 1, 0),
         ("wg-1", 128, 1, 63, 1, 0),                # workgroup tile boundary
         ("wg", 128, 1, 64, 1, 0),
         ("wg+1", 128, 1, 65, 1, 1),
         ("nodrop", 256, 2, 129, 0, 0),             # no dropout; t16 = 12, 6 slices
         ("mid128", 128, 3, 333, 1, 0),
         ("mid256", 256, 3, 1000, 1, 2),
         ("empty_slices", 256, 2, 2049, 1, 0),      # t16 = 132: 64 slices of 3 tiles, 20 of them empty
         ("grid_cap", 128, 1, None, 1, 0)]          # 2 CUs 64 + 65 rows: a second tile per workgroup, the serial route, a ragged last tile
CASE_IDS = [c[0] for c in CASES]

WIDE_CASES = [("w_one_row", 512, 1, 1, 1, 0),
              ("w_wave-1", 512, 1, 15, 1, 0),
              ("w_wave", 512, 1, 16, 1, 0),
              ("w_wave+1", 512, 1, 17, 1, 0),
              ("w_wg-1", 512, 2, 127, 1, 0),
              ("w_wg", 512, 2, 128, 1, 0),
              ("w_wg+1", 512, 2, 129, 1, 0),
              ("w_nodrop", 1024, 2, 145, 0, 0),
              ("w_deep", 512, 3, 333, 1, 0),
              ("w_1024", 1024, 2, 2065, 1, 0),
              ("w_2048", 2048, 2, 273, 1, 0),
              ("w_fan512", 512, 2, 8209, 1, 0),
              ("w_serial_cap", 512, 2, None, 1, 0)]
WIDE_IDS = [c[0] for c in WIDE_CASES]
WIDE_TILE = 128         # rows of a workgroup tile of the wide layer kernels

# what each wide row count reaches in the weight-gradient launches (wgrad_routes.plan at precision BF16; test_bf16_policy_host.py)
_ONE_TILE = dict(t16=8, route="fan", slices=4, walk="contiguous", tiles={2: 4}, grid=(4, 2, 2))      # up to 128 rows: one workgroup tile
WIDE_CLAIMS = {
    "w_one_row": _ONE_TILE, "w_wave-1": _ONE_TILE, "w_wave": _ONE_TILE, "w_wave+1": _ONE_TILE, "w_wg-1": _ONE_TILE, "w_wg": _ONE_TILE,
    "w_wg+1": dict(t16=16, route="fan", slices=8, walk="contiguous", tiles={2: 8}, grid=(8, 2, 2)),
    "w_nodrop": dict(t16=16, route="fan", slices=8, walk="contiguous", tiles={2: 8}, grid=(8, 4, 4)),
    "w_deep": dict(t16=24, route="fan", slices=12, walk="contiguous", tiles={2: 12}, grid=(12, 2, 2)),
    "w_1024": dict(t16=136, route="fan", slices=64, walk="contiguous", tiles={3: 45, 1: 1, 0: 18}, grid=(64, 4, 4)),
    "w_2048": dict(t16=24, route="fan", slices=12, walk="contiguous", tiles={2: 12}, grid=(12, 8, 8)),
    "w_fan512": dict(t16=520, route="fan", slices=64, walk="contiguous", tiles={9: 57, 7: 1, 0: 6}, grid=(64, 2, 2)),
    # (at HOST_CUS; with more CUs the row count grows and only route, slices and grid are held)
    "w_serial_cap": dict(t16=2064, route="serial", slices=128, walk="contiguous", tiles={17: 121, 7: 1, 0: 6}, grid=(128, 2, 2)),
}


def grid_cap_rows(cus=HOST_CUS):
    return 2 * cus * 64 + 65


def wide_cap_rows(cus=HOST_CUS):
    """w_serial_cap: the serial route's smallest test row count (32913 = 2048 K-tiles and 17 rows), or one full workgroup tile and 17 rows
    past one tile per CU where that is more (launch_train_chain_wide caps the layer kernels' grid at the CU count)."""
    return max(32913, WIDE_TILE * cus + 145)


def p_list(nh):
    return [0.1 * (l + 1) for l in range(nh + 1)]


def rms(e):
    e = np.asarray(e, dtype=np.float64)
    return float(np.sqrt((e ** 2).mean())) if e.size else 0.0


class Band:
    """Reference and band of one training call under the policy `step` states (O.bf16_train_step or O.bf16_wide_train_step): ref = (sums,
    grads) in float64; e_max / e_rms / r per tensor, the three loss sums first (their row terms are the rows' own summands), then the
    gradient tensors in O.param_names order."""

    def __init__(self, P, x, y, pl, masks, n_global=None, step=O.bf16_train_step):
        self.nh = (len(P) - 8) // 2
        self.step = step
        self.names = ["loss.nll", "loss.abs_logvar", "loss.sq_err"] + O.param_names(self.nh)
        sums, grads, det = step(P, x, y, pl, masks, torch.float64, n_global)
        self.sums, self.grads, self.terms = sums, [g.numpy() for g in grads], det["terms"]
        self.ref = [np.array([s]) for s in sums] + self.grads
        self.e_max, self.e_rms = [0.0] * len(self.ref), [0.0] * len(self.ref)
        for c in ORDERS:
            s32, g32, _ = step(P, x, y, pl, masks, torch.float32, n_global, k_chunk=c)
            for i, (a, b) in enumerate(zip([np.array([s]) for s in s32] + [g.double().numpy() for g in g32], self.ref)):
                self.e_max[i] = max(self.e_max[i], float(np.abs(a - b).max()))
                self.e_rms[i] = max(self.e_rms[i], rms(a - b))
        # largest single-row contribution.  Loss sums: the row's summand, from (u, logvar) of the same run
        u, s = det["u"].reshape(-1), det["logvar"].reshape(-1)
        e = y.double().reshape(-1) - u
        rows = [0.5 * torch.exp(-s) * e * e + 0.5 * s, s.abs(), e * e]
        self.r = [float(t.abs().max()) for t in rows]
        for g, inp in self.terms:
            gi = g.abs().max(dim=1).values
            self.r.append(float((gi if inp is None else gi * inp.abs().max(dim=1).values).max()))
        self.band_max = [MARGIN * e + FLIPS * FLIP * r for e, r in zip(self.e_max, self.r)]
        self.band_rms = [MARGIN * e + FLIPS * FLIP * r for e, r in zip(self.e_rms, self.r)]
        # the float32 orders' own largest error, in flip units
        self.order_flips = max(e / (FLIP * r) for e, r in zip(self.e_max, self.r) if r > 0)

    def ratios(self, sums, grads, ref=None):
        """[(name, max error / band, rms error / band)] of a result (sums [3], gradient tensors in param_names order) against the
        float64 reference, or against another result `ref` = (sums, grads)."""
        as_list = lambda sg: [np.array([float(s)]) for s in sg[0]] + [np.asarray(g, dtype=np.float64) for g in sg[1]]
        got, ref = as_list((sums, grads)), self.ref if ref is None else as_list(ref)
        out = []
        for n, a, b, bm, br in zip(self.names, got, ref, self.band_max, self.band_rms):
            d = a.reshape(-1) - b.reshape(-1)
            out.append((n, float(np.abs(d).max()) / bm if np.isfinite(d).all() else float("inf"), rms(d) / br))
        return out

    def without_rows(self, lo, hi):
        """The float64 gradients with rows [lo, hi) left out of every row sum (a mutant: what a kernel that skips them computes)."""
        out = []
        for (g, inp), full in zip(self.terms, self.grads):
            part = g[lo:hi].t() @ (g.new_ones(hi - lo, 1) if inp is None else inp[lo:hi])
            out.append(full - part.numpy().reshape(full.shape))
        return out

    def blocks_swapped(self):
        """The float64 gradients with the 256 x 256 blocks (0, 1) and (1, 0) of the hidden layer's gradient (layers.layer_1.weight)
        exchanged: what a weight-gradient workgroup that mixes up blockIdx.y and blockIdx.z stores.  -> (tensor name, gradients)."""
        name = "layers.layer_1.weight"
        i = O.param_names(self.nh).index(name)
        out = list(self.grads)
        w = self.grads[i].copy()
        w[0:256, 256:512], w[256:512, 0:256] = self.grads[i][256:512, 0:256], self.grads[i][0:256, 256:512]
        out[i] = w
        return name, out


class Case:
    def __init__(self, name, H, nh, n, mode, seed, step=O.bf16_train_step):
        from pinn_amd import synth
        self.name, self.H, self.nh, self.n, self.mode, self.seed, self.step = name, H, nh, n, mode, seed, step
        self.wide = H > 256
        self.layers = [8] + [H] * nh + [1]
        self.P = O.init_params(self.layers, seed=1000 * seed + H + nh)
        ds = synth.make_dataset(max(n, 2), (), seed=1000 * seed + n)
        self.x, self.y = ds[0][:n].contiguous(), ds[1].reshape(-1)[:n].contiguous()
        self.pl = p_list(nh)
        # (regimes.philox_masks_passes: O.philox_keep_mask bit for bit, test_regimes_host.py, at a tenth of its time for 32 833 rows)
        self.masks = R.philox_masks_passes(self.layers, n, self.pl, [STREAM], seed=SEED, row0=ROW0)[0] if mode else None

    @functools.cached_property
    def band(self):
        return Band(self.P, self.x, self.y, self.pl, self.masks, step=self.step)

    def mutant_rows(self):
        """Rows the row mutant leaves out: the last row; grid-cap case: the last tile that holds 64 rows (the ragged one behind it holds
        one row), which a workgroup reaches in its second pass over the grid."""
        if self.name != "grid_cap":
            return self.n - 1, self.n
        t = (self.n - 1) // 64 - 1
        return 64 * t, 64 * t + 64

    def row_mutants(self, cus=HOST_CUS):
        """The wide cases' row mutants, [(label, lo, hi)]: the last row; the last full 16-row K-tile of the weight gradients; from 256 rows
        on the last full 128-row workgroup tile; w_serial_cap: the first workgroup tile a workgroup reaches in its SECOND pass over the
        grid (tile index = CUs: launch_train_chain_wide launches min(tiles, CUs) workgroups)."""
        n = self.n
        out = [("last row", n - 1, n)]
        if n >= 16:
            out.append(("last full 16-row tile", n // 16 * 16 - 16, n // 16 * 16))
        if n >= 256:
            out.append(("last full 128-row tile", n // WIDE_TILE * WIDE_TILE - WIDE_TILE, n // WIDE_TILE * WIDE_TILE))
        if self.name == "w_serial_cap":
            assert WIDE_TILE * (cus + 1) <= n
            out.append(("second-pass tile %d" % cus, WIDE_TILE * cus, WIDE_TILE * (cus + 1)))
        return out

    def head_scale_mutant(self):
        """float64 gradients with the variance head's dropout SCALE taken from layer 0 (same masks): what reading drop.scale[0] for the
        head computes.  None without dropout."""
        if not self.mode:
            return None
        pl = list(self.pl)
        pl[self.nh] = pl[0]
        return [g.numpy() for g in self.step(self.P, self.x, self.y, pl, self.masks)[1]]


@functools.lru_cache(maxsize=None)
def _case(name, n):
    if name in WIDE_IDS:
        _, H, nh, _, mode, seed = WIDE_CASES[WIDE_IDS.index(name)]
        return Case(name, H, nh, n, mode, seed, step=O.bf16_wide_train_step)
    _, H, nh, _, mode, seed = CASES[CASE_IDS.index(name)]
    return Case(name, H, nh, n, mode, seed)


def case(name, cus=HOST_CUS):
    if name in WIDE_IDS:
        n = WIDE_CASES[WIDE_IDS.index(name)][3]
        return _case(name, wide_cap_rows(cus) if n is None else n)
    n = CASES[CASE_IDS.index(name)][3]
    return _case(name, grid_cap_rows(cus) if n is None else n)


def golden_case():
    """g_net128.npz ([8, 128 x 3, 1], recorded torch masks at p = 0.2) -> (P, x, y, pl, masks)."""
    from conftest import load_golden, params_from_golden, unpack_mask
    g = load_golden("g_net128.npz")
    masks = [unpack_mask(g["mask%d_p0.2_t0" % l], 128 if l < 3 else 64) for l in range(4)]
    return params_from_golden(g), torch.from_numpy(g["x"]), torch.from_numpy(g["y"]).reshape(-1), [0.2] * 4, masks


@functools.lru_cache(maxsize=None)
def golden_band():
    return Band(*golden_case())


def _drawn(H, nh, n, seed, step):
    from pinn_amd import synth
    P = O.init_params([8] + [H] * nh + [1], seed=seed)
    ds = synth.make_dataset(n, (), seed=seed + 1)
    pl = p_list(nh)
    g = torch.Generator().manual_seed(seed + 2)
    masks = [(torch.rand(n, w, generator=g) >= pl[l]).numpy() for l, w in enumerate([H] * nh + [H // 2])]
    x, y = ds[0].contiguous(), ds[1].reshape(-1).contiguous()
    return P, x, y, pl, masks, Band(P, x, y, pl, masks, step=step)


@functools.lru_cache(maxsize=None)
def drawn_mask_case():
    """65 rows of [8, 128, 128, 1] under torch-drawn masks with one p per module: one row past a workgroup tile, so the kernels' padding
    rows read the last mask row.  -> (P, x, y, pl, masks, Band)."""
    return _drawn(128, 2, 65, 31, O.bf16_train_step)


@functools.lru_cache(maxsize=None)
def wide_drawn_mask_case():
    """The same for the wide kernels' PINN_DROP_BITS branch (activate_pair_rt): 129 rows of [8, 512, 512, 1], one row past a 128-row
    workgroup tile.  -> (P, x, y, pl, masks, Band under the wide policy)."""
    return _drawn(512, 2, 129, 41, O.bf16_wide_train_step)


@functools.lru_cache(maxsize=None)
def wide_shard_case():
    """[8, 512, 512, 1] at 333 rows, Philox masks: the wide row of the repeatability / shard-additivity test (shards [0, 129) and [129, 333))."""
    return Case("w_shard", 512, 2, 333, 1, 0, step=O.bf16_wide_train_step)
