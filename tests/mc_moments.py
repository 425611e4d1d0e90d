"""Cases, float64 reference, fp32 twin and mutants of the MC-dropout moments (pred_mean, a_u, e_u), shared by test_mc_moments_host.py
(CPU: measures the twin against float64 -- the figure behind G -- and proves that the gates tell every claimed mutant from the
reference) and test_gpu_mc_moments_routes.py (GPU: holds the five accumulation codes to the gates at odd pass counts and chunk edges).

Five pieces of device code accumulate the T stochastic passes of a row:

    csrc/pinn_mlp.hip, pinn_bf16.hip     one Welford state, passes in order                                          `sequential`
    csrc/pinn_wide.hip                   the same, the state in accum[4][kWideChunk], reused by every row chunk      `sequential`
    csrc/pinn_general.hip                the same over (pass, row) virtual rows cut into workspace chunks            `sequential`
    csrc/pinn_x6.hip mlp_x6_kernel       TWO Welford states by pass parity, joined by merge_moments (Chan); kSplit: the parities
                                         are the two halves of the workgroup and for odd T the odd half computes a spare pass
                                         (pass index T, masks of pass 0) and drops it                                `parity`

Reference.  The passes themselves are inputs: u_eval [N], u_t [T, N], lv_t [T, N] in fp32 (on the GPU they come from the library's own
forward entry point with Philox stream s0 + t, so forward error is no part of the comparison).  du_t = fl32(u_t - u_eval), one fp32
subtraction as in every kernel; then in float64 pred_mean = u_eval, a_u = exp(0.5 mean_t lv_t), e_u = std_t(du_t) with ddof = 0 (01:1486).

Gates, per row:
    pred_mean   bitwise equal to the forward without dropout
    a_u         |got / a64 - 1| <= 2^-24 (0.5 T mean_t |lv_t| + 4): T - 1 fp32 additions, each one rounding of a partial sum <= sum |lv|,
                of which the exponent carries 0.5 / T; 4 units for inv_t, the two multiplications and expf
    e_u         |got - e64| <= G 2^-24 max_t |du_t| + 2^-23 e64
G is four times the largest |twin - e64| / (2^-24 max_t |du_t|) that the twin below shows over the host cases (host_case: [8,128,1] nets,
p = 0.4, 257 rows, T in HOST_T, both orders); the factor 4 because the GPU runs see other rows than the host cases and hipcc may contract
the merge's multiply-add.  test_mc_moments_host.py asserts twin_max <= G / 4, so the constant cannot drift from the measurement.

Twin: `twin(du, lv, order)` restates in numpy float32 the two accumulation orders as the source writes them, with
fma(a, b, c) = float32(float64(a) * b + c).  It is a yardstick and the base of the mutants, not an expected bit pattern.

Mutants of the twin, each a bug the kernel could have:
    1   the spare pass counted into the odd state with pass 0's data (odd T, parity order)
    2   n0 = n1 = T / 2 in the merge (parity order)
    3   inv_k = 1 / (t + 1) inside a parity state
    4   variance divided by T - 1 (either order)
CLAIMED lists the (mutant, T, output) for which test_mc_moments_host.py proves the mutant beyond MARGIN = 4 gates on at least half of
the rows of every host case.
"""
import functools
import os
import re

import numpy as np
import torch

import pinn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "physics-informed-neural-network-for-explainable-fault-diagnosis-in-fuel-cells_amd", "csrc")

U24 = 2.0 ** -24
TWIN_MAX = 2.12           # measured on the host cases: parity 2.119 (net 1, T = 3), sequential 1.649 (test_mc_moments_host.py prints every case)
G = 4.0 * TWIN_MAX
MARGIN = 4.0

HOST_T = (1, 2, 3, 5, 7, 33)
HOST_ROWS, HOST_H, HOST_NH, P_MC = 257, 128, 1, 0.4
HOST_NET_SEEDS = (1, 2, 3)
SEED, STREAM, ROW0 = (1 << 32) + 20251107, 300, 4001

# (mutant, T) claimed through e_u; mutant 1 is also claimed through a_u at every odd T.  Mutant 2 at T = 33 (n0 n1 / T = 7.76 against
# 8.24, a 6 % change of a term that is itself a small share of m2) is not claimed: it was expected to be too close, and although the
# host cases show it beyond 4 gates on 92 to 94 % of their rows its median is 320 to 430 gates where every claimed pair has thousands.
CLAIMED_E = ([(1, T) for T in HOST_T if T % 2 and T >= 3] + [(2, T) for T in (3, 5, 7)] + [(3, T) for T in HOST_T if T >= 2]
             + [(4, T) for T in HOST_T if T >= 2])
CLAIMED_A = [(1, T) for T in HOST_T if T % 2]


# ---------------------------------------------------------------------------------------------------------------------------
# reference and gates
class Reference:
    """float64 moments of fp32 passes and the gates of the module docstring.  Nothing in it is modified after construction."""

    def __init__(self, u_eval, u_t, lv_t):
        self.u_eval = np.ascontiguousarray(u_eval, dtype=np.float32).reshape(-1)
        self.u_t = np.ascontiguousarray(u_t, dtype=np.float32).reshape(-1, self.u_eval.size)
        self.lv_t = np.ascontiguousarray(lv_t, dtype=np.float32).reshape(self.u_t.shape)
        self.T, self.n = self.u_t.shape
        self.du = self.u_t - self.u_eval[None, :]                       # float32 - float32: one fp32 rounding
        assert self.du.dtype == np.float32
        du64, lv64 = self.du.astype(np.float64), self.lv_t.astype(np.float64)
        self.pred_mean = self.u_eval
        self.a64 = np.exp(0.5 * lv64.mean(axis=0))
        self.e64 = du64.std(axis=0)
        self.du_max = np.abs(du64).max(axis=0)
        self.gate_a = U24 * (0.5 * self.T * np.abs(lv64).mean(axis=0) + 4.0)          # relative
        self.gate_e = G * U24 * self.du_max + 2.0 ** -23 * self.e64                    # absolute

    @staticmethod
    def _over(err, gate):
        """err / gate per row; a zero gate (T = 1 with du = 0) admits a zero error only."""
        out = np.full(err.shape, np.inf)
        np.divide(err, gate, out=out, where=gate > 0)
        out[(gate <= 0) & (err == 0)] = 0.0
        return out

    def a_ratio(self, a_u):
        return self._over(np.abs(np.asarray(a_u, dtype=np.float64) / self.a64 - 1.0), self.gate_a)

    def e_ratio(self, e_u):
        return self._over(np.abs(np.asarray(e_u, dtype=np.float64) - self.e64), self.gate_e)

    def e_units(self, e_u):
        """|e_u - e64| in units of 2^-24 max_t |du_t|: what G is measured in."""
        return self._over(np.abs(np.asarray(e_u, dtype=np.float64) - self.e64), U24 * self.du_max)


# ---------------------------------------------------------------------------------------------------------------------------
# the fp32 twin and its mutants
def fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def _welford(mean, m2, x, inv_k):
    """welford_update (csrc/pinn_mlp_core.h)."""
    d = x - mean
    mean = fma(d, inv_k, mean)
    return mean, fma(d, x - mean, m2)


def twin(du, lv, order, mutant=0):
    """(a_u, e_u) float32 [N] of fp32 passes du, lv [T, N] in the order `sequential` or `parity`; mutant 0 = as the source states it."""
    du, lv = np.asarray(du), np.asarray(lv)
    assert du.dtype == np.float32 and lv.dtype == np.float32 and order in ("sequential", "parity")
    assert mutant in (0, 4) or order == "parity"
    T, n = du.shape
    one = np.float32(1.0)
    zero = lambda: np.zeros(n, dtype=np.float32)
    if order == "sequential":
        mean, m2, sl = zero(), zero(), zero()
        for t in range(T):
            mean, m2 = _welford(mean, m2, du[t], one / np.float32(t + 1))
            sl = sl + lv[t]
    else:
        st = [[zero(), zero(), zero()], [zero(), zero(), zero()]]          # mean, m2, sl of the even and of the odd passes
        steps = [(t, t) for t in range(T)]                                   # (pass index, pass whose data it sees)
        if mutant == 1 and T % 2:
            steps.append((T, 0))                                             # the spare: index T, c.pass = 0
        for t, src in steps:
            s = st[t & 1]
            inv_k = one / np.float32(t + 1 if mutant == 3 else t // 2 + 1)
            s[0], s[1] = _welford(s[0], s[1], du[src], inv_k)
            s[2] = s[2] + lv[src]
        a, b = st
        # merge_moments (csrc/pinn_x6.hip), a: even passes, b: odd passes
        n0, n1 = np.float32((T + 1) // 2), np.float32(T // 2)
        if mutant == 2:
            n0 = n1 = np.float32(T // 2)
        inv_n = one / np.float32(T)
        d = b[0] - a[0]
        mean = fma(d, n1 * inv_n, a[0])
        m2 = (a[1] + b[1]) + (d * d) * (n0 * n1 * inv_n)
        sl = a[2] + b[2]
    inv_t = one / np.float32(T)
    var = m2 * (one / np.float32(T - 1) if mutant == 4 else inv_t)
    a_u = np.exp(np.float32(0.5) * (sl * inv_t))
    e_u = np.sqrt(var)
    assert a_u.dtype == np.float32 and e_u.dtype == np.float32
    return a_u, e_u


# ---------------------------------------------------------------------------------------------------------------------------
# host cases: passes of the fp32 oracle on Philox masks
@functools.lru_cache(maxsize=None)
def host_passes(net_seed):
    """(u_eval [N], u_t [max T, N], lv_t [max T, N]) float32 of a [8, 128, 1] net of O.init_params(seed = net_seed); a case of T passes
    takes the first T."""
    from pinn_amd import synth
    layers = [8] + [HOST_H] * HOST_NH + [1]
    P = O.init_params(layers, seed=net_seed)
    x = synth.make_dataset(HOST_ROWS, (), seed=100 + net_seed)[0][:HOST_ROWS].contiguous()
    pl = [P_MC] * (HOST_NH + 1)
    us, lvs = [], []
    with torch.no_grad():
        u_eval = O.mlp_forward(P, x)[0].numpy().reshape(-1)
        for t in range(max(HOST_T)):
            u, lv = O.mlp_forward(P, x, pl, O.philox_masks_for_net(SEED, STREAM + t, ROW0, HOST_ROWS, HOST_H, HOST_NH, pl))
            us.append(u.numpy().reshape(-1))
            lvs.append(lv.numpy().reshape(-1))
    return u_eval, np.stack(us), np.stack(lvs)


@functools.lru_cache(maxsize=None)
def host_case(net_seed, T):
    u_eval, u_t, lv_t = host_passes(net_seed)
    return Reference(u_eval, u_t[:T], lv_t[:T])


# ---------------------------------------------------------------------------------------------------------------------------
# route plan, restated from the source
def _const(path, pattern):
    m = re.search(pattern, open(os.path.join(CSRC, path)).read())
    assert m, (path, pattern)
    return int(m.group(1))


@functools.lru_cache(maxsize=None)
def wide_chunk():
    return _const("pinn_wide.hip", r"constexpr int kWideChunk = (\d+);")


def variant(n_rows, cus):
    """launch_forward_x6 (csrc/pinn_x6.hip) for an MC call: `split` (kSplit, 64-row tiles, the two parities on the two halves of the
    workgroup) while 2 * ceil(n / 128) <= cus, else `waves8` (128-row tiles); with the tile and workgroup counts."""
    t128 = (n_rows + 127) // 128
    split = 2 * t128 <= cus
    tile_rows = 64 if split else 128
    tiles = (n_rows + tile_rows - 1) // tile_rows
    return dict(variant="split" if split else "waves8", tile_rows=tile_rows, tiles=tiles, workgroups=min(tiles, cus))


def wide_chunks(n_rows):
    """launch_forward_wide's row chunks: [(first row, rows)]."""
    c = wide_chunk()
    return [(r0, min(c, n_rows - r0)) for r0 in range(0, n_rows, c)]


def f3_rows(cus):
    """The last row count that runs `split` and the first that runs `waves8`."""
    return 128 * (cus // 2), 128 * (cus // 2) + 1


def f4_rows(cus):
    """`waves8` with more tiles than workgroups, ending in a 129-row tail that alone runs as `split`."""
    return 128 * (cus + 1) + 129


W_ROWS = 65536 + 129                                  # one full chunk of the wide path and 129 rows in the reused accum
W_WINDOWS = ((65472, 128), (65536, 129))              # (first row, rows): across the chunk edge; the second chunk alone
