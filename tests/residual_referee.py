"""Float64 referee of the residual passes' 20 columns and 26 live sums (csrc/pinn_residuals.hip), shared by
test_residual_referee_host.py (CPU: the referee reproduces the fixture's recorded tuples, losses and gradients and torch autograd's
derivative sums, its rows reach every branch they are named for, and the gates are tight) and test_gpu_residual_forward.py (GPU:
pinn_residuals, pinn_residuals_prepare + pinn_residuals_cached, pinn_lambda_stage_run and pinn_net_f_t against it).

Every pass that produces the sums is assembled from one text, csrc/pinn_physics.h, so comparing the passes with each other cannot
see an error in that text, in block_sums or in sums_finalize.  Nothing here is taken from the header: the models are the oracle's
net_f_V / net_f_T_simple / net_f_H / net_f_O / net_f_T (oracle/pinn_oracle.py, pinned to the reference by tests/golden), run by
torch on the CPU in float64 (r64) and in float32 (r32) from the same float32 de-normalised rows (O.denorm), and the per-row terms
of the sums are written from the reference's formulas and SURVEY.md 9.2:

    V   f^2, f d_k, (y - Vn)^2, (y - Vn) d_k, (y - u)^2       d_1 = -i, d_2 = b / l2, d_3 = 0.5 b i / (l3 (l3 - i)), b = 8.314 Tk / 96485,
                                                              Vn = 5 V_est vn_scale + vn_min (01:1025)
    T   f^2, f (-It6), f (-mc), -f, |f|                       It6 = 270 (I / 270 + 1e-6), mc = coolant flow + 1e-6
    H   f^2, -f, f (-(lin ? It / 100 : lH3 / 100)), f (-(lin ? 0 : lH2 / 100)), act, tgt               lin = [It <= lH3]
    O   f^2, f (-c), f (-c (lin ? It / 100 : thr / 100)), f (-c (lin ? 0 : lO2 sgn(lO3) / 100)), act, tgt
                                                              thr = |lO3|, lin = [It <= thr], c = [1.05 <= raw <= 15] (inclusive)

Rows (rows()).  synth.synth_rows normalised with the fixture's scalers; the fixture's 256 branch-edge rows (g_resid.npz) spread evenly
through them, so every branch is live at every size; marked rows at the positions where a launch changes shape (marked_positions):
an outlier in the four inputs only one model reads (u: V, coolant flow: T, H2 flow: H, air flow: O), sized with sqrt(N) so that the
row's term of each model's sum of squares is at least 100 gates, and different from marked row to marked row by 10 %, so that a
dropped, doubled or exchanged row cannot hide in a gate.  Idle rows (I = 0, -0.0027, -1 A, no gas flow) reach the 1e-8 flow clamp; the
voltage model is NaN there, so they are for the H and O models only.

Gates.  They come from the arithmetic and the referee, never from what a kernel gives:
    columns   |got - r64| <= 2 |r32 - r64| + 1e-5 max|r64| row by row (the yardstick of test_gpu_physics_autograd._within with SURVEY
              8(c)'s 1e-5); the NaN pattern is r32's; the T, H and O columns have no transcendental and equal r32.
    sums      |S - sum t64| <= 2 sum|t32 - t64| + (r + 2) 2^-24 sum|t64| + 1e-5 max|t64|
              the first term is the float32 rounding of each row's term (the factor 2: the device's <= 2 ulp transcendentals against
              the CPU's), the second the r float additions a thread makes before the float64 tree plus the two roundings of the
              accumulator's operands, the third keeps N = 1 at the column tolerance.  r follows from the launch constants
              (rows_per_thread), it is not read back from a run.
Edges.  The columns are continuous across every branch (where, clamp), the derivative factors are not: a row that sits on a threshold
(the fixture has It = lambda_H3 and It = |lambda_O3| to the ulp) or a target on the clamp's edge can fall on the other side in float64, and
its term then differs by its whole size.  The side the float32 program is on defines the derivative, so the three indicators
lin_H, lin_O and c of r64's terms are r32's (evaluate(branches=...)); everything else of r64 is its own, and the host test checks the
terms with their own indicators against torch autograd.  For the two exact-edge sets (EXACT_EDGE) r32 is the authority throughout: the
float64 value of float32(1.05) lies below 1.05, on the other side of the inclusive edge.  The columns equal r32 and the sums are
compared with sum t32; r64 only sizes the gate.
"""
import functools
import math

import numpy as np
import torch

import pinn_oracle as O
from conftest import ScalerFromArrays, load_golden

U = 2.0 ** -24
COL_REL = 1e-5
MARK_GATES = 100.0              # a marked row's term of its model's sum of squares, in gates
CAP = 1e-5                      # every sum's gate over sum|t64|, N >= 255
NAMES = O.LAMBDA_NAMES

# the enums of include/pinn_hip.h (test_residual_referee_host.py compares them with the binding)
COL_NAMES = ["FV", "VACT", "VOHM", "VCONC", "ENERNST", "VEST5", "I", "VOUT5", "FT", "TPRED", "TOUT",
             "FH", "ACTH", "TGTH", "ITOT", "FO", "ACTO", "TGTO", "QO2", "O2FLOW"]
SUM_NAMES = ["FV2", "FV_D1", "FV_D2", "FV_D3", "YV2", "YV_D1", "YV_D2", "YV_D3", "YU2",
             "FT2", "FT_D1", "FT_D3", "FT_D5", "FT_ABS", "FH2", "FH_D1", "FH_D2", "FH_D3", "ACTH", "TGTH",
             "FO2", "FO_D1", "FO_D2", "FO_D3", "ACTO", "TGTO"]
NSUMS = 32
FLAG = {"V": 1, "T": 2, "H": 4, "O": 8}
# column -> (model, index in the oracle's tuple)
COL_SRC = {"FV": ("V", 0), "VACT": ("V", 1), "VOHM": ("V", 2), "VCONC": ("V", 3), "ENERNST": ("V", 4), "VEST5": ("V", 5), "I": ("V", 6),
           "VOUT5": ("V", 8), "FT": ("T", 0), "TPRED": ("T", 1), "TOUT": ("T", 2), "FH": ("H", 0), "ACTH": ("H", 1), "TGTH": ("H", 2),
           "ITOT": ("H", 3), "FO": ("O", 0), "ACTO": ("O", 1), "TGTO": ("O", 2), "QO2": ("O", 3), "O2FLOW": ("O", 4)}
SUM_MODEL = {s: ("V" if s[:2] in ("FV", "YV", "YU") else "T" if s[:2] == "FT" else "H" if s in ("FH2", "FH_D1", "FH_D2", "FH_D3", "ACTH", "TGTH")
                 else "O") for s in SUM_NAMES}
SQUARES = {"V": "FV2", "T": "FT2", "H": "FH2", "O": "FO2"}
Y_SUMS = ["YV2", "YV_D1", "YV_D2", "YV_D3", "YU2"]          # the sums that need the measured voltage: 0 without d_y

GRID_ROWS = 256 * 1024          # threads of the row pass's grid at its cap: the second grid-stride trip starts here
EDGE_ROWS = 256

# row counts of the GPU file: the smallest at which each structure changes
ROW_COUNTS = [1, 255, 256, 257, 65536, 65537, GRID_ROWS + 1, 2 * GRID_ROWS + 3]
EDGE_COUNTS = [257, 65537]                                    # sets C, D and the exact-edge sets
PERSISTENT_COUNTS = [1, 1023, 1025, 4 * 1024 + 1, 65536]
EULER_COUNTS = [1, 2, 257, GRID_ROWS + 1]
MAIN_SETS = ["init", "s1", "moved", "A", "B"]
EDGE_SETS = ["C", "D", "edge15", "edge105"]
EXACT_EDGE = ("edge15", "edge105")                            # r32 is the authority


def cases():
    """Every (N, set, idle) the GPU file compares sums at."""
    out = [(N, s, False) for N in ROW_COUNTS for s in MAIN_SETS] + [(N, s, False) for N in EDGE_COUNTS for s in EDGE_SETS]
    out += [(N, s, False) for N in PERSISTENT_COUNTS for s in ("init", "moved", "B") if (N, s, False) not in out]
    return out + [(257, "init", True), (257, "B", True)]


@functools.lru_cache(maxsize=None)
def fixture():
    g = load_golden("g_resid.npz")
    return g, ScalerFromArrays(g, "sx."), ScalerFromArrays(g, "sy.")


@functools.lru_cache(maxsize=None)
def param_sets():
    """name -> float32 [17].  A: the low clamp of the oxygen target; B: the high clamp, with a negative threshold parameter; D: clamped
    and linear rows together; C: sgn(lambda_O3) = 0, every row past the threshold; moved: V, T and H far from the start."""
    g = fixture()[0]
    init = np.array([O.LAMBDA_INIT[k] for k in NAMES], dtype=np.float32)

    def mod(**kw):
        v = init.copy()
        for k, x in kw.items():
            v[NAMES.index(k)] = np.float32(x)
        return v
    return {"init": init, "s1": g["s1.lambdas"].astype(np.float32),
            "moved": mod(lambda_1=0.5, lambda_2=4e-6, lambda_3=9.0, lambda_T1=-0.3, lambda_T3=2.5, lambda_T5=-40.0, lambda_H1=30.0,
                         lambda_H2=-15.0, lambda_H3=60.0),
            "A": mod(lambda_O1=1.0, lambda_O2=0.03, lambda_O3=300.0), "B": mod(lambda_O1=8.0, lambda_O2=3.0, lambda_O3=-260.0),
            "C": mod(lambda_O3=0.0), "D": mod(lambda_O1=1.5, lambda_O2=5.0, lambda_O3=400.0),
            "edge15": mod(lambda_O1=15.0, lambda_O2=0.0), "edge105": mod(lambda_O1=np.float32(1.05), lambda_O2=0.0)}


# ---------------------------------------------------------------------------------------------------------------------------
# launch shapes, from the constants documented in csrc/pinn_residuals.hip and csrc/pinn_physics.h
def _ceil(a, b):
    return -(-a // b)


def row_pass_blocks(N):
    return min(max(_ceil(N, 256), 1), 1024)


def cached_blocks(N):
    return row_pass_blocks(_ceil(N, 2))                       # two rows per trip: the grid is sized for half the rows


def rows_per_thread(N, kernel):
    """Rows one thread adds in float before the float64 tree.  "rows": pinn_residuals (256 threads, at most 1024 workgroups,
    grid-stride); "cached": pinn_residuals_cached (the same with the grid of half the rows); "persistent": one workgroup of 1024."""
    if kernel == "rows":
        return _ceil(N, 256 * row_pass_blocks(N))
    if kernel == "cached":
        return _ceil(N, 256 * cached_blocks(N))
    assert kernel == "persistent"
    return _ceil(N, 1024)


def marked_positions(N):
    """0, N - 1, either side of the row pass's second grid-stride trip, and the last row of the cached pass's first two-row trip
    with the first row of the next."""
    trip = 2 * 256 * cached_blocks(N)
    return sorted({p for p in (0, N - 1, GRID_ROWS - 1, GRID_ROWS, trip - 1, trip) if 0 <= p < N})


# ---------------------------------------------------------------------------------------------------------------------------
# rows
class Rows:
    pass


def _normalise(v, mn, sc):
    return (np.asarray(v, np.float64) * sc + mn).astype(np.float32)


@functools.lru_cache(maxsize=4)
def rows(N, idle=False):
    """-> Rows with xn [N, 8], un [N], yn [N] float32 (normalised), real [N, 8] float32 (O.denorm), marked, edge, idle positions."""
    from pinn_amd import synth
    g, sx, sy = fixture()
    mn, sc = O.scaler_affine(sx)
    ymn, ysc = O.scaler_affine(sy)
    X, V = synth.synth_rows(N, seed=17)
    xn = _normalise(X, mn, sc)
    yn = _normalise(V, ymn, ysc).reshape(-1)
    un = (yn + 0.05 * np.random.default_rng(18).standard_normal(N)).astype(np.float32)
    marked = marked_positions(N)
    # the fixture's edge rows between the first and the last row (which are marked); below 258 rows as many of them as fit, from
    # the front: its rows 0..23 are the ones placed on the edges
    ne = max(0, min(EDGE_ROWS, N - 2))
    edge = 1 + (np.arange(ne) * (N - 2)) // max(ne, 1)
    xn[edge], yn[edge], un[edge] = g["x"][:ne], g["y"].reshape(-1)[:ne], g["u_eval"].reshape(-1)[:ne]
    idle_pos = []
    if idle:
        free = [p for p in range(N) if p not in set(marked)]
        idle_pos = free[100:109]
        for j, p in enumerate(idle_pos):
            xn[p, 0] = _normalise((0.0, -0.0027, -1.0)[j % 3], mn[0], sc[0])
            xn[p, 6] = _normalise(0.0, mn[6], sc[6])
            xn[p, 7] = _normalise(0.0, mn[7], sc[7])
    # marked rows: one ordinary operating point, the four single-model inputs far out
    s = max(1.0, math.sqrt(N / 256.0))
    base = np.array([230.0, 20.0, 60.0, 80.0, 70.0, 66.0, 0.0, 0.0])
    for j, p in enumerate(marked):
        k = s * (1.0 + 0.1 * j)
        row = base.copy()
        row[1], row[6], row[7] = 1000.0 * k, 300.0 * k, 1000.0 * k
        xn[p] = _normalise(row, mn, sc)
        yn[p] = _normalise(4.06, ymn[0], ysc[0])
        un[p] = np.float32(4.0 * k)
    r = Rows()
    r.N, r.xn, r.un, r.yn, r.marked, r.edge, r.idle = N, xn, un, yn, marked, edge, idle_pos
    r.real = O.denorm(xn, mn, sc)
    return r


# ---------------------------------------------------------------------------------------------------------------------------
# the referee
def _lam(lamv, dtype):
    return {k: torch.tensor([float(np.float32(v))], dtype=dtype) for k, v in zip(NAMES, lamv)}


def evaluate(real, un, yn, lamv, dtype, models="VTHO", branches=None):
    """The oracle's models in `dtype` from float32 rows -> (cols {name: [N]}, terms {sum name: [N]}, stats, branches) as float64
    numpy (a float32 result is converted, not recomputed).  branches: None, or the indicators (h_lin, o_lin, o_inside) of another
    evaluation, which the derivative factors then take in place of their own."""
    _, _, sy = fixture()
    ymn, ysc = O.scaler_affine(sy)
    vn_scale, vn_min = (t.to(dtype) for t in O.target_affine(sy))
    realt = torch.tensor(np.asarray(real, np.float32), dtype=dtype)
    u32 = torch.tensor(np.asarray(un, np.float32)).reshape(-1, 1)
    lam = _lam(lamv, dtype)
    tup, t, stats, br = {}, {}, {}, {}
    with torch.no_grad():
        if "V" in models:
            r = tup["V"] = O.net_f_V(realt, u32, ymn, ysc, lam)
            f, i = r[0], r[6]
            y, u = torch.tensor(np.asarray(yn, np.float32), dtype=dtype).reshape(-1, 1), u32.to(dtype)
            b = O._t(8.314) * (realt[:, 5:6] + O._t(273.15)) / O._t(96485)     # the reference's constants are float32 tensors
            l2, l3 = lam["lambda_2"], lam["lambda_3"]
            d = (-i, b / l2, 0.5 * b * i / (l3 * (l3 - i)))
            e = y - (r[5] * vn_scale + vn_min)
            t["FV2"], t["YV2"], t["YU2"] = f * f, e * e, (y - u) ** 2
            for k in range(3):
                t["FV_D%d" % (k + 1)], t["YV_D%d" % (k + 1)] = f * d[k], e * d[k]
        if "T" in models:
            r = tup["T"] = O.net_f_T_simple(realt, lam)
            f = r[0]
            It6 = (realt[:, 0:1] / 270 + 1e-6) * 270
            mc = realt[:, 1:2] + 1e-6
            t["FT2"], t["FT_D1"], t["FT_D3"], t["FT_D5"], t["FT_ABS"] = f * f, f * (-It6), f * (-mc), -f, f.abs()
        if "H" in models:
            r = tup["H"] = O.net_f_H(realt, lam)
            f, act, tgt, It = r[:4]
            l2, l3 = lam["lambda_H2"], lam["lambda_H3"]
            lin = br["h_lin"] = (It <= l3) if branches is None else branches["h_lin"]
            zero = torch.zeros_like(It)
            t["FH2"], t["FH_D1"] = f * f, -f
            t["FH_D2"] = f * (-torch.where(lin, It / 100, l3 / 100 + zero))
            t["FH_D3"] = f * (-torch.where(lin, zero, l2 / 100 + zero))
            t["ACTH"], t["TGTH"] = act, tgt
            stats.update(h_lin=int(lin.sum()), h_past=int((~lin).sum()), h_flow_clamped=int((It <= 0).sum()))
        if "O" in models:
            r = tup["O"] = O.net_f_O(realt, lam)
            f, act, tgt = r[:3]
            It = (realt[:, 0:1] / 270 + 1e-5) * 270
            l1, l2, l3 = lam["lambda_O1"], lam["lambda_O2"], lam["lambda_O3"]
            thr, sgn = l3.abs(), torch.sign(l3)
            own_lin = It <= thr
            zero = torch.zeros_like(It)
            raw = torch.where(own_lin, l1 + l2 * (It / 100), l1 + l2 * (thr / 100) + zero)
            lin = br["o_lin"] = own_lin if branches is None else branches["o_lin"]
            inside = br["o_inside"] = ((raw >= 1.05) & (raw <= 15.0)) if branches is None else branches["o_inside"]
            c = inside.to(dtype)
            t["FO2"], t["FO_D1"] = f * f, f * (-c)
            t["FO_D2"] = f * (-c * torch.where(lin, It / 100, thr / 100 + zero))
            t["FO_D3"] = f * (-c * torch.where(lin, zero, l2 * sgn / 100 + zero))
            t["ACTO"], t["TGTO"] = act, tgt
            stats.update(o_low=int((raw < 1.05).sum()), o_high=int((raw > 15.0).sum()), o_inside=int(c.sum()), o_lin=int(lin.sum()),
                         o_past=int((~lin).sum()), o_sgn=float(sgn), o_penalty=int((act < 1.0).sum()), o_flow_clamped=int((It <= 0).sum()),
                         o_on_edge=int(((raw == 1.05) | (raw == 15.0)).sum()))
    f64 = lambda v: v.detach().double().numpy().reshape(-1)
    cols = {c: f64(tup[m][j]) for c, (m, j) in COL_SRC.items() if m in models}
    return cols, {k: f64(v) for k, v in t.items()}, stats, br


class Referee:
    """cols64 / cols32 and t64 / t32 of one (rows, set); center [NSUMS]: what a sum is compared with (sum t64; sum t32 for an
    exact-edge set); budget, abs_sum, abs_max [NSUMS] of the gate."""

    def gate(self, r):
        return self.budget + (r + 2) * U * self.abs_sum + COL_REL * self.abs_max


def _referee_of(real, un, yn, lamv, models, authority32):
    ref = Referee()
    ref.models = models
    ref.cols32, ref.t32, ref.stats, branches = evaluate(real, un, yn, lamv, torch.float32, models)
    ref.cols64, ref.t64, ref.stats64, _ = evaluate(real, un, yn, lamv, torch.float64, models, branches)
    ref.center, ref.budget, ref.abs_sum, ref.abs_max = (np.zeros(NSUMS) for _ in range(4))
    ref.live = np.zeros(NSUMS, dtype=bool)
    for k, name in enumerate(SUM_NAMES):
        if name not in ref.t64:
            continue
        a, b = ref.t64[name], ref.t32[name]
        ref.live[k] = True
        ref.center[k] = (b if authority32 else a).sum()
        ref.budget[k] = 2.0 * np.abs(b - a).sum()
        ref.abs_sum[k] = np.abs(a).sum()
        ref.abs_max[k] = np.abs(a).max()
    ref.authority = "r32" if authority32 else "r64"
    return ref


@functools.lru_cache(maxsize=2)
def referee(N, set_name, idle=False):
    rw = rows(N, idle)
    ref = _referee_of(rw.real, rw.un, rw.yn, param_sets()[set_name], "HO" if idle else "VTHO", set_name in EXACT_EDGE)
    ref.rows = rw
    return ref


def edge_stats(set_name):
    """Branch counts of a set on the fixture's 256 edge rows alone (float32, the arithmetic the kernels follow)."""
    g = fixture()[0]
    mn, sc = O.scaler_affine(fixture()[1])
    real = O.denorm(g["x"], mn, sc)
    return evaluate(real, g["u_eval"].reshape(-1), g["y"].reshape(-1), param_sets()[set_name], torch.float32)[2]


# what each set is named for: statistic -> must be > 0 on the rows of every case that uses the set
NAMED_BRANCHES = {"init": ["o_lin", "o_past", "o_penalty", "h_lin", "h_past"], "s1": ["o_lin", "o_past", "h_lin", "h_past"],
                  "moved": ["h_past"], "A": ["o_low", "o_inside"], "B": ["o_high", "o_inside", "o_lin", "o_past"],
                  "C": ["o_past"], "D": ["o_high", "o_inside", "o_lin"], "edge15": ["o_on_edge"], "edge105": ["o_on_edge"]}


def check_conditions(ref, kernels=("rows", "cached", "persistent")):
    """The conditions on the referee's own numbers, asserted before any comparison; returns the figures it looked at."""
    N, rw = ref.rows.N, ref.rows
    out = {}
    for name in ref.t64:
        assert np.all(np.isfinite(ref.t64[name])) and np.all(np.isfinite(ref.t32[name])), name
    for kernel in kernels:
        if kernel == "persistent" and N > 65536:
            continue
        gate = ref.gate(rows_per_thread(N, kernel))
        for m in ref.models:
            k = SUM_NAMES.index(SQUARES[m])
            worst = min(ref.t64[SQUARES[m]][p] / gate[k] for p in rw.marked)
            out[(kernel, m, "marked/gate")] = worst
            assert worst >= MARK_GATES, (N, kernel, m, worst)
        if N >= 255:
            ratio = gate / np.where(ref.abs_sum > 0, ref.abs_sum, 1.0)        # (a sum whose every term is 0 has the gate 0)
            out[(kernel, "gate/abs")] = float(ratio.max())
            assert np.all(ratio <= CAP), (N, kernel, [(n, float(x)) for n, x in zip(SUM_NAMES, ratio) if x > CAP])
    out["budget/abs"] = float((ref.budget / np.where(ref.abs_sum > 0, ref.abs_sum, 1.0)).max())
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# comparisons
def check_columns(got, ref, names, what):
    """got {column: [N] float32 numpy}.  -> worst error / gate per column (printed by the caller)."""
    ratios = {}
    for c in names:
        a, r64, r32 = np.asarray(got[c], np.float64), ref.cols64[c], ref.cols32[c]
        assert np.array_equal(np.isnan(a), np.isnan(r32)), (what, c, "NaN pattern", np.flatnonzero(np.isnan(a) != np.isnan(r32))[:5])
        if COL_SRC[c][0] in "THO":                            # no transcendental: float32 torch's value
            bad = np.flatnonzero(~((a == r32) | (np.isnan(a) & np.isnan(r32))))
            assert bad.size == 0, (what, c, "differs from float32 torch", bad[:5], a[bad[:5]], r32[bad[:5]])
        fin = ~np.isnan(r32)
        err = np.abs(a - r64)[fin]
        gate = 2.0 * np.abs(r32 - r64)[fin] + COL_REL * np.abs(r64[fin]).max() + 1e-300
        ratios[c] = float((err / gate).max()) if err.size else 0.0
        assert np.all(err <= gate), (what, c, float((err / gate).max()), int(np.argmax(err / gate)))
    return ratios


def check_sums(got, ref, r, live_names, what):
    """got [NSUMS] float64.  Every sum of live_names against the referee at r rows per thread, every other entry exactly 0.
    -> {sum: error / gate}."""
    got = np.asarray(got, np.float64)
    gate = ref.gate(r)
    ratios, bad = {}, []
    for k in range(NSUMS):
        name = SUM_NAMES[k] if k < len(SUM_NAMES) else None
        if name in live_names:
            assert ref.live[k], name
            ratios[name] = abs(got[k] - ref.center[k]) / gate[k] if gate[k] > 0 else (0.0 if got[k] == ref.center[k] else np.inf)
            if not ratios[name] <= 1.0:
                bad.append((name, got[k], ref.center[k], gate[k]))
        else:
            assert got[k] == 0.0, (what, "dead sum", k, name, got[k])
    assert not bad, (what, bad)
    return ratios


def model_sums(models, with_y=True):
    return [s for s in SUM_NAMES if SUM_MODEL[s] in models and (with_y or s not in Y_SUMS)]


# ---------------------------------------------------------------------------------------------------------------------------
# net_f_T, the Euler step (01:767-867)
@functools.lru_cache(maxsize=4)
def euler(N, set_name):
    """-> (rows, {f, t_pred, t_real} float64 numpy of r64, the same of r32).  One row: T_pred[0] = T_out[0] (01:857), f = 0."""
    rw = rows(N)
    _, _, sy = fixture()
    ymn, ysc = O.scaler_affine(sy)
    out = []
    for dtype in (torch.float64, torch.float32):
        real = torch.tensor(rw.real, dtype=dtype)
        if N == 1:
            res = (torch.zeros(1, 1, dtype=dtype), real[:, 5:6], real[:, 5:6])
        else:
            with torch.no_grad():
                res = O.net_f_T(real, torch.tensor(rw.un[:-1]).reshape(-1, 1), ymn, ysc, _lam(param_sets()[set_name], dtype))
        out.append({k: v.double().numpy().reshape(-1) for k, v in zip(("f", "t_pred", "t_real"), res)})
    return rw, out[0], out[1]


def check_series(got, r64, r32, what, exact=False):
    a, r64, r32 = (np.asarray(v, np.float64) for v in (got, r64, r32))
    assert np.array_equal(np.isnan(a), np.isnan(r32)), (what, "NaN pattern")
    if exact:
        assert np.array_equal(a, r32), (what, np.flatnonzero(a != r32)[:5])
    err = np.abs(a - r64)
    gate = 2.0 * np.abs(r32 - r64) + COL_REL * np.abs(r64).max() + 1e-300
    assert np.all(err <= gate), (what, float((err / gate).max()), int(np.argmax(err / gate)))
    return float((err / gate).max())
