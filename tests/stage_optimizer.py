"""Float64 referee of the physics-stage optimizer (gradients from the 32 row sums -> Adam -> clamp), shared by
test_stage_optimizer_host.py (CPU: the referee is torch's Adam, its no-gradient list is autograd's, and a float32 twin of the
kernel's operation order stays inside the bounds) and test_gpu_stage_optimizer.py (GPU: pinn_lambda_step and the persistent
pinn_lambda_stage_run against it).

What is computed.  include/pinn_hip.h and the reference define, for n rows and the stage's sums S:
    PINN_STAGE_LAMBDA_F    physics = S[FV2] / n, total = physics + S[YU2] / n, g_k = 2 S[FV_Dk] / n                       (k = 1..3)
    PINN_STAGE_LAMBDA_PM   physics = S[YV2] / n, total = physics + S[YU2] / n, g_k = -(2 / n) 5 vn_scale S[YV_Dk]
    PINN_STAGE_THERMAL     total = physics = S[FT2] / n, g_T1, g_T3, g_T5 = 2 S[FT_D1], S[FT_D3], S[FT_D5] / n
    PINN_STAGE_HYDROGEN    total = physics = S[FH2] / n, g_Hk = 2 S[FH_Dk] / n                                           (k = 1..3)
    PINN_STAGE_OXYGEN      total = physics = S[FO2] / n, g_Ok = 2 S[FO_Dk] / n                                           (k = 1..3)
then torch's single-tensor Adam with the bias corrections 1 - 0.9^step, 1 - 0.999^step in double,
    m' = b1 m + (1 - b1) g,  v' = b2 v + (1 - b2) g^2,  denom = sqrt(v') / sqrt(bc2) + eps,  p' = p - (lr / bc1) (m' / denom),
and after the step p' = clamp(p', lo, hi).  A parameter without a gradient (lambda_4, lambda_T2, lambda_T4, lambda_H4, lambda_O4: GRAD_SUM
has no entry for it) is clamped and nothing else: neither it nor its moments move.

Where the numbers come from.  Parameter order, rates and bounds are O.STAGES' (oracle/pinn_oracle.py); a bound is the float32 value of
the oracle's double expression (np.float32(0.167 * 0.5), ...).  The five constants the kernel multiplies by enter as their float32
values promoted to double (KERNEL); TORCH holds the double values, with which the step is O.AdamState's.

Bounds.  csrc/pinn_residuals.hip is built with -ffp-contract=off and HIP's float divide and sqrtf are correctly rounded, so every
float32 operation of the kernel is one rounding of relative size u = 2^-24.  Counting them against the referee, which rounds nothing:
    g      (float) of a double expression                                                                         1 u
    m'     0.9f m: 1;  0.1f g: 1 + 1 (g's own);  the addition: 1 on each term          <= 3 u (|0.9 m| + |0.1 g|) = 3 u S_m
    v'     g g: 2 + 1;  0.001f (.): + 1;  0.999f v: 1;  the addition: + 1 on each term  <= 5 u v'     (every term is positive)
    denom  sqrt of v': 2.5;  sqrtf: + 1;  (float) sqrt(bc2): + 1;  the divide: + 1;  + eps: + 1                  <= 6.5 u denom
    step   m' / denom: 3 u S_m / denom + (6.5 + 1) u |m'| / denom <= 10.5 u S_m / denom  (|m'| <= S_m);
           (float)(lr / bc1): + 1;  the product: + 1                                       <= 12.5 u step_size S_m / denom, taken as 16
    p'     the subtraction: u |p'|
Hence |p_kernel - p'| <= u (|p'| + 16 step_size S_m / denom), |m_kernel - m'| <= 3 u S_m, |v_kernel - v'| <= 5 u v' to first order in u
(the 3.5 units between 12.5 and 16 hold the second-order terms many times over).  The two losses are one rounding each plus, for the voltage stages,
the rounding of their sum: 2 u of the referee's value.
"""
import numpy as np

import pinn_oracle as O

U = 2.0 ** -24
P_UNITS = 16.0          # roundings allowed on the step (the count gives 12.5)
M_UNITS = 3.0
V_UNITS = 5.0
LOSS_UNITS = 2.0

NLAMBDA, NSUMS = 17, 32
# the enums of include/pinn_hip.h
STAGE_LAMBDA_PM, STAGE_LAMBDA_F, STAGE_THERMAL, STAGE_HYDROGEN, STAGE_OXYGEN = range(5)
STAGE_IDS = (STAGE_LAMBDA_PM, STAGE_LAMBDA_F, STAGE_THERMAL, STAGE_HYDROGEN, STAGE_OXYGEN)
STAGE_KEY = {STAGE_LAMBDA_PM: "lambda", STAGE_LAMBDA_F: "lambda", STAGE_THERMAL: "thermal", STAGE_HYDROGEN: "hydrogen", STAGE_OXYGEN: "oxygen"}
STAGE_KIND = {STAGE_LAMBDA_PM: "V", STAGE_LAMBDA_F: "V", STAGE_THERMAL: "T", STAGE_HYDROGEN: "H", STAGE_OXYGEN: "O"}
SUM_NAMES = ["FV2", "FV_D1", "FV_D2", "FV_D3", "YV2", "YV_D1", "YV_D2", "YV_D3", "YU2",
             "FT2", "FT_D1", "FT_D3", "FT_D5", "FT_ABS", "FH2", "FH_D1", "FH_D2", "FH_D3", "ACTH", "TGTH",
             "FO2", "FO_D1", "FO_D2", "FO_D3", "ACTO", "TGTO"]
S = {n: i for i, n in enumerate(SUM_NAMES)}
# the sums a stage kind's row pass writes (first, last); the rest of d_sums is 0
LIVE = {"V": ("FV2", "YU2"), "T": ("FT2", "FT_ABS"), "H": ("FH2", "TGTH"), "O": ("FO2", "TGTO")}

# parameter -> the sum its gradient is taken from; a trainable parameter of O.STAGES that is missing here has no gradient
GRAD_SUM = {
    STAGE_LAMBDA_PM: {"lambda_1": "YV_D1", "lambda_2": "YV_D2", "lambda_3": "YV_D3"},
    STAGE_LAMBDA_F: {"lambda_1": "FV_D1", "lambda_2": "FV_D2", "lambda_3": "FV_D3"},
    STAGE_THERMAL: {"lambda_T1": "FT_D1", "lambda_T3": "FT_D3", "lambda_T5": "FT_D5"},
    STAGE_HYDROGEN: {"lambda_H1": "FH_D1", "lambda_H2": "FH_D2", "lambda_H3": "FH_D3"},
    STAGE_OXYGEN: {"lambda_O1": "FO_D1", "lambda_O2": "FO_D2", "lambda_O3": "FO_D3"},
}
PHYSICS_SUM = {STAGE_LAMBDA_PM: "YV2", STAGE_LAMBDA_F: "FV2", STAGE_THERMAL: "FT2", STAGE_HYDROGEN: "FH2", STAGE_OXYGEN: "FO2"}

# (b1, 1 - b1, b2, 1 - b2, eps): what the kernel multiplies by, and torch's doubles
KERNEL = tuple(float(np.float32(c)) for c in (0.9, 0.1, 0.999, 0.001, 1e-8))
TORCH = (0.9, 1 - 0.9, 0.999, 1 - 0.999, 1e-8)


def stage_names(stage):
    return list(O.STAGES[STAGE_KEY[stage]][0])


def stage_index(stage):
    """Slots of the stage's parameters in the 17-vector, in optimizer order."""
    return [O.LAMBDA_NAMES.index(n) for n in stage_names(stage)]


def stage_rate(stage):
    """(lr0, gamma) of the stage's trainer."""
    return O.STAGES[STAGE_KEY[stage]][1], O.STAGES[STAGE_KEY[stage]][2]


def stage_bounds(stage):
    """[(lo, hi)] as float32 values of the oracle's double expressions."""
    return [(np.float32(lo), np.float32(hi)) for lo, hi in O.STAGES[STAGE_KEY[stage]][3]]


def no_grad_names(stage):
    return [n for n in stage_names(stage) if n not in GRAD_SUM[stage]]


def live_mask(kind):
    m = np.zeros(NSUMS, dtype=bool)
    m[S[LIVE[kind][0]]:S[LIVE[kind][1]] + 1] = True
    return m


def gradients(stage, sums, n, vn_scale):
    """{name: dLoss/dname} in float64 for the parameters that have one, and (total, physics)."""
    sums = np.asarray(sums, dtype=np.float64)
    n = float(n)
    if stage == STAGE_LAMBDA_PM:
        g = {p: -(2.0 / n) * 5.0 * float(np.float32(vn_scale)) * sums[S[s]] for p, s in GRAD_SUM[stage].items()}
    else:
        g = {p: 2.0 * sums[S[s]] / n for p, s in GRAD_SUM[stage].items()}
    physics = sums[S[PHYSICS_SUM[stage]]] / n
    total = physics + sums[S["YU2"]] / n if stage in (STAGE_LAMBDA_PM, STAGE_LAMBDA_F) else physics
    return g, (total, physics)


def adam_core(g, p, m, v, lr, step, consts=KERNEL):
    """One Adam step of float64 arrays, elementwise (lr and step may be arrays): p', m', v' and the three bounds' ingredients."""
    b1, c1, b2, c2, eps = consts
    g, p, m, v = (np.asarray(a, dtype=np.float64) for a in (g, p, m, v))
    step = np.asarray(step, dtype=np.float64)
    bc1 = 1.0 - np.power(0.9, step)
    bc2 = 1.0 - np.power(0.999, step)
    step_size = np.asarray(lr, dtype=np.float64) / bc1
    m1 = m * b1 + g * c1
    v1 = v * b2 + (g * g) * c2
    denom = np.sqrt(v1) / np.sqrt(bc2) + eps
    p1 = p - step_size * (m1 / denom)
    s_m = np.abs(b1 * m) + np.abs(c1 * g)
    unit_step = U * step_size * s_m / denom          # one rounding on the step; bound_p allows P_UNITS of them and u |p'|
    return {"p": p1, "m": m1, "v": v1, "S_m": s_m, "unit_step": unit_step, "bound_p": U * np.abs(p1) + P_UNITS * unit_step,
            "bound_m": M_UNITS * U * s_m, "bound_v": V_UNITS * U * v1}


def referee_step(stage, sums, n, vn_scale, lr, step, lam, adam, consts=KERNEL):
    """One optimizer step of a stage in float64.

    sums float64[32]; lr: the float32 rate of the ABI; step 1-based; lam float32[17]; adam float32[34] (17 first moments, then 17 second).
    Returns a dict of float64 arrays over the 17 slots -- lam (after the clamp), lam_step (before it), m, v, and per slot S_m, bound_p,
    bound_m, bound_v (0 where the stage has no gradient) -- with loss = (total, physics), idx (the stage's slots in optimizer order)
    and has_grad (per entry of idx).  Slots of other stages are passed through."""
    lam = np.asarray(lam, dtype=np.float64).copy()
    adam = np.asarray(adam, dtype=np.float64)
    assert lam.shape == (NLAMBDA,) and adam.shape == (2 * NLAMBDA,)
    m, v = adam[:NLAMBDA].copy(), adam[NLAMBDA:].copy()
    g, loss = gradients(stage, sums, n, vn_scale)
    names, idx = stage_names(stage), stage_index(stage)
    out = {k: np.zeros(NLAMBDA) for k in ("S_m", "unit_step", "bound_p", "bound_m", "bound_v")}
    lam_step = lam.copy()
    has_grad = []
    for name, i in zip(names, idx):
        has_grad.append(name in g)
        if name not in g:          # torch skips a parameter whose .grad is None
            continue
        r = adam_core(g[name], lam[i], m[i], v[i], float(np.float32(lr)), step, consts)
        lam_step[i], m[i], v[i] = r["p"], r["m"], r["v"]
        for k in out:
            out[k][i] = r[k]
    clamped = lam_step.copy()
    for i, (lo, hi) in zip(idx, stage_bounds(stage)):
        clamped[i] = np.clip(lam_step[i], float(lo), float(hi))          # NaN stays NaN, as torch.clamp keeps it
    out.update(lam=clamped, lam_step=lam_step, m=m, v=v, loss=loss, idx=idx, has_grad=has_grad)
    return out


def mirror_core(g, p, m, v, lr, step):
    """The kernel's operation order in numpy float32, elementwise: one rounding per operation, as -ffp-contract=off compiles it.
    g float64 (the double expression the kernel casts), p, m, v, lr float32.  A yardstick for the bounds, not an expected bit pattern."""
    f = np.float32
    g = np.asarray(g, dtype=np.float64).astype(f)
    p, m, v, lr = (np.asarray(a, dtype=f) for a in (p, m, v, lr))
    step = np.asarray(step, dtype=np.float64)
    bc1 = 1.0 - np.power(0.9, step)
    bc2 = 1.0 - np.power(0.999, step)
    step_size = (lr.astype(np.float64) / bc1).astype(f)
    bc2_sqrt = np.sqrt(bc2).astype(f)
    m1 = (m * f(0.9)).astype(f) + (g * f(0.1)).astype(f)
    v1 = (v * f(0.999)).astype(f) + ((g * g).astype(f) * f(0.001)).astype(f)
    denom = (np.sqrt(v1).astype(f) / bc2_sqrt).astype(f) + f(1e-8)
    p1 = p - (step_size * (m1 / denom).astype(f)).astype(f)
    assert m1.dtype == f and v1.dtype == f and denom.dtype == f and p1.dtype == f
    return p1, m1, v1


def ulps(a, b):
    """Distance of two float32 arrays in units in the last place (of the ordered integer line; 0 for equal bits)."""
    def key(x):
        i = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
