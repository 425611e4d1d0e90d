"""Which physics parameter moved: per-window identification of the polarisation and thermal parameters with covariances.

The trainers fit lambda_1..3 and lambda_T1/T3/T5 once, over all normal rows, by tens of thousands of Adam steps and
without an uncertainty.  Here a window of a recording is fitted by Levenberg-Marquardt in a few row passes, and the answer
comes with its covariance, so that "the ohmic resistance rose by 40 % +- 3 % over this segment" can be said.

A *table* is a float64 array of four columns per row:
  voltage  (i, b, E, v): current density, R Tk / F, Nernst voltage (what `volt_pre` of csrc/pinn_physics.h produces) and the
           per-cell target voltage; theta = (r, q, c) = (lambda_1, ln lambda_2, 1 / lambda_3),
           V(theta) = E - b (ln i - q) - i r + 0.5 b log1p(-i c), residual V - v.
           The reciprocal of the limiting current keeps the third Jacobian column alive on windows that show no
           concentration loss: there lambda_3 runs away and its column vanishes, c -> 0 is harmless.
  thermal  (It, mc, T_in, T_out), `therm_pre`'s values; theta = (lambda_T1, lambda_T3, lambda_T5),
           residual T_out - (theta0 It + theta1 mc + 0.5 T_in + theta2): linear, one accepted step.
A row is missing (skipped, not counted) when an entry is not finite, for the voltage model also when i <= 0 or b <= 0; a
gather index outside the table reads nothing.

The solver, its stopping rule (the certificate m: the length of the undamped Gauss-Newton step in the metric of the
parameter covariance, so every component is within m standard errors of the stationary point to first order) and the
status codes are stated once in include/pinn_hip.h; the device backend is csrc/pinn_identify.hip (`pinn_id_fit`, one
workgroup per window), the host backend below is the same statement in float64 numpy.

`voltage_table` / `thermal_table` build tables, `sliding_windows` the windows, `fit_windows` / `fit_baseline` fit them
(`WindowFit`), `drift` compares windows with a baseline (z per parameter, joint Wald statistic and its chi-square tail),
`ParameterTracker` is the online form next to `FaultDiagnoser.update`.

Importing this module needs numpy only; torch and the HIP library are loaded when a device path runs.
"""
import ctypes
import math

import numpy as np

from ._device import _as_numpy, _is_tensor, _pick_backend

MAX_WINDOW, ONCHIP_ROWS, FIT_WORDS, NORMAL_WORDS = 65536, 4096, 16, 12
MODELS = {"voltage": 0, "thermal": 1}
THETA_NAMES = {"voltage": ("r", "q", "c"), "thermal": ("lambda_T1", "lambda_T3", "lambda_T5")}
LAMBDA_OF = {"voltage": ("lambda_1", "lambda_2", "lambda_3"), "thermal": ("lambda_T1", "lambda_T3", "lambda_T5")}
# the reference's initial values (01:453-456, 477-481), as model.LAMBDA_INIT
LAMBDA_START = {"voltage": (0.167897923477715, 2.36682075851268e-06, 2.43414469188443), "thermal": (10.0, 10.0, 10.0)}
# the clamp box of lambda_step_body (csrc/pinn_residuals.hip; 01:992-997)
REFERENCE_BOX = {"voltage": ((0.167 * 0.5, 0.167 * 5), (2.36e-6 * 0.1, 2.36e-6 * 2.1), (2.0, 2.0 * 5.2)),
                 "thermal": ((-10000.0, 10000.0),) * 3}
STATUS = {0: "converged", 1: "max_passes", 2: "stalled", 3: "too_few_rows", 4: "bad_start", 5: "singular", 6: "bad_window"}
TOL, XTOL, MU0, MAX_PASSES = 1e-8, 1e-14, 1e-3, 100
PIVOT_MIN, MU_MIN, MU_MAX = 2.0 ** -40, 1e-15, 1e15
_TRI = ((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2))         # packed upper triangle, column by column (csrc/pinn_rows.h: tri)


def theta_from_lambdas(values, model="voltage"):
    """theta of the three `lambda_*` values of a model: (l1, ln l2, 1 / l3) for the voltage, themselves for the thermal."""
    a = [float(v) for v in values]
    return np.array([a[0], math.log(a[1]), 1.0 / a[2]] if model == "voltage" else a, dtype=np.float64)


def _default_theta0(theta0, model):
    """None: the reference's initial values; a PhysicsInformedNN: its current parameters; else theta itself."""
    if theta0 is None:
        return theta_from_lambdas(LAMBDA_START[model], model)
    if hasattr(theta0, LAMBDA_OF[model][0]):
        return theta_from_lambdas([float(getattr(theta0, n).detach().reshape(-1)[0]) for n in LAMBDA_OF[model]], model)
    return theta0


# ------------------------------------------------------------------ tables
def _p_h2o():
    tc = 55.0
    return 10.0 ** (((-2.1794 + 0.02953 * tc) - 9.1837e-5 * (tc * tc)) + 1.4454e-7 * ((tc * tc) * tc))


def voltage_columns(rows):
    """(i, b, E) of physical rows [n, 8] in float64: `volt_pre` of csrc/pinn_physics.h (01:724-765) without its float32 rounding."""
    r = np.asarray(rows, dtype=np.float64)
    i = r[:, 0] / 270.0 + 1e-5
    tk = r[:, 5] + 273.15
    rt = 8.314 * tk
    p_h2o = _p_h2o()
    tkp = tk ** 1.334
    pp_h2 = 0.5 * ((r[:, 3] / 101.0 + 1.0) / np.exp(1.653 * i / tkp) - p_h2o)
    pp_o2 = (r[:, 4] / 101.0 + 1.0) / np.exp(4.192 * i / tkp) - p_h2o
    e = 220170.0 / 192970.0 - (rt * np.log(p_h2o / (pp_h2 * np.sqrt(pp_o2)))) / 192970.0
    return i, rt / 96485.0, e


def voltage_model(i, b, e, theta):
    """V(theta) per cell, float64."""
    return e - b * (np.log(i) - theta[1]) - i * theta[0] + 0.5 * b * np.log1p(-i * theta[2])


def voltage_table(model, X, x_scal=None, target="measured", y=None):
    """The voltage table [n, 4] = (i, b, E, v).

    With a PhysicsInformedNN: X are normalised rows, the first three columns come from `pinn_residuals_prepare`
    (PINN_RES_V, cache slots 0..2) and v is the network's voltage (target="network", slot 3) or the measured `y`
    (normalised, by default the model's training target), de-normalised and divided by 5 in float64; a device tensor.
    With model=None: X are physical rows [n, 8] and y the stack voltage [V]; a float64 numpy array for the host backend."""
    if target not in ("measured", "network"):
        raise ValueError("target must be 'measured' or 'network'")
    if model is None:
        if target != "measured" or y is None:
            raise ValueError("physical rows need the measured stack voltage y")
        i, b, e = voltage_columns(_as_numpy(X))
        return np.column_stack([i, b, e, _as_numpy(y, np.float64).reshape(-1) / 5.0])
    import torch
    from . import _lib
    xd = model._dev_rows(X)
    with torch.no_grad():
        u = model.net_u(xd)[0].detach().reshape(-1).to(torch.float32).contiguous()
    if y is None:
        y = model.u if (X is model.X or X is model.x) else None
    if y is None and target == "measured":
        raise ValueError("target='measured' needs y for rows other than the model's own")
    yd = u if y is None else (y if _is_tensor(y) else torch.as_tensor(np.asarray(y))).detach().to(xd.device, torch.float32).reshape(-1).contiguous()
    cache = _prepare(model, xd, u, yd, x_scal, _lib.RES_V)
    v = cache[3].to(torch.float64)
    if target == "measured":
        aff = model._affine(model.x_scal if x_scal is None else x_scal)
        v = ((yd.to(torch.float64) - aff.y_min) / aff.y_scale) / 5.0
    return torch.stack([cache[0].to(torch.float64), cache[1].to(torch.float64), cache[2].to(torch.float64), v], dim=1).contiguous()


def thermal_table(model, X, x_scal=None):
    """The thermal table [n, 4] = (It, mc, T_in, T_out): slots 0..3 of the PINN_RES_T cache (a device tensor), or with
    model=None from physical rows [n, 8] in float64 (a numpy array)."""
    if model is None:
        r = _as_numpy(X, np.float64)
        return np.column_stack([(r[:, 0] / 270.0 + 1e-6) * 270.0, r[:, 1] + 1e-6, r[:, 2], r[:, 5]])
    import torch
    from . import _lib
    xd = model._dev_rows(X)
    cache = _prepare(model, xd, None, None, x_scal, _lib.RES_T)
    return cache[:4].to(torch.float64).t().contiguous()


def _prepare(model, xd, u, y, x_scal, flags):
    """The stage cache of `pinn_residuals_prepare`, slot-major: [6, n] float32."""
    import torch
    from . import _lib
    from .model import _ptr, _stream
    n = xd.shape[0]
    x_scal = model.x_scal if x_scal is None else x_scal
    cache = torch.zeros(6, n, dtype=torch.float32, device=xd.device)
    if n > 0:
        rc = model._lib.pinn_residuals_prepare(_ptr(xd), _ptr(u), _ptr(y), ctypes.byref(model._affine(x_scal)), _ptr(model._lambdas()),
                                               flags, n, _ptr(cache), _stream())
        _lib.check(rc, "pinn_residuals_prepare")
    return cache


def sliding_windows(n, length, stride, segments=None):
    """(start, len) of the windows of `length` positions every `stride` inside [0, n); no window crosses a segment
    boundary.  `segments`: ascending segment starts, the first 0, as `rf_series`' seg_starts (None: one segment)."""
    n, length, stride = int(n), int(length), int(stride)
    if length < 1 or stride < 1:
        raise ValueError("length and stride must be positive")
    starts = [0] if segments is None or len(segments) == 0 else [int(s) for s in _as_numpy(segments).reshape(-1)]
    if starts[0] != 0 or any(b <= a for a, b in zip(starts, starts[1:])) or (n > 0 and starts[-1] >= n):
        raise ValueError("segments must begin with 0 and ascend strictly inside the %d positions" % n)
    out = []
    for a, b in zip(starts, starts[1:] + [n]):
        out.extend(range(a, b - length + 1, stride))
    start = np.asarray(out, dtype=np.int64)
    return start, np.full(start.shape, length, dtype=np.int64)


# ------------------------------------------------------------------ the host backend
def _chol3(M, shift, pmin):
    """Cholesky factor (packed) of the packed symmetric M + shift I, or None when a pivot is not above pmin."""
    L = [0.0] * 6
    p = M[0] + shift
    if not p > pmin:
        return None
    L[0] = math.sqrt(p)
    L[1] = M[1] / L[0]
    L[3] = M[3] / L[0]
    p = (M[2] + shift) - L[1] * L[1]
    if not p > pmin:
        return None
    L[2] = math.sqrt(p)
    L[4] = (M[4] - L[3] * L[1]) / L[2]
    p = ((M[5] + shift) - L[3] * L[3]) - L[4] * L[4]
    if not p > pmin:
        return None
    L[5] = math.sqrt(p)
    return L


def _forward(L, b):
    y0 = b[0] / L[0]
    y1 = (b[1] - L[1] * y0) / L[2]
    return [y0, y1, ((b[2] - L[3] * y0) - L[4] * y1) / L[5]]


def _backward(L, y):
    x2 = y[2] / L[5]
    x1 = (y[1] - L[4] * x2) / L[2]
    return [((y[0] - L[1] * x1) - L[3] * x2) / L[0], x1, x2]


def used_rows(rows, model):
    """The rows of a gathered [m, 4] block that are not missing."""
    ok = np.isfinite(rows).all(axis=1)
    if model == "voltage":
        ok &= (rows[:, 0] > 0.0) & (rows[:, 1] > 0.0)
    return rows[ok]


def residual_jacobian(x, theta, model):
    """(r [m], J [m, 3]) of used rows x [m, 4] at theta, float64."""
    if model == "voltage":
        i, b = x[:, 0], x[:, 1]
        ic = i * theta[2]
        with np.errstate(all="ignore"):
            r = (((x[:, 2] - b * (np.log(i) - theta[1])) - i * theta[0]) + (0.5 * b) * np.log1p(-ic)) - x[:, 3]
            J = np.column_stack([-i, b, -((0.5 * b) * i) / (1.0 - ic)])
    else:
        r = x[:, 3] - (((theta[0] * x[:, 0] + theta[1] * x[:, 1]) + 0.5 * x[:, 2]) + theta[2])
        J = np.column_stack([-x[:, 0], -x[:, 1], -np.ones(len(x))])
    return r, J


def _row_pass(x, theta, model):
    """The twelve sums of a pass: A packed [6], g [3], sse, n_used, max i."""
    r, J = residual_jacobian(x, theta, model)
    with np.errstate(all="ignore"):
        s = [float(np.sum(J[:, p] * J[:, q])) for p, q in _TRI] + [float(np.sum(J[:, k] * r)) for k in range(3)]
        s += [float(np.sum(r * r)), float(len(x)), float(np.max(x[:, 0])) if len(x) else -math.inf]
    return s


def _in_domain(theta, imax, model):
    return model != "voltage" or theta[2] * imax < 1.0


def _fit_one_host(x, theta0, model, tol, xtol, mu0, max_passes):
    """One window on the host: the solver of include/pinn_hip.h, word for word.  Returns (fit row [16], normal row [12])."""
    nan = math.nan
    th, tht = [float(v) for v in theta0], [float(v) for v in theta0]
    cur, passes, status, mu, m = [0.0] * NORMAL_WORDS, 0, -1, float(mu0), nan
    sc = C = None
    while status < 0:
        tr = _row_pass(x, tht, model)
        first = passes == 0
        passes += 1
        fine = all(math.isfinite(v) for v in tht) and _in_domain(tht, tr[11], model) and all(math.isfinite(v) for v in tr[:10])
        if first or (fine and tr[9] < cur[9]):
            th, cur = list(tht), tr
            if first:
                if cur[10] < 4:
                    status = 3
                elif not fine:
                    status = 4
            else:
                mu = max(mu / 10.0, MU_MIN)
        else:
            mu *= 10.0
            if mu > MU_MAX:
                status = 2
        if status >= 0:
            break
        if not (cur[0] > 0.0 and cur[2] > 0.0 and cur[5] > 0.0):
            status = 5
            break
        sc = [1.0 / math.sqrt(cur[0]), 1.0 / math.sqrt(cur[2]), 1.0 / math.sqrt(cur[5])]
        C = [1.0, (cur[1] * sc[0]) * sc[1], 1.0, (cur[3] * sc[0]) * sc[2], (cur[4] * sc[1]) * sc[2], 1.0]
        gs = [cur[6 + k] * sc[k] for k in range(3)]
        L = _chol3(C, 0.0, PIVOT_MIN)
        if L is None:
            status = 5
            break
        if cur[9] == 0.0:
            m, status = 0.0, 0
            break
        y = _forward(L, gs)
        m = math.sqrt(((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]) / (cur[9] / (cur[10] - 3.0)))
        if m <= tol:
            status = 0
            break
        if passes >= max_passes:
            status = 1
            break
        L = _chol3(C, mu, 0.0)
        z = _backward(L, _forward(L, gs))
        d = [-(z[k] * sc[k]) for k in range(3)]
        tht = [th[k] + d[k] for k in range(3)]
        if all(abs(d[k]) <= xtol * (abs(th[k]) + xtol) for k in range(3)):
            status = 0
    out = [nan] * 12 + [cur[10], float(passes), float(status), 0.0]
    if status not in (3, 4):
        out[0:3] = th
        out[9], out[11] = cur[9], mu
    if status <= 2:
        out[10] = m
        L = _chol3(C, 0.0, PIVOT_MIN)
        s2 = cur[9] / (cur[10] - 3.0)
        for q in range(3):
            z = _backward(L, _forward(L, [1.0 if k == q else 0.0 for k in range(3)]))
            for p in range(q + 1):
                out[3 + q * (q + 1) // 2 + p] = s2 * ((z[p] * sc[p]) * sc[q])
    return out, cur


def _fit_host(table, cols, row_index, start, length, theta0, model, tol, xtol, mu0, max_passes):
    a = _as_numpy(table, np.float64)
    if a.ndim != 2:
        raise ValueError("the table must be a 2-D array")
    a = a[:, list(cols)]
    if row_index is not None:
        ridx = _as_numpy(row_index, np.int64).reshape(-1)
        n = len(ridx)
    else:
        ridx, n = None, a.shape[0]
    W = len(start)
    fit, normal = np.full((W, FIT_WORDS), np.nan), np.full((W, NORMAL_WORDS), np.nan)
    for w in range(W):
        s, l = int(start[w]), int(length[w])
        if s < 0 or l < 0 or l > MAX_WINDOW or s > n - l:
            fit[w, 12:] = (0.0, 0.0, 6.0, 0.0)
            continue
        if ridx is None:
            rows = a[s:s + l]
        else:
            idx = ridx[s:s + l]
            ok = (idx >= 0) & (idx < a.shape[0])
            rows = np.full((l, 4), np.nan)
            rows[ok] = a[idx[ok]]
        fit[w], normal[w] = _fit_one_host(used_rows(rows, model), theta0[w if theta0.shape[0] > 1 else 0], model, tol, xtol, mu0, max_passes)
    return fit, normal


# ------------------------------------------------------------------ the device backend
def _fit_device(table, cols, row_index, start, length, theta0, model, tol, xtol, mu0, max_passes):
    from ._device import _dev_f64_rows, _dev_vec, _torch_lib, call
    torch, _lib, _ = _torch_lib()
    arr = _dev_f64_rows(torch, table)
    dev = arr.device
    if max(cols) >= arr.shape[1] or min(cols) < 0:
        raise ValueError("the table has %d columns, column %d is asked for" % (arr.shape[1], max(cols)))
    ridx = _dev_vec(torch, row_index, torch.int64, dev)
    n = arr.shape[0] if ridx is None else ridx.numel()
    ld = arr.stride(0) if arr.shape[0] > 1 else max(arr.shape[1], 1)
    ws, wl = _dev_vec(torch, start, torch.int64, dev), _dev_vec(torch, length, torch.int64, dev)
    W = ws.numel()
    th0 = _dev_vec(torch, theta0, torch.float64, dev)
    fit = torch.empty(W, FIT_WORDS, dtype=torch.float64, device=dev)
    normal = torch.empty(W, NORMAL_WORDS, dtype=torch.float64, device=dev)
    opts = _lib.IdOpts(float(tol), float(xtol), float(mu0), int(max_passes), 0)
    call("pinn_id_fit", arr, ld, arr.shape[0], (ctypes.c_int * 4)(*cols), MODELS[model], ridx, n, ws, wl, W, th0,
         3 if theta0.shape[0] > 1 else 0, ctypes.byref(opts), fit, normal)
    return fit, normal


# ------------------------------------------------------------------ results
class WindowFit:
    """The fits of W windows.  theta [W, 3], cov [W, 3, 3], se [W, 3], sse, m, mu [W], n_used, passes, status [W] (integers),
    normal [W, 12] (A packed, g, sse, n_used, max i at the returned theta); numpy arrays on the host, whichever backend ran."""

    def __init__(self, fit, normal, model, backend):
        fit, normal = _as_numpy(fit, np.float64), _as_numpy(normal, np.float64)
        self.model, self.backend, self.names = model, backend, THETA_NAMES[model]
        self.raw, self.normal = fit, normal
        self.theta = fit[:, 0:3].copy()
        self.cov = np.empty((len(fit), 3, 3))
        for k, (p, q) in enumerate(_TRI):
            self.cov[:, p, q] = self.cov[:, q, p] = fit[:, 3 + k]
        with np.errstate(invalid="ignore"):
            self.se = np.sqrt(np.stack([self.cov[:, k, k] for k in range(3)], axis=1))
        self.sse, self.m, self.mu = fit[:, 9].copy(), fit[:, 10].copy(), fit[:, 11].copy()
        self.n_used, self.passes, self.status = (fit[:, 12].astype(np.int64), fit[:, 13].astype(np.int64), fit[:, 14].astype(np.int64))

    def __len__(self):
        return len(self.theta)

    @property
    def converged(self):
        return self.status == 0

    @property
    def no_limit(self):
        """Voltage model: c <= 0, no concentration loss seen, lambda_3 reported as inf."""
        return (self.theta[:, 2] <= 0.0) if self.model == "voltage" else np.zeros(len(self), dtype=bool)

    @property
    def params(self):
        """{lambda name: (value [W], standard error [W])}: the reference's parameters, the errors by the delta method."""
        t, se = self.theta, self.se
        if self.model == "thermal":
            return {n: (t[:, k].copy(), se[:, k].copy()) for k, n in enumerate(LAMBDA_OF["thermal"])}
        with np.errstate(all="ignore"):
            l2 = np.exp(t[:, 1])
            pos = t[:, 2] > 0.0
            l3 = np.where(pos, 1.0 / np.where(pos, t[:, 2], 1.0), np.where(np.isnan(t[:, 2]), np.nan, np.inf))
            se3 = np.where(pos, se[:, 2] / np.where(pos, t[:, 2], 1.0) ** 2, np.where(np.isnan(t[:, 2]), np.nan, np.inf))
        return {"lambda_1": (t[:, 0].copy(), se[:, 0].copy()), "lambda_2": (l2, l2 * se[:, 1]), "lambda_3": (l3, se3)}

    @property
    def in_reference_box(self):
        """[W, 3]: whether each lambda lies inside the clamp box of the reference's trainers (the fit itself is unconstrained)."""
        p = self.params
        with np.errstate(invalid="ignore"):
            return np.stack([(p[n][0] >= lo) & (p[n][0] <= hi) for n, (lo, hi) in zip(LAMBDA_OF[self.model], REFERENCE_BOX[self.model])], axis=1)


def fit_windows(table, start, length, model="voltage", theta0=None, tol=TOL, xtol=XTOL, max_passes=MAX_PASSES, backend="auto",
                row_index=None, cols=None, mu0=MU0):
    """Fit every window (start[w], length[w]) of the table's gathered positions; returns a WindowFit.

    theta0: None (the reference's initial values), a PhysicsInformedNN (its current parameters), [3] for all windows or
    [W, 3].  backend: "auto" (a tensor stays where it is, as the sibling modules), "device", "host" or its synonym "numpy".
    `row_index` is a gather list over the table's rows, `cols` its four columns (default 0..3)."""
    if model not in MODELS:
        raise ValueError("model must be 'voltage' or 'thermal'")
    backend = _pick_backend("host" if backend == "numpy" else backend, table)
    start, length = _as_numpy(start, np.int64).reshape(-1), _as_numpy(length, np.int64).reshape(-1)
    if start.shape != length.shape:
        raise ValueError("start and length must have one entry per window")
    cols = [0, 1, 2, 3] if cols is None else [int(c) for c in cols]
    if len(cols) != 4:
        raise ValueError("a table has four columns")
    th0 = np.asarray(_as_numpy(_default_theta0(theta0, model)), dtype=np.float64)
    th0 = th0.reshape(1, 3) if th0.size == 3 else th0.reshape(-1, 3)
    if th0.shape[0] not in (1, len(start)):
        raise ValueError("theta0 must be [3] or [n_windows, 3]")
    if not (tol > 0 and xtol > 0 and mu0 > 0 and max_passes >= 0):
        raise ValueError("tol, xtol and mu0 must be positive, max_passes not negative")
    if len(start) == 0:
        return WindowFit(np.empty((0, FIT_WORDS)), np.empty((0, NORMAL_WORDS)), model, backend)
    run = _fit_device if backend == "device" else _fit_host
    fit, normal = run(table, cols, row_index, start, length, th0, model, tol, xtol, mu0, int(max_passes))
    return WindowFit(fit, normal, model, backend)


def fit_baseline(table, model="voltage", row_index=None, **kw):
    """One window over all positions (at most 65536): the baseline the windows are compared with."""
    n = len(row_index) if row_index is not None else table.shape[0]
    if n > MAX_WINDOW:
        raise ValueError("a single fit takes at most %d rows, got %d: pass a row_index that thins them" % (MAX_WINDOW, n))
    return fit_windows(table, [0], [n], model=model, row_index=row_index, **kw)


def chi2_sf3(x):
    """The upper tail of chi-square with 3 degrees of freedom in closed form: erfc(sqrt(x/2)) + sqrt(2 x / pi) exp(-x / 2)."""
    x = float(x)
    if math.isnan(x):
        return math.nan
    if x <= 0.0:
        return 1.0
    return math.erfc(math.sqrt(0.5 * x)) + math.sqrt(2.0 * x / math.pi) * math.exp(-0.5 * x)


def drift(fit, baseline, index=0):
    """Windows against window `index` of `baseline`, on the host in float64: {"delta" [W, 3], "z" [W, 3] =
    delta / sqrt(se_w^2 + se_ref^2), "wald" [W] = delta' (cov_w + cov_ref)^-1 delta, "p" [W] its chi-square(3) tail}."""
    ref_t, ref_c, ref_se = baseline.theta[index], baseline.cov[index], baseline.se[index]
    delta = fit.theta - ref_t
    with np.errstate(invalid="ignore", divide="ignore"):
        z = delta / np.sqrt(fit.se ** 2 + ref_se ** 2)
    wald = np.full(len(fit), np.nan)
    for w in range(len(fit)):
        S = fit.cov[w] + ref_c
        if np.all(np.isfinite(S)) and np.all(np.isfinite(delta[w])):
            try:
                wald[w] = float(delta[w] @ np.linalg.solve(S, delta[w]))
            except np.linalg.LinAlgError:
                pass
    return {"delta": delta, "z": z, "wald": wald, "p": np.array([chi2_sf3(v) for v in wald])}


class ParameterTracker:
    """The online form: keeps the last `length` table rows in a ring and refits them at every update, warm-started from the
    previous theta; each update is one fit of one window read through a gather list (on the device one `pinn_id_fit` launch).

    update(chunk) -> {"theta", "se", "z", "wald", "p", "status", "n_used", "blamed"}; z is against the baseline, `blamed` the
    name of the parameter with the largest |z| (None while the fit has no covariance)."""

    def __init__(self, baseline, length, model=None, backend="auto", tol=TOL, xtol=XTOL, max_passes=MAX_PASSES):
        self.model = baseline.model if model is None else model
        if not 4 <= int(length) <= MAX_WINDOW:
            raise ValueError("length must lie in 4 .. %d" % MAX_WINDOW)
        self.baseline, self.length, self.backend = baseline, int(length), backend
        self.opts = dict(tol=tol, xtol=xtol, max_passes=max_passes)
        self.ring, self.head, self.count = None, 0, 0
        self.theta = baseline.theta[0].copy()
        self.theta_start, self.last = self.theta.copy(), None

    def _store(self, chunk):
        L = self.length
        if self.ring is None:
            self.backend = _pick_backend("host" if self.backend == "numpy" else self.backend, chunk)
            if self.backend == "device":
                import torch
                self._torch = torch
                dev = chunk.device if _is_tensor(chunk) and chunk.is_cuda else "cuda"
                self.ring = torch.full((L, 4), float("nan"), dtype=torch.float64, device=dev)
            else:
                self.ring = np.full((L, 4), np.nan)
        if self.backend == "device":
            torch = self._torch
            c = (chunk if _is_tensor(chunk) else torch.from_numpy(np.asarray(chunk, dtype=np.float64))).detach().to(self.ring.device, torch.float64)
            c = c.reshape(-1, 4)[-L:]
            k = c.shape[0]
            pos = (torch.arange(k, device=self.ring.device) + self.head) % L
        else:
            c = _as_numpy(chunk, np.float64).reshape(-1, 4)[-L:]
            k = c.shape[0]
            pos = (np.arange(k) + self.head) % L
        self.ring[pos] = c
        self.head = (self.head + k) % L
        self.count = min(self.count + k, L)

    def window_index(self):
        """The gather list of the trailing window, oldest row first."""
        return (self.head - self.count + np.arange(self.count)) % self.length

    def update(self, chunk):
        self._store(chunk)
        self.theta_start = self.theta.copy()
        f = fit_windows(self.ring, [0], [self.count], model=self.model, theta0=self.theta_start, backend=self.backend,
                        row_index=self.window_index(), **self.opts)
        d = drift(f, self.baseline)
        if f.status[0] <= 2:
            self.theta = f.theta[0].copy()
        z = d["z"][0]
        blamed = THETA_NAMES[self.model][int(np.nanargmax(np.abs(z)))] if np.any(np.isfinite(z)) else None
        self.last = f
        return {"theta": f.theta[0], "se": f.se[0], "z": z, "wald": d["wald"][0], "p": d["p"][0], "status": int(f.status[0]),
                "n_used": int(f.n_used[0]), "blamed": blamed}
