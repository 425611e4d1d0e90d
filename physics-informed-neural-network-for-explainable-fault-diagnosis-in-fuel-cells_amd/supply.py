"""Which supply parameter moved: the hydrogen and oxygen excess-ratio laws fitted per window, breakpoint included.

Both supply models of the reference are one law (`hydrogen_target` / `oxygen_target` of csrc/pinn_physics.h; 01:697-701, 586-590),

    target(It) = l1 + l2 min(It, l3) / 100,

fitted against the measured excess ratio `act`, the flow over the stoichiometric flow (`hydrogen_pre` / `oxygen_pre`).  The
trainers fit it once, over all normal rows, by thousands of Adam steps and without an uncertainty; `identify` cannot take it
over, because the objective is only piecewise smooth in l3 and has a local minimum at every data point.  Here a window is
fitted exactly: for a fixed split of the rows sorted by current the model is linear, all splits are evaluated from running
sums, and the optimum is one of at most 2 m candidates (include/pinn_hip.h, section pinn_bp_fit, states the solver once).

A *table* is a float64 array of two columns per row, (x, y) = (It [A], act); theta = (a, b, c) = (l1, l2, l3).  A row is
missing (skipped, not counted) when an entry is not finite; a gather index outside the table reads nothing.

What is not part of the fit: the oxygen target's clamp to [1.05, 15] and the 10 x penalty on act < 1 do not depend on theta
(`inside_oxygen_clamp` says whether the fitted law stays inside the clamp on the window's currents).  The reference's
|lambda_O3| means that c is reported non-negative: it is a knot of, or lies between, the window's own currents.

`flow_table` builds tables, `fit_breakpoints` / `fit_breakpoint_baseline` fit them (`BreakpointFit`, which `identify.drift`
takes as it takes a `WindowFit`), `SupplyTracker` is the online form next to `identify.ParameterTracker`.  The device
backend is csrc/pinn_breakpoint.hip (`pinn_bp_fit`, one workgroup per window), the host backend below the same solver in
float64 numpy.

Importing this module needs numpy only; torch and the HIP library are loaded when a device path runs.
"""
import ctypes
import math

import numpy as np

from ._device import _as_numpy, _is_tensor, _pick_backend
from .identify import PIVOT_MIN, _TRI, _backward, _chol3, _forward, _prepare, drift, sliding_windows  # noqa: F401

MAX_WINDOW, FIT_WORDS = 4096, 24
Q95 = 3.841458820694124                                          # the 95 % point of chi-square with one degree of freedom
GASES = ("hydrogen", "oxygen")
THETA_NAMES = ("l1", "l2", "l3")
LAMBDA_OF = {"hydrogen": ("lambda_H1", "lambda_H2", "lambda_H3"), "oxygen": ("lambda_O1", "lambda_O2", "lambda_O3")}
KIND = {0: "free", 1: "knot", 2: "line", 3: "constant"}
STATUS = {0: "ok", 3: "too_few_rows", 5: "singular", 6: "bad_window", 7: "one_current"}
OXYGEN_CLAMP = (1.05, 15.0)


# ------------------------------------------------------------------ tables
def flow_columns(rows, gas):
    """(It, act) of physical rows [n, 8] in float64: `hydrogen_pre` / `oxygen_pre` of csrc/pinn_physics.h (01:660-667, 564-566)
    without their float32 rounding."""
    if gas not in GASES:
        raise ValueError("gas must be 'hydrogen' or 'oxygen'")
    r = np.asarray(rows, dtype=np.float64)
    It = (r[:, 0] / 270.0 + 1e-5) * 270.0
    if gas == "hydrogen":
        Q = np.maximum((((It / 192970.0) * 5.0) * 22.4) * 60.0, 1e-8)
        return It, (r[:, 6] + 1e-6) / Q
    Q = np.maximum((((It * 5.0) / 385940.0) * 22.4) * 60.0, 1e-8)
    return It, ((r[:, 7] + 1e-6) * 0.21) / Q


def flow_table(model, X, gas, x_scal=None):
    """The supply table [n, 2] = (It, act) of a gas.

    With a PhysicsInformedNN: X are normalised rows and the columns are slots 0..1 of the PINN_RES_H / PINN_RES_O stage cache
    of `pinn_residuals_prepare`; a float64 device tensor.  With model=None: X are physical rows [n, 8]; a float64 numpy array."""
    if gas not in GASES:
        raise ValueError("gas must be 'hydrogen' or 'oxygen'")
    if model is None:
        return np.column_stack(flow_columns(_as_numpy(X), gas))
    import torch
    from . import _lib
    xd = model._dev_rows(X)
    cache = _prepare(model, xd, None, None, x_scal, _lib.RES_H if gas == "hydrogen" else _lib.RES_O)
    return cache[:2].to(torch.float64).t().contiguous()


def supply_law(x, theta):
    """a + b min(x, c) / 100 in float64; c = inf is the line."""
    x = np.asarray(x, dtype=np.float64)
    return theta[0] + theta[1] * (np.minimum(x, theta[2]) / 100.0)


# ------------------------------------------------------------------ the host backend
def _empty_row(n_used, status):
    out = [math.nan] * 10 + [0.0, 0.0, float(n_used), 0.0, float(status)] + [math.nan] * 6 + [0.0] * 3
    return out


def _knot(P, T, m, z, two):
    """Vectorised over k: (sse, alpha, beta, constant) of the knot candidates from prefix sums P [m, 6] and totals T [6]."""
    rem = m - P[:, 0]
    Su, Suu, Suy = P[:, 1] + rem * z, P[:, 3] + rem * (z * z), P[:, 4] + z * (T[2] - P[:, 2])
    with np.errstate(all="ignore"):
        Duu, Duy, Dyy = Suu - Su * Su / m, Suy - Su * T[2] / m, T[5] - T[2] * T[2] / m
        lin = two & (Duu > 0.0)
        beta = np.where(lin, Duy / np.where(lin, Duu, 1.0), 0.0)
        alpha = np.where(lin, (T[2] - beta * Su) / m, T[2] / m)
        sse = np.where(lin, Dyy - Duy * Duy / np.where(lin, Duu, 1.0), Dyy)
    return sse, alpha, beta, ~lin


def _fit_one_host(x, y, q):
    """One window on the host: the solver of include/pinn_hip.h (section pinn_bp_fit).  x, y: the used rows in position order."""
    nan, inf = math.nan, math.inf
    m = len(x)
    if m < 4:
        return _empty_row(m, 3)
    order = np.argsort(x, kind="stable")                         # by (x, position)
    xs, ys = x[order], y[order]
    dm = float(m)
    with np.errstate(all="ignore"):
        zbar, ybar = float(np.sum(xs / 100.0)) / dm, float(np.sum(ys)) / dm
        z, yc = xs / 100.0 - zbar, ys - ybar
        P = np.cumsum(np.column_stack([np.ones(m), z, yc, z * z, z * yc, yc * yc]), axis=0)
        T = P[-1]
        valid = np.append(xs[:-1] < xs[1:], True)
        two = xs > xs[0]
        ks = np.arange(1, m + 1)
        s_knot, alpha, beta, constant = _knot(P, T, dm, z, two)
        # free candidates
        dk, nr = P[:, 0], dm - P[:, 0]
        nr = np.where(nr > 0, nr, 1.0)
        Lzz, Lzy, Lyy = P[:, 3] - P[:, 1] * P[:, 1] / dk, P[:, 4] - P[:, 1] * P[:, 2] / dk, P[:, 5] - P[:, 2] * P[:, 2] / dk
        bl = Lzy / Lzz
        al = (P[:, 2] - bl * P[:, 1]) / dk
        ry = T[2] - P[:, 2]
        s_free = (Lyy - Lzy * Lzy / Lzz) + ((T[5] - P[:, 5]) - ry * ry / nr)
        c_free = ((ry / nr - al) / bl + zbar) * 100.0
        xn = np.append(xs[1:], inf)
        adm = valid & (ks >= 2) & (ks <= m - 1) & two & (Lzz > 0.0) & (bl != 0.0) & (c_free >= xs) & (c_free <= xn)
    s_knot = np.where(valid & ~np.isnan(s_knot), s_knot, inf)
    s_free = np.where(adm & ~np.isnan(s_free), s_free, inf)
    kk, kf = int(np.argmin(s_knot)), int(np.argmin(s_free))     # argmin: the smallest k among equals
    x_first, x_last = float(xs[0]), float(xs[-1])
    out = [nan] * 9 + [0.0] * 15
    out[12], out[19], out[20] = dm, x_first, x_last
    if not (s_knot[kk] < inf or s_free[kf] < inf):
        out[9] = out[15] = out[16] = out[17] = out[18] = nan
        out[14] = 5.0
        return out
    if s_free[kf] < s_knot[kk]:                                  # on equal SSE a knot beats a free candidate
        kind, k, sse_min = 0, kf + 1, float(s_free[kf])
        b = float(bl[kf])
        a, c = (ybar + float(al[kf])) - b * zbar, float(c_free[kf])
        c_own = c
    else:
        k, sse_min = kk + 1, float(s_knot[kk])
        kind = 3 if constant[kk] else (2 if k == m else 1)
        b = float(beta[kk])
        a, c_own = (ybar + float(alpha[kk])) - b * zbar, float(xs[kk])
        c = inf if kind == 2 else c_own
    # the pass at the winner
    u = np.minimum(xs, c) / 100.0
    r = (ys - a) - b * u
    Su, Suu, nR, sse = float(np.sum(u)), float(np.sum(u * u)), float(np.count_nonzero(xs > c)), float(np.sum(r * r))
    thr = sse_min * (1.0 + q / (dm - 3.0))
    inside = xs[s_knot <= thr]
    out[0:3] = [a, b, c]
    out[9], out[10], out[11], out[13] = sse, float(kind), float(k), float(np.count_nonzero(valid))
    out[15], out[16] = float(_knot(P[-1:], T, dm, z[-1:], two[-1:])[0][0]), float(T[5] - T[2] * T[2] / dm)
    lo = min([c_own] + ([float(inside.min())] if len(inside) else []))
    hi = max([c_own] + ([float(inside.max())] if len(inside) else []))
    i_lo, i_hi = int(np.searchsorted(xs, lo, "left")), int(np.searchsorted(xs, hi, "right"))
    out[17] = float(xs[i_lo - 1]) if i_lo > 0 else lo            # outwards to the next current: the profile crosses inside that gap
    out[18] = float(xs[i_hi]) if i_hi < m else hi
    if not x_first < x_last:
        out[2] = out[17] = out[18] = nan
        out[14] = 7.0
        return out
    g = b / 100.0
    line = kind == 2
    A22 = 1.0 if line else (g * g) * nR
    if not (Suu > 0.0 and A22 > 0.0):
        out[14] = 5.0
        return out
    sc = [1.0 / math.sqrt(dm), 1.0 / math.sqrt(Suu), 1.0 / math.sqrt(A22)]
    C = [1.0, (Su * sc[0]) * sc[1], 1.0, 0.0 if line else ((g * nR) * sc[0]) * sc[2],
         0.0 if line else (((g * (c / 100.0)) * nR) * sc[1]) * sc[2], 1.0]
    L = _chol3(C, 0.0, PIVOT_MIN)
    if L is None:
        out[14] = 5.0
        return out
    s2 = sse / (dm - (2.0 if line else 3.0))
    for qq in range(3):
        zc = _backward(L, _forward(L, [1.0 if i == qq else 0.0 for i in range(3)]))
        for pp in range(qq + 1):
            out[3 + qq * (qq + 1) // 2 + pp] = nan if (line and qq == 2) else s2 * ((zc[pp] * sc[pp]) * sc[qq])
    return out


def _fit_host(table, cols, row_index, start, length, q):
    a = _as_numpy(table, np.float64)
    if a.ndim != 2:
        raise ValueError("the table must be a 2-D array")
    a = a[:, list(cols)]
    if row_index is not None:
        ridx = _as_numpy(row_index, np.int64).reshape(-1)
        n = len(ridx)
    else:
        ridx, n = None, a.shape[0]
    fit = np.empty((len(start), FIT_WORDS))
    for w in range(len(start)):
        s, l = int(start[w]), int(length[w])
        if s < 0 or l < 0 or l > MAX_WINDOW or s > n - l:
            fit[w] = _empty_row(0, 6)
            continue
        if ridx is None:
            rows = a[s:s + l]
        else:
            idx = ridx[s:s + l]
            ok = (idx >= 0) & (idx < a.shape[0])
            rows = np.full((l, 2), np.nan)
            rows[ok] = a[idx[ok]]
        rows = rows[np.isfinite(rows).all(axis=1)]
        fit[w] = _fit_one_host(rows[:, 0], rows[:, 1], q)
    return fit


# ------------------------------------------------------------------ the device backend
def _fit_device(table, cols, row_index, start, length, q):
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
    longest = int(min(max(int(np.max(length)), 0), MAX_WINDOW))  # sizes the LDS; a longer window answers status 6
    fit = torch.empty(W, FIT_WORDS, dtype=torch.float64, device=dev)
    opts = _lib.BpOpts(float(q), 0, 0)
    call("pinn_bp_fit", arr, ld, arr.shape[0], (ctypes.c_int * 2)(*cols), ridx, n, ws, wl, W, longest, ctypes.byref(opts), fit)
    return fit


# ------------------------------------------------------------------ results
class BreakpointFit:
    """The fits of W windows.  theta [W, 3] = (l1, l2, l3), cov [W, 3, 3], se [W, 3], sse [W], n_used, status [W] (integers),
    names: as `identify.WindowFit`'s, so `identify.drift(fit, baseline)` takes it unchanged.  Also kind [W] (0 free: c between
    two currents, 1 knot: c at a current and the covariance a one-sided linearisation, 2 line: no row beyond c, c = inf and
    its covariance entries NaN, 3 constant), k [W] (rows at or below c), distinct [W] (currents), c_interval [W, 2] (the
    profile interval of c, to the resolution of the window's currents), x_range [W, 2], sse_line and sse_const [W].  numpy
    arrays on the host, whichever backend ran.

    The oxygen target's clamp and the 10 x penalty on act < 1 do not depend on theta and are not part of the fit; the
    reference's |lambda_O3| means c is reported non-negative."""

    names = THETA_NAMES

    def __init__(self, fit, backend):
        fit = _as_numpy(fit, np.float64)
        self.backend, self.raw = backend, fit
        self.theta = fit[:, 0:3].copy()
        self.cov = np.empty((len(fit), 3, 3))
        for k, (p, q) in enumerate(_TRI):
            self.cov[:, p, q] = self.cov[:, q, p] = fit[:, 3 + k]
        with np.errstate(invalid="ignore"):
            self.se = np.sqrt(np.stack([self.cov[:, k, k] for k in range(3)], axis=1))
        self.sse, self.sse_line, self.sse_const = fit[:, 9].copy(), fit[:, 15].copy(), fit[:, 16].copy()
        self.kind, self.k, self.n_used, self.distinct, self.status = (fit[:, j].astype(np.int64) for j in (10, 11, 12, 13, 14))
        self.c_interval, self.x_range = fit[:, 17:19].copy(), fit[:, 19:21].copy()

    def __len__(self):
        return len(self.theta)

    @property
    def plateau_F(self):
        """(sse_line - sse) / (sse / (m - 3)): the evidence that a plateau is seen at all, an F statistic of the line against the law."""
        with np.errstate(all="ignore"):
            return (self.sse_line - self.sse) / (self.sse / (self.n_used - 3.0))

    def params(self, gas):
        """{lambda name: (value [W], standard error [W])} of a gas; lambda_*3 = inf for kind 2."""
        if gas not in GASES:
            raise ValueError("gas must be 'hydrogen' or 'oxygen'")
        return {n: (self.theta[:, k].copy(), self.se[:, k].copy()) for k, n in enumerate(LAMBDA_OF[gas])}

    @property
    def target_range(self):
        """[W, 2]: the minimum and maximum of the fitted law over [x_min, x_max] (it is monotone, so they sit at the ends)."""
        with np.errstate(invalid="ignore"):
            ends = np.stack([self.theta[:, 0] + self.theta[:, 1] * (np.minimum(self.x_range[:, j], self.theta[:, 2]) / 100.0) for j in (0, 1)], axis=1)
            c_nan = np.isnan(self.theta[:, 2]) & ~np.isnan(self.theta[:, 0])           # status 7: the constant a
            ends = np.where(c_nan[:, None], self.theta[:, 0:1], ends)
            return np.stack([np.min(ends, axis=1), np.max(ends, axis=1)], axis=1)

    @property
    def inside_oxygen_clamp(self):
        """[W]: whether the fitted law stays within the oxygen target's clamp [1.05, 15] on the window's currents."""
        t = self.target_range
        with np.errstate(invalid="ignore"):
            return (t[:, 0] >= OXYGEN_CLAMP[0]) & (t[:, 1] <= OXYGEN_CLAMP[1])


def fit_breakpoints(table, start, length, backend="auto", row_index=None, cols=None, q=Q95):
    """Fit every window (start[w], length[w]) of the table's gathered positions; returns a BreakpointFit.

    backend: "auto" (a tensor stays where it is, as the sibling modules), "device", "host" or its synonym "numpy".
    `row_index` is a gather list over the table's rows, `cols` its two columns (default 0, 1), `q` the profile threshold of
    the interval of c (default: the 95 % point of chi-square with one degree of freedom)."""
    backend = _pick_backend("host" if backend == "numpy" else backend, table)
    start, length = _as_numpy(start, np.int64).reshape(-1), _as_numpy(length, np.int64).reshape(-1)
    if start.shape != length.shape:
        raise ValueError("start and length must have one entry per window")
    cols = [0, 1] if cols is None else [int(c) for c in cols]
    if len(cols) != 2:
        raise ValueError("a table has two columns")
    q = float(q)
    if not (q > 0.0 and math.isfinite(q)):
        raise ValueError("q must be finite and positive")
    if len(start) == 0:
        return BreakpointFit(np.empty((0, FIT_WORDS)), backend)
    run = _fit_device if backend == "device" else _fit_host
    return BreakpointFit(run(table, cols, row_index, start, length, q), backend)


def fit_breakpoint_baseline(table, row_index=None, **kw):
    """One window over all positions (at most 4096): the baseline the windows are compared with."""
    n = len(row_index) if row_index is not None else table.shape[0]
    if n > MAX_WINDOW:
        raise ValueError("a single fit takes at most %d rows, got %d: pass a row_index that thins them" % (MAX_WINDOW, n))
    return fit_breakpoints(table, [0], [n], row_index=row_index, **kw)


class SupplyTracker:
    """The online form: keeps the last `length` <= 4096 table rows in a ring (on the device for the device backend) and refits
    them at every update: one window read through a gather list, on the device one `pinn_bp_fit` launch.

    update(chunk) -> {"theta", "se", "z", "wald", "p", "status", "kind", "n_used", "blamed"}; z, wald and p are `identify.drift`
    against the baseline, `blamed` the name of the parameter with the largest |z| (None while the fit has no covariance)."""

    def __init__(self, baseline, length, backend="auto", q=Q95):
        if not 4 <= int(length) <= MAX_WINDOW:
            raise ValueError("length must lie in 4 .. %d" % MAX_WINDOW)
        self.baseline, self.length, self.backend, self.q = baseline, int(length), backend, q
        self.ring, self.head, self.count, self.last = None, 0, 0, None

    def _store(self, chunk):
        L = self.length
        if self.ring is None:
            self.backend = _pick_backend("host" if self.backend == "numpy" else self.backend, chunk)
            if self.backend == "device":
                import torch
                self._torch = torch
                dev = chunk.device if _is_tensor(chunk) and chunk.is_cuda else "cuda"
                self.ring = torch.full((L, 2), float("nan"), dtype=torch.float64, device=dev)
            else:
                self.ring = np.full((L, 2), np.nan)
        if self.backend == "device":
            torch = self._torch
            c = (chunk if _is_tensor(chunk) else torch.from_numpy(np.asarray(chunk, dtype=np.float64))).detach().to(self.ring.device, torch.float64)
            c = c.reshape(-1, 2)[-L:]
            k = c.shape[0]
            pos = (torch.arange(k, device=self.ring.device) + self.head) % L
        else:
            c = _as_numpy(chunk, np.float64).reshape(-1, 2)[-L:]
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
        f = fit_breakpoints(self.ring, [0], [self.count], backend=self.backend, row_index=self.window_index(), q=self.q)
        d = drift(f, self.baseline)
        z = d["z"][0]
        blamed = THETA_NAMES[int(np.nanargmax(np.abs(z)))] if np.any(np.isfinite(z)) else None
        self.last = f
        return {"theta": f.theta[0], "se": f.se[0], "z": z, "wald": d["wald"][0], "p": d["p"][0], "status": int(f.status[0]),
                "kind": int(f.kind[0]), "n_used": int(f.n_used[0]), "blamed": blamed}
