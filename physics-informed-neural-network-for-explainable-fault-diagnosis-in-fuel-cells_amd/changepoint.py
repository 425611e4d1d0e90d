"""Change-point segmentation: where the statistics of the residual columns change, without a label column.

The reference takes the regimes of a recording from the experimenter's notebook (`create_fault_labels` turns known row ranges
into column 17), and `estimate_mu_sigma_normal`, the label-posterior mappings, `rf_series`, `DeviceHMM` and `sliding_windows`
all lean on those boundaries.  This module finds them: exact penalised segmentation (optimal partitioning with PELT's
pruning) of up to 8 columns.

The problem.  Rows x_t, optionally standardised, z = (x - mu) / sigma, and centred on the first row of their recording
segment.  For a segment of m rows a partition 0 = tau_0 < ... < tau_k < tau_{k+1} = m with pieces of at least `min_len` and
at most `max_len` rows minimises sum_i C(tau_i, tau_{i+1}) + penalty * k.  With S, Q the prefix sums of the centred rows and
of their squares, len = t - s and SS_d(s, t) = max(Q_d(t) - Q_d(s) - (S_d(t) - S_d(s))^2 / len, 0):

  kind="mean"      C = sum_d SS_d                                   a change in mean at unit variance (z-scores); min_len >= 1
  kind="meanvar"   C = sum_d [len log v_d + SS_d / v_d]             a change in mean and variance per column; min_len >= 2
                   v_d = max(SS_d / len, var_floor)                 (the constrained maximum-likelihood value)

F(0) = -penalty, F(t) = min over admissible s of F(s) + C(s, t) + penalty, ties to the smallest s; the change points are the
walk of the arg-mins back from m.  With prune=True a candidate s with F(s) + C(s, t) > F(t) is dropped, but only from step
t + min_len on: t is no admissible last change point before that, and dropping s at once loses the optimum when
min_len > 1 (tests/golden/changepoint_immediate_pruning.json is such a case).  Pruning never changes the result, only the
number of cost evaluations (`Segmentation.evaluations`).

backend="auto" | "device" | "numpy" ("host" is the same as "numpy").  The device backend is csrc/pinn_changepoint.hip: a
tiled prefix pass, then one workgroup per (segment, penalty) that owns the whole recursion, continued by queued launches
when a segment is long.  The numpy backend states the same arithmetic in the same order (the prefix tiles of TILE rows, the
step blocks of BLOCK steps at whose ends candidates leave the list): F and the change points of kind="mean" are the
device's to the bit, and the evaluation counts are the same integers.  It serves machines without a GPU and is what the
device is held to.  Importing this module needs numpy only.
"""
import ctypes

import numpy as np

from ._device import _DevRows, _as_numpy, _dev_vec, _host_rows, _is_tensor, _pick_backend, _torch_lib, call, columns_of

MAX_FEAT, MAX_PEN, MAX_SEGMENTS, MAX_WINDOW = 8, 16, 65535, 4096        # include/pinn_hip.h: PINN_CP_*
TILE, BLOCK, LAUNCH_EVALS = 256, 64, 1 << 24
KINDS = {"mean": 0, "meanvar": 1}
MIN_LEN = {"mean": 1, "meanvar": 2}
BAD_ROW, OVERFLOW, INFEASIBLE = 1, 2, 4
DEFAULT_FEATURES = "pV,pT,pH,pO"
DEFAULT_VAR_FLOOR = 1e-8
DEFAULT_CONFIRM = 2                     # ChangeMonitor: a change point is new once it has been found in this many updates in a row


# ---------------------------------------------------------------------------------------------- results
class Segmentation:
    """What `segment` returns.  `change_points` [n_seg] lists of positions (a piece starts at each); `seg_starts` the
    recording's own starts merged with them, ready for rf_series, DeviceHMM and sliding_windows(segments=); `F`,
    `status`, `evaluations` [n_seg]; `n`, `penalty`, `kind`, `min_len`, `recording_starts`."""

    def __init__(self, n, recording_starts, change_points, F, status, evaluations, penalty, kind, min_len):
        self.n, self.penalty, self.kind, self.min_len = int(n), float(penalty), kind, int(min_len)
        self.recording_starts = np.asarray(recording_starts, dtype=np.int64)
        self.change_points = [np.asarray(c, dtype=np.int64) for c in change_points]
        self.F, self.status = np.asarray(F, dtype=np.float64), np.asarray(status, dtype=np.int64)
        self.evaluations = np.asarray(evaluations, dtype=np.int64)
        allp = [self.recording_starts] + self.change_points
        self.seg_starts = np.unique(np.concatenate(allp)) if self.n > 0 else np.zeros(0, dtype=np.int64)

    @property
    def n_change_points(self):
        return int(sum(c.size for c in self.change_points))

    def bounds(self):
        """(start, stop) of every found segment."""
        edges = list(self.seg_starts) + [self.n]
        return [(int(edges[i]), int(edges[i + 1])) for i in range(len(self.seg_starts))]


class PenaltyPath:
    """What `penalty_path` returns: per penalty the number of change points, F summed over the recording's segments and
    the unpenalised cost (F - penalty * change points), the evaluations, and the change points themselves."""

    def __init__(self, penalties, n_change_points, F, cost, evaluations, change_points, n, D, kind):
        self.penalties, self.n_change_points, self.F, self.cost = penalties, n_change_points, F, cost
        self.evaluations, self.change_points, self.n, self.D, self.kind = evaluations, change_points, n, D, kind


# ---------------------------------------------------------------------------------------------- arguments
def default_penalty(n, D, kind="mean"):
    """The BIC penalty: (D + 1) log n for "mean", (2 D + 1) log n for "meanvar"."""
    if kind not in KINDS:
        raise ValueError("kind must be 'mean' or 'meanvar'")
    return float(((D + 1) if kind == "mean" else (2 * D + 1)) * np.log(max(int(n), 2)))


def _backend(backend, data):
    return _pick_backend("host" if backend == "numpy" else backend, data)


def _bounds(seg_starts, n):
    if seg_starts is None or len(seg_starts) == 0:
        return np.zeros(1, dtype=np.int64), [(0, n)]
    starts = _as_numpy(seg_starts, np.int64).reshape(-1)
    if starts[0] != 0 or np.any(np.diff(starts) <= 0) or starts[-1] >= max(n, 1):
        raise ValueError("seg_starts must begin with 0 and ascend strictly inside the %d positions" % n)
    if starts.size > MAX_SEGMENTS:
        raise ValueError("at most %d recording segments" % MAX_SEGMENTS)
    edges = list(starts) + [n]
    return starts, [(int(edges[i]), int(edges[i + 1])) for i in range(len(starts))]


class _Problem:
    """The checked arguments both backends share."""

    def __init__(self, features, kind, min_len, max_len, mu, sigma, prune, var_floor, block_steps=None, launch_evals=None):
        if kind not in KINDS:
            raise ValueError("kind must be 'mean' or 'meanvar'")
        self.columns = columns_of(DEFAULT_FEATURES if features is None else features, _parse)
        self.D = len(self.columns)
        if not 1 <= self.D <= MAX_FEAT:
            raise NotImplementedError("change-point segmentation takes 1 to %d columns, got %d" % (MAX_FEAT, self.D))
        self.kind = kind
        self.min_len = MIN_LEN[kind] if min_len is None else int(min_len)
        if self.min_len < MIN_LEN[kind]:
            raise ValueError("min_len must be at least %d for kind=%r" % (MIN_LEN[kind], kind))
        self.max_len = 0 if max_len is None else int(max_len)
        if max_len is not None and self.max_len < self.min_len:
            raise ValueError("max_len must not be below min_len")
        if (mu is None) != (sigma is None):
            raise ValueError("mu and sigma go together")
        self.mu = None if mu is None else np.array(_as_numpy(mu, float), dtype=np.float64).reshape(-1)
        self.sigma = None if sigma is None else np.array(_as_numpy(sigma, float), dtype=np.float64).reshape(-1)
        if self.mu is not None and (self.mu.shape != (self.D,) or self.sigma.shape != (self.D,) or not np.all(np.isfinite(self.mu))
                                    or not np.all(np.isfinite(self.sigma)) or np.any(self.sigma <= 0)):
            raise ValueError("mu and sigma must hold %d finite values, sigma positive" % self.D)
        self.var_floor = float(var_floor)
        if not (np.isfinite(self.var_floor) and self.var_floor >= 0):
            raise ValueError("var_floor must be finite and not negative")
        self.prune = bool(prune)
        self.block = BLOCK if block_steps is None else int(block_steps)
        if not 1 <= self.block <= BLOCK:
            raise ValueError("the step block holds 1 to %d steps" % BLOCK)
        self.launch_evals = 0 if launch_evals is None else int(launch_evals)

    def penalties(self, penalty, n):
        pens = [default_penalty(n, self.D, self.kind)] if penalty is None else [float(p) for p in np.atleast_1d(_as_numpy(penalty, float))]
        if not pens or not all(np.isfinite(p) and p >= 0 for p in pens):
            raise ValueError("a penalty must be finite and not negative")
        return pens


def _parse(spec):
    from .diagnosis import parse_features
    return parse_features(spec)


# ---------------------------------------------------------------------------------------------- numpy backend
def _host_z(arr, columns, row_index, mu, sigma):
    """The standardised rows [n, D] and which of them read nothing or hold a non-finite value."""
    a = _as_numpy(arr)
    if a.ndim != 2:
        raise ValueError("results must be a 2-D array")
    a = np.asarray(a, dtype=np.float64)
    if row_index is None:
        Z, missing = a[:, columns], np.zeros(a.shape[0], dtype=bool)
    else:
        idx = _as_numpy(row_index, np.int64).reshape(-1)
        missing = (idx < 0) | (idx >= a.shape[0])
        Z = a[np.where(missing, 0, idx)][:, columns] if a.shape[0] > 0 else np.zeros((idx.size, len(columns)))
    Z = np.array(Z, dtype=np.float64)
    if mu is not None:
        with np.errstate(all="ignore"):
            Z = (Z - mu) / sigma
    return Z, missing | ~np.all(np.isfinite(Z), axis=1)


def _host_prefix(Z):
    """Prefix table [m + 1, 2 D] of one segment: tiles of TILE rows, a running sum inside each tile, the tile totals summed
    tile by tile into offsets (csrc/pinn_changepoint.hip: tile_scan, tile_offsets, tile_finish)."""
    m, D = Z.shape
    c = Z - Z[0]
    A = np.concatenate([c, c * c], axis=1)
    tiles = (m + TILE - 1) // TILE
    pad = np.zeros((tiles * TILE, 2 * D))
    pad[:m] = A
    local = np.cumsum(pad.reshape(tiles, TILE, 2 * D), axis=1)
    off = np.zeros((tiles, 2 * D))
    if tiles > 1:
        off[1:] = np.cumsum(local[:, -1, :], axis=0)[:-1]
    P = np.zeros((m + 1, 2 * D))
    P[1:] = (off[:, None, :] + local).reshape(tiles * TILE, 2 * D)[:m]
    return P


def _cost(P, s, t, kind, D, var_floor):
    """C(s, t) for broadcastable index arrays; pairs with t <= s give garbage and are masked by the caller."""
    ln = np.asarray(t - s, dtype=np.float64)
    with np.errstate(all="ignore"):
        inv = 1.0 / ln
        c = np.zeros(np.broadcast(s, t).shape)
        for d in range(D):
            dS, dQ = P[t, d] - P[s, d], P[t, D + d] - P[s, D + d]
            x = dQ - (dS * dS) * inv
            ssq = np.where(x > 0.0, x, 0.0)
            if kind == "mean":
                c = c + ssq
            else:
                vv = ssq * inv
                v = np.where(vv > var_floor, vv, var_floor)
                c = c + (ln * np.log(v) + ssq / v)
    return c


def _host_solve(P, beta, kind, min_len, max_len, var_floor, prune, block, immediate=False):
    """Optimal partitioning of one segment in step blocks (csrc/pinn_changepoint.hip: solve_pair).  Returns F [m + 1],
    last [m + 1] and the evaluations.  immediate=True tests a candidate at the block's last step instead of the last step that
    permits leaving: the rule that is wrong for min_len > 1, kept for the test that shows it."""
    m, D = P.shape[0] - 1, P.shape[1] // 2
    maxl = max_len if max_len > 0 else m
    F, last = np.full(m + 1, np.inf), np.full(m + 1, -1, dtype=np.int64)
    F[0] = -beta
    cand = np.zeros(0, dtype=np.int64)
    evals, t0 = 0, 0
    with np.errstate(all="ignore"):
        while t0 < m:
            t1 = min(t0 + block, m)
            nb = t1 - t0
            s_new = np.arange(t0 + 1 - min_len, t0 + 1 - min_len + nb)
            s_new = s_new[(s_new >= 0) & (s_new <= t0)]
            cand = np.concatenate([cand, s_new[F[s_new] < np.inf]])
            t = np.arange(t0 + 1, t1 + 1)
            bv, bs = np.full(nb, np.inf), np.full(nb, -1, dtype=np.int64)
            if cand.size:
                ln = t[None, :] - cand[:, None]
                adm = (ln >= min_len) & (ln <= maxl)
                V = (F[cand][:, None] + _cost(P, cand[:, None], t[None, :], kind, D, var_floor)) + beta
                evals += int(adm.sum())
                V = np.where(adm & ~np.isnan(V), V, np.inf)
                idx = np.argmin(V, axis=0)                      # the first of equal values: the smallest s
                bv = V[idx, np.arange(nb)]
                bs = np.where(bv < np.inf, cand[idx], -1)
            for i in range(nb - min_len):                       # the triangular part: candidate t0 + 1 + i
                if not bv[i] < np.inf:
                    continue
                k = np.arange(i + min_len, min(nb, i + maxl + 1))
                v = (bv[i] + _cost(P, t0 + 1 + i, t[k], kind, D, var_floor)) + beta
                evals += k.size
                up = v < bv[k]
                bv[k[up]], bs[k[up]] = v[up], t0 + 1 + i
            F[t], last[t] = bv, bs
            cand = np.concatenate([cand, t[(t + min_len <= t1) & (bv < np.inf)]])
            keep = cand >= t1 + 1 - maxl
            tstar = t1 if immediate else t1 + 1 - min_len
            if prune and tstar >= 1:
                tested = keep & (tstar - cand >= min_len)
                v = F[cand] + _cost(P, cand, np.full(cand.shape, tstar), kind, D, var_floor)
                keep &= ~(tested & (v > F[tstar]))
            cand = cand[keep]
            t0 = t1
    return F, last, evals


def _walk(last, m):
    cps, u = [], m
    while last[u] > 0:
        u = int(last[u])
        cps.append(u)
    return cps[::-1]


def _host_segment(arr, pb, pens, row_index, bounds, immediate=False):
    Z, bad = _host_z(arr, pb.columns, row_index, pb.mu, pb.sigma)
    ns, npn = len(bounds), len(pens)
    F, status = np.full((ns, npn), np.nan), np.zeros((ns, npn), dtype=np.int64)
    evals, cps = np.zeros((ns, npn), dtype=np.int64), [[np.zeros(0, dtype=np.int64)] * npn for _ in range(ns)]
    for si, (lo, hi) in enumerate(bounds):
        if hi <= lo:
            continue
        if bad[lo:hi].any():
            status[si] = BAD_ROW
            continue
        P = _host_prefix(Z[lo:hi])
        for pi, beta in enumerate(pens):
            Fv, last, ev = _host_solve(P, beta, pb.kind, pb.min_len, pb.max_len, pb.var_floor, pb.prune, pb.block, immediate)
            F[si, pi], evals[si, pi] = Fv[hi - lo], ev
            if Fv[hi - lo] < np.inf:
                cps[si][pi] = np.asarray(_walk(last, hi - lo), dtype=np.int64) + lo
            else:
                status[si, pi] = INFEASIBLE
    return F, status, evals, cps


# ---------------------------------------------------------------------------------------------- device backend
def _opts(_lib, pb):
    return _lib.CpOpts(KINDS[pb.kind], pb.min_len, pb.max_len, int(pb.prune), pb.block, pb.var_floor, pb.launch_evals)


def _c_doubles(v):
    return None if v is None else (ctypes.c_double * len(v))(*[float(x) for x in v])


def _outputs(torch, dev, pairs, cap):
    return (torch.empty(pairs, dtype=torch.float64, device=dev), torch.zeros(pairs, dtype=torch.int64, device=dev),
            torch.zeros(pairs * max(cap, 1), dtype=torch.int64, device=dev), torch.zeros(pairs, dtype=torch.int64, device=dev),
            torch.zeros(pairs, dtype=torch.int64, device=dev))


def _collect(out, ns, npn, cap, retry):
    """The outputs of a call on the host, or None when a pair overflowed `cap` and `retry` is set."""
    F, ncp, cp, ev, st = [o.cpu().numpy() for o in out]
    if retry and np.any(st & OVERFLOW):
        return None
    cp = cp.reshape(ns * npn, max(cap, 1))
    cps = [[cp[s * npn + p, :min(int(ncp[s * npn + p]), cap)].copy() for p in range(npn)] for s in range(ns)]
    return F.reshape(ns, npn), st.reshape(ns, npn), ev.reshape(ns, npn), cps


def _device_segment(arr, pb, pens, row_index, starts, bounds, cp_cap=None):
    torch, _lib, lib = _torch_lib()
    rows = _DevRows.within(torch, arr, pb.columns, row_index, lambda D: None)
    n, ns, npn = rows.n, len(bounds), len(pens)
    if n == 0:
        return (np.full((ns, npn), np.nan), np.zeros((ns, npn), dtype=np.int64), np.zeros((ns, npn), dtype=np.int64),
                [[np.zeros(0, dtype=np.int64)] * npn for _ in range(ns)])
    if npn > MAX_PEN:
        raise ValueError("at most %d penalties in one call" % MAX_PEN)
    multi = ns > 1
    c_starts = (ctypes.c_longlong * ns)(*[int(s) for s in starts]) if multi else None
    d_starts = _dev_vec(torch, starts, torch.int64, rows.dev) if multi else None
    ws = torch.empty(lib.pinn_cp_workspace_bytes(n, pb.D, ns if multi else 0, npn), dtype=torch.uint8, device=rows.dev)
    cap = 64 if cp_cap is None else int(cp_cap)
    while True:
        out = _outputs(torch, rows.dev, ns * npn, cap)
        call("pinn_cp_segment", *rows.head(), _c_doubles(pb.mu), _c_doubles(pb.sigma), c_starts, d_starts, ns if multi else 0,
             ctypes.byref(_opts(_lib, pb)), _c_doubles(pens), npn, out[0], out[1], out[2], cap, out[3], out[4], ws, ws.numel())
        got = _collect(out, ns, npn, cap, retry=cp_cap is None)
        if got is not None:
            return got
        cap = int(out[1].max().item())                          # every pair's count is exact: one more call holds them all


# ---------------------------------------------------------------------------------------------- the public functions
def _run(results, penalty, features, kind, min_len, max_len, mu, sigma, row_index, seg_starts, prune, var_floor, backend,
         _block_steps, _launch_evals, _cp_cap=None):
    pb = _Problem(features, kind, min_len, max_len, mu, sigma, prune, var_floor, _block_steps, _launch_evals)
    n = int(np.shape(results)[0]) if row_index is None else int(np.shape(row_index)[0] if np.ndim(row_index) else 1)
    starts, bounds = _bounds(seg_starts, n)
    pens = pb.penalties(penalty, n)
    if _backend(backend, results) == "host":
        out = _host_segment(results, pb, pens, row_index, bounds)
    else:
        out = _device_segment(results, pb, pens, row_index, starts, bounds, _cp_cap)
    return pb, n, starts, pens, out


def segment(results, features=DEFAULT_FEATURES, penalty=None, kind="mean", min_len=None, max_len=None, mu=None, sigma=None,
            row_index=None, seg_starts=None, prune=True, var_floor=DEFAULT_VAR_FLOOR, backend="auto", _block_steps=None,
            _launch_evals=None):
    """Segment the rows of `results` (or the rows `row_index` lists, in that order) on the columns `features`; `seg_starts`
    cuts the rows into independent recordings as in rf_series.  penalty=None takes default_penalty; min_len=None the
    kind's minimum.  `_block_steps` and `_launch_evals` are for the tests: fewer steps in a block, so that candidates leave
    the list at small sizes, and a lower cap of a launch, so that a few hundred rows need a second one."""
    pb, n, starts, pens, (F, status, evals, cps) = _run(results, penalty, features, kind, min_len, max_len, mu, sigma, row_index,
                                                        seg_starts, prune, var_floor, backend, _block_steps, _launch_evals)
    if len(pens) != 1:
        raise ValueError("segment takes one penalty; penalty_path takes several")
    return Segmentation(n, starts, [c[0] for c in cps], F[:, 0], status[:, 0], evals[:, 0], pens[0], pb.kind, pb.min_len)


def penalty_path(results, penalties, features=DEFAULT_FEATURES, kind="mean", min_len=None, max_len=None, mu=None, sigma=None,
                 row_index=None, seg_starts=None, prune=True, var_floor=DEFAULT_VAR_FLOOR, backend="auto", _block_steps=None,
                 _launch_evals=None):
    """All `penalties` (at most MAX_PEN a device call; more are sent in groups) over the same prefix sums."""
    pens_all = [float(p) for p in np.atleast_1d(_as_numpy(penalties, float))]
    parts = []
    for i in range(0, len(pens_all), MAX_PEN):
        parts.append(_run(results, pens_all[i:i + MAX_PEN], features, kind, min_len, max_len, mu, sigma, row_index, seg_starts, prune,
                          var_floor, backend, _block_steps, _launch_evals))
    pb, n = parts[0][0], parts[0][1]
    F = np.concatenate([p[4][0] for p in parts], axis=1)
    status = np.concatenate([p[4][1] for p in parts], axis=1)
    evals = np.concatenate([p[4][2] for p in parts], axis=1)
    cps = [sum((p[4][3][s] for p in parts), []) for s in range(F.shape[0])]
    good = (status & (BAD_ROW | INFEASIBLE)) == 0
    k = np.array([[cps[s][p].size for p in range(F.shape[1])] for s in range(F.shape[0])], dtype=np.int64)
    pens = np.asarray(pens_all)
    Fsum = np.where(good, F, 0.0).sum(axis=0)
    ksum = np.where(good, k, 0).sum(axis=0)
    change_points = [np.sort(np.concatenate([cps[s][p] for s in range(F.shape[0])])) if F.shape[0] else np.zeros(0, dtype=np.int64)
                     for p in range(F.shape[1])]
    return PenaltyPath(pens, ksum, Fsum, Fsum - pens * ksum, evals.sum(axis=0), change_points, n, pb.D, pb.kind)


def select_penalty(path, rule="bic"):
    """The index of the chosen penalty of a PenaltyPath.  "bic": the smallest cost + default_penalty(n, D, kind) * change
    points, ties to the larger penalty.  "elbow": the penalties in ascending order, the point of the (change points, cost)
    curve farthest from the chord between its ends (both axes scaled to [0, 1])."""
    k, cost = np.asarray(path.n_change_points, dtype=float), np.asarray(path.cost, dtype=float)
    if rule == "bic":
        crit = cost + default_penalty(path.n, path.D, path.kind) * k
        best = np.flatnonzero(crit == crit.min())
        return int(best[np.argmax(path.penalties[best])])
    if rule != "elbow":
        raise ValueError("rule must be 'bic' or 'elbow'")
    order = np.argsort(path.penalties)
    x, y = k[order], cost[order]
    if np.ptp(x) == 0 or np.ptp(y) == 0:
        return int(order[-1])
    x, y = (x - x.min()) / np.ptp(x), (y - y.min()) / np.ptp(y)
    dist = np.abs((y[-1] - y[0]) * (x - x[0]) - (x[-1] - x[0]) * (y - y[0]))
    return int(order[int(np.argmax(dist))])


def segment_table(results, segmentation, features=DEFAULT_FEATURES, row_index=None):
    """Start, length, mean [D] and variance [D] (ddof = 0) of every found segment, as a dict of arrays.  Runs on the host."""
    cols = columns_of(features, _parse)
    X = _host_rows(results, cols, row_index)
    b = segmentation.bounds()
    return {"start": np.array([lo for lo, _ in b], dtype=np.int64), "length": np.array([hi - lo for lo, hi in b], dtype=np.int64),
            "mean": np.array([X[lo:hi].mean(axis=0) for lo, hi in b]).reshape(len(b), len(cols)),
            "var": np.array([X[lo:hi].var(axis=0) for lo, hi in b]).reshape(len(b), len(cols))}


def labels_from_segments(segmentation, n=None):
    """The index of the found segment of every row [n]."""
    n = segmentation.n if n is None else int(n)
    return (np.searchsorted(segmentation.seg_starts, np.arange(n), side="right") - 1).astype(np.int64)


def diagnose_segments(segmentation, y_prob):
    """One diagnosis per regime: the mean posterior [n_found, C] and its arg-max class [n_found] over the rows of each
    found segment (rows with a non-finite posterior are left out)."""
    P = _as_numpy(y_prob, float)
    b = segmentation.bounds()
    mean = np.full((len(b), P.shape[1]), np.nan)
    for i, (lo, hi) in enumerate(b):
        rows = P[lo:hi]
        rows = rows[np.all(np.isfinite(rows), axis=1)]
        if rows.shape[0]:
            mean[i] = rows.mean(axis=0)
    cls = np.where(np.all(np.isfinite(mean), axis=1), np.argmax(np.where(np.isfinite(mean), mean, -np.inf), axis=1), -1)
    return mean, cls.astype(np.int64)


# ---------------------------------------------------------------------------------------------- the online form
class ChangeMonitor:
    """Change points of the last `window` rows (at most MAX_WINDOW), chunk by chunk, next to RiskMonitor and FaultDiagnoser.

    `update(chunk)` appends the rows of `chunk` (all columns of the results array, or exactly the D feature columns) to
    a ring, segments the window in one launch (pinn_cp_window) and returns (change_points, new): the change points inside
    the window in absolute row numbers, and those among them that have now been found in `confirm` consecutive updates
    for the first time.  penalty=None takes default_penalty(window, D, kind)."""

    def __init__(self, window, features=DEFAULT_FEATURES, penalty=None, kind="mean", min_len=None, max_len=None, mu=None, sigma=None,
                 prune=True, var_floor=DEFAULT_VAR_FLOOR, confirm=DEFAULT_CONFIRM, backend="auto", _block_steps=None):
        self.window = int(window)
        if not 1 <= self.window <= MAX_WINDOW:
            raise ValueError("window must be 1 .. %d" % MAX_WINDOW)
        self._pb = _Problem(features, kind, min_len, max_len, mu, sigma, prune, var_floor, _block_steps)
        self.columns = self._pb.columns
        self.penalty = self._pb.penalties(penalty, self.window)[0]
        self.confirm = max(int(confirm), 1)
        if backend not in ("auto", "device", "numpy", "host"):
            raise ValueError("backend must be 'auto', 'device' or 'numpy'")
        self.backend = backend
        self.n_seen = 0
        self._ring, self._streak, self._reported = None, {}, set()
        self._packed = _Problem(list(range(self._pb.D)), kind, min_len, max_len, mu, sigma, prune, var_floor, _block_steps)
        self.F, self.status, self.evaluations = float("nan"), 0, 0

    def _take(self, chunk):
        D = self._pb.D
        if _is_tensor(chunk):
            c = chunk.detach()
            c = c if c.shape[1] == D else c[:, self.columns]
        else:
            c = np.asarray(chunk, dtype=np.float64)
            c = c if c.shape[1] == D else c[:, self.columns]
        return c

    def update(self, chunk):
        if len(np.shape(chunk)) != 2:
            raise ValueError("a chunk is a 2-D array of rows")
        c = self._take(chunk)
        device = _backend(self.backend, chunk) == "device"
        W, D, k = self.window, self._pb.D, int(c.shape[0])
        if self._ring is None:
            if device:
                torch = _torch_lib()[0]
                self._torch = torch
                self._ring = torch.zeros((W, D), dtype=torch.float64, device=chunk.device if _is_tensor(chunk) and chunk.is_cuda else "cuda")
                self._out = _outputs(torch, self._ring.device, 1, W)
                lib = _torch_lib()[2]
                self._ws = torch.empty(lib.pinn_cp_workspace_bytes(W, D, 0, 1), dtype=torch.uint8, device=self._ring.device)
            else:
                self._ring = np.zeros((W, D))
            self._device = device
        if self._device:
            torch = self._torch
            c = (c if _is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c))).to(self._ring.device, torch.float64)
        else:
            c = _as_numpy(c, np.float64)
        if k > W:                                               # only the last W rows of a long chunk can be in the window
            self.n_seen += k - W
            c, k = c[k - W:], W
        pos = self.n_seen % W
        first = min(k, W - pos)
        self._ring[pos:pos + first] = c[:first]
        if k > first:
            self._ring[:k - first] = c[first:]
        self.n_seen += k
        m = min(self.n_seen, W)
        start = (self.n_seen - m) % W                           # the ring row of the window's first row
        offset = self.n_seen - m
        if k == 0 and m == 0:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        pb = self._packed
        if self._device:
            _, _lib, lib = _torch_lib()
            out = self._out
            cols = (ctypes.c_int * D)(*range(D))
            call("pinn_cp_window", self._ring, D, W, cols, D, start if self.n_seen > W else 0, m, _c_doubles(pb.mu), _c_doubles(pb.sigma),
                 ctypes.byref(_opts(_lib, pb)), _c_doubles([self.penalty]), 1, out[0], out[1], out[2], W, out[3], out[4],
                 self._ws, self._ws.numel())
            F, status, evals, cps = _collect(out, 1, 1, W, retry=False)
        else:
            idx = (start + np.arange(m)) % W if self.n_seen > W else np.arange(m)
            F, status, evals, cps = _host_segment(self._ring, pb, [self.penalty], idx, [(0, m)])
        self.F, self.status, self.evaluations = float(F[0, 0]), int(status[0, 0]), int(evals[0, 0])
        found = cps[0][0] + offset
        streak = {int(p): self._streak.get(int(p), 0) + 1 for p in found}
        self._streak = streak
        new = [p for p, cnt in streak.items() if cnt >= self.confirm and p not in self._reported]
        self._reported.update(new)
        return found, np.asarray(sorted(new), dtype=np.int64)

    def window_rows(self):
        """The rows of the current window in order [m, D], on the host."""
        m = min(self.n_seen, self.window)
        ring = _as_numpy(self._ring) if self._ring is not None else np.zeros((0, self._pb.D))
        idx = ((self.n_seen - m) % self.window + np.arange(m)) % self.window if self.n_seen > self.window else np.arange(m)
        return ring[idx]
