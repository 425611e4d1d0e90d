"""Are the voltage network's standard deviations honest?  Reliability scores, exact conformal quantiles and an online band
over the uncertainty columns of the results array (`ale` 10, `epi` 11, next to `y_true` 8 and `y_pred` 9).

Definitions (the same words as include/pinn_hip.h; csrc/pinn_uncertainty.hip is the device backend):

Predictive law.  Per row y ~ N(y_pred, v) with v = a ale^2 + b epi^2 + c, computed as ((a ale) ale + (b epi) epi) + c.  The
`var_model` is (a, b, c), non-negative, by default (1, 1, 0).  s = sqrt(v), r = y_true - y_pred, z = r / s.

Valid rows.  A row is valid when its gather index lies inside the array, its label maps to a group, y_true and y_pred are
finite, and v is finite and > 0.  Every other row is skipped and counted (`n_skipped`).

Groups.  `groups={"normal": [0], "flooding": [1, 2, 3], ...}` maps labels (integers 0 .. 63, read from column 17 and
truncated; a label outside 0 <= label < n_labels maps to nothing) to at most 16 groups; `risk.FAULT_RANGE_MAP` is accepted as
it is.  `groups=None` puts every row in one group, called "all", and reads no label.

Arithmetic.  float64, every operation rounded on its own.  z, |z| and every comparison use +, *, sqrt, / and <= only, and the
two backends state the same expressions in the same order: z and everything counted from it (coverage hits, the PIT
histogram, every quantile and rank, the monitor's flags and state) are bit-identical between them.  log, erfc and exp enter
only nll = 0.5 (log 2 pi + log v + z^2), Phi(z) = 0.5 erfc(-z / sqrt 2) and the Gaussian's closed-form
crps = s (z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt pi); their sums agree to a stated tolerance.  Coverage thresholds and PIT
edges are z-values, computed once with statistics.NormalDist().inv_cdf, so no count depends on an erfc.

Consecutive rows of a recording are correlated: a binomial band around a coverage (sqrt(p (1 - p) / n)) is optimistic, and
the conformal guarantee (coverage >= level on exchangeable rows) holds across recordings of one kind, not within a drift.

backend="host" is float64 numpy and the referee; "device" runs the HIP kernels on rows read in place; "auto" follows
_device._pick_backend.  Importing this module needs numpy only.
"""
import ctypes
import math
from statistics import NormalDist

import numpy as np

from ._device import _DevRows, _as_numpy, _is_tensor, _pick_backend, _torch_lib, call

COLUMNS = (8, 9, 10, 11, 17)            # y_true, y_pred, ale, epi, label (results.create_comprehensive_results_array_v2)
LEVELS = (0.5, 0.8, 0.9, 0.95, 0.99)
KINDS = {"abs_z": 0, "z": 1, "column": 2}
SUM_NAMES = ("1", "r", "r2", "s", "s2", "z", "z2", "nll", "crps")
# limits and constants of csrc/pinn_uncertainty.hip (include/pinn_hip.h: PINN_UNC_*)
MAX_GROUPS, MAX_LABELS, MAX_LEVELS, MAX_BINS, MAX_QUANTILES, MAX_TARGETS, MAX_WINDOW, MAX_CHUNK, STATE_HEADER = 16, 64, 16, 64, 8, 64, 4096, 2048, 8
TILE, MAX_BLOCKS = 2048, 1024
ST_FILL, ST_POS, ST_ALPHA, ST_Q, ST_VALID, ST_MISS = range(6)

LOG_2PI, INV_SQRT2, INV_SQRT2PI, INV_SQRTPI = 1.8378770664093453, 0.7071067811865476, 0.3989422804014327, 0.5641895835477563


class UncertaintyReport:
    """Reliability of one group.  coverage[l] = hits[l] / n is the share of rows with |z| <= the two-sided normal point of
    levels[l]; pit[b] counts the rows whose Phi(z) falls in the b-th of `bins` equal bins; `miscalibration` is the mean
    |coverage - level|, `pit_chi2` the chi-square of the PIT histogram against a flat one (bins - 1 degrees of freedom on
    independent rows), `scale` = sqrt(sum z^2 / n) the maximum-likelihood factor for s."""

    def __init__(self, name, levels, sums, n, hits, pit, n_skipped):
        self.name, self.levels, self.n, self.n_skipped = name, tuple(levels), int(n), int(n_skipped)
        self.sums = dict(zip(SUM_NAMES, (float(v) for v in sums)))
        self.hits, self.pit = np.asarray(hits, np.int64), np.asarray(pit, np.int64)
        nan = float("nan")
        d = float(self.n) if self.n > 0 else nan
        S = self.sums
        self.rmse = math.sqrt(S["r2"] / d) if self.n > 0 else nan
        self.sharpness = S["s"] / d
        self.z_mean = S["z"] / d
        self.z_var = S["z2"] / d - self.z_mean * self.z_mean
        self.nll = S["nll"] / d
        self.crps = S["crps"] / d
        self.scale = math.sqrt(S["z2"] / d) if self.n > 0 else nan
        self.coverage = self.hits / d
        self.miscalibration = float(np.mean(np.abs(self.coverage - np.asarray(self.levels)))) if self.n > 0 else nan
        e = d / len(self.pit)
        self.pit_chi2 = float(np.sum((self.pit - e) ** 2) / e) if self.n > 0 else nan

    def __repr__(self):
        return "UncertaintyReport(%s: n=%d, rmse=%.4g, sharpness=%.4g, scale=%.4g, nll=%.4g, crps=%.4g, coverage=%s)" % (
            self.name, self.n, self.rmse, self.sharpness, self.scale, self.nll, self.crps, np.round(self.coverage, 4).tolist())


class Quantiles:
    """q[g][i]: the rank[g][i]-th smallest score of group g's n[g] valid rows (+inf when the rank is beyond n[g], NaN for an
    empty group); `names` and `levels` label the two axes."""

    def __init__(self, q, rank, n, n_skipped, names, levels, kind, conformal):
        self.q, self.rank, self.n, self.n_skipped = q, rank, n, int(n_skipped)
        self.names, self.levels, self.kind, self.conformal = tuple(names), tuple(levels), kind, bool(conformal)

    def __getitem__(self, name):
        return self.q[self.names.index(name)]

    def __repr__(self):
        return "Quantiles(kind=%s, levels=%s, q=%s, n=%s)" % (self.kind, self.levels, self.q.tolist(), self.n.tolist())


# ---------------------------------------------------------------------------------------------- arguments
def _columns(columns, need_label):
    c = list(COLUMNS if columns is None else columns)
    if len(c) == 4 and not need_label:
        c.append(-1)
    if len(c) != 5:
        raise ValueError("columns are (y_true, y_pred, ale, epi, label)" if need_label else "columns are (y_true, y_pred, ale, epi[, label])")
    return [int(v) for v in c[:4]], int(c[4])


def _var_model(var_model):
    vm = [float(v) for v in var_model]
    if len(vm) != 3 or not all(math.isfinite(v) and v >= 0.0 for v in vm):
        raise ValueError("var_model is (a, b, c), finite and non-negative")
    return vm


def _group_table(groups):
    """names, table (label -> group or -1): None for one group."""
    if groups is None:
        return ["all"], None
    names, table = [], {}
    for g, (name, labels) in enumerate(groups.items()):
        names.append(name)
        for lab in labels:
            lab = int(lab)
            if lab < 0 or lab >= MAX_LABELS:
                raise ValueError("labels are integers 0 .. %d, got %d" % (MAX_LABELS - 1, lab))
            if lab in table:
                raise ValueError("label %d is in two groups" % lab)
            table[lab] = g
    if not 1 <= len(names) <= MAX_GROUPS or not table:
        raise ValueError("1 to %d groups with at least one label" % MAX_GROUPS)
    t = np.full(max(table) + 1, -1, dtype=np.int32)
    for lab, g in table.items():
        t[lab] = g
    return names, t


def _z_points(levels, bins):
    nd = NormalDist()
    levels = [float(v) for v in levels]
    if not 1 <= len(levels) <= MAX_LEVELS or not all(0.0 < v < 1.0 for v in levels):
        raise ValueError("1 to %d coverage levels inside (0, 1)" % MAX_LEVELS)
    if not 1 <= int(bins) <= MAX_BINS:
        raise ValueError("1 to %d PIT bins" % MAX_BINS)
    z_level = np.array([nd.inv_cdf(0.5 + 0.5 * v) for v in levels], dtype=np.float64)
    z_edge = np.array([nd.inv_cdf(i / float(bins)) for i in range(1, int(bins))], dtype=np.float64)
    return levels, z_level, z_edge


def _quantile_levels(levels, n_groups):
    levels = [float(v) for v in (levels if np.ndim(levels) else [levels])]
    if not 1 <= len(levels) <= MAX_QUANTILES or len(levels) * n_groups > MAX_TARGETS or not all(0.0 < v <= 1.0 for v in levels):
        raise ValueError("1 to %d levels inside (0, 1], at most %d (group, level) pairs" % (MAX_QUANTILES, MAX_TARGETS))
    return levels


# ---------------------------------------------------------------------------------------------- host backend
class _HostRows:
    """The rows of a call on the host: validity, group and the law's terms per position, in the kernels' own expressions."""

    def __init__(self, results, cols, label_col, table, vm, row_index=None, score_col=None):
        A = _as_numpy(results, np.float64)
        if A.ndim != 2:
            raise ValueError("results must be a 2-D array")
        N = A.shape[0]
        need = max(cols + [label_col if table is not None else 0, score_col if score_col is not None else 0])
        if need >= A.shape[1] or min(cols) < 0:
            raise ValueError("results has %d columns, column %d is asked for" % (A.shape[1], need))
        if row_index is None:
            inside = np.ones(N, dtype=bool)
            R = A
        else:
            idx = _as_numpy(row_index, np.int64).reshape(-1)
            inside = (idx >= 0) & (idx < N)
            R = A[np.where(inside, idx, 0)] if N > 0 else np.full((idx.size, A.shape[1]), np.nan)
        self.n = R.shape[0]
        with np.errstate(all="ignore"):
            if table is None:
                g = np.zeros(self.n, dtype=np.int64)
            else:
                lab = R[:, label_col]
                okl = (lab >= 0.0) & (lab < float(len(table)))
                g = np.where(okl, np.asarray(table, np.int64)[np.where(okl, lab, 0.0).astype(np.int64)], -1)
            g = np.where(inside, g, -1)
            if score_col is not None:
                x = R[:, score_col]
                self.valid = (g >= 0) & np.isfinite(x)
                self.score = np.where(self.valid, x, np.nan)
                self.g = np.where(self.valid, g, -1)
                return
            yt, yp, ale, epi = (R[:, c] for c in cols)
            v = (vm[0] * ale) * ale + (vm[1] * epi) * epi + vm[2]
            self.valid = (g >= 0) & np.isfinite(yt) & np.isfinite(yp) & np.isfinite(v) & (v > 0.0)
            nan = np.full(self.n, np.nan)
            self.g = np.where(self.valid, g, -1)
            self.v = np.where(self.valid, v, nan)
            self.yp = np.where(self.valid, yp, nan)
            self.s = np.sqrt(self.v)
            self.r = np.where(self.valid, yt - yp, nan)
            self.z = self.r / self.s

    def terms(self):
        """Per-row Phi(z), nll and crps (NaN on rows that are not valid)."""
        with np.errstate(all="ignore"):
            z, zz = self.z, self.z * self.z
            phi = 0.5 * np.array([math.erfc(x) if x == x else float("nan") for x in (-z * INV_SQRT2).tolist()], dtype=np.float64).reshape(z.shape)
            pdf = np.exp(-0.5 * zz) * INV_SQRT2PI
            nll = 0.5 * (LOG_2PI + np.log(self.v) + zz)
            crps = self.s * (z * (2.0 * phi - 1.0) + 2.0 * pdf - INV_SQRTPI)
        return phi, nll, crps


def _rank(n_g, level, conformal):
    if n_g == 0:
        return 0
    if conformal:
        return int(math.ceil(float(n_g + 1) * level))
    return min(max(int(math.ceil(float(n_g) * level)), 1), n_g)


def _fsum(x):
    """math.fsum, which refuses inf - inf and an overflowing partial sum; numpy's answer (NaN, +-inf) there."""
    try:
        return math.fsum(x)
    except (ValueError, OverflowError):
        with np.errstate(all="ignore"):
            return float(np.sum(np.asarray(x, dtype=np.float64)))


def _host_score(H, G, z_level, z_edge):
    phi, nll, crps = H.terms()
    with np.errstate(all="ignore"):
        per = [np.ones(H.n), H.r, H.r * H.r, H.s, H.v, H.z, H.z * H.z, nll, crps]
    sums = np.zeros((G, len(SUM_NAMES)))
    n = np.zeros(G, np.int64)
    hits = np.zeros((G, len(z_level)), np.int64)
    pit = np.zeros((G, len(z_edge) + 1), np.int64)
    az = np.abs(H.z)
    for g in range(G):
        m = H.g == g
        n[g] = int(m.sum())
        for i, t in enumerate(per):
            sums[g, i] = _fsum(t[m].tolist())
        for l, zl in enumerate(z_level):
            hits[g, l] = int((az[m] <= zl).sum())
        b = (z_edge[None, :] <= H.z[m][:, None]).sum(axis=1)
        pit[g] = np.bincount(b, minlength=len(z_edge) + 1)
    return sums, n, hits, pit, int(H.n - n.sum()), dict(z=H.z, pit=phi, crps=crps, nll=nll)


def _host_quantiles(H, score, G, levels, conformal):
    Q = len(levels)
    q = np.full((G, Q), np.nan)
    rank = np.zeros((G, Q), np.int64)
    n = np.zeros(G, np.int64)
    for g in range(G):
        sc = np.sort(score[H.g == g] + 0.0)                   # -0 + 0 = +0: the key map's canonical zero
        n[g] = sc.size
        for i, lv in enumerate(levels):
            k = _rank(sc.size, lv, conformal)
            rank[g, i] = k
            if sc.size:
                q[g, i] = np.inf if k > sc.size else sc[k - 1]
    return q, rank, n, int(H.n - n.sum())


def _host_update(state, W, H, level, gamma, alpha_min, alpha_max, learn):
    """One chunk (at most MAX_CHUNK rows) against the state words (uint64 [STATE_HEADER + W]); the kernel's own steps."""
    f = state.view(np.float64)
    i = state.view(np.int64)
    q, alpha, fill, pos = float(f[ST_Q]), float(f[ST_ALPHA]), int(i[ST_FILL]), int(i[ST_POS])
    with np.errstate(all="ignore"):
        az = np.abs(H.z)
        half = q * H.s
        lo, hi = H.yp - half, H.yp + half
        flag = np.where(H.valid, np.where(az <= q, 0, 1), -1).astype(np.int32)
    if learn:
        sc = az[H.valid]
        nv, nm = int(sc.size), int((flag == 1).sum())
        e = np.arange(max(0, nv - W), nv)
        f[STATE_HEADER + (pos + e) % W] = sc[e]
        m = min(fill + nv, W)
        if nv > 0:
            alpha = alpha + gamma * ((1.0 - level) - float(nm) / float(nv))
            alpha = min(max(alpha, alpha_min), alpha_max)
        k = max(1, int(math.ceil(float(m + 1) * (1.0 - alpha))))
        f[ST_Q] = np.inf if k > m else np.sort(f[STATE_HEADER:STATE_HEADER + m])[k - 1]
        f[ST_ALPHA] = alpha
        i[ST_FILL], i[ST_POS] = m, (pos + nv) % W
        i[ST_VALID] += nv
        i[ST_MISS] += nm
    return lo, hi, H.z, flag


# ---------------------------------------------------------------------------------------------- device backend
def _c_doubles(v):
    v = [float(x) for x in v]
    return (ctypes.c_double * max(len(v), 1))(*v)


class _DevCall:
    """What the three entry points share: the row head, the group arguments and the variance model."""

    def __init__(self, results, cols, label_col, table, vm, row_index):
        self.torch, self._lib, self.lib = _torch_lib()
        self.rows = _DevRows(self.torch, results, cols, row_index)
        if table is not None and not 0 <= label_col < self.rows.arr.shape[1]:
            raise ValueError("results has %d columns, label column %d is asked for" % (self.rows.arr.shape[1], label_col))
        self.n, self.dev = self.rows.n, self.rows.dev
        self.G = 1 if table is None else int(max(table)) + 1
        self.c_table = None if table is None else (ctypes.c_int * len(table))(*[int(v) for v in table])
        self.groups = (-1, None, 0, 1) if table is None else (label_col, self.c_table, len(table), self.G)
        self.vm = _c_doubles(vm)

    def out(self, shape, dtype, fill=None):
        t = self.torch.empty(shape, dtype=dtype, device=self.dev)
        return t if fill is None else t.fill_(fill)

    def workspace(self, Q):
        wb = self.lib.pinn_unc_workspace_bytes(self.n, self.G, Q)
        return self.out(wb, self.torch.uint8), wb


def _device_score(results, cols, label_col, table, vm, row_index, G, z_level, z_edge, per_row):
    d = _DevCall(results, cols, label_col, table, vm, row_index)
    torch, L, B = d.torch, len(z_level), len(z_edge) + 1
    with torch.cuda.device(d.dev):
        sums = d.out((G, len(SUM_NAMES)), torch.float64, 0.0)
        n, hits, pit, skipped = (d.out(s, torch.int64, 0) for s in ((G,), (G, L), (G, B), (1,)))
        rows = [d.out((d.n,), torch.float64) for _ in range(4)] if per_row else [None] * 4
        ws, wb = d.workspace(1)
        call("pinn_unc_score", *d.rows.head(), *d.groups, d.vm, _c_doubles(z_level), L, _c_doubles(z_edge), B, sums, n, hits, pit, skipped,
             *rows, ws, wb)
        per = dict(zip(("z", "pit", "crps", "nll"), rows)) if per_row else None
        return sums.cpu().numpy(), n.cpu().numpy(), hits.cpu().numpy(), pit.cpu().numpy(), int(skipped.item()), per


def _device_quantiles(results, cols, label_col, table, vm, row_index, G, kind, score_col, levels, conformal):
    d = _DevCall(results, cols, label_col, table, vm, row_index)
    torch, Q = d.torch, len(levels)
    if kind == KINDS["column"] and not 0 <= score_col < d.rows.arr.shape[1]:
        raise ValueError("results has %d columns, column %d is asked for" % (d.rows.arr.shape[1], score_col))
    with torch.cuda.device(d.dev):
        q = d.out((G, Q), torch.float64, float("nan"))
        rank, n, skipped = (d.out(s, torch.int64, 0) for s in ((G, Q), (G,), (1,)))
        ws, wb = d.workspace(Q)
        call("pinn_unc_quantiles", *d.rows.head(), *d.groups, d.vm, kind, max(score_col, 0), _c_doubles(levels), Q, 1 if conformal else 0,
             q, rank, n, skipped, ws, wb)
        return q.cpu().numpy(), rank.cpu().numpy(), n.cpu().numpy(), int(skipped.item())


def _device_update(state, W, results, cols, vm, row_index, level, gamma, alpha_min, alpha_max, learn):
    """Every chunk of at most MAX_CHUNK positions in turn, one launch each; lo, hi, z, flag as device tensors."""
    d = _DevCall(results, cols, -1, None, vm, row_index)
    torch = d.torch
    with torch.cuda.device(d.dev):
        lo, hi, z = (d.out((d.n,), torch.float64) for _ in range(3))
        flag = d.out((d.n,), torch.int32)
        arr, ld, n_arr, c_cols, D, ridx, n = d.rows.head()
        for j0 in range(0, n, MAX_CHUNK):
            m = min(MAX_CHUNK, n - j0)
            if d.rows.ridx is None:
                head = (arr + j0 * ld * 8, ld, n_arr - j0, c_cols, D, None, m)
            else:
                head = (arr, ld, n_arr, c_cols, D, ridx + j0 * 8, m)
            call("pinn_unc_update", *head, d.vm, level, gamma, alpha_min, alpha_max, W, 1 if learn else 0, state, lo[j0:], hi[j0:], z[j0:],
                 flag[j0:])
    return lo, hi, z, flag


# ---------------------------------------------------------------------------------------------- public interface
def score_uncertainty(results, levels=LEVELS, bins=20, groups=None, var_model=(1.0, 1.0, 0.0), row_index=None, columns=None,
                      backend="auto", per_row=False):
    """Reliability of the predictive law per group: {name: UncertaintyReport}.  With per_row=True also a dict of the per-row
    z, pit (= Phi(z)), crps and nll (NaN on rows that are not valid): numpy arrays from the host backend, device tensors from
    the device backend.  Rows are read in place from `results` (`row_index`: a gather list; `columns`: (y_true, y_pred, ale,
    epi, label) when the array is not laid out as the results array)."""
    names, table = _group_table(groups)
    cols, label_col = _columns(columns, table is not None)
    vm = _var_model(var_model)
    levels, z_level, z_edge = _z_points(levels, bins)
    G = len(names)
    n_pos = np.shape(results)[0] if row_index is None else int(np.shape(row_index)[0])
    if _pick_backend(backend, results, n_pos) == "device":
        sums, n, hits, pit, skipped, per = _device_score(results, cols, label_col, table, vm, row_index, G, z_level, z_edge, per_row)
    else:
        H = _HostRows(results, cols, label_col, table, vm, row_index)
        sums, n, hits, pit, skipped, per = _host_score(H, G, z_level, z_edge)
    rep = {name: UncertaintyReport(name, levels, sums[g], n[g], hits[g], pit[g], skipped) for g, name in enumerate(names)}
    return (rep, per) if per_row else rep


def conformal_quantiles(results, levels=(0.9,), kind="abs_z", conformal=True, groups=None, var_model=(1.0, 1.0, 0.0), column=None,
                        row_index=None, columns=None, backend="auto"):
    """Exact order statistics of a score per group -> Quantiles.  kind "abs_z": |z| (q[.] is the half-width of the band
    y_pred -+ q s in units of s), "z": signed, "column": the raw value of `column` (valid = finite).  conformal=True takes the
    ceil((n + 1) level)-th smallest of a group's n scores (+inf when that is beyond n): on exchangeable rows the band then
    covers a fresh row with probability >= level.  conformal=False takes the ceil(n level)-th, clipped to [1, n]."""
    if kind not in KINDS:
        raise ValueError("kind is one of %s" % (tuple(KINDS),))
    if (kind == "column") != (column is not None):
        raise ValueError("kind='column' goes with column=, and only it")
    names, table = _group_table(groups)
    cols, label_col = _columns(columns, table is not None)
    vm = _var_model(var_model)
    G = len(names)
    levels = _quantile_levels(levels, G)
    score_col = -1 if column is None else int(column)
    n_pos = np.shape(results)[0] if row_index is None else int(np.shape(row_index)[0])
    if _pick_backend(backend, results, n_pos) == "device":
        out = _device_quantiles(results, cols, label_col, table, vm, row_index, G, KINDS[kind], score_col, levels, conformal)
    else:
        H = _HostRows(results, cols, label_col, table, vm, row_index, score_col=None if column is None else score_col)
        with np.errstate(all="ignore"):
            score = H.score if kind == "column" else (np.abs(H.z) if kind == "abs_z" else H.z)
        out = _host_quantiles(H, score, G, levels, conformal)
    return Quantiles(*out, names, levels, kind, conformal)


def _fresh_state(W, level, q0):
    st = np.zeros(STATE_HEADER + W, dtype=np.uint64)
    f = st.view(np.float64)
    f[ST_ALPHA], f[ST_Q] = 1.0 - level, q0
    return st


def conformal_band(results, q, var_model=(1.0, 1.0, 0.0), row_index=None, columns=None, backend="auto"):
    """lo, hi = y_pred -+ q s per row (NaN on rows that are not valid), q a half-width in units of s as conformal_quantiles
    with kind "abs_z" gives it.  The device backend runs the monitor's kernel without learning, chunk by chunk."""
    cols, _ = _columns(columns, False)
    vm = _var_model(var_model)
    q = float(q)
    n_pos = np.shape(results)[0] if row_index is None else int(np.shape(row_index)[0])
    if _pick_backend(backend, results, n_pos) == "device":
        torch = _torch_lib()[0]
        arr_dev = results.device if _is_tensor(results) else "cuda"
        state = torch.from_numpy(_fresh_state(1, 0.5, q).view(np.int64)).to(arr_dev)
        lo, hi, _, _ = _device_update(state, 1, results, cols, vm, row_index, 0.5, 0.0, 0.0, 1.0, False)
        return lo, hi
    H = _HostRows(results, cols, -1, None, vm, row_index)
    with np.errstate(all="ignore"):
        half = q * H.s
        return H.yp - half, H.yp + half


class BandUpdate:
    """What UncertaintyMonitor.update returns: lo, hi, z per row, miss (1: y_true outside the band, 0: inside, -1: the row is
    not valid), and q, alpha as they stand after the chunk (None from the device backend, which does not synchronise: read
    the monitor's own `q` / `alpha` when they are needed)."""

    def __init__(self, lo, hi, z, miss, q, alpha):
        self.lo, self.hi, self.z, self.miss, self.q, self.alpha = lo, hi, z, miss, q, alpha


class UncertaintyMonitor:
    """The online band.  Every row gets y_pred -+ q_t s with the q_t in force when its chunk arrives; with learn=True the chunk's
    scores |z| then enter a ring of the last `window` scores, alpha moves by gamma ((1 - level) - the chunk's miss rate)
    inside [alpha_min, alpha_max] (adaptive conformal inference; gamma = 0 is plain rolling split-conformal), and q becomes
    the ceil((m + 1) (1 - alpha))-th smallest of the m ring entries (+inf beyond m, so an empty ring gives an infinite band
    unless `init`, a Quantiles of kind "abs_z", supplies q_0).  A chunk is at most 2048 rows on the device; longer ones are
    taken 2048 rows at a time, each part as a chunk of its own, by both backends.  `columns` are (y_true, y_pred, ale, epi),
    so chunks shaped like the results array go in as they are."""

    def __init__(self, level=0.9, window=1024, var_model=(1.0, 1.0, 0.0), gamma=0.0, init=None, alpha_min=0.0, alpha_max=1.0,
                 columns=None, backend="auto"):
        if not 0.0 < level < 1.0 or not 1 <= int(window) <= MAX_WINDOW or not (math.isfinite(gamma) and gamma >= 0.0):
            raise ValueError("0 < level < 1, 1 <= window <= %d, gamma >= 0" % MAX_WINDOW)
        if not 0.0 <= alpha_min <= alpha_max <= 1.0:
            raise ValueError("0 <= alpha_min <= alpha_max <= 1")
        if backend not in ("auto", "device", "host"):
            raise ValueError("backend must be 'auto', 'device' or 'host'")
        self.level, self.window, self.gamma = float(level), int(window), float(gamma)
        self.alpha_min, self.alpha_max = float(alpha_min), float(alpha_max)
        self.vm = _var_model(var_model)
        self.cols, _ = _columns(columns, False)
        self.backend = backend
        q0 = float("inf")
        if init is not None:
            q0 = float(np.asarray(init.q if isinstance(init, Quantiles) else init).reshape(-1)[0])
        self._state = _fresh_state(self.window, self.level, q0)

    def _resolve(self, rows):
        if self.backend == "auto":
            self.backend = _pick_backend("auto", rows)
        if self.backend == "device" and isinstance(self._state, np.ndarray):
            torch = _torch_lib()[0]
            self._state = torch.from_numpy(self._state.view(np.int64)).to(rows.device if _is_tensor(rows) and rows.is_cuda else "cuda")

    def update(self, rows, learn=True):
        self._resolve(rows)
        if self.backend == "device":
            lo, hi, z, flag = _device_update(self._state, self.window, rows, self.cols, self.vm, None, self.level, self.gamma,
                                             self.alpha_min, self.alpha_max, learn)
            return BandUpdate(lo, hi, z, flag, None, None)
        A = _as_numpy(rows, np.float64)
        out = []
        for j0 in range(0, A.shape[0], MAX_CHUNK):
            H = _HostRows(A[j0:j0 + MAX_CHUNK], self.cols, -1, None, self.vm)
            out.append(_host_update(self._state, self.window, H, self.level, self.gamma, self.alpha_min, self.alpha_max, learn))
        if not out:
            out = [(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, np.int32))]
        lo, hi, z, flag = (np.concatenate(v) for v in zip(*out))
        return BandUpdate(lo, hi, z, flag, self.q, self.alpha)

    def state_words(self):
        """The state as the kernel keeps it: uint64 words, header then ring (a host copy)."""
        if isinstance(self._state, np.ndarray):
            return self._state.copy()
        return self._state.cpu().numpy().view(np.uint64).copy()

    @property
    def q(self):
        return float(self.state_words().view(np.float64)[ST_Q])

    @property
    def alpha(self):
        return float(self.state_words().view(np.float64)[ST_ALPHA])

    @property
    def n_valid(self):
        return int(self.state_words().view(np.int64)[ST_VALID])

    @property
    def n_miss(self):
        return int(self.state_words().view(np.int64)[ST_MISS])
