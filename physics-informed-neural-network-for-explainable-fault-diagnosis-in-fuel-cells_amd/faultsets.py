"""Which faults can still be true, and is it none of them?  Conformal fault sets with class-conditional coverage and the
rejection of unknown faults, on top of any diagnoser's posterior `y_prob` and, for a fitted `DeviceGMM`, of its densities.

Definitions (the same words as include/pinn_hip.h; csrc/pinn_faultsets.hip is the device backend):

Inputs.  `y_prob [n, C]` float64 with 1 <= C <= 16, classes `y` int64.  A row is *missing* when any entry is non-finite or
negative or all entries are zero (temporal's rule), or when one of its scores is NaN: it gets counts -1, empty masks,
missing = 1, and enters no tally.  A calibration row that is missing, or whose y lies outside [0, C), is skipped and counted
(`n_skipped`).

Scores.  float64, every operation rounded on its own, every sum in ascending class or component order.
  lac      s_c = 1 - p_c.
  margin   s_c = max_{k != c} p_k - p_c; for C = 1 it is -p_c.
  aps      s_c = sum_{k : p_k > p_c or (p_k == p_c and k < c)} p_k + u p_c, the sum from 0 in ascending k.  u = 1 when
           randomized=False; otherwise u = ((w0 << 21) | (w1 >> 11)) 2^-53 with (w0, w1, ., .) the Philox4x32-10 block
           (anomaly.philox4x32_10) of the counter (row_lo, row_hi, kind, 0) under the key `seed`, row = first + the position
           in the call (so chunking changes nothing), kind = DRAW_CAL for calibration rows and DRAW_TEST for test rows.
  density  for a fitted mixture with label map m = comp_fault_prob [K, C]:
           s_c = -(logsumexp_{k : m_kc > 0}(lp_k + log m_kc) - log pi_c), lp_k = log(w_k N(x | mu_k, Sigma_k)) as the mixture's
           E-step forms it, the logsumexp as max, sum in ascending k, log; pi_c = sum_k w_k m_kc, and s_c = +inf when pi_c = 0.
           log m_kc and log pi_c are computed once on the host and handed to both backends.  The pooled typicality score is
           s_any = -log_prob_norm.  A row of this kind is missing when a feature is non-finite or its gather index lies
           outside the array.

Calibration.  T_c: the ascending sorted s_{y_i}(x_i) + 0 (so a zero is +0) of the used calibration rows with y_i = c, n_c of
them; T_any the same, pooled, for s_any.  Tables hold no NaN.

p-value and set.  count_c(x) = #{t in T_c : t >= s_c(x)} = n_c - #{t < s_c(x)}, p_c = (count_c + 1) / (n_c + 1).  At level l,
alpha = 1 - l, class c is in the set iff p_c > alpha, decided in integers: count_c >= kmin[c][l] = floor(alpha (n_c + 1)),
computed once in exact rational arithmetic from the float's value.  kmin = 0: the class can never be excluded at that level
(too few calibration rows), reported as can_reject[c][l] = False.  Guarantee: P(y in set | y = c) >= l for rows exchangeable
with class c's calibration rows.  A row that is not missing is *novel* at a level when its set is empty there.

backend="host" is float64 numpy and the referee; "device" runs the HIP kernels; "auto" follows _device._pick_backend.
Counts, masks and tallies are integers and bit-identical between the backends for lac, margin and aps; the density score
passes through exp and log, so a count can differ where a calibration score lies within a few spacings of the test score.
Importing this module needs numpy only.
"""
import ctypes
from fractions import Fraction

import numpy as np

from ._device import _DevRows, _as_numpy, _is_tensor, _pick_backend, _torch_lib, call, columns_of
from .anomaly import philox4x32_10

KINDS = {"lac": 0, "margin": 1, "aps": 2, "density": 3}
# limits and constants of csrc/pinn_faultsets.hip (include/pinn_hip.h: PINN_FS_*)
MAX_CLASSES, MAX_LEVELS, MAX_CAL, TILE, MAX_BLOCKS, LINE, HEADER = 16, 8, 1 << 20, 256, 1024, 16, 64
DRAW_CAL, DRAW_TEST = 3, 4               # Philox draw kinds (0, 1: the isolation forest's, 2: the ROC bootstrap's)
REGIMES = {"auto": 0, "lds": 1, "sampled": 2, "global": 3}
LDS_ENTRIES = 7680                       # table entries (regime "lds") or sampled entries (regime "sampled") a forced regime may stage
AUTO_LDS_ENTRIES, STAGE_MIN_ROWS = 1536, 1 << 20      # "auto" stages tables of at most so many entries under at least so many rows
H_MAGIC, H_C, H_KIND, H_SEED, H_RANDOMIZED, H_SKIPPED, H_STATUS, H_NCAL, H_OFFSET = 0, 1, 2, 3, 4, 5, 6, 16, 40
MAGIC = 0x46534554
# int64 words of the tallies: n [16], covered [16][8], size_hist [8][17], singleton_correct [8], outside_n, outside_novel [8]
T_N, T_COVERED, T_HIST, T_SINGLE, T_OUT_N, T_OUT_NOVEL, TALLY_WORDS = 0, 16, 144, 280, 288, 289, 304
MAX_CHUNK = 2048
_M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------- results
class SetCalibration:
    """The sorted calibration scores per class.  `n_cal [C]`, `n_any` (the pooled table of the density kind), `n_skipped`;
    `table(c)` is class c's table as numpy (c = "any": the pooled one)."""

    def __init__(self, kind, n_classes, n_cal, n_any, n_skipped, seed, randomized, tables=None, state=None):
        self.kind, self.n_classes, self.seed, self.randomized = kind, int(n_classes), int(seed), bool(randomized)
        self.n_cal, self.n_any, self.n_skipped = np.asarray(n_cal, np.int64), int(n_any), int(n_skipped)
        self._tables, self._state = tables, state

    @property
    def backend(self):
        return "host" if self._state is None else "device"

    def _counts(self):
        return [int(v) for v in self.n_cal] + [self.n_any]

    def table(self, c):
        c = self.n_classes if c == "any" else int(c)
        if not 0 <= c <= self.n_classes:
            raise ValueError("class %d of %d" % (c, self.n_classes))
        if self._state is None:
            return self._tables[c].copy()
        off, cnt = _offsets(self._counts()), self._counts()
        return self._state[HEADER + off[c]:HEADER + off[c] + cnt[c]].cpu().numpy()

    def _host_tables(self):
        return self._tables if self._state is None else [self.table(c) for c in range(self.n_classes)] + [self.table("any")]

    def _device_state(self, torch, dev):
        if self._state is None:
            cnt = self._counts()
            off = _offsets(cnt)
            s = np.zeros(HEADER + off[-1] + _pad(cnt[-1]))
            for c, t in enumerate(self._tables):
                s[HEADER + off[c]:HEADER + off[c] + cnt[c]] = t
                s[HEADER + off[c] + cnt[c]:HEADER + off[c] + _pad(cnt[c])] = np.inf
            return torch.from_numpy(s).to(dev)
        return self._state if self._state.device == dev else self._state.to(dev)

    def __repr__(self):
        return "SetCalibration(kind=%s, n_cal=%s, n_skipped=%d)" % (self.kind, self.n_cal.tolist(), self.n_skipped)


class PValues:
    """count [n, C] int32 (-1 on a missing row), p = (count + 1) / (n_cal + 1) [n, C] float64 (NaN on a missing row)."""

    def __init__(self, count, n_cal):
        self.count, self.n_cal = count, np.asarray(n_cal, np.int64)
        if _is_tensor(count):
            import torch
            den = torch.from_numpy(self.n_cal + 1).to(count.device).to(torch.float64)
            p = (count + 1).to(torch.float64) / den
            self.p = torch.where(count < 0, torch.full_like(p, float("nan")), p)
        else:
            with np.errstate(all="ignore"):
                self.p = np.where(count < 0, np.nan, (count + 1).astype(np.float64) / (self.n_cal + 1).astype(np.float64))


class FaultSets:
    """mask [n, L] uint16 (bit c: class c is in the set), size [n, L] uint8, novel [n, L] bool (the set is empty and the row is
    not missing), missing [n] bool, count [n, C] int32, can_reject [C, L] bool (False: kmin = 0, the class is in every set).
    From the density kind also count_any [n] and p_any [n], the pooled typicality p-value.  Device tensors carry the mask as
    int16 with the same 16 bits (torch has few operations on uint16): with 16 classes bit 15 makes such a word negative, so
    test bits with (mask >> c) & 1 or through `members`, or reinterpret with mask.view(torch.uint16); numpy results are uint16."""

    def __init__(self, mask, size, novel, missing, count, can_reject, levels, n_cal, count_any=None, n_any=0):
        self.mask, self.size, self.novel, self.missing, self.count = mask, size, novel, missing, count
        self.can_reject, self.levels, self.n_cal = can_reject, tuple(levels), np.asarray(n_cal, np.int64)
        self.count_any, self.n_any = count_any, int(n_any)

    @property
    def p_any(self):
        if self.count_any is None:
            return None
        c = self.count_any
        if _is_tensor(c):
            import torch
            p = (c + 1).to(torch.float64) / float(self.n_any + 1)
            return torch.where(c < 0, torch.full_like(p, float("nan")), p)
        return np.where(c < 0, np.nan, (c + 1) / float(self.n_any + 1))

    def members(self, i, level=None):
        """The classes in row i's set at `level` (by default the first level), ascending."""
        l = 0 if level is None else self.levels.index(level)
        m = int(self.mask[i, l])
        return [c for c in range(MAX_CLASSES) if (m >> c) & 1]


class SetReport:
    """Tallies of sets against known classes, all int64: n [C] rows of class c, covered [C, L] of them with c in the set,
    size_hist [L, C + 1] set sizes and singleton_correct [L] over the rows with y inside [0, C); outside_n and outside_novel [L]
    over the rows with y outside (a held-back condition).  Missing rows enter nothing."""

    def __init__(self, tally, C, levels, can_reject):
        t = np.asarray(tally, np.int64)
        L = len(levels)
        self.levels, self.can_reject = tuple(levels), can_reject
        self.n = t[T_N:T_N + C].copy()
        self.covered = t[T_COVERED:T_HIST].reshape(MAX_CLASSES, MAX_LEVELS)[:C, :L].copy()
        self.size_hist = t[T_HIST:T_SINGLE].reshape(MAX_LEVELS, MAX_CLASSES + 1)[:L, :C + 1].copy()
        self.singleton_correct = t[T_SINGLE:T_SINGLE + L].copy()
        self.outside_n = int(t[T_OUT_N])
        self.outside_novel = t[T_OUT_NOVEL:T_OUT_NOVEL + L].copy()

    @property
    def coverage(self):
        with np.errstate(all="ignore"):
            return self.covered / self.n[:, None].astype(np.float64)

    @property
    def mean_size(self):
        with np.errstate(all="ignore"):
            return (self.size_hist * np.arange(self.size_hist.shape[1])).sum(axis=1) / self.size_hist.sum(axis=1).astype(np.float64)

    @property
    def novel_share(self):
        with np.errstate(all="ignore"):
            return self.outside_novel / float(self.outside_n) if self.outside_n else np.full(len(self.levels), np.nan)


# ---------------------------------------------------------------------------------------------- arguments
def _pad(n):
    return (int(n) + LINE - 1) // LINE * LINE


def _offsets(counts):
    """Entry offsets of the tables behind the header: every table starts on a 128-byte line."""
    off, o = [], 0
    for n in counts:
        off.append(o)
        o += _pad(n)
    return off


def _kind(kind, posterior_only=False):
    if kind not in KINDS or (posterior_only and kind == "density"):
        raise ValueError("kind is one of %s%s" % (tuple(k for k in KINDS if not (posterior_only and k == "density")),
                                                  "; the density kind needs the mixture: calibrate_gmm, GMMSetDiagnoser" if posterior_only else ""))
    return KINDS[kind]


def _levels(levels):
    levels = [float(v) for v in (levels if np.ndim(levels) else [levels])]
    if not 1 <= len(levels) <= MAX_LEVELS or not all(0.0 < v < 1.0 for v in levels):
        raise ValueError("1 to %d coverage levels inside (0, 1)" % MAX_LEVELS)
    return levels


def kmin_table(n_cal, levels):
    """kmin [C, L] = floor((1 - level) (n_c + 1)) in exact rational arithmetic from each float's value."""
    return np.array([[((1 - Fraction(lv)) * (int(n) + 1)).__floor__() for lv in levels] for n in n_cal], dtype=np.int64).reshape(len(n_cal), len(levels))


def _prob(y_prob, C=None):
    P = _as_numpy(y_prob, np.float64)
    if P.ndim != 2 or not 1 <= P.shape[1] <= MAX_CLASSES or (C is not None and P.shape[1] != C):
        raise ValueError("y_prob must be [n, %s]" % ("1..%d classes" % MAX_CLASSES if C is None else C))
    return P


# ---------------------------------------------------------------------------------------------- host backend
def _missing(P):
    with np.errstate(all="ignore"):
        return ~np.all(np.isfinite(P) & (P >= 0.0), axis=1) | ~np.any(P > 0.0, axis=1)


def uniforms(seed, draw, first, n):
    """u of the aps score for the rows first .. first + n - 1."""
    rows = np.uint64(first) + np.arange(n, dtype=np.uint64)
    w0, w1, _, _ = philox4x32_10(rows & _M32, rows >> np.uint64(32), draw, 0, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    return ((w0 << np.uint64(21)) | (w1 >> np.uint64(11))).astype(np.float64) * 2.0 ** -53


def _host_scores(P, kind, u=None):
    """[n, C] scores of the three posterior kinds, NaN on missing rows; `u` [n] or None for 1."""
    n, C = P.shape
    miss = _missing(P)
    with np.errstate(all="ignore"):
        if kind == KINDS["lac"]:
            S = 1.0 - P
        elif kind == KINDS["margin"]:
            if C == 1:
                S = -P
            else:
                S = np.empty_like(P)
                for c in range(C):
                    S[:, c] = np.max(np.delete(P, c, axis=1), axis=1) - P[:, c]
        else:
            S = np.empty_like(P)
            for c in range(C):
                acc = np.zeros(n)
                for k in range(C):
                    sel = (P[:, k] > P[:, c]) | ((P[:, k] == P[:, c]) & (k < c))
                    acc = np.where(sel, acc + P[:, k], acc)
                S[:, c] = acc + (P[:, c] if u is None else u * P[:, c])
    S = np.where(miss[:, None], np.nan, S)
    return S, miss | np.isnan(S).any(axis=1)


def _log_map(weights, comp_map):
    """log m [K, C] (-inf where m = 0) and log pi [C] (-inf where pi = 0), pi_c = sum_k w_k m_kc in ascending k."""
    m = np.ascontiguousarray(_as_numpy(comp_map, np.float64))
    w = _as_numpy(weights, np.float64).reshape(-1)
    pi = np.zeros(m.shape[1])
    for k in range(m.shape[0]):
        pi = pi + w[k] * m[k]
    with np.errstate(divide="ignore"):
        return np.where(m > 0.0, np.log(np.where(m > 0.0, m, 1.0)), -np.inf), np.where(pi > 0.0, np.log(np.where(pi > 0.0, pi, 1.0)), -np.inf)


def _host_lp(X, weights, means, pchol):
    """lp [n, K] = log(w_k N(x | mu_k, Sigma_k)) and log_prob_norm [n], diagnosis._host_estep's formulas."""
    n, D = X.shape
    K = means.shape[0]
    lp = np.empty((n, K))
    with np.errstate(all="ignore"):
        for k in range(K):
            y = (X - means[k]) @ pchol[k]
            lp[:, k] = -0.5 * (D * np.log(2 * np.pi) + np.sum(y * y, axis=1)) + np.sum(np.log(np.diag(pchol[k])))
        lp += np.log(weights)
        m = lp.max(axis=1)
        lpn = np.where(m == -np.inf, m, np.log(np.exp(lp - m[:, None]).sum(axis=1)) + m)
    return lp, lpn


def _host_density(lp, logm, logpi):
    """[n, C] density scores from lp [n, K]."""
    n, K = lp.shape
    C = logm.shape[1]
    S = np.empty((n, C))
    with np.errstate(all="ignore"):
        for c in range(C):
            ks = [k for k in range(K) if logm[k, c] > -np.inf]
            if not ks or logpi[c] == -np.inf:
                S[:, c] = np.inf
                continue
            t = np.stack([lp[:, k] + logm[k, c] for k in ks], axis=1)
            m = t.max(axis=1)
            acc = np.zeros(n)
            for i in range(len(ks)):
                acc = acc + np.exp(t[:, i] - m)
            lse = np.where(m == -np.inf, m, np.log(acc) + m)
            S[:, c] = -(lse - logpi[c])
    return S


def _host_build(S, y, C, any_score=None):
    """tables (C of them and the pooled one), n_skipped, from the score matrix and the classes."""
    yh = _as_numpy(y).astype(np.int64).reshape(-1)
    if yh.size != S.shape[0]:
        raise ValueError("y must hold one class per row")
    inside = (yh >= 0) & (yh < C)
    pick = S[np.arange(S.shape[0]), np.where(inside, yh, 0)] if S.shape[0] else np.zeros(0)
    used = inside & ~np.isnan(pick)
    if any_score is not None:
        used &= ~np.isnan(any_score)
    tables = [np.sort(pick[used & (yh == c)] + 0.0) for c in range(C)]
    tables.append(np.sort(any_score[used] + 0.0) if any_score is not None else np.zeros(0))
    if max(t.size for t in tables[:C]) > MAX_CAL:
        raise ValueError("at most %d calibration rows per class" % MAX_CAL)
    return tables, int(S.shape[0] - used.sum())


def _host_rank(tables, S, miss, kmin):
    """count [n, C] int32, mask [n, L] uint16, size [n, L] uint8, novel [n, L] bool."""
    n, C = S.shape
    L = kmin.shape[1]
    count = np.full((n, C), -1, np.int32)
    ok = ~miss
    for c in range(C):
        count[ok, c] = tables[c].size - np.searchsorted(tables[c], S[ok, c], side="left")
    mask = np.zeros((n, L), np.uint16)
    size = np.zeros((n, L), np.uint8)
    for l in range(L):
        for c in range(C):
            inc = ok & (count[:, c] >= kmin[c, l])
            mask[:, l] |= (inc.astype(np.uint16) << np.uint16(c))
            size[:, l] += inc.astype(np.uint8)
    return count, mask, size, (size == 0) & ok[:, None]


def _host_tally(mask, size, miss, y, C):
    t = np.zeros(TALLY_WORDS, np.int64)
    yh = _as_numpy(y).astype(np.int64).reshape(-1)
    if yh.size != mask.shape[0]:
        raise ValueError("y must hold one class per row")
    L = mask.shape[1]
    ok = ~miss
    inside = ok & (yh >= 0) & (yh < C)
    out = ok & ~((yh >= 0) & (yh < C))
    cov = t[T_COVERED:T_HIST].reshape(MAX_CLASSES, MAX_LEVELS)
    hist = t[T_HIST:T_SINGLE].reshape(MAX_LEVELS, MAX_CLASSES + 1)
    yi = yh[inside]
    t[T_N:T_N + C] = np.bincount(yi, minlength=C)
    for l in range(L):
        bit = (mask[inside, l].astype(np.int64) >> yi) & 1
        cov[:C, l] = np.bincount(yi, weights=bit, minlength=C).astype(np.int64)
        hist[l, :C + 1] = np.bincount(size[inside, l].astype(np.int64), minlength=C + 1)
        t[T_SINGLE + l] = int(((size[inside, l] == 1) & (bit == 1)).sum())
        t[T_OUT_NOVEL + l] = int((size[out, l] == 0).sum())
    t[T_OUT_N] = int(out.sum())
    return t


# ---------------------------------------------------------------------------------------------- device backend
def _c_ll(v):
    v = [int(x) for x in v]
    return (ctypes.c_longlong * max(len(v), 1))(*v)


def _dev_prob(torch, y_prob):
    t = y_prob if _is_tensor(y_prob) else torch.from_numpy(np.ascontiguousarray(np.asarray(y_prob, dtype=np.float64)))
    if t.dim() != 2 or not 1 <= t.shape[1] <= MAX_CLASSES:
        raise ValueError("y_prob must be [n, 1..%d classes]" % MAX_CLASSES)
    return t.detach().to("cuda" if not t.is_cuda else t.device, torch.float64).contiguous()


def _dev_classes(torch, y, n, dev):
    if y is None:
        return None
    t = y if _is_tensor(y) else torch.from_numpy(np.ascontiguousarray(_as_numpy(y).astype(np.int64).reshape(-1)))
    t = t.detach().to(dev, torch.int64).reshape(-1).contiguous()
    if t.numel() != n:
        raise ValueError("y must hold one class per row")
    return t


class _Outputs:
    """The per-row outputs of a ranking launch, every one optional."""

    def __init__(self, torch, dev, n, C, L, want):
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        self.count = e((n, C), torch.int32) if "count" in want else None
        self.mask = e((n, L), torch.int16) if "mask" in want else None
        self.size = e((n, L), torch.uint8) if "mask" in want else None
        self.novel = e((n, L), torch.uint8) if "mask" in want else None
        self.missing = e((n,), torch.uint8) if "missing" in want else None
        self.scores = e((n, C), torch.float64) if "scores" in want else None
        self.tally = torch.zeros(TALLY_WORDS, dtype=torch.int64, device=dev) if "tally" in want else None

    def args(self, sl=slice(None)):
        s = lambda t: None if t is None else t[sl]
        return (s(self.count), s(self.mask), s(self.size), s(self.novel), s(self.missing), s(self.scores), self.tally)


def _rank_args(cal, kmin, first, draw, regime):
    C, L = kmin.shape if kmin is not None else (cal.n_classes, 0)
    return (_c_ll(cal._counts()), None if kmin is None else _c_ll(kmin.reshape(-1)), L,
            KINDS[cal.kind], 1 if cal.randomized else 0, cal.seed, draw, int(first), REGIMES[regime])


def _device_rank(cal, y_prob, kmin, first, draw, y, want, regime="auto"):
    torch, _lib, lib = _torch_lib()
    P = _dev_prob(torch, y_prob)
    n, C = P.shape
    if C != cal.n_classes:
        raise ValueError("y_prob must be [n, %d]" % cal.n_classes)
    with torch.cuda.device(P.device):
        st = cal._device_state(torch, P.device) if kmin is not None else None
        o = _Outputs(torch, P.device, n, C, 0 if kmin is None else kmin.shape[1], want)
        call("pinn_fs_rank", P, n, C, st, *_rank_args(cal, kmin, first, draw, regime), _dev_classes(torch, y, n, P.device), *o.args())
    return o


def _device_build(torch, S, y, C, kind, seed, randomized, any_score=None):
    """The calibration state on S's device from the score matrix [n, C] (and the pooled scores [n]); one copy of the header
    to the host for the counts."""
    n = S.shape[0]
    lib = _torch_lib()[2]
    if n > C * MAX_CAL:
        raise ValueError("at most %d calibration rows per class" % MAX_CAL)
    with torch.cuda.device(S.device):
        st = torch.zeros(lib.pinn_fs_state_bytes(n, C) // 8, dtype=torch.float64, device=S.device)
        wb = lib.pinn_fs_workspace_bytes(n, C)
        ws = torch.empty(wb, dtype=torch.uint8, device=S.device)
        call("pinn_fs_build", S, any_score, _dev_classes(torch, y, n, S.device), n, C, kind, seed, 1 if randomized else 0, st, ws, wb)
        h = st[:HEADER].cpu().numpy().view(np.int64)
    if h[H_STATUS] != 0:
        raise ValueError("at most %d calibration rows per class" % MAX_CAL)
    return st, h[H_NCAL:H_NCAL + C].copy(), int(h[H_NCAL + C]) if any_score is not None else 0, int(h[H_SKIPPED])


def _to_host(o, kmin):
    """numpy views of a launch's outputs in the host backend's types."""
    g = lambda t: None if t is None else t.cpu().numpy()
    mask = g(o.mask)
    return (g(o.count), None if mask is None else mask.view(np.uint16), g(o.size), None if o.novel is None else g(o.novel).astype(bool),
            None if o.missing is None else g(o.missing).astype(bool))


# ---------------------------------------------------------------------------------------------- public interface
def scores(y_prob, kind="lac", randomized=False, seed=0, first=0, backend="auto", _draw=DRAW_TEST):
    """The conformity scores [n, C] of a posterior kind (NaN on missing rows)."""
    k = _kind(kind, posterior_only=True)
    rnd = bool(randomized) and kind == "aps"
    if _pick_backend(backend, y_prob) == "device":
        cal = SetCalibration(kind, np.shape(y_prob)[1], np.zeros(np.shape(y_prob)[1], np.int64), 0, 0, seed, rnd)
        S = _device_rank(cal, y_prob, None, first, _draw, None, ("scores",)).scores
        return S if _is_tensor(y_prob) else S.cpu().numpy()
    P = _prob(y_prob)
    return _host_scores(P, k, uniforms(seed, _draw, first, P.shape[0]) if rnd else None)[0]


def calibrate(y_prob, y, kind="lac", n_classes=None, randomized=False, seed=0, backend="auto"):
    """Sort the calibration rows' scores of their own class into per-class tables -> SetCalibration."""
    k = _kind(kind, posterior_only=True)
    C = int(np.shape(y_prob)[1] if n_classes is None else n_classes)
    if len(np.shape(y_prob)) != 2 or np.shape(y_prob)[1] != C or not 1 <= C <= MAX_CLASSES:
        raise ValueError("y_prob must be [n, n_classes] with 1..%d classes" % MAX_CLASSES)
    rnd = bool(randomized) and kind == "aps"
    if _pick_backend(backend, y_prob) == "device":
        torch = _torch_lib()[0]
        S = scores(_dev_prob(torch, y_prob), kind, rnd, seed, 0, "device", DRAW_CAL)
        st, n_cal, _, skipped = _device_build(torch, S, y, C, k, seed, rnd)
        return SetCalibration(kind, C, n_cal, 0, skipped, seed, rnd, state=st)
    S = scores(_prob(y_prob), kind, rnd, seed, 0, "host", DRAW_CAL)
    tables, skipped = _host_build(S, y, C)
    return SetCalibration(kind, C, [t.size for t in tables[:C]], 0, skipped, seed, rnd, tables=tables)


def _sets(cal, y_prob, levels, first, y, want, backend, regime="auto"):
    if cal.kind == "density":
        raise ValueError("a density calibration ranks rows of the mixture: GMMSetDiagnoser")
    levels = _levels(levels)
    kmin = kmin_table(cal.n_cal, levels)
    # "auto": a tensor stays where it is, a host array goes where the calibration lies
    be = _pick_backend(backend, y_prob) if backend != "auto" or _is_tensor(y_prob) else cal.backend
    if be == "device":
        return levels, kmin, _device_rank(cal, y_prob, kmin, first, DRAW_TEST, y, want, regime), True
    P = _prob(y_prob, cal.n_classes)
    S, miss = _host_scores(P, KINDS[cal.kind], uniforms(cal.seed, DRAW_TEST, first, P.shape[0]) if cal.randomized else None)
    return levels, kmin, (S, miss, _host_rank(cal._host_tables(), S, miss, kmin)), False


def p_values(cal, y_prob, first=0, backend="auto"):
    """count and p = (count + 1) / (n_cal + 1) per row and class -> PValues."""
    _, _, r, dev = _sets(cal, y_prob, (0.5,), first, None, ("count",), backend)
    if dev:
        return PValues(r.count if _is_tensor(y_prob) else r.count.cpu().numpy(), cal.n_cal)
    return PValues(r[2][0], cal.n_cal)


def prediction_sets(cal, y_prob, levels=(0.9,), first=0, backend="auto", force_regime="auto"):
    """The fault sets of every row at every level -> FaultSets.  `force_regime` ("lds", "sampled", "global") overrides the
    device backend's choice of where it searches the tables; the integers do not depend on it."""
    levels, kmin, r, dev = _sets(cal, y_prob, levels, first, None, ("count", "mask", "missing"), backend, force_regime)
    if dev:
        if _is_tensor(y_prob):
            out = (r.count, r.mask, r.size, r.novel.bool(), r.missing.bool())
        else:
            out = _to_host(r, kmin)
    else:
        count, mask, size, novel = r[2]
        out = (count, mask, size, novel, r[1])
    count, mask, size, novel, missing = out
    return FaultSets(mask, size, novel, missing, count, kmin > 0, levels, cal.n_cal)


def evaluate_sets(cal, y_prob, y, levels=(0.9,), backend="auto", force_regime="auto"):
    """Coverage and set sizes against known classes -> SetReport; on the device nothing per row is stored."""
    levels, kmin, r, dev = _sets(cal, y_prob, levels, 0, y, ("tally",), backend, force_regime)
    if dev:
        tally = r.tally.cpu().numpy()
    else:
        _, mask, size, _ = r[2]
        tally = _host_tally(mask, size, r[1], y, cal.n_classes)
    return SetReport(tally, cal.n_classes, levels, kmin > 0)


# ---------------------------------------------------------------------------------------------- the mixture's own sets
class _Mixture:
    """A fitted DeviceGMM with its label map: the rows' posterior and scores on either backend."""

    def __init__(self, gmm, comp_fault_prob):
        gmm._check_fitted()
        self.gmm, self.K = gmm, gmm.n_components
        self.map = np.ascontiguousarray(_as_numpy(comp_fault_prob, np.float64)).reshape(self.K, -1)
        self.C = self.map.shape[1]
        if not 1 <= self.C <= MAX_CLASSES:
            raise ValueError("comp_fault_prob must be [n_components, 1..%d classes]" % MAX_CLASSES)
        self.logm, self.logpi = _log_map(gmm.weights_, self.map)
        self._dev = {}

    def backend(self, backend, X):
        return _pick_backend(self.gmm.backend if backend == "auto" else backend, X)

    # ---- host
    def host(self, X, columns, row_index, kind, randomized, seed, first, draw):
        """y_prob, y_pred, scores [n, C], s_any [n] or None, missing [n]."""
        g = self.gmm
        a = _as_numpy(X)
        if a.ndim != 2:
            raise ValueError("X must be a 2-D array")
        inside = None
        if row_index is not None:
            idx = _as_numpy(row_index, np.int64).reshape(-1)
            inside = (idx >= 0) & (idx < a.shape[0])
            a = a[np.where(inside, idx, 0)] if a.shape[0] else np.full((idx.size, a.shape[1]), np.nan)
        Xh = np.ascontiguousarray(a if columns is None else a[:, list(columns)], dtype=np.float64)
        if inside is not None:
            Xh[~inside] = np.nan
        lp, lpn = _host_lp(Xh, *(_as_numpy(v, np.float64) for v in (g.weights_, g.means_, g.precisions_cholesky_)))
        with np.errstate(all="ignore"):
            resp = np.exp(lp - lpn[:, None])
            yp = np.clip(resp @ self.map, 1e-12, 1.0)
            yp = yp / yp.sum(axis=1, keepdims=True)
            pred = np.where(np.isnan(yp).any(axis=1), 0, np.argmax(np.where(np.isnan(yp), -np.inf, yp), axis=1)).astype(np.int64)
        bad = ~np.isfinite(Xh).all(axis=1)
        if kind == KINDS["density"]:
            S = np.where(bad[:, None], np.nan, _host_density(lp, self.logm, self.logpi))
            s_any = np.where(bad, np.nan, -lpn)
            miss = bad | np.isnan(S).any(axis=1) | np.isnan(s_any)
        else:
            S, miss = _host_scores(yp, kind, uniforms(seed, draw, first, Xh.shape[0]) if randomized else None)
            s_any = None
        return yp, pred, S, s_any, miss

    # ---- device
    def device_parts(self, torch, dev, D):
        if dev not in self._dev:
            st = self.gmm._device_state(torch, dev, D)
            self._dev[dev] = (st, torch.from_numpy(self.map).to(dev), torch.from_numpy(np.concatenate([self.logm.reshape(-1), self.logpi])).to(dev))
        return self._dev[dev]

    def launch(self, X, columns, row_index, cal, kmin, first, draw, y, want, regime="auto", chunk=None):
        """One pinn_fs_gmm launch (or one per `chunk` rows): dict of device tensors."""
        torch, _lib, lib = _torch_lib()
        rows = _DevRows(torch, X, columns, row_index)
        n, C, dev = rows.n, self.C, rows.dev
        density = cal.kind == "density"
        L = 0 if kmin is None else kmin.shape[1]
        with torch.cuda.device(dev):
            gst, cmap, lmap = self.device_parts(torch, dev, rows.D)
            st = cal._device_state(torch, dev) if kmin is not None else None
            o = _Outputs(torch, dev, n, C, L, want)
            e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
            y_prob, y_pred = (e((n, C), torch.float64), e((n,), torch.int64)) if "y_prob" in want else (None, None)
            lpn = e((n,), torch.float64) if "lpn" in want else None
            any_score = e((n,), torch.float64) if density and "scores" in want else None
            any_count = e((n,), torch.int32) if density and "count" in want else None
            yd = _dev_classes(torch, y, n, dev)
            arr, ld, n_arr, c_cols, D, ridx, _ = rows.head()
            step = n if chunk is None else chunk
            for j0 in range(0, max(n, 1), max(step, 1)):
                m = min(step, n - j0)
                if rows.ridx is None:
                    head = (arr + j0 * ld * 8, ld, n_arr - j0, c_cols, D, None, m)
                else:
                    head = (arr, ld, n_arr, c_cols, D, ridx + j0 * 8, m)
                sl = slice(j0, j0 + m)
                s = lambda t: None if t is None else t[sl]
                call("pinn_fs_gmm", *head, self.K, gst, cmap, C, lmap if density else None, st, *_rank_args(cal, kmin, first + j0, draw, regime),
                     s(yd), *o.args(sl), s(y_prob), s(y_pred), s(lpn), s(any_score), s(any_count))
        return dict(o=o, y_prob=y_prob, y_pred=y_pred, lpn=lpn, any_score=any_score, any_count=any_count)


def calibrate_gmm(gmm, comp_fault_prob, X, y, kind="density", columns=None, row_index=None, randomized=False, seed=0, backend="auto"):
    """Calibrate on rows of the mixture, read in place as DeviceGMM.diagnose reads them: the density kind, or a posterior
    kind computed from the mixture's own y_prob."""
    k = _kind(kind)
    mix = _Mixture(gmm, comp_fault_prob)
    rnd = bool(randomized) and kind == "aps"
    if mix.backend(backend, X) == "device":
        torch = _torch_lib()[0]
        cal0 = SetCalibration(kind, mix.C, np.zeros(mix.C, np.int64), 0, 0, seed, rnd)
        r = mix.launch(X, columns, row_index, cal0, None, 0, DRAW_CAL, None, ("scores",))
        st, n_cal, n_any, skipped = _device_build(torch, r["o"].scores, y, mix.C, k, seed, rnd, r["any_score"])
        return SetCalibration(kind, mix.C, n_cal, n_any, skipped, seed, rnd, state=st)
    _, _, S, s_any, _ = mix.host(X, columns, row_index, k, rnd, seed, 0, DRAW_CAL)
    tables, skipped = _host_build(S, y, mix.C, s_any)
    return SetCalibration(kind, mix.C, [t.size for t in tables[:mix.C]], tables[-1].size, skipped, seed, rnd, tables=tables)


class GMMSetDiagnoser:
    """The mixture's diagnosis with its fault sets.  `predict(X)` returns (y_prob, y_pred, FaultSets) with the y_prob and
    y_pred of DeviceGMM.diagnose; `evaluate(X, y)` a SetReport; `update(rows)` is the online form next to
    FaultDiagnoser.update, rows of the results array in, the same triple out: on the device one launch per chunk of at most
    2048 rows from the rows in place (posterior, label map, scores, ranks, masks)."""

    def __init__(self, gmm, comp_fault_prob, cal, levels=(0.9,), features=None, backend="auto"):
        from .diagnosis import DEFAULT_FEATURES, parse_features
        self.mix = _Mixture(gmm, comp_fault_prob)
        if cal.n_classes != self.mix.C:
            raise ValueError("the calibration has %d classes, the label map %d" % (cal.n_classes, self.mix.C))
        self.cal, self.levels = cal, _levels(levels)
        self.kmin = kmin_table(cal.n_cal, self.levels)
        self.columns = columns_of(DEFAULT_FEATURES if features is None else features, parse_features)
        self.backend = backend
        self.n_seen = 0
        self.force_regime = "auto"

    def _run(self, X, columns, row_index, y, want, first=0, chunk=None):
        cal, mix = self.cal, self.mix
        if mix.backend(self.backend, X) == "device":
            return mix.launch(X, columns, row_index, cal, self.kmin, first, DRAW_TEST, y, want, self.force_regime, chunk), True
        yp, pred, S, s_any, miss = mix.host(X, columns, row_index, KINDS[cal.kind], cal.randomized, cal.seed, first, DRAW_TEST)
        tabs = cal._host_tables()
        r = _host_rank(tabs, S, miss, self.kmin)
        any_count = None
        if s_any is not None:
            any_count = np.full(S.shape[0], -1, np.int32)
            any_count[~miss] = tabs[-1].size - np.searchsorted(tabs[-1], s_any[~miss], side="left")
        return (yp, pred, S, miss, r, any_count), False

    def _fault_sets(self, r, dev, as_tensor):
        if dev:
            o = r["o"]
            if as_tensor:
                count, mask, size, novel, missing = o.count, o.mask, o.size, o.novel.bool(), o.missing.bool()
                ac = r["any_count"]
            else:
                count, mask, size, novel, missing = _to_host(o, self.kmin)
                ac = None if r["any_count"] is None else r["any_count"].cpu().numpy()
            yp, pred = (r["y_prob"], r["y_pred"]) if as_tensor else (r["y_prob"].cpu().numpy(), r["y_pred"].cpu().numpy())
        else:
            yp, pred, _, missing, (count, mask, size, novel), ac = r
        return yp, pred, FaultSets(mask, size, novel, missing, count, self.kmin > 0, self.levels, self.cal.n_cal, ac, self.cal.n_any)

    def predict(self, X, columns=None, row_index=None, first=0):
        r, dev = self._run(X, columns, row_index, None, ("count", "mask", "missing", "y_prob"), first)
        return self._fault_sets(r, dev, _is_tensor(X))

    def evaluate(self, X, y, columns=None, row_index=None):
        r, dev = self._run(X, columns, row_index, y, ("tally",))
        if dev:
            tally = r["o"].tally.cpu().numpy()
        else:
            _, _, _, miss, (_, mask, size, _), _ = r
            tally = _host_tally(mask, size, miss, y, self.mix.C)
        return SetReport(tally, self.mix.C, self.levels, self.kmin > 0)

    def update(self, rows):
        r, dev = self._run(rows, self.columns, None, None, ("count", "mask", "missing", "y_prob"), self.n_seen, MAX_CHUNK)
        self.n_seen += int(rows.shape[0])
        return self._fault_sets(r, dev, _is_tensor(rows))
