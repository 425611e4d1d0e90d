"""ROC inference: how sure is an AUC, and do two AUCs on the same test rows differ?  DeLong's covariance of K AUCs with its
intervals and paired test, and the stratified paired bootstrap.  The reference has no counterpart: script 02 prints one AUC
per feature group from one split and stops there.

Definitions, integers first as `detection.roc_counts` does.  `y_true` is made binary by `detection._binary_truth`, `scores`
is [K, N] (or [N]): K score vectors on the same N rows, m positives and n negatives.  psi(x, y) = 1 if x > y, 1/2 if x == y,
else 0 (+0.0 == -0.0).  Per classifier k, as exact int64:
    a_k[i] = 2 #{neg < s_i} + #{neg == s_i}   for a positive row i   (= 2 n V10_k(i))
    b_k[j] = 2 #{pos > s_j} + #{pos == s_j}   for a negative row j   (= 2 m V01_k(j))
both from the tied groups of the ascending order and two integer scans; sum_i a_k[i] = sum_j b_k[j] = U2_k, the integer
`roc_counts` reports, and AUC_k = U2_k / (2 m n).  The cross sums P10[k, l] = sum_i a_k[i] a_l[i], P01[k, l] = sum_j b_k[j]
b_l[j] are exact 128-bit integers, and the host finishes in Python integers and `fractions.Fraction`:
    S10[k, l] = (m P10[k, l] - U2_k U2_l) / (4 n^2 m (m - 1)),   S01[k, l] = (n P01[k, l] - U2_k U2_l) / (4 m^2 n (n - 1)),
    cov = S10 / m + S01 / n
(the sample covariances, ddof = 1, of V10 and V01: DeLong, DeLong and Clarke-Pearson 1988), each entry rounded once to the
nearest float64.  Both backends therefore give the same bytes.

The bootstrap is stratified and paired: resample r draws n negatives and m positives with replacement and all K classifiers
share the draw.  Draw t of stratum s (0 negatives, 1 positives) of resample r takes 64 bits of the package's Philox4x32-10
(`anomaly.philox4x32_10`): the words (2 (t & 1), 2 (t & 1) + 1) as (low, high) of the call at the counter
(t >> 1, r, DRAW_BOOT, s) under the key (seed & 0xffffffff, seed >> 32), and the drawn position within the stratum (in row
order) is the high 64 bits of bits x stratum size.  A resample depends on (seed, r) only: not on the launch, the chunking or
n_boot.  No library's bootstrap draws are reproduced.

Two backends, as in detection.py.  "device": the HIP kernels of csrc/pinn_rocstat.hip, sorting by torch.sort as `roc_counts`
does; device tensors in, device tensors out.  "host": integer numpy, the referee.  There is no online form: an interval is
a statement about a finished test set (as embedding.py has no `transform`).  Importing this module needs numpy only.
"""
import ctypes
import math
from fractions import Fraction
from statistics import NormalDist

import numpy as np

from ._device import _as_numpy, _is_tensor, _on_gpu, _pick_backend, _torch_lib, call
from .anomaly import philox4x32_10
from .detection import _binary_truth

# include/pinn_hip.h: PINN_AUC_*
MAX_SCORES, SCAN_TILE, BOOT_LDS_GROUPS, DRAW_BOOT, _COUNTS = 8, 256, 12288, 2, 8
_C_POS, _C_NEG, _C_GROUPS, _C_U2, _C_U2B = range(5)
MAX_ROWS = (1 << 31) - 1
DEFAULT_WORKSPACE_CAP = 1 << 30         # bytes of bootstrap histograms held in the workspace at a time (the resamples are chunked)
_M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------- arguments
def _too_many(K):
    raise NotImplementedError("the device backend takes 1 to %d score vectors, got %d" % (MAX_SCORES, K))


def _inputs(y_true, scores, pos_label, backend, least):
    """(backend, scores [K, N], positives [N] as booleans, m, n), on the host or on the device as the backend says."""
    shape = tuple(scores.shape) if hasattr(scores, "shape") else np.shape(scores)
    if len(shape) not in (1, 2) or shape[-1] < 1 or (len(shape) == 2 and shape[0] < 1):
        raise ValueError("scores must be [N] or [K, N] with K >= 1 and N >= 1")
    K, N = (1, shape[0]) if len(shape) == 1 else shape
    be = _pick_backend(backend, scores, n=N)
    if N > MAX_ROWS:
        raise NotImplementedError("at most 2^31 - 1 rows")
    if be == "host":
        s = np.ascontiguousarray(_as_numpy(scores, np.float64).reshape(K, N))
        pos = _as_numpy(_binary_truth(_as_numpy(y_true).reshape(-1), pos_label)).astype(bool)
        if pos.size != N:
            raise ValueError("y_true has %d entries and the scores have %d" % (pos.size, N))
        if not np.isfinite(s).all():
            raise ValueError("the scores must be finite")
        m = int(pos.sum())
    else:
        if K > MAX_SCORES:
            _too_many(K)
        torch, _, _ = _torch_lib()
        dev = scores.device if _on_gpu(scores) else torch.device("cuda")
        s = scores.detach() if _is_tensor(scores) else torch.from_numpy(np.ascontiguousarray(np.asarray(scores, dtype=np.float64)))
        s = s.to(dev, torch.float64).reshape(K, N).contiguous()
        yt = y_true.reshape(-1) if _is_tensor(y_true) else np.asarray(y_true).reshape(-1)
        pos = _binary_truth(yt, pos_label)
        pos = (pos if _is_tensor(pos) else torch.from_numpy(np.ascontiguousarray(pos))).to(dev).reshape(-1).to(torch.bool)
        if pos.numel() != N:
            raise ValueError("y_true has %d entries and the scores have %d" % (pos.numel(), N))
        if not bool(torch.isfinite(s).all()):
            raise ValueError("the scores must be finite")
        m = int(pos.sum())
    if m < least or N - m < least:
        raise ValueError("%d positive and %d negative rows: at least %d of each are needed" % (m, N - m, least))
    return be, s, pos, m, N - m


# ---------------------------------------------------------------------------------------------- components
def _host_components(s, pos, m):
    K, N = s.shape
    a, b = np.empty((K, m), dtype=np.int64), np.empty((K, N - m), dtype=np.int64)
    group, groups = np.empty((K, N), dtype=np.int32), np.empty(K, dtype=np.int64)
    for k in range(K):
        order = np.argsort(s[k], kind="stable")
        ss, pp = s[k][order], pos[order]
        gid = np.cumsum(np.concatenate([[True], ss[1:] != ss[:-1]])) - 1
        G = int(gid[-1]) + 1
        n_pos, n_neg = np.bincount(gid[pp], minlength=G), np.bincount(gid[~pp], minlength=G)
        neg_below, pos_above = np.cumsum(n_neg) - n_neg, m - np.cumsum(n_pos)
        v = np.where(pp, 2 * neg_below[gid] + n_neg[gid], 2 * pos_above[gid] + n_pos[gid])
        comp = np.empty(N, dtype=np.int64)
        comp[order] = v
        group[k, order] = gid
        a[k], b[k], groups[k] = comp[pos], comp[~pos], G
    return a, b, group, groups, np.flatnonzero(pos), np.flatnonzero(~pos)


def _device_components(s, pos, m):
    torch, _lib, lib = _torch_lib()
    K, N = s.shape
    dev = s.device
    with torch.cuda.device(dev):
        s_sorted, order = torch.sort(s, dim=1, stable=True)
        pos_sorted = pos.to(torch.int64)[order].contiguous()
        counts = torch.empty(K * _COUNTS, dtype=torch.int64, device=dev)
        comp = torch.empty((K, N), dtype=torch.int64, device=dev)
        group = torch.empty((K, N), dtype=torch.int32, device=dev)
        wb = lib.pinn_auc_components_workspace_bytes(N, K)
        ws = torch.empty(wb, dtype=torch.uint8, device=dev)
        call("pinn_auc_components", s_sorted.contiguous(), pos_sorted, order.contiguous(), N, K, counts, comp, group, ws, wb)
        c = counts.cpu().numpy().reshape(K, _COUNTS)
        pos_rows, neg_rows = torch.nonzero(pos).reshape(-1), torch.nonzero(~pos).reshape(-1)
        a, b = comp[:, pos_rows].contiguous(), comp[:, neg_rows].contiguous()
    if not (np.all(c[:, _C_POS] == m) and np.all(c[:, _C_NEG] == N - m) and np.all(c[:, _C_U2] == c[:, _C_U2B])):
        raise _lib.PinnError("pinn_auc_components: the counts of the classifiers disagree")
    return a, b, group, c[:, _C_GROUPS].copy(), pos_rows, neg_rows, c[:, _C_U2].copy()


def _components(y_true, scores, pos_label, backend, least=2):
    be, s, pos, m, n = _inputs(y_true, scores, pos_label, backend, least)
    if be == "host":
        a, b, group, groups, pos_rows, neg_rows = _host_components(s, pos, m)
        U2 = a.sum(axis=1)
        if not np.array_equal(U2, b.sum(axis=1)):
            raise AssertionError("sum a != sum b")
    else:
        a, b, group, groups, pos_rows, neg_rows, U2 = _device_components(s, pos, m)
    out = {"n_pos": m, "n_neg": n, "U2": U2.astype(np.int64), "a": a, "b": b, "pos_rows": pos_rows, "neg_rows": neg_rows,
           "group": group, "n_groups": groups.astype(np.int64)}
    if be == "device" and not _is_tensor(scores):
        for key in ("a", "b", "pos_rows", "neg_rows", "group"):
            out[key] = out[key].cpu().numpy()
    return out, be


def auc_components(y_true, scores, pos_label=None, backend="auto"):
    """DeLong's structural components as integers.  Returns a dict: `n_pos` = m, `n_neg` = n, `U2` [K] (int64, on the host),
    `a` [K, m] and `b` [K, n] (int64; a / (2 n) = V10, b / (2 m) = V01), `pos_rows` and `neg_rows` (row numbers, ascending: the
    columns of `a` and `b`), and `group` [K, N] (int32: every row's tied group, numbered in ascending score order) with
    `n_groups` [K].  ValueError for non-finite scores, a length mismatch, or fewer than two rows of either class."""
    return _components(y_true, scores, pos_label, backend)[0]


def _host_cross(comp):
    K = comp.shape[0]
    P = [[0] * K for _ in range(K)]
    small = comp.size == 0 or (int(comp.max()) < (1 << 32) and int(comp.min()) >= 0)
    if small:
        # 16-bit halves: a product of halves is below 2^32 and a sum over fewer than 2^31 rows stays inside int64
        lo, hi = comp & 0xFFFF, comp >> 16
    for l in range(K):
        for k in range(l + 1):
            if small:
                v = (int(np.dot(lo[k], lo[l])) + ((int(np.dot(lo[k], hi[l])) + int(np.dot(hi[k], lo[l]))) << 16)
                     + (int(np.dot(hi[k], hi[l])) << 32))
            else:
                v = sum(int(x) * int(y) for x, y in zip(comp[k].tolist(), comp[l].tolist()))
            P[k][l] = P[l][k] = v
    return P


def _device_cross(comp):
    torch, _lib, lib = _torch_lib()
    K, rows = comp.shape
    dev = comp.device
    pairs = K * (K + 1) // 2
    with torch.cuda.device(dev):
        out = torch.empty(pairs * 2, dtype=torch.int64, device=dev)
        wb = lib.pinn_auc_cross_sums_workspace_bytes(rows, K)
        ws = torch.empty(wb, dtype=torch.uint8, device=dev)
        call("pinn_auc_cross_sums", comp, comp.stride(0), rows, K, out, ws, wb)
        w = out.cpu().numpy().view(np.uint64).reshape(pairs, 2)
    P = [[0] * K for _ in range(K)]
    for l in range(K):
        for k in range(l + 1):
            p = l * (l + 1) // 2 + k
            P[k][l] = P[l][k] = int(w[p, 0]) + (int(w[p, 1]) << 64)
    return P


def component_cross_sums(comp, backend="auto"):
    """P[k][l] = sum_i comp[k, i] comp[l, i] as Python integers, exact below 2^128: comp is [K, rows] of non-negative 64-bit
    integers (read as unsigned).  The device adds 128-bit integers (two 64-bit words, the high half of a product by
    __umul64hi), workgroup partials in index order."""
    shape = tuple(comp.shape)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError("comp must be [K, rows] with K >= 1 and rows >= 1")
    be = _pick_backend(backend, comp, n=shape[1])
    if be == "host":
        return _host_cross(np.ascontiguousarray(_as_numpy(comp, np.int64)))
    if shape[0] > MAX_SCORES:
        _too_many(shape[0])
    torch, _, _ = _torch_lib()
    t = comp.detach() if _is_tensor(comp) else torch.from_numpy(np.ascontiguousarray(np.asarray(comp, dtype=np.int64)))
    return _device_cross(t.to(comp.device if _on_gpu(comp) else "cuda", torch.int64).contiguous())


# ---------------------------------------------------------------------------------------------- DeLong
def _delong_exact(y_true, scores, pos_label, backend):
    """(components, backend, theta [K], cov [K][K], S10, S01) as Fractions."""
    c, be = _components(y_true, scores, pos_label, backend)
    m, n, U2 = c["n_pos"], c["n_neg"], [int(u) for u in c["U2"]]
    if be == "host" or not _is_tensor(c["a"]):
        P10, P01 = _host_cross(np.asarray(c["a"])), _host_cross(np.asarray(c["b"]))
    else:
        P10, P01 = _device_cross(c["a"]), _device_cross(c["b"])
    K = len(U2)
    S10 = [[Fraction(m * P10[k][l] - U2[k] * U2[l], 4 * n * n * m * (m - 1)) for l in range(K)] for k in range(K)]
    S01 = [[Fraction(n * P01[k][l] - U2[k] * U2[l], 4 * m * m * n * (n - 1)) for l in range(K)] for k in range(K)]
    cov = [[S10[k][l] / m + S01[k][l] / n for l in range(K)] for k in range(K)]
    return c, be, [Fraction(u, 2 * m * n) for u in U2], cov, S10, S01


def _floats(M):
    return np.array([[float(v) for v in row] for row in M], dtype=np.float64)


def delong_covariance(y_true, scores, pos_label=None, backend="auto"):
    """DeLong's covariance matrix of the K AUCs.  Returns a dict: `auc` [K], `cov` [K, K], `S10`, `S01` [K, K] (float64, each
    entry the exact rational rounded once), `n_pos`, `n_neg`, `U2` [K].  ValueError as `auc_components`."""
    c, _, theta, cov, S10, S01 = _delong_exact(y_true, scores, pos_label, backend)
    return {"auc": np.array([float(t) for t in theta]), "cov": _floats(cov), "S10": _floats(S10), "S01": _floats(S01),
            "n_pos": c["n_pos"], "n_neg": c["n_neg"], "U2": c["U2"]}


def _z_of(level):
    if not 0.0 < float(level) < 1.0:
        raise ValueError("level must lie strictly between 0 and 1")
    return NormalDist().inv_cdf(0.5 + float(level) / 2.0)


def _interval(theta, var, level, method):
    z, se = _z_of(level), math.sqrt(var)
    if method == "logit" and 0.0 < theta < 1.0:
        if se == 0.0:
            return theta, theta
        mid, half = math.log(theta / (1.0 - theta)), z * se / (theta * (1.0 - theta))
        return 1.0 / (1.0 + math.exp(-(mid - half))), 1.0 / (1.0 + math.exp(-(mid + half)))
    return max(theta - z * se, 0.0), min(theta + z * se, 1.0)


def auc_ci(y_true, score, level=0.95, method="delong", pos_label=None, backend="auto", n_boot=2000, random_state=0):
    """(auc, lo, hi) of one score vector.  "delong": theta -+ z se, clipped to [0, 1].  "logit": the same interval on
    logit(theta) with se / (theta (1 - theta)), mapped back; for theta of 0 or 1 it is the "delong" interval.  "bootstrap": the
    percentile interval of `bootstrap_auc(n_boot, random_state)`."""
    if method not in ("delong", "logit", "bootstrap"):
        raise ValueError("method must be 'delong', 'logit' or 'bootstrap'")
    if len(score.shape if hasattr(score, "shape") else np.shape(score)) != 1:
        raise ValueError("score must be one vector [N]")
    if method == "bootstrap":
        r = bootstrap_auc(y_true, score, n_boot=n_boot, random_state=random_state, backend=backend, pos_label=pos_label, level=level)
        return float(r["auc"][0]), float(r["ci"][0, 0]), float(r["ci"][0, 1])
    _, _, theta, cov, _, _ = _delong_exact(y_true, score, pos_label, backend)
    t = float(theta[0])
    lo, hi = _interval(t, float(cov[0][0]), level, method)
    return t, lo, hi


def _z_test(diff, var):
    """(z, two-sided p) of an exact difference and its exact variance."""
    if var == 0:
        if diff == 0:
            return float("nan"), 1.0
        return math.copysign(float("inf"), diff), 0.0
    z = float(diff) / math.sqrt(float(var))
    return z, math.erfc(abs(z) / math.sqrt(2.0))


def delong_test(y_true, score_a, score_b, pos_label=None, backend="auto"):
    """DeLong's paired test of AUC(score_a) = AUC(score_b) on the same rows.  Returns a dict: `diff` = AUC_a - AUC_b, `z`, `p`
    (two-sided, by math.erfc), `var_diff`, `auc` (both).  A zero variance gives z = nan, p = 1.0 when diff is 0 and
    z = +-inf, p = 0.0 otherwise."""
    if _is_tensor(score_a) and _is_tensor(score_b):
        import torch
        both = torch.stack([score_a.reshape(-1), score_b.reshape(-1).to(score_a.device)])
    else:
        both = np.stack([_as_numpy(score_a, np.float64).reshape(-1), _as_numpy(score_b, np.float64).reshape(-1)])
    _, _, theta, cov, _, _ = _delong_exact(y_true, both, pos_label, backend)
    diff, var = theta[0] - theta[1], cov[0][0] + cov[1][1] - 2 * cov[0][1]
    z, p = _z_test(diff, var)
    return {"diff": float(diff), "z": z, "p": p, "var_diff": float(var), "auc": (float(theta[0]), float(theta[1]))}


def holm_adjust(p):
    """Holm's step-down adjustment of a list of p-values: the i-th smallest becomes max_{j <= i} min(1, (M - j) p_(j))."""
    p = np.asarray(p, dtype=np.float64)
    order = np.argsort(p, kind="stable")
    out, run = np.empty_like(p), 0.0
    for rank, i in enumerate(order):
        run = max(run, min(1.0, (p.size - rank) * p[i]))
        out[i] = run
    return out


def compare_aucs(y_true, scores, names=None, level=0.95, pos_label=None, backend="auto"):
    """All K AUCs with their DeLong intervals and every paired test.  Returns a dict: `names`, `auc` [K], `se` [K], `ci`
    [K, 2], `cov` [K, K], and the K x K matrices `diff` (row minus column), `z`, `p` and `p_holm`: Holm's step-down adjustment
    over the K (K - 1) / 2 pairs, computed on the host.  The diagonals are 0, nan, 1, 1."""
    c, _, theta, cov, _, _ = _delong_exact(y_true, scores, pos_label, backend)
    K = len(theta)
    names = list(names) if names is not None else list(range(K))
    if len(names) != K:
        raise ValueError("%d names for %d score vectors" % (len(names), K))
    diff, z, p = np.zeros((K, K)), np.full((K, K), np.nan), np.ones((K, K))
    pairs = [(k, l) for k in range(K) for l in range(k + 1, K)]
    for k, l in pairs:
        d, v = theta[k] - theta[l], cov[k][k] + cov[l][l] - 2 * cov[k][l]
        zz, pp = _z_test(d, v)
        diff[k, l], diff[l, k], z[k, l], z[l, k], p[k, l], p[l, k] = float(d), -float(d), zz, -zz, pp, pp
    p_holm = np.ones((K, K))
    if pairs:
        for (k, l), v in zip(pairs, holm_adjust([p[k, l] for k, l in pairs])):
            p_holm[k, l] = p_holm[l, k] = v
    auc = np.array([float(t) for t in theta])
    covf = _floats(cov)
    ci = np.array([_interval(auc[k], covf[k, k], level, "delong") for k in range(K)])
    return {"names": names, "auc": auc, "se": np.sqrt(np.diag(covf)), "ci": ci, "cov": covf, "diff": diff, "z": z, "p": p,
            "p_holm": p_holm, "level": float(level), "n_pos": c["n_pos"], "n_neg": c["n_neg"]}


# ---------------------------------------------------------------------------------------------- bootstrap
def _mulhi64(x, size):
    """High 64 bits of x * size for uint64 x and size < 2^31, in uint64 arithmetic."""
    s = np.uint64(size)
    return (((x >> np.uint64(32)) * s + (((x & _M32) * s) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def bootstrap_draws(seed, resample, stratum, size):
    """The `size` positions that resample `resample` draws in a stratum of `size` rows (0: negatives, 1: positives)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    q = np.arange((size + 1) // 2, dtype=np.uint64)
    o = philox4x32_10(q, int(resample), DRAW_BOOT, int(stratum), seed & 0xFFFFFFFF, seed >> 32)
    bits = np.empty(2 * q.size, dtype=np.uint64)
    bits[0::2], bits[1::2] = o[0] | (o[1] << np.uint64(32)), o[2] | (o[3] << np.uint64(32))
    return _mulhi64(bits[:size], size)


def _host_bootstrap(gpos, gneg, groups, m, n, seed, first, n_boot):
    K = gpos.shape[0]
    out = np.empty((n_boot, K), dtype=np.int64)
    for i in range(n_boot):
        ineg, ipos = bootstrap_draws(seed, first + i, 0, n), bootstrap_draws(seed, first + i, 1, m)
        for k in range(K):
            c = np.concatenate([[0], np.cumsum(np.bincount(gneg[k][ineg], minlength=int(groups[k])))])
            g = gpos[k][ipos]
            out[i, k] = int((c[g + 1] + c[g]).sum())
    return out


def _device_bootstrap(gpos, gneg, groups, m, n, seed, first, n_boot, cap):
    torch, _lib, lib = _torch_lib()
    K = gpos.shape[0]
    dev = gpos.device
    g = (ctypes.c_longlong * K)(*[int(v) for v in groups])
    per = lib.pinn_auc_bootstrap_workspace_bytes(1, K, g)
    chunk = n_boot if per == 0 else max(1, min(n_boot, int(cap) // per))
    with torch.cuda.device(dev):
        out = torch.empty((n_boot, K), dtype=torch.int64, device=dev)
        ws = torch.empty(per * chunk, dtype=torch.uint8, device=dev) if per else None
        for lo in range(0, n_boot, chunk):
            nb = min(chunk, n_boot - lo)
            call("pinn_auc_bootstrap", gpos, gneg, m, n, K, g, seed, first + lo, nb, out[lo:lo + nb], ws, per * nb)
    return out


def bootstrap_auc(y_true, scores, n_boot=2000, random_state=0, first=0, backend="auto", pos_label=None, level=0.95,
                  workspace_cap=DEFAULT_WORKSPACE_CAP):
    """The stratified paired bootstrap of K AUCs: resamples first .. first + n_boot - 1 of the run seeded by `random_state`
    (the module's docstring has the keying; two calls with first=0, n_boot=B1 and first=B1, n_boot=B2 equal one call of
    B1 + B2).  Returns a dict: `U2_boot` [n_boot, K] int64 and `auc_boot` = U2_boot / (2 m n) (device tensors for a device
    tensor in), and on the host `auc` [K], `U2` [K], `cov_boot` [K, K] (ddof = 1), `ci` [K, 2] and `diff_ci` [K, K, 2]: the
    percentile intervals at `level` of every AUC and of every difference (row minus column), `n_pos`, `n_neg`, `first`.
    One row of each class is enough.  On the device a workgroup takes a resample; with more tied groups than a workgroup
    holds in LDS its histogram lives in the workspace, and the resamples go in chunks that keep it under `workspace_cap`."""
    n_boot, first = int(n_boot), int(first)
    if n_boot < 1 or first < 0 or first + n_boot > 1 << 32:
        raise ValueError("n_boot >= 1, first >= 0 and first + n_boot <= 2^32 are needed")
    _z_of(level)
    seed = int(random_state) & 0xFFFFFFFFFFFFFFFF
    c, be = _components(y_true, scores, pos_label, backend, least=1)
    m, n = c["n_pos"], c["n_neg"]
    if be == "host":
        grp = np.asarray(c["group"])
        U2b = _host_bootstrap(grp[:, c["pos_rows"]], grp[:, c["neg_rows"]], c["n_groups"], m, n, seed, first, n_boot)
        host, auc_boot = U2b, U2b / (2 * m * n)
    else:
        torch, _, _ = _torch_lib()
        grp, pr, nr = c["group"], c["pos_rows"], c["neg_rows"]
        if not _is_tensor(grp):
            grp, pr, nr = (torch.from_numpy(np.ascontiguousarray(v)).to("cuda") for v in (grp, pr, nr))
        U2b = _device_bootstrap(grp[:, pr].contiguous(), grp[:, nr].contiguous(), c["n_groups"], m, n, seed, first, n_boot, workspace_cap)
        host = U2b.cpu().numpy()
        if _is_tensor(scores):
            # divided on the host (n_boot x K numbers) and sent back: the device's float64 division is not the correctly
            # rounded one, and the two backends are to give the same bytes
            auc_boot = torch.from_numpy(host / (2 * m * n)).to(U2b.device)
        else:
            U2b, auc_boot = host, host / (2 * m * n)
    ab = host / (2 * m * n)
    K = ab.shape[1]
    cov = np.atleast_2d(np.cov(ab, rowvar=False, ddof=1)) if n_boot >= 2 else np.full((K, K), np.nan)
    q = [50.0 * (1.0 - float(level)), 50.0 * (1.0 + float(level))]
    ci = np.percentile(ab, q, axis=0).T
    diff_ci = np.zeros((K, K, 2))
    for k in range(K):
        for l in range(K):
            if k != l:
                diff_ci[k, l] = np.percentile(ab[:, k] - ab[:, l], q)
    return {"U2_boot": U2b, "auc_boot": auc_boot, "auc": c["U2"] / (2 * m * n), "U2": c["U2"], "cov_boot": cov, "ci": ci,
            "diff_ci": diff_ci, "level": float(level), "n_pos": m, "n_neg": n, "first": first, "n_boot": n_boot}


# ---------------------------------------------------------------------------------------------- feature groups
def compare_feature_groups(evals, level=0.95, n_boot=0, random_state=0, backend="auto"):
    """The comparison script 02's four AUCs ask for.  `evals` is the list `detection.evaluate_feature_groups` returns; all
    groups must have been scored on the same original rows in the same order (`kept_rows[idx_test]` equal), else ValueError
    names the groups that differ from the first.  Runs `compare_aucs` on the groups' `p_fault` vectors (and `bootstrap_auc`
    when n_boot > 0); when group 0 carries `anomaly_score` (unsupervised=True) it joins as the column "unsup".  The truth is
    "not the normal class" of group 0's `y_test`.  Scores that are device tensors stay on the device.
    Returns a dict keyed by each group's `spec`: `auc`, `ci` (lo, hi), `se`, and per other group `diff`, `z`, `p`, `p_holm`
    (and `boot_ci`, `boot_diff_ci` with n_boot > 0), each a dict keyed by the other group's spec."""
    evals = list(evals)
    if not evals:
        raise ValueError("no evaluated groups")

    def test_rows(e):
        kept, idx = e["kept_rows"], np.asarray(e["idx_test"], dtype=np.int64)
        if _is_tensor(kept):
            import torch
            return kept[torch.from_numpy(idx).to(kept.device)]
        return np.asarray(kept)[idx]

    def same(x, y):
        if tuple(x.shape) != tuple(y.shape):
            return False
        if _is_tensor(x) or _is_tensor(y):
            import torch
            xt = x if _is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
            yt = y if _is_tensor(y) else torch.from_numpy(np.ascontiguousarray(y))
            return bool(torch.equal(xt, yt.to(xt.device)))
        return bool(np.array_equal(x, y))

    rows0 = test_rows(evals[0])
    bad = [str(e["spec"]) for e in evals[1:] if not same(rows0, test_rows(e))]
    if bad:
        raise ValueError("the groups %s were not scored on the test rows of %r: a paired comparison needs one split"
                         % (", ".join(repr(b) for b in bad), str(evals[0]["spec"])))
    names = [e["spec"] if isinstance(e["spec"], str) else ",".join(str(c) for c in e["spec"]) for e in evals]
    cols = [e["p_fault"] for e in evals]
    if evals[0].get("anomaly_score") is not None:
        names.append("unsup")
        cols.append(evals[0]["anomaly_score"])
    if len(set(names)) != len(names):
        raise ValueError("group specs repeat: %r" % (names,))
    if any(_on_gpu(c) for c in cols):
        import torch
        dev = next(c.device for c in cols if _on_gpu(c))
        scores = torch.stack([(c if _is_tensor(c) else torch.from_numpy(np.asarray(c, dtype=np.float64))).to(dev, torch.float64).reshape(-1)
                              for c in cols])
    else:
        scores = np.stack([_as_numpy(c, np.float64).reshape(-1) for c in cols])
    cn = evals[0]["class_names"]
    normal = cn.index("normal") if "normal" in cn else 0
    truth = np.asarray(evals[0]["y_test"]).reshape(-1) != normal
    r = compare_aucs(truth, scores, names=names, level=level, pos_label=True, backend=backend)
    b = bootstrap_auc(truth, scores, n_boot=n_boot, random_state=random_state, backend=backend, pos_label=True, level=level) if n_boot > 0 else None
    table = {}
    for k, name in enumerate(names):
        row = {"auc": float(r["auc"][k]), "ci": (float(r["ci"][k, 0]), float(r["ci"][k, 1])), "se": float(r["se"][k])}
        for key in ("diff", "z", "p", "p_holm"):
            row[key] = {other: float(r[key][k, l]) for l, other in enumerate(names) if l != k}
        if b is not None:
            row["boot_ci"] = (float(b["ci"][k, 0]), float(b["ci"][k, 1]))
            row["boot_diff_ci"] = {other: (float(b["diff_ci"][k, l, 0]), float(b["diff_ci"][k, l, 1])) for l, other in enumerate(names) if l != k}
        table[name] = row
    return table
