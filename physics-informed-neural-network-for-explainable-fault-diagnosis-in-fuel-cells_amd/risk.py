"""Risk function RF(t) and early-warning index: the stage after `comprehensive_results` (reference script 04).

Public names, argument names and defaults follow script 04, so a call written for it runs here:
`estimate_mu_sigma_normal`, `compute_rf_time_series`, `find_first_alarm_index`, `compute_rf_advance_for_condition`.
Added: `rf_series` (gather lists, segments, carried state), `rf_advance_for_conditions` (all conditions in one device
call) and `RiskMonitor` (online use, chunk by chunk).

    z = (R - mu) / sigma,  a = max(0, |z| - z_safe)                   per residual column
    S_l = (sum_d w_d a_d^p)^(1/p) per layer,  S_tot = sum_l beta_l S_l
    C(t) = lambda C(t-1) + S_tot(t),  C(first) = 0
    RF_inst = clip((logistic(k (clip(C, 0, C_max) - C0)) - L0) / (L_max - L0), 0, 1)
    RF_smooth(t) = alpha RF_inst(t) + (1 - alpha) RF_smooth(t-1),  RF_smooth(first) = RF_inst(first)

Two backends.  "device": the HIP kernels of csrc/pinn_risk.hip (float64, the recurrences as segmented scans).  "host": plain
float64 numpy with the two sequential loops, for machines without a GPU and as the referee of the device tests.  Importing
this module needs numpy only; torch and the HIP library are loaded when a device path is first used.
"""
import ctypes

import numpy as np

from ._device import AUTO_DEVICE_ROWS, _as_numpy, _dev_f64_rows, _dev_vec, _is_tensor, _pick_backend, _torch_lib, call  # noqa: F401

# column layout of the results array (results.create_comprehensive_results_array_v2)
INDEX = {"x0": 0, "x1": 1, "x2": 2, "x3": 3, "x4": 4, "x5": 5, "x6": 6, "x7": 7,
         "y_true": 8, "y_pred": 9, "ale": 10, "epi": 11, "res": 12, "pV": 13, "pT": 14, "pH": 15, "pO": 16, "label": 17}
CURRENT_COL = "x0"

# fault class -> labels; the reference's own keys are accepted as aliases
FAULT_RANGE_MAP = {
    "flooding": range(1, 4),
    "oxygen_starvation": range(4, 7),
    "membrane_drying": range(7, 10),
    "hydrogen_starvation": range(10, 13),
}
FAULT_ALIASES = {"水淹": "flooding", "氧饥饿": "oxygen_starvation", "膜干": "membrane_drying", "氢饥饿": "hydrogen_starvation"}

NORMAL_LABELS = (0,)
RF_RES_KEYS = ("res", "pV", "pT", "pH", "pO")
RF_LAYER_CONFIG = {"voltage": ["res", "pV"], "gas": ["pH", "pO"], "temp": ["pT"]}
RF_FEATURE_WEIGHTS = np.ones(5, dtype=float)
RF_LAYER_WEIGHTS = {"voltage": 1.0, "gas": 1.0, "temp": 1.0}
RF_P_LAYER = 2.0
RF_Z_SAFE = 2.0
RF_LAMBDA_DECAY = 0.9971
RF_K_LOGISTIC = 0.0005
RF_C0_LOGISTIC = 500.0
RF_C_MAX = 1000.0
RF_ALPHA_SMOOTH = 0.2
V_THRESHOLD_FULL = 0.7
RF_THRESHOLD_FULL = 0.4
V_THRESHOLD_COND = 3.1
RF_THRESHOLD_COND = 0.4
CURRENT_TOL = 0.5
RF_WARN_THRESHOLD = 0.3
RF_DANGER_THRESHOLD = 0.6
V_ALARM_DROP = 0.1                      # voltage alarm: V <= V[first] - 0.1
RF_CONDITIONS = [
    (108.0, "flooding", (0, 1050)), (108.0, "oxygen_starvation", None), (108.0, "membrane_drying", None),
    (108.0, "hydrogen_starvation", None), (270.0, "flooding", None), (270.0, "membrane_drying", None),
    (270.0, "oxygen_starvation", None), (270.0, "hydrogen_starvation", None), (405.0, "flooding", None),
    (405.0, "oxygen_starvation", None), (405.0, "membrane_drying", None), (405.0, "hydrogen_starvation", None),
]

MAX_COLS, MAX_LAYERS = 8, 4


# ---------------------------------------------------------------------------------------------- configuration
class _Config:
    """Column list, weights and layers of one RF evaluation, checked once."""

    def __init__(self, res_keys=RF_RES_KEYS, feature_weights=RF_FEATURE_WEIGHTS, layer_config=RF_LAYER_CONFIG,
                 layer_weights=RF_LAYER_WEIGHTS, p_layer=RF_P_LAYER, z_safe=RF_Z_SAFE, lambda_decay=RF_LAMBDA_DECAY,
                 k_logistic=RF_K_LOGISTIC, C0_logistic=RF_C0_LOGISTIC, C_max=RF_C_MAX, alpha_smooth=RF_ALPHA_SMOOTH,
                 columns=None):
        self.res_keys = tuple(res_keys)
        D = len(self.res_keys)
        self.cols = [int(c) for c in columns] if columns is not None else [INDEX[k] for k in self.res_keys]
        if len(self.cols) != D:
            raise ValueError("columns must name one column per residual key (%d), got %d" % (D, len(self.cols)))
        self.w = np.ones(D, dtype=float) if feature_weights is None else np.asarray(feature_weights, dtype=float).reshape(-1)
        if self.w.shape[0] != D:
            raise ValueError("feature_weights must have length %d, got %d" % (D, self.w.shape[0]))
        pos = {k: i for i, k in enumerate(self.res_keys)}
        self.layer_names = list(layer_config.keys())
        self.layers = [[pos[k] for k in layer_config[name] if k in pos] for name in self.layer_names]
        self.beta = [float(layer_weights.get(name, 1.0)) for name in self.layer_names]
        self.p, self.z_safe, self.lam = float(p_layer), float(z_safe), float(lambda_decay)
        self.k, self.C0, self.C_max, self.alpha = float(k_logistic), float(C0_logistic), float(C_max), float(alpha_smooth)

    def c_struct(self):
        from . import _lib
        D = len(self.cols)
        if D < 1 or D > MAX_COLS:
            raise ValueError("the device backend takes 1 to %d residual columns, got %d" % (MAX_COLS, D))
        if len(self.layers) > MAX_LAYERS:
            raise ValueError("the device backend takes at most %d layers, got %d" % (MAX_LAYERS, len(self.layers)))
        prm = _lib.RFParams()
        prm.n_cols, prm.n_layers = D, len(self.layers)
        layer_of = [-1] * D
        for li, members in enumerate(self.layers):
            for d in members:
                if layer_of[d] != -1:
                    raise ValueError("residual %r is in more than one layer: the device backend needs disjoint layers" % self.res_keys[d])
                layer_of[d] = li
            if members != sorted(members):
                raise ValueError("the device backend sums a layer in column order: list layer %r in res_keys order" % self.layer_names[li])
        for d in range(D):
            prm.col[d], prm.layer_of[d], prm.w[d] = self.cols[d], layer_of[d], float(self.w[d])
        for li, b in enumerate(self.beta):
            prm.beta[li] = b
        prm.p_layer, prm.z_safe, prm.lambda_decay = self.p, self.z_safe, self.lam
        prm.k_logistic, prm.c0_logistic, prm.c_max, prm.alpha_smooth = self.k, self.C0, self.C_max, self.alpha
        return prm


_PARAM_NAMES = ("res_keys", "feature_weights", "layer_config", "layer_weights", "p_layer", "z_safe", "lambda_decay",
                "k_logistic", "C0_logistic", "C_max", "alpha_smooth", "columns")


def _fault_labels(fault_name):
    """Labels of a fault class: a class name, one of the reference's keys, or an explicit iterable of labels."""
    if isinstance(fault_name, str):
        name = FAULT_ALIASES.get(fault_name, fault_name)
        if name not in FAULT_RANGE_MAP:
            raise ValueError("unknown fault class %r; choose one of %s or pass the labels themselves"
                             % (fault_name, list(FAULT_RANGE_MAP) + list(FAULT_ALIASES)))
        return [int(v) for v in FAULT_RANGE_MAP[name]]
    return [int(v) for v in fault_name]


# ---------------------------------------------------------------------------------------------- host backend
def _host_stats(arr, cols, label_col, normal_labels):
    labels = arr[:, label_col].astype(int)
    normal = np.isin(labels, list(normal_labels))
    if not normal.any():
        raise ValueError("no rows carry a normal label %s" % (tuple(normal_labels),))
    block = np.stack([arr[normal, c].astype(float) for c in cols], axis=1)
    mu = np.nanmean(block, axis=0)
    sigma = np.nanstd(block, axis=0, ddof=1)
    sigma[sigma == 0] = 1e-6
    return mu, sigma


def _host_series(R, mu, sigma, cfg, seg_starts=None, carry_in=None):
    """Float64 numpy restatement; R is [n, D].  Both recurrences are the sequential loops, restarted at every segment start.
    Returns S_layers (list), S_tot, C, RF_inst, RF_smooth, carry_out [n_seg, 2]."""
    n = R.shape[0]
    z = (R - np.asarray(mu, dtype=float).reshape(1, -1)) / np.asarray(sigma, dtype=float).reshape(1, -1)
    excess = np.maximum(0.0, np.abs(z) - cfg.z_safe)
    S_layers = []
    for members in cfg.layers:
        if not members:
            S_layers.append(np.zeros(n, dtype=float))
            continue
        weighted = cfg.w[members].reshape(1, -1) * np.power(excess[:, members], cfg.p)
        S_layers.append(np.power(weighted.sum(axis=1), 1.0 / cfg.p))
    S_tot = np.zeros(n, dtype=float)
    for beta, S_l in zip(cfg.beta, S_layers):
        S_tot += beta * S_l

    starts = [0] if seg_starts is None or len(seg_starts) == 0 else [int(s) for s in seg_starts]
    bounds = starts + [n]
    carry = None if carry_in is None else np.asarray(carry_in, dtype=float).reshape(len(starts), 2)
    lam, alpha = cfg.lam, cfg.alpha
    C = np.zeros(n, dtype=float)
    for si in range(len(starts)):
        b, e = bounds[si], bounds[si + 1]
        if e <= b:
            continue
        if carry is not None:
            C[b] = lam * carry[si, 0] + S_tot[b]
        for t in range(b + 1, e):
            C[t] = lam * C[t - 1] + S_tot[t]

    L0 = 1.0 / (1.0 + np.exp(-cfg.k * (0.0 - cfg.C0)))
    L_max = 1.0 / (1.0 + np.exp(-cfg.k * (cfg.C_max - cfg.C0)))
    denom = (L_max - L0) if (L_max - L0) != 0 else 1e-6
    RF_inst = np.clip((1.0 / (1.0 + np.exp(-cfg.k * (np.clip(C, 0.0, cfg.C_max) - cfg.C0))) - L0) / denom, 0.0, 1.0)

    RF_smooth = np.zeros(n, dtype=float)
    carry_out = np.full((len(starts), 2), np.nan)
    for si in range(len(starts)):
        b, e = bounds[si], bounds[si + 1]
        if e <= b:
            continue
        RF_smooth[b] = RF_inst[b] if carry is None else alpha * RF_inst[b] + (1.0 - alpha) * carry[si, 1]
        for t in range(b + 1, e):
            RF_smooth[t] = alpha * RF_inst[t] + (1.0 - alpha) * RF_smooth[t - 1]
        carry_out[si] = (C[e - 1], RF_smooth[e - 1])
    return S_layers, S_tot, C, RF_inst, RF_smooth, carry_out


def _host_first(series, threshold, mode):
    if mode == "above":
        hits = np.flatnonzero(series >= threshold)
    elif mode == "below":
        hits = np.flatnonzero(series <= threshold)
    else:
        raise ValueError("mode must be 'above' or 'below'")
    return int(hits[0]) if hits.size else None


# ---------------------------------------------------------------------------------------------- device backend
def _device_stats(arr, cols, label_col, normal_labels):
    torch, _lib, lib = _torch_lib()
    D = len(cols)
    if D < 1 or D > MAX_COLS or len(normal_labels) < 1 or len(normal_labels) > MAX_COLS:
        raise ValueError("the device backend takes 1 to %d columns and 1 to %d normal labels" % (MAX_COLS, MAX_COLS))
    with torch.cuda.device(arr.device):
        out = torch.empty(2, MAX_COLS, dtype=torch.float64, device=arr.device)
        count = torch.empty(MAX_COLS + 1, dtype=torch.int64, device=arr.device)
        ws = torch.empty(lib.pinn_rf_stats_workspace_bytes(), dtype=torch.uint8, device=arr.device)
        c_cols = (ctypes.c_int * D)(*cols)
        c_norm = (ctypes.c_longlong * len(normal_labels))(*[int(v) for v in normal_labels])
        ld = arr.stride(0) if arr.shape[0] > 0 else arr.shape[1]
        call("pinn_rf_stats", arr, ld, arr.shape[0], c_cols, D, label_col, c_norm, len(normal_labels), out[0], out[1], count, ws, ws.numel())
        if int(count[MAX_COLS].item()) == 0:
            raise ValueError("no rows carry a normal label %s" % (tuple(normal_labels),))
    return out[0, :D], out[1, :D]


def _device_series(arr, mu, sigma, cfg, row_index=None, seg_starts=None, carry_in=None, want=("RF_inst", "RF_smooth", "S_layers", "S_tot", "C")):
    """One pinn_rf_series call.  Returns a dict of device tensors: the wanted series and "carry_out" [n_seg, 2]."""
    torch, _lib, lib = _torch_lib()
    dev = arr.device
    prm = cfg.c_struct()
    if arr.shape[1] <= max(cfg.cols):
        raise ValueError("results has %d columns, column %d is needed" % (arr.shape[1], max(cfg.cols)))
    with torch.cuda.device(dev):
        mu_d, sg_d = _dev_vec(torch, mu, torch.float64, dev), _dev_vec(torch, sigma, torch.float64, dev)
        if mu_d.numel() != prm.n_cols or sg_d.numel() != prm.n_cols:
            raise ValueError("mu and sigma must have one entry per residual key (%d)" % prm.n_cols)
        ridx = _dev_vec(torch, row_index, torch.int64, dev)
        n = arr.shape[0] if ridx is None else ridx.numel()
        seg = _dev_vec(torch, seg_starts, torch.int64, dev)
        n_seg = 1 if seg is None or seg.numel() == 0 else seg.numel()
        if seg is not None and seg.numel() == 0:
            seg = None
        cin = None
        if carry_in is not None:
            cin = _dev_vec(torch, carry_in, torch.float64, dev)
            if cin.numel() != 2 * n_seg:
                raise ValueError("carry_in must hold (C, RF_smooth) per segment")
        out = {}
        for name in ("S_tot", "C", "RF_inst", "RF_smooth"):
            out[name] = torch.empty(n, dtype=torch.float64, device=dev) if name in want else None
        layers = torch.empty(prm.n_layers, n, dtype=torch.float64, device=dev) if "S_layers" in want else None
        cout = torch.full((n_seg, 2), float("nan"), dtype=torch.float64, device=dev)
        wb = lib.pinn_rf_workspace_bytes(n, n_seg)
        ws = torch.empty(wb, dtype=torch.uint8, device=dev) if wb else None
        ld = arr.stride(0) if arr.shape[0] > 0 else max(arr.shape[1], 1)
        call("pinn_rf_series", arr, ld, arr.shape[0], ctypes.byref(prm), mu_d, sg_d, ridx, n, seg, 0 if seg is None else n_seg, cin, layers,
             out["S_tot"], out["C"], out["RF_inst"], out["RF_smooth"], cout, ws, wb)
    res = {k: v for k, v in out.items() if v is not None}
    if layers is not None:
        res["S_layers"] = {name: layers[i] for i, name in enumerate(cfg.layer_names)}
    res["carry_out"] = cout
    return res


def _device_first(series, threshold, mode, stride=1, n_src=None, row_index=None, seg_starts=None, relative=False):
    """pinn_rf_first_alarm -> int64 device tensor [n_seg] (-1: none)."""
    torch, _lib, lib = _torch_lib()
    if mode not in ("above", "below"):
        raise ValueError("mode must be 'above' or 'below'")
    dev = series.device
    with torch.cuda.device(dev):
        ridx = _dev_vec(torch, row_index, torch.int64, dev)
        seg = _dev_vec(torch, seg_starts, torch.int64, dev)
        if seg is not None and seg.numel() == 0:
            seg = None
        n_src = series.numel() if n_src is None else n_src
        n = n_src if ridx is None else ridx.numel()
        first = torch.empty(1 if seg is None else seg.numel(), dtype=torch.int64, device=dev)
        call("pinn_rf_first_alarm", series, stride, n_src, ridx, n, seg, 0 if seg is None else seg.numel(),
             _lib.RF_ABOVE if mode == "above" else _lib.RF_BELOW, 1 if relative else 0, float(threshold), first)
    return first


# ---------------------------------------------------------------------------------------------- public functions
def estimate_mu_sigma_normal(results, res_keys=RF_RES_KEYS, normal_labels=NORMAL_LABELS, backend="auto"):
    """Mean and standard deviation (ddof=1, NaN-aware) of the residual columns over the rows with a normal label."""
    cols = [INDEX[k] for k in res_keys]
    if _pick_backend(backend, results) == "host":
        return _host_stats(_as_numpy(results), cols, INDEX["label"], normal_labels)
    import torch
    arr = _dev_f64_rows(torch, results)
    if arr.shape[1] <= INDEX["label"]:
        raise ValueError("results has %d columns, the label column %d is needed" % (arr.shape[1], INDEX["label"]))
    mu, sigma = _device_stats(arr, cols, INDEX["label"], tuple(normal_labels))
    return (mu, sigma) if _is_tensor(results) else (mu.cpu().numpy(), sigma.cpu().numpy())


def rf_series(results, mu, sigma, row_index=None, seg_starts=None, carry_in=None, backend="auto", **params):
    """The RF series over `results` rows (or over the rows `row_index` lists, in that order), restarted at every position in
    `seg_starts` (ascending, the first 0), optionally continued from `carry_in` = (C, RF_smooth) per segment.
    `params`: the keyword arguments of compute_rf_time_series, and `columns` to read the residuals from other columns.
    Returns a dict: "S_layers" (dict), "S_tot", "C", "RF_inst", "RF_smooth", "carry_out" [n_seg, 2]."""
    unknown = set(params) - set(_PARAM_NAMES)
    if unknown:
        raise TypeError("unknown arguments: %s" % sorted(unknown))
    cfg = _Config(**params)
    if seg_starts is not None and not _is_tensor(seg_starts) and len(seg_starts) > 0:
        starts = np.asarray(seg_starts, dtype=np.int64).reshape(-1)
        n_pos = np.shape(results)[0] if row_index is None else len(row_index)
        if starts[0] != 0 or np.any(np.diff(starts) <= 0) or starts[-1] >= max(n_pos, 1):
            raise ValueError("seg_starts must begin with 0 and ascend strictly inside the %d positions" % n_pos)
    if _pick_backend(backend, results) == "host":
        arr = _as_numpy(results)
        rows = arr if row_index is None else arr[_as_numpy(row_index, np.int64)]
        R = np.stack([rows[:, c].astype(float) for c in cfg.cols], axis=1)
        starts = None if seg_starts is None else _as_numpy(seg_starts, np.int64)
        cin = None if carry_in is None else _as_numpy(carry_in, float)
        S_layers, S_tot, C, RF_inst, RF_smooth, cout = _host_series(R, _as_numpy(mu, float), _as_numpy(sigma, float), cfg, starts, cin)
        return {"S_layers": dict(zip(cfg.layer_names, S_layers)), "S_tot": S_tot, "C": C, "RF_inst": RF_inst,
                "RF_smooth": RF_smooth, "carry_out": cout}
    import torch
    res = _device_series(_dev_f64_rows(torch, results), mu, sigma, cfg, row_index, seg_starts, carry_in)
    if _is_tensor(results):
        return res
    res["S_layers"] = {k: v.cpu().numpy() for k, v in res["S_layers"].items()}
    return {k: (v if k == "S_layers" else v.cpu().numpy()) for k, v in res.items()}


def compute_rf_time_series(results, mu, sigma, res_keys=RF_RES_KEYS, feature_weights=RF_FEATURE_WEIGHTS,
                           layer_config=RF_LAYER_CONFIG, layer_weights=RF_LAYER_WEIGHTS, p_layer=RF_P_LAYER, z_safe=RF_Z_SAFE,
                           lambda_decay=RF_LAMBDA_DECAY, k_logistic=RF_K_LOGISTIC, C0_logistic=RF_C0_LOGISTIC, C_max=RF_C_MAX,
                           alpha_smooth=RF_ALPHA_SMOOTH, backend="auto"):
    """RF_inst, RF_smooth, {"S_layers", "S_tot", "C"} over all rows as one series."""
    r = rf_series(results, mu, sigma, backend=backend, res_keys=res_keys, feature_weights=feature_weights,
                  layer_config=layer_config, layer_weights=layer_weights, p_layer=p_layer, z_safe=z_safe,
                  lambda_decay=lambda_decay, k_logistic=k_logistic, C0_logistic=C0_logistic, C_max=C_max, alpha_smooth=alpha_smooth)
    return r["RF_inst"], r["RF_smooth"], {"S_layers": r["S_layers"], "S_tot": r["S_tot"], "C": r["C"]}


def find_first_alarm_index(series, threshold, mode="above", backend="auto"):
    """First index with series >= threshold ("above") or <= threshold ("below"); None when there is none.  NaN never matches."""
    if _pick_backend(backend, series) == "host":
        return _host_first(_as_numpy(series), threshold, mode)
    import torch
    s = series if _is_tensor(series) else torch.from_numpy(np.ascontiguousarray(np.asarray(series, dtype=np.float64)))
    s = s.detach().to("cuda" if not s.is_cuda else s.device, torch.float64).reshape(-1).contiguous()
    first = int(_device_first(s, threshold, mode).item())
    return None if first < 0 else first


def _none_if_negative(v):
    v = int(v)
    return None if v < 0 else v


def rf_advance_for_conditions(results, mu, sigma, conditions=None, current_tol=CURRENT_TOL, backend="auto", **params):
    """Early-warning lead of every (current_target, fault, [index_range]) in `conditions` (default RF_CONDITIONS).

    The rows of a condition (label in the fault's labels, |current - target| <= tol, then the optional relative
    index_range) form one sub-series.  The device backend concatenates the gather lists and evaluates all sub-series in
    ONE pinn_rf_series call, one segment per condition; the two alarms are one pinn_rf_first_alarm call each.
    Returns one dict per condition: n (rows used), idx_v_alarm (first V <= V[0] - 0.1), idx_rf_warn (first RF_smooth >=
    RF_WARN_THRESHOLD), delta_idx (= idx_v_alarm - idx_rf_warn, positive: RF warns earlier; None unless both fire), and
    n_total (rows before index_range), v_threshold."""
    conditions = RF_CONDITIONS if conditions is None else list(conditions)
    unknown = set(params) - set(_PARAM_NAMES)
    if unknown:
        raise TypeError("unknown arguments: %s" % sorted(unknown))
    cfg = _Config(**params)
    parsed = []
    for cond in conditions:
        if len(cond) not in (2, 3):
            raise ValueError("a condition is (current_target, fault[, index_range]), got %r" % (cond,))
        parsed.append((float(cond[0]), _fault_labels(cond[1]), cond[2] if len(cond) == 3 else None))

    def window(total, index_range):
        if index_range is None:
            return 0, total
        start, end = index_range
        start = max(int(start), 0)
        end = total if end is None or end > total else int(end)
        return (start, end) if start < end else (0, 0)

    host = _pick_backend(backend, results) == "host"
    if host:
        arr = _as_numpy(results)
        labels = arr[:, INDEX["label"]].astype(int)
        current = arr[:, INDEX[CURRENT_COL]].astype(float)
        picks = [np.flatnonzero(np.isin(labels, labs) & (np.abs(current - target) <= current_tol)) for target, labs, _ in parsed]
    else:
        import torch
        arr = _dev_f64_rows(torch, results)
        labels = arr[:, INDEX["label"]].long()
        current = arr[:, INDEX[CURRENT_COL]]
        picks = [torch.nonzero(torch.isin(labels, torch.tensor(labs, device=arr.device)) & ((current - target).abs() <= current_tol)).reshape(-1)
                 for target, labs, _ in parsed]
    out, used = [], []
    for (target, labs, index_range), idx in zip(parsed, picks):
        total = int(idx.shape[0])
        a, b = window(total, index_range)
        out.append({"n": b - a, "n_total": total, "idx_v_alarm": None, "idx_rf_warn": None, "delta_idx": None, "v_threshold": None})
        used.append(idx[a:b])
    live = [i for i, u in enumerate(used) if u.shape[0] > 0]
    if not live:
        return out
    if host:
        for i in live:
            sub = arr[used[i]]
            R = np.stack([sub[:, c].astype(float) for c in cfg.cols], axis=1)
            RF_smooth = _host_series(R, _as_numpy(mu, float), _as_numpy(sigma, float), cfg)[4]
            V = sub[:, INDEX["y_true"]].astype(float)
            thr = float(V[0]) - V_ALARM_DROP
            out[i].update(v_threshold=thr, idx_v_alarm=_host_first(V, thr, "below"),
                          idx_rf_warn=_host_first(RF_smooth, RF_WARN_THRESHOLD, "above"))
    else:
        ridx = torch.cat([used[i] for i in live])
        lens = [int(used[i].shape[0]) for i in live]
        starts = torch.tensor(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), device=arr.device)
        r = _device_series(arr, mu, sigma, cfg, ridx, starts, None, want=("RF_smooth",))
        rf_first = _device_first(r["RF_smooth"], RF_WARN_THRESHOLD, "above", seg_starts=starts)
        ycol = arr[:, INDEX["y_true"]]
        v_first = _device_first(ycol, -V_ALARM_DROP, "below", stride=arr.stride(0), n_src=arr.shape[0], row_index=ridx,
                                seg_starts=starts, relative=True)
        v0 = ycol[ridx[starts]] - V_ALARM_DROP
        rf_first, v_first, v0 = rf_first.cpu().numpy(), v_first.cpu().numpy(), v0.cpu().numpy()
        for k, i in enumerate(live):
            out[i].update(v_threshold=float(v0[k]), idx_v_alarm=_none_if_negative(v_first[k]), idx_rf_warn=_none_if_negative(rf_first[k]))
    for o in out:
        if o["idx_v_alarm"] is not None and o["idx_rf_warn"] is not None:
            o["delta_idx"] = o["idx_v_alarm"] - o["idx_rf_warn"]
    return out


def compute_rf_advance_for_condition(results, mu, sigma, fault_name, current_target, current_tol=CURRENT_TOL, res_keys=RF_RES_KEYS,
                                     feature_weights=RF_FEATURE_WEIGHTS, layer_config=RF_LAYER_CONFIG,
                                     layer_weights=RF_LAYER_WEIGHTS, p_layer=RF_P_LAYER, z_safe=RF_Z_SAFE,
                                     lambda_decay=RF_LAMBDA_DECAY, k_logistic=RF_K_LOGISTIC, C0_logistic=RF_C0_LOGISTIC,
                                     C_max=RF_C_MAX, alpha_smooth=RF_ALPHA_SMOOTH, V_THRESHOLD=V_THRESHOLD_COND,
                                     RF_THRESHOLD=RF_THRESHOLD_COND, plot=False, index_range=None, backend="auto"):
    """Samples by which the RF warning precedes the voltage alarm for one current plateau and fault class (positive: RF is
    earlier); None when the condition has no rows or one of the two alarms does not fire.  `fault_name`: a class name of
    FAULT_RANGE_MAP, one of the reference's keys, or the labels themselves.  V_THRESHOLD and RF_THRESHOLD are accepted and
    unused, as in the reference.  No figure is drawn."""
    if plot:
        raise NotImplementedError("plot=True: figures (matplotlib) are out of scope of pinn_amd.risk; pass plot=False")
    _fault_labels(fault_name)             # an unknown name fails before any work
    tag = "[%sA %s]" % (current_target, fault_name if isinstance(fault_name, str) else list(fault_name))
    r = rf_advance_for_conditions(results, mu, sigma, [(current_target, fault_name, index_range)], current_tol=current_tol,
                                  backend=backend, res_keys=res_keys, feature_weights=feature_weights, layer_config=layer_config,
                                  layer_weights=layer_weights, p_layer=p_layer, z_safe=z_safe, lambda_decay=lambda_decay,
                                  k_logistic=k_logistic, C0_logistic=C0_logistic, C_max=C_max, alpha_smooth=alpha_smooth)[0]
    if r["n_total"] == 0:
        print("%s no rows match this condition." % tag)
        return None
    if r["n"] == 0:
        print("%s index_range %s leaves none of the %d matching rows." % (tag, index_range, r["n_total"]))
        return None
    if index_range is not None:
        print("%s index_range %s: %d of %d matching rows used" % (tag, tuple(index_range), r["n"], r["n_total"]))
    else:
        print("%s no index_range: all %d matching rows used" % (tag, r["n_total"]))
    print(tag)
    print("  sub-series length: %d (matching rows: %d)" % (r["n"], r["n_total"]))
    print("  voltage alarm threshold = V(0) - %.1f = %.4f" % (V_ALARM_DROP, r["v_threshold"]))
    print("  RF warning threshold = %s" % RF_WARN_THRESHOLD)
    print("  RF danger threshold = %s" % RF_DANGER_THRESHOLD)
    print("  first voltage alarm (sub-series index): %s" % r["idx_v_alarm"])
    print("  first RF warning (sub-series index): %s" % r["idx_rf_warn"])
    if r["delta_idx"] is None:
        print("  one of the two alarms did not fire: no lead to report.")
    else:
        print("  ==> the RF warning precedes the voltage alarm by %d samples (positive: earlier)." % r["delta_idx"])
    return r["delta_idx"]


# ---------------------------------------------------------------------------------------------- online monitor
class RiskMonitor:
    """RF(t) chunk by chunk on the device: `update` continues both recurrences from the carried (C, RF_smooth) and latches
    the first global row at which RF_smooth reaches the warning and the danger threshold.  A chunk of up to 2048 rows is
    one kernel launch.  `params`: the keyword arguments of compute_rf_time_series."""

    def __init__(self, mu, sigma, warn_threshold=RF_WARN_THRESHOLD, danger_threshold=RF_DANGER_THRESHOLD, **params):
        unknown = set(params) - set(_PARAM_NAMES)
        if unknown:
            raise TypeError("unknown arguments: %s" % sorted(unknown))
        self._params = dict(params)
        self._cfg = _Config(**params)
        self._mu, self._sigma = mu, sigma
        self.warn_threshold, self.danger_threshold = float(warn_threshold), float(danger_threshold)
        self._five = None
        self.reset()

    def reset(self):
        """Forget the carried state and the latched alarms."""
        self._carry = None
        self._first = None
        self.n_seen = 0

    def _series(self, arr, cfg, return_C=False):
        torch, _, _ = _torch_lib()
        n = arr.shape[0]
        if n == 0:
            empty = torch.empty(0, dtype=torch.float64, device=arr.device)
            return (empty, empty.clone()) if return_C else empty
        if not _is_tensor(self._mu) or self._mu.device != arr.device:
            self._mu = _dev_vec(torch, self._mu, torch.float64, arr.device)
            self._sigma = _dev_vec(torch, self._sigma, torch.float64, arr.device)
        r = _device_series(arr, self._mu, self._sigma, cfg, None, None, self._carry, want=("RF_smooth", "C") if return_C else ("RF_smooth",))
        rf = r["RF_smooth"]
        self._carry = r["carry_out"]
        hits = torch.cat([_device_first(rf, self.warn_threshold, "above"), _device_first(rf, self.danger_threshold, "above")])
        if self._first is None:
            self._first = torch.full((2,), -1, dtype=torch.int64, device=arr.device)
        self._first = torch.where((self._first < 0) & (hits >= 0), hits + self.n_seen, self._first)
        self.n_seen += n
        return (rf, r["C"]) if return_C else rf

    def update(self, rows, return_C=False):
        """`rows`: the next chunk of results rows [n, >= 17] (device tensor, or a host array that is uploaded).
        Returns the chunk's RF_smooth as a device tensor; with return_C=True the pair (RF_smooth, C)."""
        import torch
        return self._series(_dev_f64_rows(torch, rows), self._cfg, return_C)

    def update_rows(self, model, x_norm, y_norm, scaler_X, scaler_Y, return_C=False):
        """Online form: the next chunk as normalised inputs and targets.  One eval-mode forward and one fused residual pass
        give res, pV, pT, pH, pO (columns 12-16 of the results array: 9 is the eval forward, de-normalised in float64 with
        +1e-12 in the scale as results.py does; 8 is the float32 inverse transform of the target); no MC-dropout runs."""
        torch, _lib, _ = _torch_lib()
        if self._cfg.res_keys != RF_RES_KEYS or "columns" in self._params:
            raise ValueError("update_rows builds the five default residual columns %s" % (RF_RES_KEYS,))
        model.dnn.eval()
        xd = model._dev_rows(x_norm)
        yd = y_norm.detach().to(xd.device, torch.float32).reshape(-1).contiguous()
        u, _ = model.net_u(xd)
        cols = model._residuals(xd, scaler_X, _lib.RES_ALL, u=u.reshape(-1))
        lo, hi = float(scaler_Y.feature_range[0]), float(scaler_Y.feature_range[1])
        data_min = float(np.asarray(scaler_Y.data_min_, dtype=np.float64).reshape(-1)[0])
        data_max = float(np.asarray(scaler_Y.data_max_, dtype=np.float64).reshape(-1)[0])
        scale_y = (hi - lo) / (data_max - data_min + 1e-12)
        min_y = lo - data_min * scale_y
        y_min = float(np.asarray(scaler_Y.min_, dtype=np.float64).reshape(-1)[0])
        y_scale = float(np.asarray(scaler_Y.scale_, dtype=np.float64).reshape(-1)[0])
        y_true = ((yd.double() - y_min).float().double() / y_scale).float().double()
        y_pred = (u.detach().reshape(-1).double() - min_y) / (scale_y + 1e-12)
        C = _lib.C
        five = torch.stack([y_true - y_pred, cols[C["FV"]].double(), cols[C["FT"]].double(), cols[C["FH"]].double(),
                            cols[C["FO"]].double()], dim=1)
        if self._five is None:
            self._five = _Config(**dict(self._params, columns=range(5)))
        self.last_columns = five
        return self._series(five, self._five, return_C)

    @property
    def state(self):
        """(C, RF_smooth) after the last row seen, or None before the first."""
        if self._carry is None:
            return None
        c = self._carry.cpu().numpy().reshape(-1)
        return float(c[0]), float(c[1])

    def _latched(self, k):
        if self._first is None:
            return None
        return _none_if_negative(self._first[k].item())

    @property
    def first_warning(self):
        """Global row number of the first RF_smooth >= warn_threshold, or None."""
        return self._latched(0)

    @property
    def first_danger(self):
        return self._latched(1)
