"""Risk function RF(t) and early-warning index: the stage after `comprehensive_results` (reference script 04).

Public names, argument names and defaults follow script 04, so a call written for it runs here:
`estimate_mu_sigma_normal`, `compute_rf_time_series`, `find_first_alarm_index`, `compute_rf_advance_for_condition`.
Added: `rf_series` (gather lists, segments, carried state), `rf_advance_for_conditions` (all conditions in one device
call), `RiskMonitor` (online use, chunk by chunk), and the calibration of the hand-set parameters: `rf_grid`, `rf_sweep`
(P parameter sets over all conditions and the normal rows in one device call) and `calibrate_rf`.

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


def _condition_rows(results, conditions, current_tol, backend):
    """The sub-series of every (current_target, fault[, index_range]): rows whose label is one of the fault's and whose
    current lies within the tolerance of the target, then the optional relative index_range.  Returns (host, arr, out,
    used): the backend taken, the array on its side, one result dict per condition (n and n_total filled in) and the row
    lists (numpy on the host, tensors on the device)."""
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
    return host, arr, out, used


def _device_voltage_alarm(arr, ridx, starts):
    """First V <= V[first] - 0.1 of every segment of the gathered rows (04:389-390) -> (first [n_seg], threshold [n_seg]), device."""
    ycol = arr[:, INDEX["y_true"]]
    v_first = _device_first(ycol, -V_ALARM_DROP, "below", stride=arr.stride(0), n_src=arr.shape[0], row_index=ridx,
                            seg_starts=starts, relative=True)
    return v_first, ycol[ridx[starts]] - V_ALARM_DROP


def rf_advance_for_conditions(results, mu, sigma, conditions=None, current_tol=CURRENT_TOL, backend="auto",
                              warn_threshold=RF_WARN_THRESHOLD, danger_threshold=RF_DANGER_THRESHOLD, **params):
    """Early-warning lead of every (current_target, fault, [index_range]) in `conditions` (default RF_CONDITIONS).

    The rows of a condition (label in the fault's labels, |current - target| <= tol, then the optional relative
    index_range) form one sub-series.  The device backend concatenates the gather lists and evaluates all sub-series in
    ONE pinn_rf_series call, one segment per condition; the two alarms are one pinn_rf_first_alarm call each.
    Returns one dict per condition: n (rows used), idx_v_alarm (first V <= V[0] - 0.1), idx_rf_warn (first RF_smooth >=
    warn_threshold), delta_idx (= idx_v_alarm - idx_rf_warn, positive: RF warns earlier; None unless both fire), and
    n_total (rows before index_range), v_threshold.  `danger_threshold` is accepted and unused, so that a calibrated
    parameter set (calibrate_rf's `.params`) replays here as it stands."""
    conditions = RF_CONDITIONS if conditions is None else list(conditions)
    unknown = set(params) - set(_PARAM_NAMES)
    if unknown:
        raise TypeError("unknown arguments: %s" % sorted(unknown))
    cfg = _Config(**params)
    warn_threshold = float(warn_threshold)
    host, arr, out, used = _condition_rows(results, conditions, current_tol, backend)
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
                          idx_rf_warn=_host_first(RF_smooth, warn_threshold, "above"))
    else:
        import torch
        ridx = torch.cat([used[i] for i in live])
        lens = [int(used[i].shape[0]) for i in live]
        starts = torch.tensor(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), device=arr.device)
        r = _device_series(arr, mu, sigma, cfg, ridx, starts, None, want=("RF_smooth",))
        rf_first = _device_first(r["RF_smooth"], warn_threshold, "above", seg_starts=starts)
        v_first, v0 = _device_voltage_alarm(arr, ridx, starts)
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
                                     RF_THRESHOLD=RF_THRESHOLD_COND, plot=False, index_range=None, backend="auto",
                                     warn_threshold=RF_WARN_THRESHOLD):
    """Samples by which the RF warning precedes the voltage alarm for one current plateau and fault class (positive: RF is
    earlier); None when the condition has no rows or one of the two alarms does not fire.  `fault_name`: a class name of
    FAULT_RANGE_MAP, one of the reference's keys, or the labels themselves.  V_THRESHOLD and RF_THRESHOLD are accepted and
    unused, as in the reference; `warn_threshold` is the RF warning level (the reference reads its module constant).  No
    figure is drawn."""
    if plot:
        raise NotImplementedError("plot=True: figures (matplotlib) are out of scope of pinn_amd.risk; pass plot=False")
    _fault_labels(fault_name)             # an unknown name fails before any work
    tag = "[%sA %s]" % (current_target, fault_name if isinstance(fault_name, str) else list(fault_name))
    r = rf_advance_for_conditions(results, mu, sigma, [(current_target, fault_name, index_range)], current_tol=current_tol,
                                  backend=backend, res_keys=res_keys, feature_weights=feature_weights, layer_config=layer_config,
                                  layer_weights=layer_weights, p_layer=p_layer, z_safe=z_safe, lambda_decay=lambda_decay,
                                  k_logistic=k_logistic, C0_logistic=C0_logistic, C_max=C_max, alpha_smooth=alpha_smooth,
                                  warn_threshold=warn_threshold)[0]
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
    print("  RF warning threshold = %s" % warn_threshold)
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


# ---------------------------------------------------------------------------------------------- sweep and calibration
_STRUCTURAL_NAMES = ("res_keys", "layer_config", "columns")
_SWEEP_SCALARS = ("p_layer", "z_safe", "lambda_decay", "k_logistic", "C0_logistic", "C_max", "alpha_smooth",
                  "warn_threshold", "danger_threshold")               # words 12..20 of a candidate, in this order
_SWEEP_NAMES = ("feature_weights", "layer_weights") + _SWEEP_SCALARS
_SWEEP_DEFAULTS = {"feature_weights": None, "layer_weights": RF_LAYER_WEIGHTS, "p_layer": RF_P_LAYER, "z_safe": RF_Z_SAFE,
                   "lambda_decay": RF_LAMBDA_DECAY, "k_logistic": RF_K_LOGISTIC, "C0_logistic": RF_C0_LOGISTIC, "C_max": RF_C_MAX,
                   "alpha_smooth": RF_ALPHA_SMOOTH, "warn_threshold": RF_WARN_THRESHOLD, "danger_threshold": RF_DANGER_THRESHOLD}
SWEEP_WORDS = 24                        # float64 words of one candidate (include/pinn_hip.h: PINN_RF_SWEEP_WORDS)


def _check_sweep_names(names, what):
    for name in names:
        if name in _STRUCTURAL_NAMES:
            raise ValueError("%s: %r is structure (which columns, which layers), fixed per call and not swept" % (what, name))
        if name not in _SWEEP_NAMES:
            raise TypeError("%s: unknown name %r; choose among %s" % (what, name, list(_SWEEP_NAMES)))


def rf_grid(**axes):
    """The Cartesian product of the named axes, e.g. rf_grid(z_safe=[1.5, 2, 3], lambda_decay=[0.99, 1.0]): one array of
    length P per name, the first axis slowest and the last fastest (itertools.product order).  Axes: the scalar arguments
    of compute_rf_time_series, warn_threshold, danger_threshold, feature_weights (a list of weight vectors -> [P, D]) and
    layer_weights (a list of dicts -> an object array of dicts).  Structural names (res_keys, layer_config, columns) and
    unknown ones raise."""
    import itertools
    _check_sweep_names(axes, "rf_grid")
    values = {k: list(v) for k, v in axes.items()}
    for k, v in values.items():
        if not v:
            raise ValueError("rf_grid: axis %r is empty" % k)
    combos = list(itertools.product(*values.values())) if values else []
    out = {}
    for pos, name in enumerate(values):
        col = [c[pos] for c in combos]
        if name == "layer_weights":
            arr = np.empty(len(col), dtype=object)
            for i, d in enumerate(col):
                arr[i] = dict(d)
            out[name] = arr
        elif name == "feature_weights":
            out[name] = np.asarray(col, dtype=float).reshape(len(col), -1)
        else:
            out[name] = np.asarray(col, dtype=float)
    return out


def _candidate_table(candidates, fixed):
    """-> (cfg0, structure, P, table [P, 24] float64).  `cfg0` carries the structure: columns, layers and their names."""
    _check_sweep_names(candidates, "candidates")
    unknown = set(fixed) - set(_PARAM_NAMES) - {"warn_threshold", "danger_threshold"}
    if unknown:
        raise TypeError("unknown arguments: %s" % sorted(unknown))
    both = set(candidates) & set(fixed)
    if both:
        raise ValueError("%s given both per candidate and fixed" % sorted(both))
    if not candidates:
        raise ValueError("candidates is empty: name at least one swept parameter (rf_grid builds the table)")
    lengths = {k: len(v) for k, v in candidates.items()}
    P = next(iter(lengths.values()))
    if P < 1 or any(n != P for n in lengths.values()):
        raise ValueError("every candidate array needs the same length >= 1, got %s" % lengths)
    structure = {k: fixed[k] for k in _STRUCTURAL_NAMES if k in fixed}
    cfg0 = _Config(**structure)
    D, names = len(cfg0.cols), cfg0.layer_names
    if D > MAX_COLS or len(names) > MAX_LAYERS:
        raise ValueError("a sweep takes at most %d residual columns and %d layers" % (MAX_COLS, MAX_LAYERS))

    def column(name):
        return candidates[name] if name in candidates else fixed.get(name, _SWEEP_DEFAULTS[name])

    table = np.zeros((P, SWEEP_WORDS), dtype=np.float64)
    fw = column("feature_weights")
    w = np.ones(D, dtype=float) if fw is None else np.asarray(fw, dtype=float)
    if w.shape not in ((D,), (P, D)) or ("feature_weights" in candidates and w.shape != (P, D)):
        raise ValueError("feature_weights must have length %d per candidate, got an array of shape %s" % (D, w.shape))
    table[:, :D] = w
    lw = column("layer_weights")
    if "layer_weights" in candidates:
        for i in range(P):
            table[i, MAX_COLS:MAX_COLS + len(names)] = [float(lw[i].get(name, 1.0)) for name in names]
    else:
        table[:, MAX_COLS:MAX_COLS + len(names)] = [float(lw.get(name, 1.0)) for name in names]
    for k, name in enumerate(_SWEEP_SCALARS):
        table[:, MAX_COLS + MAX_LAYERS + k] = np.asarray(column(name), dtype=float)
    return cfg0, structure, P, table


def _table_params(table, i, cfg0, structure):
    """Keyword arguments of candidate i: they feed rf_series, rf_advance_for_conditions and RiskMonitor as they stand."""
    D, names = len(cfg0.cols), cfg0.layer_names
    row = table[i]
    out = dict(structure)
    out["feature_weights"] = row[:D].copy()
    out["layer_weights"] = {name: float(row[MAX_COLS + k]) for k, name in enumerate(names)}
    for k, name in enumerate(_SWEEP_SCALARS):
        out[name] = float(row[MAX_COLS + MAX_LAYERS + k])
    return out


def _table_bad(table):
    return ~np.isfinite(table).all(axis=1) | (table[:, MAX_COLS + MAX_LAYERS] == 0.0)


def _quiet_ranges(quiet, labels_of, n_rows):
    """Row ranges on which a warning is a false alarm: "normal" -> every maximal run of consecutive rows with a label in
    NORMAL_LABELS; a list of (start, end); None -> none."""
    if quiet is None:
        return []
    if isinstance(quiet, str):
        if quiet != "normal":
            raise ValueError("quiet must be 'normal', a list of (start, end) row ranges, or None")
        mask = np.isin(labels_of(), list(NORMAL_LABELS))
        edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
        return [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]
    out = []
    for a, b in quiet:
        a, b = int(a), int(b)
        if not 0 <= a < b <= n_rows:
            raise ValueError("quiet range (%d, %d) does not lie inside the %d rows" % (a, b, n_rows))
        out.append((a, b))
    return out


def _host_sweep(arr, mu, sigma, cfg0, structure, table, ridx, starts):
    """The referee: _host_series per candidate over the gathered rows, one restart per segment, then the searches."""
    P, S, n = table.shape[0], len(starts), len(ridx)
    bounds = list(starts) + [n]
    raw = {"first_warn": np.full((P, S), -1, dtype=np.int64), "first_danger": np.full((P, S), -1, dtype=np.int64),
           "n_warn": np.zeros((P, S), dtype=np.int64), "peak": np.full((P, S), np.nan), "carry": np.full((P, S, 2), np.nan)}
    bad = _table_bad(table)
    rows = arr[ridx] if n else np.zeros((0, arr.shape[1]))
    R = np.stack([rows[:, c].astype(float) for c in cfg0.cols], axis=1) if n else np.zeros((0, len(cfg0.cols)))
    mu, sigma = _as_numpy(mu, float), _as_numpy(sigma, float)
    for i in range(P):
        if bad[i] or n == 0:
            continue
        prm = _table_params(table, i, cfg0, structure)
        warn, danger = prm.pop("warn_threshold"), prm.pop("danger_threshold")
        with np.errstate(all="ignore"):
            RF_smooth, carry = _host_series(R, mu, sigma, _Config(**prm), list(starts))[4:6]
        raw["carry"][i] = carry
        for s in range(S):
            seg = RF_smooth[bounds[s]:bounds[s + 1]]
            hit = seg >= warn
            fw, fd = _host_first(seg, warn, "above"), _host_first(seg, danger, "above")
            raw["first_warn"][i, s] = -1 if fw is None else fw
            raw["first_danger"][i, s] = -1 if fd is None else fd
            raw["n_warn"][i, s] = int(hit.sum())
            if not np.isnan(seg).all():
                raw["peak"][i, s] = np.nanmax(seg)
    raw["bad"] = bad
    return raw


def _device_sweep(arr, mu, sigma, cfg0, table, ridx, starts):
    """One pinn_rf_sweep call -> the same dict as _host_sweep, of device tensors."""
    torch, _lib, lib = _torch_lib()
    dev = arr.device
    prm = cfg0.c_struct()
    if arr.shape[1] <= max(cfg0.cols):
        raise ValueError("results has %d columns, column %d is needed" % (arr.shape[1], max(cfg0.cols)))
    P, S, n = table.shape[0], int(starts.numel()), int(ridx.numel())
    if P * S > 2 ** 31 - 1:
        raise ValueError("%d candidates x %d segments exceed one launch (2^31 - 1 workgroups): sweep in parts" % (P, S))
    with torch.cuda.device(dev):
        mu_d, sg_d = _dev_vec(torch, mu, torch.float64, dev), _dev_vec(torch, sigma, torch.float64, dev)
        if mu_d.numel() != prm.n_cols or sg_d.numel() != prm.n_cols:
            raise ValueError("mu and sigma must have one entry per residual key (%d)" % prm.n_cols)
        cand = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
        raw = {"first_warn": torch.empty(P, S, dtype=torch.int64, device=dev), "first_danger": torch.empty(P, S, dtype=torch.int64, device=dev),
               "n_warn": torch.empty(P, S, dtype=torch.int64, device=dev), "peak": torch.empty(P, S, dtype=torch.float64, device=dev),
               "carry": torch.empty(P, S, 2, dtype=torch.float64, device=dev)}
        bad = torch.empty(P, dtype=torch.int32, device=dev)
        wb = lib.pinn_rf_sweep_workspace_bytes(n, prm.n_cols)
        ws = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
        ld = arr.stride(0) if arr.shape[0] > 0 else max(arr.shape[1], 1)
        call("pinn_rf_sweep", arr, ld, arr.shape[0], ctypes.byref(prm), mu_d, sg_d, ridx, n, starts, S, cand, P, raw["first_warn"],
             raw["first_danger"], raw["n_warn"], raw["peak"], raw["carry"], bad, ws, wb)
    raw["bad"] = bad != 0
    return raw


class RFSweep:
    """What rf_sweep returns.  Segments are the conditions that have rows (in order), then the quiet ranges; `raw` holds the
    kernel's outputs per (candidate, segment) as they came (device tensors from the device backend): "first_warn",
    "first_danger", "n_warn", "peak" [P, S], "carry" [P, S, 2], "bad" [P].  Everything else is numpy, computed from `raw` when
    first asked for:

      idx_v_alarm [n_cond]        first V <= V[0] - 0.1 of each condition, -1: none (or no rows)
      idx_rf_warn, idx_rf_danger  [P, n_cond] first RF_smooth >= the candidate's threshold, -1: none
      delta_idx, fired [P, n_cond] idx_v_alarm - idx_rf_warn where both alarms fire (`fired`), 0 elsewhere
      n_rows [n_cond], quiet_alarm_rows [P] (rows of the quiet segments with RF_smooth >= warn), quiet_peak [P], bad [P]

    `row_index` and `seg_starts` are the gather list and the segment starts the sweep ran on (rf_series takes them as they
    stand), `table` the [P, 24] candidate words, `quiet_ranges` the quiet (start, end) row ranges."""

    def __init__(self, raw, idx_v_alarm, n_rows, live, table, cfg0, structure, quiet_ranges, backend, row_index=None, seg_starts=None):
        self.raw, self.n_rows, self.table, self.backend = raw, np.asarray(n_rows, dtype=np.int64), table, backend
        self.row_index, self.seg_starts = row_index, seg_starts
        self.idx_v_alarm = np.asarray(idx_v_alarm, dtype=np.int64)
        self.quiet_ranges = list(quiet_ranges)
        self._live, self._cfg0, self._structure, self._np = list(live), cfg0, structure, None
        self.n_candidates, self.n_conditions = table.shape[0], self.n_rows.shape[0]

    def _host(self):
        if self._np is None:
            self._np = {k: _as_numpy(v) for k, v in self.raw.items()}
        return self._np

    def _per_condition(self, key, fill):
        a = self._host()[key]
        out = np.full((self.n_candidates, self.n_conditions), fill, dtype=a.dtype)
        out[:, self._live] = a[:, :len(self._live)]
        return out

    @property
    def idx_rf_warn(self):
        return self._per_condition("first_warn", -1)

    @property
    def idx_rf_danger(self):
        return self._per_condition("first_danger", -1)

    @property
    def peak(self):
        """[P, n_cond] maximum of RF_smooth over each condition, NaN where there is none."""
        return self._per_condition("peak", np.nan)

    @property
    def fired(self):
        return (self.idx_v_alarm[None, :] >= 0) & (self.idx_rf_warn >= 0)

    @property
    def delta_idx(self):
        return np.where(self.fired, self.idx_v_alarm[None, :] - self.idx_rf_warn, 0)

    @property
    def quiet_alarm_rows(self):
        return self._host()["n_warn"][:, len(self._live):].sum(axis=1)

    @property
    def quiet_peak(self):
        q = self._host()["peak"][:, len(self._live):]
        out = np.full(self.n_candidates, np.nan)
        if q.shape[1]:
            some = ~np.isnan(q).all(axis=1)
            out[some] = np.nanmax(q[some], axis=1)
        return out

    @property
    def bad(self):
        return self._host()["bad"].astype(bool)

    def candidate(self, i):
        """Keyword arguments of candidate i, for RiskMonitor(mu, sigma, **kw) and rf_advance_for_conditions(..., **kw)."""
        return _table_params(self.table, int(i), self._cfg0, self._structure)


def rf_sweep(results, mu, sigma, candidates, conditions=None, quiet="normal", current_tol=CURRENT_TOL, backend="auto", **fixed):
    """Evaluate P parameter sets over every condition's sub-series and over the quiet rows, where a warning is a false alarm.

    `candidates`: a dict of per-candidate arrays of length P, as rf_grid returns; names it lacks come from `fixed`, or
    else from the module's defaults.  `fixed` also takes the structure (res_keys, layer_config, columns), the same for all
    candidates.  Segments: the conditions' sub-series, selected as rf_advance_for_conditions selects them, then the quiet
    ranges: quiet="normal" -> every maximal run of consecutive rows labelled NORMAL_LABELS, or a list of (start, end), or
    None.  The device backend stages the z-scores once and runs all candidates in ONE pinn_rf_sweep call (one workgroup per
    candidate and segment; nothing per row is written); the voltage alarms are one pinn_rf_first_alarm call.  The host
    backend loops the float64 numpy series per candidate: the referee, and the path of machines without a GPU.
    Returns an RFSweep."""
    conditions = RF_CONDITIONS if conditions is None else list(conditions)
    cfg0, structure, P, table = _candidate_table(dict(candidates), fixed)
    host, arr, out, used = _condition_rows(results, conditions, current_tol, backend)
    live = [i for i, u in enumerate(used) if u.shape[0] > 0]
    n_rows = [o["n"] for o in out]
    if host:
        ranges = _quiet_ranges(quiet, lambda: arr[:, INDEX["label"]].astype(int), arr.shape[0])
        lists = [used[i] for i in live] + [np.arange(a, b, dtype=np.int64) for a, b in ranges]
        if not lists:
            raise ValueError("nothing to sweep over: no condition has rows and there are no quiet rows")
        ridx = np.concatenate(lists).astype(np.int64)
        starts = np.concatenate([[0], np.cumsum([len(l) for l in lists])[:-1]]).astype(np.int64)
        raw = _host_sweep(arr, mu, sigma, cfg0, structure, table, ridx, starts)
        v_first = np.full(len(conditions), -1, dtype=np.int64)
        for i in live:
            V = arr[used[i], INDEX["y_true"]].astype(float)
            f = _host_first(V, float(V[0]) - V_ALARM_DROP, "below")
            v_first[i] = -1 if f is None else f
    else:
        import torch
        ranges = _quiet_ranges(quiet, lambda: arr[:, INDEX["label"]].long().cpu().numpy(), arr.shape[0])
        lists = [used[i] for i in live] + [torch.arange(a, b, dtype=torch.int64, device=arr.device) for a, b in ranges]
        if not lists:
            raise ValueError("nothing to sweep over: no condition has rows and there are no quiet rows")
        ridx = torch.cat(lists)
        starts_h = np.concatenate([[0], np.cumsum([int(l.shape[0]) for l in lists])[:-1]]).astype(np.int64)
        starts = torch.from_numpy(starts_h).to(arr.device)
        raw = _device_sweep(arr, mu, sigma, cfg0, table, ridx, starts)
        v_first = np.full(len(conditions), -1, dtype=np.int64)
        if live:
            n_live = sum(int(used[i].shape[0]) for i in live)
            v_first[live] = _device_voltage_alarm(arr, ridx[:n_live], starts[:len(live)])[0].cpu().numpy()
    return RFSweep(raw, v_first, n_rows, live, table, cfg0, structure, ranges, "host" if host else "device", ridx, starts)


def _calibration_choice(idx_v_alarm, idx_rf_warn, quiet_alarm_rows, bad, max_quiet_alarm_rows=0, require_all=True):
    """The calibration rule, on integers alone.  idx_v_alarm [n_cond] and idx_rf_warn [P, n_cond] (-1: none),
    quiet_alarm_rows [P], bad [P].  Over the conditions whose voltage alarm fires: a candidate is feasible if it is not bad,
    has at most max_quiet_alarm_rows alarm rows on the quiet segments and (require_all) warns on every such condition
    (otherwise on at least one).  Among the feasible: the largest minimum lead idx_v_alarm - idx_rf_warn over the
    conditions on which both fire, then the largest sum of leads, then the lowest index.  Returns that index; raises
    ValueError, naming how many candidates failed which rule, when none is feasible."""
    iv = np.asarray(idx_v_alarm, dtype=np.int64).reshape(-1)
    ir = np.asarray(idx_rf_warn, dtype=np.int64)
    quiet_rows = np.asarray(quiet_alarm_rows, dtype=np.int64).reshape(-1)
    bad = np.asarray(bad, dtype=bool).reshape(-1)
    P = ir.shape[0]
    target = iv >= 0
    if not target.any():
        raise ValueError("no condition's voltage alarm fires: there is no lead to calibrate against")
    warned = ir[:, target] >= 0
    lead = iv[target][None, :] - ir[:, target]
    noisy = quiet_rows > int(max_quiet_alarm_rows)
    silent = ~warned.all(axis=1) if require_all else ~warned.any(axis=1)
    feasible = ~bad & ~noisy & ~silent
    if not feasible.any():
        raise ValueError("no feasible candidate among %d: %d bad, %d with more than %d alarm rows on the quiet segments, "
                         "%d silent on %s condition whose voltage alarm fires"
                         % (P, int(bad.sum()), int(noisy.sum()), int(max_quiet_alarm_rows), int(silent.sum()),
                            "a" if require_all else "every"))
    big = np.iinfo(np.int64).max
    worst = np.where(warned, lead, big).min(axis=1)
    total = np.where(warned, lead, 0).sum(axis=1)
    best = None
    for i in np.flatnonzero(feasible):
        key = (int(worst[i]), int(total[i]))
        if best is None or key > best[0]:
            best = (key, int(i))
    return best[1]


class RFCalibration:
    """What calibrate_rf returns: `index` of the chosen candidate, its keyword arguments `params` (they feed
    RiskMonitor(mu, sigma, **params) and rf_advance_for_conditions(..., **params)), `table` (the per-condition dicts of
    rf_advance_for_conditions at these parameters) and the whole `sweep`."""

    def __init__(self, index, params, table, sweep):
        self.index, self.params, self.table, self.sweep = index, params, table, sweep


def calibrate_rf(results, mu, sigma, candidates, conditions=None, quiet="normal", current_tol=CURRENT_TOL, backend="auto",
                 max_quiet_alarm_rows=0, require_all=True, **fixed):
    """Choose among `candidates` (see rf_sweep) the parameter set whose RF warning leads the voltage alarm by the most
    samples in the worst condition while staying silent on the quiet rows: _calibration_choice's rule on rf_sweep's output."""
    sweep = rf_sweep(results, mu, sigma, candidates, conditions=conditions, quiet=quiet, current_tol=current_tol, backend=backend, **fixed)
    index = _calibration_choice(sweep.idx_v_alarm, sweep.idx_rf_warn, sweep.quiet_alarm_rows, sweep.bad, max_quiet_alarm_rows, require_all)
    params = sweep.candidate(index)
    table = rf_advance_for_conditions(results, mu, sigma, conditions, current_tol=current_tol, backend=backend, **params)
    return RFCalibration(index, params, table, sweep)
