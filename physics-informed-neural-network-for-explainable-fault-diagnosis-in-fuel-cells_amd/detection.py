"""Fault detection: is this row a fault at all, and how well does the model tell?  (reference script 02, and the logistic
baseline of script 05.)

A StandardScaler + multinomial logistic regression is fitted on feature columns of the results array (script 02's groups:
`epi,res` / `x0,x3,x4,x5` / `res` / `y_true`), and the ROC curve and AUC of `1 - P(normal)` say how well the group separates
normal from faulty rows.  Script 02's names, defaults and error types are kept: `parse_features`, `parse_group_spec`,
`build_label_mapper`, `extract_X_y`, `build_classifier`, `explain_coefficients`; from script 05 `run_supervised_lr` and
`compute_macro_metrics`.  Added: `DeviceStandardScaler`, `DeviceLogisticRegression`, `roc_curve`, `auc`, `auc_score`,
`stratified_split`, `evaluate_feature_groups` (script 02's main loop without figures; its unsupervised curve comes from
anomaly.py) and `FaultDetector` (online use).

The model.  With z = (x - mean_) / scale_, sample weights sw_i = n / (C count[y_i]) ("balanced"; 1 otherwise) the fit minimises
    F(W, b) = sum_i sw_i (logsumexp_c s_ic - s_i,y_i) + 1 / (2 C_reg) sum_c |W_c|^2,   s_ic = W_c . z_i + b_c
over a full [C, D] matrix and [C] intercepts, as scikit-learn's lbfgs solver does, and stops when
max |grad F| / sum sw <= tol (scikit-learn's meaning of tol).  The solver here is a damped Newton iteration, so `n_iter_`
counts Newton iterations and is not comparable with scikit-learn's.  For two classes `coef_` is [1, D] (= W[1] = -W[0]) and
predict_proba = softmax([-d, d]), as scikit-learn reports a two-class multinomial fit.

Two backends, as in risk.py and diagnosis.py.  "device": the HIP kernels of csrc/pinn_lr.hip.  "host": float64 numpy.
Importing this module needs numpy only; scikit-learn is never imported.
"""
import functools
import re
import warnings

import numpy as np

from . import diagnosis as _dg
from ._classify import dev_classes, host_classes, labels_of, scaler_stats, wanted_outputs
from ._device import _DevRows, _as_numpy, _dev_vec, _host_rows, _is_tensor, _on_gpu, _pick_backend, _torch_lib, call, columns_of
from .diagnosis import (build_label_mapper, classification_metrics, extract_X_y, list_available_features,  # noqa: F401
                        normalize_feature_spec)
from .risk import FAULT_ALIASES, INDEX

FEAT_GRP1 = "epi,res"
FEAT_GRP2 = "x0,x3,x4,x5"
FEAT_GRP3 = "res"
FEAT_GRP4 = "y_true"
FEATURE_GROUPS = (FEAT_GRP1, FEAT_GRP2, FEAT_GRP3, FEAT_GRP4)
DEFAULT_GROUP_SPEC = "normal:0 | fault:1,2,3,4,5,6,7,8,9,10,11,12"
FIVE_CLASS_GROUP_SPEC = "normal:0 | flooding:1,2,3 | oxygen_starvation:4,5,6 | membrane_drying:7,8,9 | hydrogen_starvation:10,11,12"
DEFAULT_TEST_SIZE = 0.9
DEFAULT_RANDOM_STATE = 49
DEFAULT_BALANCED = True
DEFAULT_SHOW_COEF = 5
CLASS_ALIASES = dict(FAULT_ALIASES, **{"正常": "normal", "故障": "fault"})
MAX_CLASSES, MAX_FEAT, MAX_HESS = 13, 8, 1365          # include/pinn_hip.h: PINN_LR_MAX_*
EPS = np.finfo(np.float64).eps
_HDR = 16
_STATUS_TEXT = {1: "the Hessian is not positive definite", 2: "the loss or its gradient is not finite"}


# ---------------------------------------------------------------------------------------------- script 02's helpers
def parse_features(spec):
    """Column indices of a feature spec (names of INDEX or numbers), first occurrence kept.  KeyError for an unknown name,
    ValueError when the label column is asked for; script 02's variant warns when `y_true` is a feature (02:148-149)."""
    out = []
    for tok in normalize_feature_spec(spec).split(","):
        if tok == "":
            continue
        if re.match(r"^-?\d+$", tok):                       # script 02 takes a signed number as it stands (02:132)
            idx = int(tok)
        elif tok in INDEX:
            idx = INDEX[tok]
        else:
            raise KeyError("unknown feature name %r; available: %s" % (tok, list_available_features()))
        if idx == INDEX["label"]:
            raise ValueError("'label' is not allowed as an input feature")
        if idx not in out:
            out.append(idx)
    if INDEX["y_true"] in out:
        warnings.warn("the features include y_true (the measured output): target leakage; use it for comparison only")
    return out


def parse_group_spec(spec, translate=True):
    """As diagnosis.parse_group_spec; with translate=True the reference's Chinese class names (also 正常 / 故障 = normal /
    fault) become the English ones."""
    groups = _dg.parse_group_spec(spec, translate=False)
    if not translate:
        return groups
    out = {}
    for name, ids in groups.items():
        name = CLASS_ALIASES.get(name, name)
        if name in out:
            raise ValueError("group name %r is repeated" % name)
        out[name] = ids
    return out


def limits_ok(n_classes, n_features):
    """True when the device kernels are built for this shape (the limits of include/pinn_hip.h)."""
    C, D = int(n_classes), int(n_features)
    return 2 <= C <= MAX_CLASSES and 1 <= D <= MAX_FEAT and (C * (C + 1) // 2) * ((D + 1) * (D + 2) // 2) <= MAX_HESS


# ---------------------------------------------------------------------------------------------- host backend
def _host_scaler_stats(X):
    """mean_, var_, scale_ as StandardScaler.fit: population variance in two passes, scale 1 for a constant feature
    (scikit-learn's _is_constant_feature and _handle_zeros_in_scale)."""
    n = X.shape[0]
    mean = X.sum(axis=0) / n
    var = ((X - mean) ** 2).sum(axis=0) / n
    scale = np.sqrt(var)
    const = var <= n * EPS * var + (n * mean * EPS) ** 2
    scale[const | (scale < 10 * EPS)] = 1.0
    return mean, var, scale


def _softmax(s):
    m = s.max(axis=1, keepdims=True)
    e = np.exp(s - m)
    sm = e.sum(axis=1, keepdims=True)
    return e / sm, (np.log(sm) + m)[:, 0]


def _host_sums(X, yi, C, mean, scale, theta, cw, want_abs=False):
    """The sums of one row pass in the device's layout [1 + P + H]: loss; gradient [C][D + 1]; Hessian blocks c <= d (pairs
    by columns d), i <= j (by columns j).  With want_abs also the sums of the absolute terms."""
    n, D = X.shape
    ok = (yi >= 0) & (yi < C)
    X, yi = X[ok], yi[ok]
    U = np.concatenate([(X - mean) / scale, np.ones((X.shape[0], 1))], axis=1)
    s = U @ theta.T
    p, lse = _softmax(s)
    sw = cw[yi]
    Y = np.zeros_like(p)
    Y[np.arange(len(yi)), yi] = 1.0
    lterm = sw * (lse - s[np.arange(len(yi)), yi])
    ii, jj = zip(*[(i, j) for j in range(D + 1) for i in range(j + 1)])
    ii, jj = np.array(ii), np.array(jj)
    R = (sw[:, None] * (p - Y))
    S = [np.array([lterm.sum()]), (R.T @ U).reshape(-1)]
    A = [np.array([np.abs(lterm).sum()]), (np.abs(R).T @ np.abs(U)).reshape(-1)] if want_abs else None
    aU = np.abs(U)
    for d in range(C):
        for c in range(d + 1):
            w = sw * p[:, c] * ((1.0 if c == d else 0.0) - p[:, d])
            S.append(((U * w[:, None]).T @ U)[ii, jj])
            if want_abs:
                A.append(((aU * np.abs(w)[:, None]).T @ aU)[ii, jj])
    S = np.concatenate(S)
    return (S, np.concatenate(A)) if want_abs else S


def _objective(S, theta, C, D, l2, fit_intercept):
    """F, gradient [C, D + 1] and the full Hessian [P, P] (penalty and the intercept pin included) from the pass sums."""
    D1, P = D + 1, C * (D + 1)
    nT = D1 * (D1 + 1) // 2
    F = S[0] + 0.5 * l2 * (theta[:, :D] ** 2).sum()
    g = S[1:1 + P].reshape(C, D1).copy()
    g[:, :D] += l2 * theta[:, :D]
    if not fit_intercept:
        g[:, D] = 0.0
    return F, g, nT


def _host_hessian(S, C, D, l2, sw_sum, fit_intercept):
    D1, P = D + 1, C * (D + 1)
    nT = D1 * (D1 + 1) // 2
    H = np.zeros((P, P))
    tri = np.zeros((D1, D1), dtype=np.int64)
    for j in range(D1):
        for i in range(j + 1):
            tri[i, j] = tri[j, i] = j * (j + 1) // 2 + i
    for d in range(C):
        for c in range(d + 1):
            blk = S[1 + P + (d * (d + 1) // 2 + c) * nT:][:nT][tri]
            H[c * D1:(c + 1) * D1, d * D1:(d + 1) * D1] = blk
            H[d * D1:(d + 1) * D1, c * D1:(c + 1) * D1] = blk
    coef = np.array([i % D1 < D for i in range(P)])
    H[np.flatnonzero(coef), np.flatnonzero(coef)] += l2
    icpt = np.flatnonzero(~coef)
    H[np.ix_(icpt, icpt)] += sw_sum / C                  # the rank-one term that pins the sum of the intercepts
    if not fit_intercept:
        H[icpt, :] = 0.0
        H[:, icpt] = 0.0
        H[icpt, icpt] = 1.0
    return H


def _host_newton(X, yi, C, mean, scale, cw, theta, l2, tol, max_iter, fit_intercept, trace=None):
    """The device's state machine in numpy.  Returns theta, n_iter, converged, passes, gmax, F."""
    n, D = X.shape
    sw_sum = float(cw[yi[(yi >= 0) & (yi < C)]].sum())
    prev, direction, step, dd, Fp = theta.copy(), None, 1.0, 0.0, np.inf
    n_iter, passes, gmax = 0, 0, np.inf
    first = True
    while n_iter < max_iter:
        S = _host_sums(X, yi, C, mean, scale, theta, cw)
        F, g, _ = _objective(S, theta, C, D, l2, fit_intercept)
        bad = not (np.isfinite(F) and np.isfinite(g).all())
        passes += 1
        if first:
            if bad:
                raise ValueError("logistic regression failed: %s" % _STATUS_TEXT[2])
        elif bad or not F <= Fp + 1e-4 * step * dd + 4.0 * n * EPS * abs(S[0]):
            step *= 0.5
            if step < 2.0 ** -40:
                warnings.warn("the Newton direction gives no decrease: stopped at the last accepted point")
                return prev, n_iter, False, passes, gmax, Fp
            theta = prev + step * direction
            continue
        if not first:
            n_iter += 1
        first = False
        prev, Fp = theta.copy(), F
        gmax = np.abs(g).max() / sw_sum
        if trace is not None:
            trace.append(F)
        if gmax <= tol:
            return prev, n_iter, True, passes, gmax, Fp
        H = _host_hessian(S, C, D, l2, sw_sum, fit_intercept)
        for ridge in (0.0, 1e-6, 1e-4, 1e-2):            # far from the minimum the factorisation can fail in rounding
            try:
                L = np.linalg.cholesky(H + ridge * sw_sum * np.eye(H.shape[0]))
                break
            except np.linalg.LinAlgError:
                L = None
        if L is None or not np.isfinite(L).all():
            raise ValueError("logistic regression failed: %s" % _STATUS_TEXT[1])
        direction = -np.linalg.solve(L.T, np.linalg.solve(L, g.reshape(-1))).reshape(C, D + 1)
        dd = float((g * direction).sum())
        if not dd < 0.0:
            return prev, n_iter, dd == 0.0, passes, gmax, Fp
        step = 1.0
        theta = prev + direction
    return prev, n_iter, False, passes, gmax, Fp


def _scores(X, mean, scale, coef, intercept):
    """decision scores [n, C] of sklearn-shaped parameters (coef [1, D] for two classes: (-d, d))."""
    s = ((X - mean) / scale) @ coef.T + intercept
    return np.concatenate([-s, s], axis=1) if coef.shape[0] == 1 else s


# ---------------------------------------------------------------------------------------------- scaler
class DeviceStandardScaler:
    """StandardScaler (with_mean and with_std): `mean_`, `var_`, `scale_` (population standard deviation, 1 for a constant
    feature), `n_samples_seen_`.  `fit` and `transform` take X [n, D], or any array plus `columns` (and `row_index`)."""

    def __init__(self, backend="auto"):
        if backend not in ("auto", "device", "host"):
            raise ValueError("backend must be 'auto', 'device' or 'host'")
        self.backend = backend

    def _set(self, mean, var, scale, n, as_tensor=False):
        self.mean_, self.var_, self.scale_, self.n_samples_seen_ = mean, var, scale, int(n)

    def fit(self, X, y=None, columns=None, row_index=None):
        if _pick_backend(self.backend, X) == "host":
            Xh = _host_rows(X, columns, row_index)
            if Xh.shape[0] < 1:
                raise ValueError("X holds no rows")
            self._set(*_host_scaler_stats(Xh), Xh.shape[0])
            return self
        torch, _lib, lib = _torch_lib()
        rows = _DevRows(torch, X, columns, row_index)
        if rows.n < 1:
            raise ValueError("X holds no rows")
        with torch.cuda.device(rows.dev):
            st = torch.zeros(_state_words(2, rows.D), dtype=torch.float64, device=rows.dev)
            yz = torch.zeros(rows.n, dtype=torch.int64, device=rows.dev)
            wb = lib.pinn_lr_workspace_bytes(rows.n, 2, rows.D)
            ws = torch.empty(wb, dtype=torch.uint8, device=rows.dev)
            call("pinn_lr_scaler", *rows.head(), yz, 2, 0, st, ws, wb)
            o = _offsets(2, rows.D)
            stats = [st[o[k]:o[k] + rows.D].clone() for k in ("mean", "var", "scale")]
        if not _is_tensor(X):
            stats = [s.cpu().numpy() for s in stats]
        self._set(*stats, rows.n)
        return self

    def transform(self, X, columns=None, row_index=None):
        if not hasattr(self, "mean_"):
            raise RuntimeError("this DeviceStandardScaler is not fitted yet")
        if _pick_backend(self.backend, X) == "host":
            return (_host_rows(X, columns, row_index) - _as_numpy(self.mean_)) / _as_numpy(self.scale_)
        torch, _lib, lib = _torch_lib()
        rows = _DevRows(torch, X, columns, row_index)
        out = (rows.packed(torch) - _dev_vec(torch, self.mean_, torch.float64, rows.dev)) / _dev_vec(torch, self.scale_, torch.float64, rows.dev)
        return out if _is_tensor(X) else out.cpu().numpy()

    def fit_transform(self, X, y=None, columns=None, row_index=None):
        return self.fit(X, columns=columns, row_index=row_index).transform(X, columns, row_index)


# ---------------------------------------------------------------------------------------------- device state
def _offsets(C, D):
    P = C * (D + 1)
    o = {"theta": _HDR, "prev": _HDR + P, "dir": _HDR + 2 * P, "grad": _HDR + 3 * P, "mean": _HDR + 4 * P}
    o["scale"], o["var"], o["cw"] = o["mean"] + D, o["mean"] + 2 * D, o["mean"] + 3 * D
    o["count"] = o["cw"] + C
    o["end"] = o["count"] + C
    return o


def _state_words(C, D):
    return _offsets(C, D)["end"]


def n_pass_sums(C, D):
    return 1 + C * (D + 1) + (C * (C + 1) // 2) * ((D + 1) * (D + 2) // 2)


_rows = functools.partial(_DevRows.within, on_excess=lambda D: _check_limits(2, D))


def _too_few(classes):
    return "this solver needs samples of at least 2 classes in the data, but the data contains only one class: %r" % (classes[0],)


def _check_limits(C, D):
    if not limits_ok(C, D):
        raise NotImplementedError("the device backend is built for 2..%d classes, 1..%d features and at most %d Hessian sums "
                                  "(every C <= 5, D <= 8 and C <= 13, D <= 4); got C = %d, D = %d" % (MAX_CLASSES, MAX_FEAT, MAX_HESS, C, D))


class DeviceLogisticRegression:
    """Multinomial logistic regression with an L2 penalty: scikit-learn's LogisticRegression(solver="lbfgs") arguments,
    objective, stopping rule and attribute shapes (`coef_` [1, D] for two classes, `intercept_`, `classes_`, `n_iter_`,
    `converged_`), solved by damped Newton iterations.  `coef_init` [C, D] and `intercept_init` [C] give a starting point
    (zeros by default, as scikit-learn's).  Also set by fit: `n_passes_` (row passes), `grad_max_` (max |grad F| / sum sw at
    the solution), `loss_` (F there), `class_weight_` [C], `class_count_` [C].

    `fit`, `predict`, `predict_proba`, `decision_function` take X [n, D], or any array plus `columns` (and `row_index`):
    the device backend then reads the rows in place.  `scaler=` (a fitted DeviceStandardScaler) standardises inside the
    row pass.  numpy in -> numpy out, device tensor in -> device tensors out."""

    def __init__(self, penalty="l2", *, C=1.0, tol=1e-4, max_iter=1000, class_weight=None, fit_intercept=True, solver="lbfgs",
                 multi_class="multinomial", random_state=None, coef_init=None, intercept_init=None, backend="auto", chunk=4):
        if penalty != "l2":
            raise NotImplementedError("penalty=%r: only 'l2' is implemented" % (penalty,))
        if solver not in ("lbfgs", "newton"):
            raise NotImplementedError("solver=%r: the objective of 'lbfgs' is minimised by Newton iterations; nothing else is implemented" % (solver,))
        if multi_class not in ("multinomial", "auto"):
            raise NotImplementedError("multi_class=%r: only the multinomial model is implemented" % (multi_class,))
        if class_weight not in (None, "balanced"):
            raise NotImplementedError("class_weight must be None or 'balanced'")
        if backend not in ("auto", "device", "host"):
            raise ValueError("backend must be 'auto', 'device' or 'host'")
        if not C > 0 or tol < 0 or int(max_iter) < 0 or int(chunk) < 1:
            raise ValueError("C > 0, tol >= 0, max_iter >= 0 and chunk >= 1 are required")
        self.penalty, self.C, self.tol, self.max_iter, self.class_weight = penalty, float(C), float(tol), int(max_iter), class_weight
        self.fit_intercept, self.solver, self.multi_class, self.random_state = bool(fit_intercept), solver, multi_class, random_state
        self.coef_init, self.intercept_init, self.backend, self.chunk = coef_init, intercept_init, backend, int(chunk)
        self._model = None               # device model block of the posterior kernel, by device

    # ---- shared
    def _check_fitted(self):
        if not hasattr(self, "coef_"):
            raise RuntimeError("this DeviceLogisticRegression is not fitted yet")

    def _theta0(self, C, D):
        th = np.zeros((C, D + 1))
        if self.coef_init is not None:
            ci = np.asarray(_as_numpy(self.coef_init), dtype=np.float64)
            th[:, :D] = np.concatenate([-ci, ci]) if (C == 2 and ci.shape == (1, D)) else ci.reshape(C, D)
        if self.intercept_init is not None:
            bi = np.asarray(_as_numpy(self.intercept_init), dtype=np.float64).reshape(-1)
            th[:, D] = np.concatenate([-bi, bi]) if (C == 2 and bi.size == 1) else bi.reshape(C)
        return th

    def _publish(self, theta, classes, n_iter, converged, passes, gmax, F, cw, count, as_tensor, dev=None):
        C, D1 = theta.shape
        if not converged and self.max_iter > 0:
            warnings.warn("the Newton iteration did not reach tol = %g in max_iter = %d iterations (max |grad| / sum sw = %.3e)"
                          % (self.tol, self.max_iter, gmax))
        coef, icpt = (theta[1:, :-1], theta[1:, -1]) if C == 2 else (theta[:, :-1], theta[:, -1])
        out = [np.ascontiguousarray(coef), np.ascontiguousarray(icpt), np.asarray(cw, dtype=np.float64), np.asarray(count, dtype=np.int64)]
        if as_tensor:
            import torch
            out = [torch.from_numpy(a).to(dev) for a in out]
        self.coef_, self.intercept_, self.class_weight_, self.class_count_ = out
        self.classes_ = classes
        self.n_iter_, self.converged_, self.n_passes_, self.grad_max_, self.loss_ = int(n_iter), bool(converged), int(passes), float(gmax), float(F)
        self.n_features_in_ = D1 - 1
        self._model = None

    # ---- fit
    def fit(self, X, y, sample_weight=None, columns=None, row_index=None, scaler=None, fit_scaler=None, trace=None):
        """`scaler`: a fitted DeviceStandardScaler whose statistics standardise the rows; `fit_scaler`: an unfitted one that
        is fitted on the same rows first (on the device inside the same launch sequence).  `trace`: a list that receives F
        at every accepted point (host backend)."""
        if sample_weight is not None:
            raise NotImplementedError("sample_weight is not implemented (class_weight='balanced' is)")
        balanced = self.class_weight == "balanced"
        l2 = 1.0 / self.C
        if _pick_backend(self.backend, X) == "host":
            Xh = _host_rows(X, columns, row_index)
            classes, yi, count = host_classes(y, Xh.shape[0], _too_few)
            C, D = len(classes), Xh.shape[1]
            if fit_scaler is not None:
                scaler = fit_scaler.fit(Xh)
            mean, scale = scaler_stats(scaler, D)
            cw = len(yi) / (C * count) if balanced else np.ones(C)
            theta, n_iter, conv, passes, gmax, F = _host_newton(Xh, yi, C, mean, scale, cw, self._theta0(C, D), l2, self.tol, self.max_iter,
                                                                 self.fit_intercept, trace)
            self._publish(theta, classes, n_iter, conv, passes, gmax, F, cw, count, False)
            return self
        return self._fit_device(X, y, columns, row_index, scaler, fit_scaler, balanced, l2, trace)

    def _fit_device(self, X, y, columns, row_index, scaler, fit_scaler, balanced, l2, trace):
        torch, _lib, lib = _torch_lib()
        rows = _rows(torch, X, columns, row_index)
        if rows.n < 1:
            raise ValueError("X holds no rows")
        with torch.cuda.device(rows.dev):
            classes, yi, _ = dev_classes(torch, y, rows, _too_few)
            C, D = int(classes.numel()), rows.D
            _check_limits(C, D)
            stream = torch.cuda.current_stream().cuda_stream
            o = _offsets(C, D)
            s0 = np.zeros(o["end"])
            s0[:_HDR].view(np.int64)[_dev_hdr("MAXITER")] = self.max_iter
            th0 = self._theta0(C, D).reshape(-1)
            s0[o["theta"]:o["theta"] + th0.size] = th0
            s0[o["prev"]:o["prev"] + th0.size] = th0
            st = torch.from_numpy(s0).to(rows.dev)
            wb = lib.pinn_lr_workspace_bytes(rows.n, C, D)
            ws = torch.empty(wb, dtype=torch.uint8, device=rows.dev)
            head = rows.head() + (yi, C)
            call("pinn_lr_scaler", *head, int(balanced), st, ws, wb, stream=stream)
            if fit_scaler is not None:
                stats = [st[o[k]:o[k] + D].clone() for k in ("mean", "var", "scale")]
                fit_scaler._set(*(stats if _is_tensor(X) else [s.cpu().numpy() for s in stats]), rows.n)
            else:                                        # a given scaler, or none: its statistics replace the pass's
                mean, scale = scaler_stats(scaler, D)
                st[o["mean"]:o["mean"] + D] = torch.from_numpy(mean).to(rows.dev)
                st[o["scale"]:o["scale"] + D] = torch.from_numpy(scale).to(rows.dev)
            self._state, self._ws = st, ws
            # every pass is a pair of launches; the block is read once per chunk of `chunk` passes
            while True:
                call("pinn_lr_newton", *head, self.chunk, self.tol, l2, int(self.fit_intercept), st, ws, wb, stream=stream)
                s = st.cpu().numpy()
                hdr = s[:_HDR].view(np.int64)
                if trace is not None:
                    trace.append(float(s[_dev_hdr("F")]))
                status = int(hdr[_dev_hdr("STATUS")])
                if status in _STATUS_TEXT:
                    raise ValueError("logistic regression failed: %s (status %d)" % (_STATUS_TEXT[status], status))
                if status != 0:
                    warnings.warn("the Newton direction gives no decrease: stopped at the last accepted point")
                if hdr[_dev_hdr("CONVERGED")] or status != 0 or hdr[_dev_hdr("ITER")] >= self.max_iter:
                    break
            P = C * (D + 1)
            theta = s[o["prev"]:o["prev"] + P].reshape(C, D + 1)
            cls = classes if _is_tensor(X) else classes.cpu().numpy()
            self._publish(theta, cls, hdr[_dev_hdr("ITER")], hdr[_dev_hdr("CONVERGED")], hdr[_dev_hdr("PASSES")], s[_dev_hdr("GMAX")],
                          s[_dev_hdr("F")], s[o["cw"]:o["cw"] + C], s[o["count"]:o["count"] + C].view(np.int64), _is_tensor(X), rows.dev)
        return self

    def pass_sums(self, X, y, theta, columns=None, row_index=None, scaler=None, want_abs=False):
        """The sums of one row pass at theta [C, D + 1] (n_pass_sums(C, D) numbers: loss, gradient, Hessian blocks; no
        penalty), y holding class indices 0..C-1.  For tests and tools.  The host backend can also return the sums of the
        absolute terms."""
        theta = np.asarray(_as_numpy(theta), dtype=np.float64)
        C, D = theta.shape[0], theta.shape[1] - 1
        balanced = self.class_weight == "balanced"
        if _pick_backend(self.backend, X) == "host":
            Xh = _host_rows(X, columns, row_index)
            yi = _as_numpy(y).astype(np.int64).reshape(-1)
            mean, scale = scaler_stats(scaler, D)
            count = np.bincount(yi[(yi >= 0) & (yi < C)], minlength=C)
            with np.errstate(divide="ignore"):
                cw = np.where(count > 0, count.sum() / (C * np.maximum(count, 1)), 0.0) if balanced else np.ones(C)
            return _host_sums(Xh, yi, C, mean, scale, theta, cw, want_abs)
        torch, _lib, lib = _torch_lib()
        rows = _DevRows(torch, X, columns, row_index)
        _check_limits(C, D)
        if rows.D != D:
            raise ValueError("theta is for %d features, the rows have %d" % (D, rows.D))
        with torch.cuda.device(rows.dev):
            yi = _dev_vec(torch, y, torch.int64, rows.dev)
            stream = torch.cuda.current_stream().cuda_stream
            o = _offsets(C, D)
            s0 = np.zeros(o["end"])
            s0[o["theta"]:o["theta"] + theta.size] = theta.reshape(-1)
            st = torch.from_numpy(s0).to(rows.dev)
            wb = lib.pinn_lr_workspace_bytes(rows.n, C, D)
            ws = torch.empty(wb, dtype=torch.uint8, device=rows.dev)
            head = rows.head() + (yi, C)
            call("pinn_lr_scaler", *head, int(balanced), st, ws, wb, stream=stream)
            mean, scale = scaler_stats(scaler, D)
            st[o["mean"]:o["mean"] + D] = torch.from_numpy(mean).to(rows.dev)
            st[o["scale"]:o["scale"] + D] = torch.from_numpy(scale).to(rows.dev)
            call("pinn_lr_pass", *head, st, ws, wb, stream=stream)
            out = ws[:n_pass_sums(C, D) * 8].view(torch.float64).clone()
        return out if _is_tensor(X) else out.cpu().numpy()

    # ---- posterior
    def _device_model(self, torch, dev, scaler):
        key = (str(dev), id(scaler))
        if self._model is None or self._model[0] != key:
            D = self.n_features_in_
            mean, scale = scaler_stats(scaler, D)
            m = np.concatenate([mean, scale, _as_numpy(self.coef_, np.float64).reshape(-1), _as_numpy(self.intercept_, np.float64).reshape(-1)])
            self._model = (key, torch.from_numpy(m).to(dev))
        return self._model[1]

    def _posterior(self, X, columns=None, row_index=None, scaler=None, normal_class=0, want=("proba",)):
        """dict with the wanted of "decision", "proba", "pred" (class indices) and "p_fault"."""
        self._check_fitted()
        C, D = len(self.classes_), self.n_features_in_
        if not 0 <= int(normal_class) < C:
            raise ValueError("normal_class must be one of the %d classes" % C)
        if _pick_backend(self.backend, X) == "host":
            Xh = _host_rows(X, columns, row_index)
            if Xh.shape[1] != D:
                raise ValueError("the model was fitted on %d features, got %d" % (D, Xh.shape[1]))
            mean, scale = scaler_stats(scaler, D)
            s = _scores(Xh, mean, scale, _as_numpy(self.coef_, np.float64), _as_numpy(self.intercept_, np.float64))
            p = _softmax(s)[0]
            out = {"decision": s[:, 1] if C == 2 else s, "proba": p, "pred": s.argmax(axis=1), "p_fault": 1.0 - p[:, int(normal_class)]}
            return {k: out[k] for k in want}
        torch, _lib, lib = _torch_lib()
        rows = _DevRows(torch, X, columns, row_index)
        _check_limits(C, D)
        if rows.D != D:
            raise ValueError("the model was fitted on %d features, got %d" % (D, rows.D))
        with torch.cuda.device(rows.dev):
            model, n, f64 = self._device_model(torch, rows.dev, scaler), rows.n, torch.float64
            spec = {"decision": ((n,) if C == 2 else (n, C), f64), "proba": ((n, C), f64), "pred": ((n,), torch.int64), "p_fault": ((n,), f64)}
            return wanted_outputs(torch, X, rows.dev, spec, want, self._launch_posterior, rows, C, model, int(normal_class))

    @staticmethod
    def _launch_posterior(rows, C, model, normal_class, out):
        call("pinn_lr_posterior", *rows.head(), C, model, normal_class, out["decision"], out["proba"], out["pred"], out["p_fault"])

    def _labels(self, pred):
        return labels_of(self.classes_, pred)

    def decision_function(self, X, columns=None, row_index=None, scaler=None):
        return self._posterior(X, columns, row_index, scaler, want=("decision",))["decision"]

    def predict_proba(self, X, columns=None, row_index=None, scaler=None):
        return self._posterior(X, columns, row_index, scaler, want=("proba",))["proba"]

    def predict(self, X, columns=None, row_index=None, scaler=None):
        return self._labels(self._posterior(X, columns, row_index, scaler, want=("pred",))["pred"])


def _dev_hdr(name):
    return {"ITER": 0, "CONVERGED": 1, "STATUS": 2, "C": 3, "D": 4, "F": 5, "STEP": 6, "DD": 7, "PASSES": 8, "GMAX": 9, "SWSUM": 10,
            "PHASE": 11, "NSEEN": 12, "MAXITER": 13}[name]


# ---------------------------------------------------------------------------------------------- pipeline
class DetectionPipeline:
    """The two steps of script 02's classifier: `named_steps["scaler"]` and `named_steps["logreg"]`.  `fit` standardises
    inside the row pass: no standardised copy of X is written."""

    def __init__(self, scaler, logreg):
        self.named_steps = {"scaler": scaler, "logreg": logreg}
        self.steps = [("scaler", scaler), ("logreg", logreg)]

    def fit(self, X, y, columns=None, row_index=None, trace=None):
        self.named_steps["logreg"].fit(X, y, columns=columns, row_index=row_index, fit_scaler=self.named_steps["scaler"], trace=trace)
        return self

    @property
    def classes_(self):
        return self.named_steps["logreg"].classes_

    def _post(self, X, columns, row_index, normal_class, want):
        return self.named_steps["logreg"]._posterior(X, columns, row_index, self.named_steps["scaler"], normal_class, want)

    def decision_function(self, X, columns=None, row_index=None):
        return self._post(X, columns, row_index, 0, ("decision",))["decision"]

    def predict_proba(self, X, columns=None, row_index=None):
        return self._post(X, columns, row_index, 0, ("proba",))["proba"]

    def predict(self, X, columns=None, row_index=None):
        return self.named_steps["logreg"]._labels(self._post(X, columns, row_index, 0, ("pred",))["pred"])

    def p_fault(self, X, normal_class=0, columns=None, row_index=None, with_pred=False):
        """1 - P(class index normal_class) per row; with_pred=True also the predicted class indices, from the same launch."""
        r = self._post(X, columns, row_index, normal_class, ("p_fault", "pred") if with_pred else ("p_fault",))
        return (r["p_fault"], r["pred"]) if with_pred else r["p_fault"]


def build_classifier(balanced=False, backend="auto", **lr_args):
    """Script 02's pipeline (02:195-207): StandardScaler, then multinomial logistic regression with max_iter = 1000."""
    lr_args.setdefault("max_iter", 1000)
    return DetectionPipeline(DeviceStandardScaler(backend=backend),
                             DeviceLogisticRegression(class_weight="balanced" if balanced else None, backend=backend, **lr_args))


def explain_coefficients(clf, feature_indices, class_names, topn=DEFAULT_SHOW_COEF, verbose=False):
    """Per row of `coef_` (one per class; one row, that of the second class, for two classes) the `topn` most positive and
    most negative features in the standardised space (02:209-229).  Returns [{"class", "positive", "negative"}] with
    (feature name, coefficient) pairs; verbose=True also prints them."""
    if topn <= 0:
        return []
    inv = {v: k for k, v in INDEX.items()}
    names = [inv.get(i, "col%d" % i) for i in feature_indices]
    coefs = _as_numpy(clf.named_steps["logreg"].coef_)
    rows = [1] if coefs.shape[0] == 1 else range(coefs.shape[0])
    out = []
    for r, c_idx in enumerate(rows):
        w = coefs[r]
        pos = [(names[i], float(w[i])) for i in np.argsort(-w, kind="stable")[:topn]]
        neg = [(names[i], float(w[i])) for i in np.argsort(w, kind="stable")[:topn]]
        cname = class_names[c_idx] if c_idx < len(class_names) else str(c_idx)
        out.append({"class": cname, "positive": pos, "negative": neg})
        if verbose:
            print("- class[%d] %s:" % (c_idx, cname))
            print("  top %d positive: " % topn + ", ".join("%s(+%.3f)" % p for p in pos))
            print("  top %d negative: " % topn + ", ".join("%s(%.3f)" % p for p in neg))
    return out


# ---------------------------------------------------------------------------------------------- ROC and AUC
def _binary_truth(y_true, pos_label):
    """(positives as a 0/1 array or tensor of y_true's kind); pos_label=None takes 1 for labels in {0, 1} or {-1, 1}."""
    if pos_label is None:
        vals = set(np.unique(_as_numpy(y_true) if not _on_gpu(y_true) else y_true.unique().cpu().numpy()).tolist())
        if not (vals <= {0, 1} or vals <= {-1, 1}):
            raise ValueError("y_true takes values in %r and pos_label is not given" % (sorted(vals),))
        pos_label = 1
    return y_true == pos_label


def roc_counts(y_true, y_score, pos_label=None, drop_intermediate=True, backend="auto", curve=True):
    """The integers behind the ROC curve: dict with `fps`, `tps`, `thresholds` (scikit-learn's leading (0, 0, inf) point
    included; after drop_intermediate), `fpr`, `tpr`, and `n_pos`, `n_neg`, `n_distinct`, `U2` = sum dfps (tps_prev + tps) over
    all distinct scores: AUC = U2 / (2 n_pos n_neg) exactly.  curve=False returns the four numbers only."""
    if _pick_backend(backend, y_score) == "host":
        s = _as_numpy(y_score, np.float64).reshape(-1)
        pos = _as_numpy(_binary_truth(_as_numpy(y_true).reshape(-1), pos_label)).astype(np.int64)
        if s.shape != pos.shape or s.size < 1:
            raise ValueError("y_true and y_score must be two non-empty arrays of one length")
        order = np.argsort(s, kind="mergesort")[::-1]
        s, pos = s[order], pos[order]
        idx = np.concatenate([np.flatnonzero(np.diff(s)), [s.size - 1]])
        tps = np.cumsum(pos)[idx]
        fps = 1 + idx - tps
        thr = s[idx]
        P, N = int(tps[-1]), int(fps[-1])
        U2 = int((np.diff(np.concatenate([[0], fps])) * (np.concatenate([[0], tps[:-1]]) + tps)).sum())
        out = {"n_pos": P, "n_neg": N, "n_distinct": int(idx.size), "U2": U2}
        if not curve:
            return out
        if drop_intermediate and fps.size > 2:
            keep = np.flatnonzero(np.concatenate([[True], np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), [True]]))
            fps, tps, thr = fps[keep], tps[keep], thr[keep]
        fps, tps, thr = np.concatenate([[0], fps]), np.concatenate([[0], tps]), np.concatenate([[np.inf], thr])
        with np.errstate(invalid="ignore", divide="ignore"):
            fpr = fps / N if N > 0 else np.full(fps.shape, np.nan)
            tpr = tps / P if P > 0 else np.full(tps.shape, np.nan)
        out.update(fps=fps, tps=tps, thresholds=thr, fpr=fpr, tpr=tpr)
        return out
    torch, _lib, lib = _torch_lib()
    as_tensor = _is_tensor(y_score)
    dev = y_score.device if _on_gpu(y_score) else torch.device("cuda")
    s = _dev_vec(torch, y_score, torch.float64, dev)
    yt = y_true if _is_tensor(y_true) else np.asarray(y_true).reshape(-1)
    pos = _binary_truth(yt, pos_label)
    pos = (pos if _is_tensor(pos) else torch.from_numpy(np.ascontiguousarray(pos))).to(dev).reshape(-1)
    n = s.numel()
    if pos.numel() != n or n < 1:
        raise ValueError("y_true and y_score must be two non-empty arrays of one length")
    with torch.cuda.device(dev):
        # scikit-learn sorts ascending and stably, then reverses: equal scores stand in reverse input order.  A stable descending
        # sort of the reversed input gives that order, so the threshold of a group is the same element (+0.0 and -0.0 are equal)
        s_sorted, order = torch.sort(s.flip(0), descending=True, stable=True)
        pos_sorted = pos.flip(0)[order].to(torch.int64).contiguous()
        counts = torch.empty(8, dtype=torch.int64, device=dev)
        wb = lib.pinn_lr_roc_workspace_bytes(n)
        ws = torch.empty(wb, dtype=torch.uint8, device=dev)
        i64, f64 = dict(dtype=torch.int64, device=dev), dict(dtype=torch.float64, device=dev)
        bufs = [torch.empty(n + 1, **i64), torch.empty(n + 1, **i64), torch.empty(n + 1, **f64), torch.empty(n + 1, **f64),
                torch.empty(n + 1, **f64)] if curve else [None] * 5
        call("pinn_lr_roc", s_sorted, pos_sorted, n, int(bool(drop_intermediate)), counts, *bufs, ws, wb)
        c = counts.cpu().numpy()
    out = {"n_pos": int(c[0]), "n_neg": int(c[1]), "n_distinct": int(c[2]), "U2": int(c[4])}
    if not curve:
        return out
    m = int(c[3]) + 1
    arrs = [b[:m].clone() for b in bufs]
    if not as_tensor:
        arrs = [a.cpu().numpy() for a in arrs]
    if out["n_neg"] == 0:                                # scikit-learn: the whole rate is NaN, the origin included
        arrs[3][:] = float("nan")
    if out["n_pos"] == 0:
        arrs[4][:] = float("nan")
    out.update(zip(("fps", "tps", "thresholds", "fpr", "tpr"), arrs))
    return out


def roc_curve(y_true, y_score, pos_label=None, drop_intermediate=True, backend="auto"):
    """(fpr, tpr, thresholds) as scikit-learn 1.7's roc_curve, with its leading (0, 0, inf) point.  Unit sample weights.
    A class that does not occur gives NaN in its rate and a warning, as scikit-learn does."""
    r = roc_counts(y_true, y_score, pos_label, drop_intermediate, backend)
    if r["n_neg"] <= 0:
        warnings.warn("no negative samples in y_true: the false positive rate is meaningless")
    if r["n_pos"] <= 0:
        warnings.warn("no positive samples in y_true: the true positive rate is meaningless")
    return r["fpr"], r["tpr"], r["thresholds"]


def auc(x, y):
    """Area under a curve by the trapezoid rule (scikit-learn's auc): x monotonic, increasing or decreasing."""
    xh, yh = _as_numpy(x, np.float64).reshape(-1), _as_numpy(y, np.float64).reshape(-1)
    if xh.shape != yh.shape or xh.size < 2:
        raise ValueError("at least two points are needed, in two arrays of one length")
    dx = np.diff(xh)
    sign = 1.0
    if np.any(dx < 0):
        if np.all(dx <= 0):
            sign = -1.0
        else:
            raise ValueError("x is neither increasing nor decreasing")
    return float(sign * (dx * (yh[1:] + yh[:-1]) / 2.0).sum())


def auc_score(y_true, y_score, pos_label=None, backend="auto"):
    """Area under the ROC curve without materialising the curve: U2 / (2 n_pos n_neg) from integers, the float64 nearest to
    the exact ratio.  ValueError when only one class occurs."""
    r = roc_counts(y_true, y_score, pos_label, True, backend, curve=False)
    if r["n_pos"] == 0 or r["n_neg"] == 0:
        raise ValueError("only one class is present in y_true: the ROC AUC is not defined")
    return r["U2"] / (2 * r["n_pos"] * r["n_neg"])


# ---------------------------------------------------------------------------------------------- split and evaluation
def stratified_split(y, test_size=DEFAULT_TEST_SIZE, random_state=DEFAULT_RANDOM_STATE):
    """(idx_train, idx_test): row numbers of one stratified shuffle split, int64, usable as gather lists.  Every class gets
    floor(test_size count) test rows, and the rows still owed to ceil(test_size n) go to the classes with the largest
    remainders; a class with two or more rows keeps one for training.  The draws come from numpy's default_rng(random_state):
    the split has scikit-learn's properties, not its rows."""
    yh = _as_numpy(y).reshape(-1)
    if not 0.0 < float(test_size) < 1.0:
        raise ValueError("test_size must lie strictly between 0 and 1")
    n = yh.size
    classes, inv, count = np.unique(yh, return_inverse=True, return_counts=True)
    exact = float(test_size) * count
    k = np.floor(exact + 1e-9).astype(np.int64)
    owed = int(np.ceil(float(test_size) * n - 1e-9)) - int(k.sum())
    for c in np.argsort(-(exact - k), kind="stable")[:max(owed, 0)]:
        k[c] += 1
    k = np.where((count >= 2) & (k >= count), count - 1, k)
    rng = np.random.default_rng(random_state)
    tr, te = [], []
    for c in range(len(classes)):
        rows = rng.permutation(np.flatnonzero(inv == c))
        te.append(rows[:k[c]])
        tr.append(rows[k[c]:])
    tr, te = np.concatenate(tr), np.concatenate(te)
    return rng.permutation(tr).astype(np.int64), rng.permutation(te).astype(np.int64)


def compute_macro_metrics(y_true, y_pred):
    """accuracy and macro precision / recall / F1 with a zero division counted as 0 (script 05)."""
    t, p = _as_numpy(y_true).reshape(-1), _as_numpy(y_pred).reshape(-1)
    classes = np.unique(np.concatenate([t, p]))
    m = classification_metrics(np.searchsorted(classes, t), np.searchsorted(classes, p), len(classes))
    return {k: m[k] for k in ("accuracy", "macro_precision", "macro_recall", "macro_f1")}


def run_supervised_lr(X_tr, y_tr, X_te, backend="auto", **lr_args):
    """Script 05's supervised baseline: the balanced pipeline fitted on (X_tr, y_tr), predictions for X_te."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = build_classifier(balanced=True, backend=backend, **lr_args).fit(X_tr, y_tr)
    return clf.predict(X_te)


def evaluate_feature_groups(results, feature_groups=FEATURE_GROUPS, group_spec=DEFAULT_GROUP_SPEC, test_size=DEFAULT_TEST_SIZE,
                            random_state=DEFAULT_RANDOM_STATE, balanced=DEFAULT_BALANCED, split=None, backend="auto", unsupervised=False,
                            **lr_args):
    """Script 02's main loop without figures (02:503-569).  Per feature group: rows with a label of `group_spec` and finite
    features, a stratified split (or `split = (idx_tr, idx_te)`, positions among the kept rows), the classifier fitted on the
    training rows read in place, and on the test rows: accuracy, `classification_metrics`, the ROC arrays and AUC of
    p_fault = 1 - P(normal) against "not the normal class" (the class named `normal`, else class 0).
    Returns a list of dicts: spec, features, class_names, n_train, n_test, clf, accuracy, metrics, auc, fpr, tpr, thresholds,
    y_test, y_pred, p_fault, idx_train, idx_test, kept_rows.

    `unsupervised=True` adds script 02's unsupervised curve to the first group (02:571-596): an isolation forest of 200 trees
    (anomaly.DeviceIsolationForest, seeded with `random_state`) fitted on the normal training rows, on all training rows when
    there are not more than 10 normal ones, and the ROC and AUC of `anomaly_score` = -score_samples of the test rows read in
    place: keys auc_unsup, fpr_unsup, tpr_unsup, thresholds_unsup, anomaly_score, iforest.  `unsupervised=<a fitted or imported
    forest>` scores with that forest instead of fitting one."""
    label_map, class_names = build_label_mapper(parse_group_spec(group_spec))
    normal = class_names.index("normal") if "normal" in class_names else 0
    out = []
    for spec in feature_groups:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fidx = parse_features(spec) if isinstance(spec, str) else [int(c) for c in spec]
        be = _pick_backend(backend, results)
        X, y, kept = extract_X_y(results, fidx, label_map, return_index=True, backend=be)
        yh = _as_numpy(y).astype(np.int64)
        idx_tr, idx_te = split if split is not None else stratified_split(yh, test_size, random_state)
        idx_tr, idx_te = np.asarray(_as_numpy(idx_tr), dtype=np.int64), np.asarray(_as_numpy(idx_te), dtype=np.int64)
        if _is_tensor(kept):
            import torch
            r_tr, r_te = kept[torch.from_numpy(idx_tr).to(kept.device)], kept[torch.from_numpy(idx_te).to(kept.device)]
            y_tr, y_te = y[torch.from_numpy(idx_tr).to(y.device)], y[torch.from_numpy(idx_te).to(y.device)]
        else:
            r_tr, r_te, y_tr, y_te = kept[idx_tr], kept[idx_te], yh[idx_tr], yh[idx_te]
        clf = build_classifier(balanced=balanced, backend=be, **lr_args).fit(results, y_tr, columns=fidx, row_index=r_tr)
        cls = _as_numpy(clf.classes_).astype(np.int64)
        pf, pred = clf.p_fault(results, int(np.searchsorted(cls, normal)), columns=fidx, row_index=r_te, with_pred=True)
        y_pred = cls[_as_numpy(pred)]
        yte_h = _as_numpy(y_te).astype(np.int64)
        truth = (y_te != normal) if _is_tensor(y_te) else (yte_h != normal)
        r = roc_counts(truth, pf, pos_label=True, backend=be)
        area = r["U2"] / (2 * r["n_pos"] * r["n_neg"]) if r["n_pos"] and r["n_neg"] else float("nan")
        m = classification_metrics(yte_h, y_pred, len(class_names))
        out.append({"spec": spec, "features": fidx, "class_names": class_names, "n_train": len(idx_tr), "n_test": len(idx_te), "clf": clf,
                    "accuracy": m["accuracy"], "metrics": m, "auc": area, "fpr": r["fpr"], "tpr": r["tpr"], "thresholds": r["thresholds"],
                    "y_test": yte_h, "y_pred": y_pred, "p_fault": pf, "idx_train": idx_tr, "idx_test": idx_te, "kept_rows": kept})
        if unsupervised is not False and unsupervised is not None and len(out) == 1:
            from .anomaly import DeviceIsolationForest
            forest = unsupervised
            if unsupervised is True:
                is_normal = _as_numpy(y_tr).astype(np.int64) == normal
                if _is_tensor(r_tr):
                    import torch
                    sel = torch.from_numpy(is_normal).to(r_tr.device)
                else:
                    sel = is_normal
                r_fit = r_tr[sel] if int(is_normal.sum()) > 10 else r_tr
                forest = DeviceIsolationForest(n_estimators=200, contamination="auto", random_state=random_state, backend=be)
                forest.fit(results, columns=fidx, row_index=r_fit)
            saved, forest.backend = forest.backend, be
            try:
                score = -forest.score_samples(results, columns=fidx, row_index=r_te)
            finally:
                forest.backend = saved
            ru = roc_counts(truth, score, pos_label=True, backend=be)
            area_u = ru["U2"] / (2 * ru["n_pos"] * ru["n_neg"]) if ru["n_pos"] and ru["n_neg"] else float("nan")
            out[0].update(auc_unsup=area_u, fpr_unsup=ru["fpr"], tpr_unsup=ru["tpr"], thresholds_unsup=ru["thresholds"], anomaly_score=score,
                          iforest=forest)
    return out


class FaultDetector:
    """Fault probability chunk by chunk: `update(rows)` takes the next rows of the results array [n, >= 17] (device tensor,
    or a host array) and returns (p_fault, pred) for them, pred being class indices.  On the device a chunk is one kernel
    launch that reads the feature columns in place; it can run next to risk.RiskMonitor and diagnosis.FaultDiagnoser."""

    def __init__(self, pipeline, features=FEAT_GRP1, normal_class=0, backend="auto"):
        pipeline.named_steps["logreg"]._check_fitted()
        self.pipeline, self.normal_class, self.backend = pipeline, int(normal_class), backend
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            self.columns = columns_of(features, parse_features)
        self.n_seen = 0

    def update(self, rows):
        lr = self.pipeline.named_steps["logreg"]
        saved = lr.backend
        lr.backend = self.backend if self.backend != "auto" else saved
        try:
            out = self.pipeline.p_fault(rows, self.normal_class, columns=self.columns, with_pred=True)
        finally:
            lr.backend = saved
        self.n_seen += int(rows.shape[0])
        return out
