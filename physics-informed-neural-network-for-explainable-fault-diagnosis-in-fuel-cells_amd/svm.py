"""Script 05's Sup_SVM: a one-vs-one linear support vector classifier solved to the optimum on the device.

Script 05 runs `StandardScaler`, then `SVC(kernel="linear", C=0.05, class_weight="balanced")` (05:323-341).  libsvm's SMO
iterate at its default tolerance is no target, but the problem is: every pair (a, b), a < b, of the sorted classes solves

    min over (w, b) of  1/2 |w|^2 + sum_i c_i max(0, 1 - t_i (w . z_i + b)),   t_i = +1 for class a, -1 for class b,

over the rows of the two classes, z = (x - mean_) / scale_, c_i = C class_weight[y_i] ("balanced": n / (n_classes count) over
all training rows).  It is strictly convex in w, so w is unique, and any free support vector pins b.  Here the dual
(min 1/2 a'Qa - e'a, t'a = 0, 0 <= a <= c, Q = V V', V = diag(t) Z of rank <= D) is solved by a primal-dual interior-point
method with Mehrotra's predictor and corrector.  An iteration needs sums over the rows and a (D + 1) x (D + 1) solve: three
row passes, each followed by a one-workgroup launch, queued without a host synchronisation (csrc/pinn_svm.hip).  All pairs
advance together; a row of class k owns C - 1 slots (the other classes in increasing order) of alpha, s and z.

`DeviceLinearSVC` keeps scikit-learn's SVC names and defaults, `run_supervised_svm_rbf` is script 05's function (the name
is the reference's, the kernel is linear), `SVMDiagnoser` the online form.  Two backends as in risk.py: "device", and
"host": the same state machine in float64 numpy, for machines without a GPU and as the referee of the device tests.
Importing this module needs numpy only; scikit-learn is never imported.
"""
import warnings

import numpy as np

from ._classify import OneVsOneSVC, ovr_decision_function, pairs_of, scaler_stats, slot_of  # noqa: F401
from ._device import _DevRows, _as_numpy, _host_rows, _is_tensor, _pick_backend, _torch_lib, call, columns_of
from .detection import DeviceStandardScaler
from .diagnosis import DEFAULT_FEATURES, parse_features

# limits, status words and the 8-byte words of the state block: one copy, next to the bindings (include/pinn_hip.h)
from ._lib import (SVM_MAX_CLASSES as MAX_CLASSES, SVM_MAX_FEAT as MAX_FEAT, SVM_NAN, SVM_P_A as _P_A, SVM_P_B as _P_B, SVM_P_BETA as _P_BETA,
                   SVM_P_CONVERGED as _P_CONV, SVM_P_GAP as _P_GAP, SVM_P_ITER as _P_ITER, SVM_P_KA as _P_KA, SVM_P_KB as _P_KB,
                   SVM_P_M as _P_M, SVM_P_W as _P_W, SVM_PAIR_WORDS as _PW, SVM_RANGE, SVM_SINGULAR, SVM_ST_C, SVM_ST_CONVERGED,
                   SVM_ST_HEADER as _HDR, SVM_ST_STATUS)

START_SLACK = 1.0                        # s and z start at max(+-(t f - 1), 0) + this
STEP_TO_BOUNDARY = 0.995
START_ALPHA = 0.5                        # alpha starts at this fraction of its bound (on the lighter side of a pair)
MU_FLOOR = 0.1                           # the corrector aims at no mu below this x gap_tol max(1, primal) / (2 m)
_STATUS_TEXT = {SVM_NAN: "the rows hold values that are not finite", SVM_SINGULAR: "the normal equations could not be factorised",
                SVM_RANGE: "a row index or a class index lies outside its range"}


def _check_limits(D, C):
    if not (1 <= D <= MAX_FEAT and 2 <= C <= MAX_CLASSES):
        raise NotImplementedError("the linear SVC takes 1..%d features and 2..%d classes, got %d and %d" % (MAX_FEAT, MAX_CLASSES, D, C))


def n_pass_sums(D):
    """Sums of one row pass per pair: the upper triangle of sum u u' / d (u = (z, 1)), sum g t u / d, sum alpha t u (the last
    is t'alpha), then the sum of s alpha + z (c - alpha), sum alpha and the hinge sum."""
    return (D + 1) * (D + 2) // 2 + 2 * (D + 1) + 3


# ---------------------------------------------------------------------------------------------- host backend
def _tri_index(D1):
    return [(i, j) for j in range(D1) for i in range(j + 1)]          # tri(i, j) = j (j + 1) / 2 + i, i <= j


def _host_pair_sums(U, t, c, al, s, z, w, beta, want_abs=False):
    """The sums of a row pass of one pair at (alpha, s, z, w, beta): n_pass_sums(D) numbers, and optionally the sums of the
    absolute terms.  U = (Z, 1) [m, D + 1]."""
    D1 = U.shape[1]
    f = U[:, :D1 - 1] @ w + beta
    tf = t * f
    dinv = 1.0 / (s / al + z / (c - al))
    gq = dinv * (1.0 - tf) * t
    at = al * t
    cols = [dinv * U[:, i] * U[:, j] for i, j in _tri_index(D1)]
    cols += [gq * U[:, i] for i in range(D1)] + [at * U[:, i] for i in range(D1)]
    cols += [s * al + z * (c - al), al, c * np.maximum(0.0, 1.0 - tf)]
    T = np.stack(cols, axis=0)                                      # a term per row of T: numpy adds a contiguous row pairwise
    return (T.sum(axis=1), np.abs(T).sum(axis=1)) if want_abs else T.sum(axis=1)


def _chol_solve(L, rhs):
    return np.linalg.solve(L.T, np.linalg.solve(L, rhs))


def _boundary(v, dv):
    """The largest step that keeps v + step dv >= 0."""
    neg = dv < 0
    return float(np.min(-v[neg] / dv[neg])) if neg.any() else np.inf


def _host_ipm(Z, t, c, gap_tol, max_iter, trace=None):
    """One pair on the host.  Returns alpha, w, beta, n_iter, gap, primal, converged."""
    m, D = Z.shape
    U = np.concatenate([Z, np.ones((m, 1))], axis=1)
    if not np.isfinite(Z).all():
        raise ValueError(_STATUS_TEXT[SVM_NAN])
    Ca, Cb = c[t > 0].sum(), c[t < 0].sum()
    al = START_ALPHA * c * np.where(t > 0, min(Ca, Cb) / Ca, min(Ca, Cb) / Cb)
    w, beta = (al * t) @ Z, 0.0
    rho = t * (Z @ w + beta) - 1.0
    s, z = np.maximum(rho, 0.0) + START_SLACK, np.maximum(-rho, 0.0) + START_SLACK
    nT = (D + 1) * (D + 2) // 2
    tri = _tri_index(D + 1)
    it, conv = 0, False
    while True:
        S = _host_pair_sums(U, t, c, al, s, z, w, beta)
        M = np.zeros((D + 1, D + 1))
        for k, (i, j) in enumerate(tri):
            M[i, j] = M[j, i] = S[k]
        M[np.arange(D), np.arange(D)] += 1.0
        R, Wsum = S[nT:nT + D + 1], S[nT + D + 1:nT + 2 * D + 2]
        compl, sum_al, hinge = S[nT + 2 * D + 2:nT + 2 * D + 5]
        mu = compl / (2 * m)
        primal = 0.5 * float(w @ w) + hinge
        dual = sum_al - 0.5 * float(Wsum[:D] @ Wsum[:D])
        gap = primal - dual
        if trace is not None:
            trace.append({"iter": it, "mu": mu, "gap": gap, "primal": primal})
        if gap <= gap_tol * max(1.0, primal) and abs(Wsum[D]) <= 1e-12 * sum_al and np.abs(w - Wsum[:D]).max() <= 1e-13 * sum_al:
            conv = True
            break
        if it >= max_iter:
            break
        rhs = R.copy()
        rhs[:D] -= w - Wsum[:D]
        rhs[D] += Wsum[D]
        try:
            L = np.linalg.cholesky(M)
        except np.linalg.LinAlgError:
            raise ValueError(_STATUS_TEXT[SVM_SINGULAR]) from None
        d_aff = _chol_solve(L, rhs)
        # predictor
        f = Z @ w + beta
        dinv = 1.0 / (s / al + z / (c - al))
        g_aff = 1.0 - t * f
        da = dinv * (g_aff - t * (U @ d_aff))
        dsa, dza = -s - s * da / al, -z + z * da / (c - al)
        th = min(1.0, _boundary(al, da), _boundary(c - al, -da), _boundary(s, dsa), _boundary(z, dza))
        a1 = float(np.sum(s * da + al * dsa + dza * (c - al) - z * da))
        a2 = float(np.sum(dsa * da - dza * da))
        mu_aff = (compl + th * a1 + th * th * a2) / (2 * m)
        sigma = min(1.0, max(0.0, mu_aff / mu)) ** 3
        # no complementarity below a tenth of what gap_tol asks for: the matrix entries grow like 1 / mu, and so does the rounding
        sigmu = max(sigma * mu, MU_FLOOR * gap_tol * max(1.0, primal) / (2 * m))
        q1 = dinv * (1.0 / al - 1.0 / (c - al)) * t
        q2 = dinv * (-dsa * da / al - dza * da / (c - al)) * t
        d = _chol_solve(L, rhs + sigmu * (q1 @ U) + q2 @ U)
        # corrector
        g = g_aff + sigmu * (1.0 / al - 1.0 / (c - al)) - dsa * da / al - dza * da / (c - al)
        dal = dinv * (g - t * (U @ d))
        ds = (sigmu - s * al - dsa * da - s * dal) / al
        dz = (sigmu - z * (c - al) + dza * da + z * dal) / (c - al)
        th = min(1.0, STEP_TO_BOUNDARY * min(_boundary(al, dal), _boundary(c - al, -dal), _boundary(s, ds), _boundary(z, dz)))
        # The entries of the normal equations grow like 1 / mu, so the row directions satisfy V'dal = dw and t'dal = -t'al only
        # to about eps |M| |d|: near the end that is 1e-12, which the hinge sum does not forgive.  One step of refinement with
        # the sums of the row directions themselves puts it right: M fix = (V'dal - (w - V'al) - dw, t'dal + t'al), dal_i -= t_i u_i.fix / d_i.
        E = (dal * t) @ U
        e = E - d
        e[:D] -= w - Wsum[:D]
        e[D] = E[D] + Wsum[D]
        fix = _chol_solve(L, e)
        dfix = -dinv * t * (U @ fix)
        al, s, z = al + th * (dal + dfix), s + th * (ds - s / al * dfix), z + th * (dz + z / (c - al) * dfix)
        w, beta = w + th * (d[:D] + fix[:D]), beta + th * (d[D] + fix[D])
        it += 1
    return al, w, beta, it, gap, primal, conv


def _dot_in_order(Z, w):
    """sum_i w_i z_i of every row, products added in feature order as the kernel does."""
    v = np.zeros(Z.shape[0])
    for i in range(Z.shape[1]):
        v = v + w[i] * Z[:, i]
    return v


# ---------------------------------------------------------------------------------------------- the classifier
class DeviceLinearSVC(OneVsOneSVC):
    """One-vs-one linear SVC with scikit-learn's SVC arguments and defaults; `kernel="linear"` only.  `tol` is accepted for
    compatibility: the solver stops when primal - dual <= gap_tol max(1, primal) of every pair.

    Attributes: `classes_`, `class_weight_` [C], `coef_` [P, D] and `intercept_` [P] (standardised coordinates when a scaler
    is attached; scikit-learn's pair order and signs: positive for the pair's first class, and negated for two classes), `n_iter_` [P], `dual_gap_` [P] (primal - dual at the returned
    point), `converged_` [P], `alpha_` [n, C - 1] (slot j of a row: its j-th other class in increasing order),
    `n_support_` [C] (rows with any alpha above 1e-8 c).  `pair_alpha(a, b)` gives (row positions, alpha) of a pair.

    `fit`, `decision_function`, `predict` take X [n, D], or any array plus `columns` (and `row_index`): the device backend
    then reads the rows in place; `scaler=` (a fitted DeviceStandardScaler) standardises inside the row pass.  numpy in ->
    numpy out, device tensor in -> device tensors out."""

    def __init__(self, *, C=1.0, kernel="linear", class_weight=None, tol=1e-3, max_iter=-1, decision_function_shape="ovr", break_ties=False,
                 random_state=None, gap_tol=1e-11, backend="auto", chunk=8):
        if kernel != "linear":
            raise NotImplementedError("kernel=%r: only 'linear' is implemented" % (kernel,))
        super().__init__(C, class_weight, max_iter, decision_function_shape, break_ties, random_state, backend, chunk, "gap_tol", gap_tol)
        self.kernel, self.tol, self.gap_tol = kernel, float(tol), float(gap_tol)

    _FITTED, _NOT_FINITE, _LAYOUT = "coef_", _STATUS_TEXT[SVM_NAN], (_HDR, _PW, _P_A, _P_B, SVM_ST_C)
    _check_limits = staticmethod(_check_limits)

    def _limit(self):
        return 500 if self.max_iter == -1 else self.max_iter      # no limit in scikit-learn; 10 to 200 iterations are taken

    def _publish(self, classes, cw, coef, icpt, n_iter, gap, conv, alpha, yi, as_tensor, dev=None):
        C = len(cw)
        if not np.all(conv):
            warnings.warn("the interior-point iteration did not reach gap_tol = %g in %d iterations (largest gap %.3e)"
                          % (self.gap_tol, self._limit(), float(np.max(gap))))
        self._w, self._b = np.ascontiguousarray(coef), np.ascontiguousarray(icpt)      # positive for the pair's first class
        sign = -1.0 if C == 2 else 1.0                                                   # scikit-learn negates the binary model
        out = [sign * self._w, sign * self._b, np.asarray(cw, dtype=np.float64)]
        if as_tensor:
            import torch
            out = [torch.from_numpy(a).to(dev) for a in out]
        self.coef_, self.intercept_, self.class_weight_ = out
        self.classes_, self.alpha_ = classes, alpha
        self.n_iter_, self.dual_gap_, self.converged_ = np.asarray(n_iter, dtype=np.int64), np.asarray(gap, dtype=np.float64), np.asarray(conv, dtype=bool)
        self.n_features_in_ = coef.shape[1]
        self._yi = yi
        a_h, y_h = _as_numpy(alpha), _as_numpy(yi)
        sup = (a_h > 1e-8 * (self.C * np.asarray(cw))[y_h][:, None]).any(axis=1)
        self.n_support_ = np.bincount(y_h[sup], minlength=C).astype(np.int64)
        self._model = None

    # ---- fit
    def fit(self, X, y, sample_weight=None, columns=None, row_index=None, scaler=None, trace=None):
        """`scaler`: a fitted DeviceStandardScaler whose statistics standardise the rows.  `trace`: a list that receives one
        list per pair of (iter, mu, gap, primal) dicts; host backend only, the device backend raises NotImplementedError."""
        if sample_weight is not None:
            raise NotImplementedError("sample_weight is not implemented (class_weight is)")
        if _pick_backend(self.backend, X) != "host":
            if trace is not None:
                raise NotImplementedError("trace= is kept by the host backend only: the device reads its state once per chunk")
            return self._fit_device(X, y, columns, row_index, scaler)
        Z, yi, classes, cw, _ = self._host_setup(X, y, columns, row_index, scaler)
        C, D = len(classes), Z.shape[1]
        pairs = pairs_of(C)
        P = len(pairs)
        coef, icpt, n_iter, gap, conv = np.zeros((P, D)), np.zeros(P), np.zeros(P, dtype=np.int64), np.zeros(P), np.zeros(P, dtype=bool)
        alpha = np.zeros((len(yi), C - 1))
        for p, (a, b) in enumerate(pairs):
            ia, ib = np.nonzero(yi == a)[0], np.nonzero(yi == b)[0]
            idx = np.concatenate([ia, ib])
            t = np.concatenate([np.ones(len(ia)), -np.ones(len(ib))])
            tr = [] if trace is not None else None
            al, coef[p], icpt[p], n_iter[p], gap[p], _, conv[p] = _host_ipm(Z[idx], t, self.C * cw[yi[idx]], self.gap_tol, self._limit(), tr)
            alpha[ia, slot_of(a, b)], alpha[ib, slot_of(b, a)] = al[:len(ia)], al[len(ia):]
            if trace is not None:
                trace.append(tr)
        self._publish(classes, cw, coef, icpt, n_iter, gap, conv, alpha, yi, False)
        return self

    def _state0(self, n, C, D, count, bound, mean, scale):
        s0 = super()._state0(n, C, D, bound, mean, scale)
        for p, (a, b) in enumerate(pairs_of(C)):
            o = _HDR + p * _PW
            Ca, Cb = bound[a] * count[a], bound[b] * count[b]
            s0[o + _P_M] = count[a] + count[b]
            s0[o + _P_KA], s0[o + _P_KB] = START_ALPHA * min(Ca, Cb) / Ca, START_ALPHA * min(Ca, Cb) / Cb
        return s0

    def _fit_device(self, X, y, columns, row_index, scaler):
        torch, _lib, lib = _torch_lib()
        rows, yi, classes, cls_h, count, cw, mean, scale = self._dev_setup(torch, X, y, columns, row_index, scaler)
        with torch.cuda.device(rows.dev):
            C, D, n = len(cw), rows.D, rows.n
            P = C * (C - 1) // 2
            s0 = self._state0(n, C, D, count, self.C * cw, mean, scale)
            words = lib.pinn_svm_state_bytes(n, C, D) // 8
            st = torch.zeros(words, dtype=torch.float64, device=rows.dev)
            st[:len(s0)] = torch.from_numpy(s0).to(rows.dev)
            wb = lib.pinn_svm_workspace_bytes(n, C, D)
            ws = torch.empty(wb, dtype=torch.uint8, device=rows.dev)
            stream = torch.cuda.current_stream().cuda_stream
            head = rows.head() + (yi, C)
            done, init, limit = 0, 1, self._limit()
            while True:
                step = min(self.chunk, limit - done)
                call("pinn_svm_ipm", *head, init, step, self.gap_tol, st, ws, wb, stream=stream)
                done, init = done + step, 0
                h = st[:_HDR + P * _PW].cpu().numpy()              # one read of the header and the pair blocks per chunk
                hi = h.view(np.int64)
                if hi[SVM_ST_CONVERGED] or hi[SVM_ST_STATUS] or done >= limit:
                    break
            status = int(hi[SVM_ST_STATUS])
            if status:
                raise ValueError("the linear SVC failed: %s (status %d)" % (_STATUS_TEXT.get(status, "several failures"), status))
            pb = h[_HDR:].reshape(P, _PW)
            pi = hi[_HDR:].reshape(P, _PW)
            o = len(s0)
            alpha = st[o:o + n * (C - 1)].reshape(n, C - 1).clone()
            as_tensor = _is_tensor(X)
            self._publish(classes if as_tensor else cls_h, cw, pb[:, _P_W:_P_W + D].copy(), pb[:, _P_BETA].copy(), pi[:, _P_ITER].copy(),
                          pb[:, _P_GAP].copy(), pi[:, _P_CONV] != 0, alpha if as_tensor else alpha.cpu().numpy(),
                          yi if as_tensor else yi.cpu().numpy(), as_tensor, rows.dev)
        return self

    def pass_sums(self, X, y, alpha, s, z, coef, intercept, columns=None, row_index=None, scaler=None, want_abs=False):
        """The sums of one row pass at the given interior point: [P, n_pass_sums(D)], y holding class indices 0..C-1, alpha, s
        and z [n, C - 1], coef [P, D], intercept [P].  For tests and tools.  The host backend can also return the sums of
        the absolute terms."""
        coef, icpt = np.asarray(_as_numpy(coef), dtype=np.float64), np.asarray(_as_numpy(intercept), dtype=np.float64).reshape(-1)
        P, D = coef.shape
        C = int(round((1 + np.sqrt(1 + 8 * P)) / 2))
        _check_limits(D, C)
        yh = _as_numpy(y).astype(np.int64).reshape(-1)
        count = np.bincount(yh, minlength=C)
        cw = self._weights(np.arange(C), count)
        mean, scale = scaler_stats(scaler, D)
        a_h, s_h, z_h = (np.asarray(_as_numpy(v), dtype=np.float64).reshape(len(yh), C - 1) for v in (alpha, s, z))
        if _pick_backend(self.backend, X) == "host":
            Z = (_host_rows(X, columns, row_index) - mean) / scale
            S, A = np.zeros((P, n_pass_sums(D))), np.zeros((P, n_pass_sums(D)))
            for p, (a, b) in enumerate(pairs_of(C)):
                # rows in position order: the order the device adds a tile's terms in
                idx = np.nonzero((yh == a) | (yh == b))[0]
                t = np.where(yh[idx] == a, 1.0, -1.0)
                sl = np.where(yh[idx] == a, slot_of(a, b), slot_of(b, a))
                U = np.concatenate([Z[idx], np.ones((len(idx), 1))], axis=1)
                S[p], A[p] = _host_pair_sums(U, t, self.C * cw[yh[idx]], a_h[idx, sl], s_h[idx, sl], z_h[idx, sl], coef[p], icpt[p], True)
            return (S, A) if want_abs else S
        torch, _lib, lib = _torch_lib()
        rows = _DevRows(torch, X, columns, row_index)
        if rows.D != D or rows.n != len(yh):
            raise ValueError("coef is for %d features and y for %d rows, the rows are [%d, %d]" % (D, len(yh), rows.n, rows.D))
        with torch.cuda.device(rows.dev):
            n = rows.n
            s0 = self._state0(n, C, D, count, self.C * cw, mean, scale)
            for p in range(P):
                o = _HDR + p * _PW
                s0[o + _P_W:o + _P_W + D], s0[o + _P_BETA] = coef[p], icpt[p]
            st = torch.from_numpy(np.concatenate([s0, a_h.reshape(-1), s_h.reshape(-1), z_h.reshape(-1)])).to(rows.dev)
            assert st.numel() * 8 == lib.pinn_svm_state_bytes(n, C, D)
            wb = lib.pinn_svm_workspace_bytes(n, C, D)
            ws = torch.empty(wb, dtype=torch.uint8, device=rows.dev)
            yi = torch.from_numpy(yh).to(rows.dev)
            call("pinn_svm_pass", *rows.head(), yi, C, st, ws, wb)
            out = ws[:P * n_pass_sums(D) * 8].view(torch.float64).reshape(P, n_pass_sums(D)).clone()
        return out if _is_tensor(X) else out.cpu().numpy()

    # ---- decision
    def _device_model(self, torch, dev, scaler):
        key = (str(dev), id(scaler))
        if self._model is None or self._model[0] != key:
            mean, scale = scaler_stats(scaler, self.n_features_in_)
            m = np.concatenate([mean, scale, self._w.reshape(-1), self._b.reshape(-1)])
            self._model = (key, torch.from_numpy(m).to(dev))
        return self._model[1]

    def _host_values(self, Z):
        if not self._w.shape[0]:
            return np.zeros((len(Z), 0))
        return np.stack([_dot_in_order(Z, self._w[p]) + self._b[p] for p in range(self._w.shape[0])], axis=1)

    def _launch_decision(self, torch, rows, scaler, C, out):
        call("pinn_svm_decision", *rows.head(), C, self._device_model(torch, rows.dev, scaler), out["decision"], out["votes"], out["pred"])


class SVCPipeline:
    """Script 05's pipeline: `named_steps["scaler"]` and `named_steps["svc"]`; the rows are standardised inside the passes."""

    def __init__(self, scaler, svc):
        self.named_steps = {"scaler": scaler, "svc": svc}
        self.steps = [("scaler", scaler), ("svc", svc)]

    def fit(self, X, y, columns=None, row_index=None):
        sc = self.named_steps["scaler"].fit(X, columns=columns, row_index=row_index)
        self.named_steps["svc"].fit(X, y, columns=columns, row_index=row_index, scaler=sc)
        return self

    @property
    def classes_(self):
        return self.named_steps["svc"].classes_

    def decision_function(self, X, columns=None, row_index=None, shape=None):
        return self.named_steps["svc"].decision_function(X, columns, row_index, self.named_steps["scaler"], shape)

    def predict(self, X, columns=None, row_index=None):
        return self.named_steps["svc"].predict(X, columns, row_index, self.named_steps["scaler"])


def build_svm_classifier(backend="auto", **svc_args):
    """Script 05's Sup_SVM pipeline (05:323-341): StandardScaler, then SVC(kernel="linear", C=0.05, class_weight="balanced")."""
    svc_args.setdefault("C", 0.05)
    svc_args.setdefault("class_weight", "balanced")
    return SVCPipeline(DeviceStandardScaler(backend=backend), DeviceLinearSVC(backend=backend, **svc_args))


def run_supervised_svm_rbf(X_tr, y_tr, X_te, backend="auto", **svc_args):
    """Script 05's function of this name (the kernel is linear there too): y_pred [n_te]."""
    return build_svm_classifier(backend, **svc_args).fit(X_tr, y_tr).predict(X_te)


class SVMDiagnoser:
    """Predicted classes chunk by chunk from a fitted pipeline (build_svm_classifier): `update(rows)` takes the next rows of
    the results array [n, >= 17] (device tensor, or a host array) and returns y_pred for them.  On the device a chunk is one
    kernel launch that reads the feature columns in place; it can run next to comparison.ClusterDiagnoser on the same chunk."""

    def __init__(self, pipeline, features=DEFAULT_FEATURES):
        pipeline.named_steps["svc"]._check_fitted()
        self.pipeline = pipeline
        self.columns = columns_of(features, parse_features)
        self.n_seen = 0

    def update(self, rows):
        y_pred = self.pipeline.predict(rows, columns=self.columns)
        self.n_seen += int(rows.shape[0])
        return y_pred
