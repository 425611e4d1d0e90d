"""The RBF-kernel SVC that script 05 names: a one-vs-one support vector classifier with K(x, y) = exp(-gamma |x - y|^2),
every pair solved by sequential minimal optimisation in float64 on the device.

Script 05 announces Sup_SVM as an RBF machine (its header list, the name `run_supervised_svm_rbf`, `gamma="scale"`) and runs
`kernel="linear"` (05:323-341); svm.py is what it runs, this module is what it names.  Every pair (a, b), a < b, of the
sorted classes solves, over the rows of its two classes in the order `fit` was given them,

    min 1/2 al'Q al - e'al,   0 <= al_i <= c_i,   t'al = 0,   Q_ij = t_i t_j exp(-gamma |z_i - z_j|^2),

t = +1 for class a and -1 for class b, c_i = C class_weight[y_i] (svm.py's rules), z = (x - mean_) / scale_ when a scaler is
attached.  The Gram matrix of distinct rows is positive definite, so the optimum is unique.  The iteration is libsvm's SMO
on the gradient G = Q al - e from al = 0: i = the first maximum of -t G over I_up, j = the first minimum of -b^2 / a over
the rows of I_low with b = gmax + t_j G_j > 0, a = 2 - 2 K_ij (1e-12 where that is not positive), libsvm's clipped update of
the two, G += t (t_i K_i dal_i + t_j K_j dal_j), until gmax - gmin <= tol.  The first of equal candidates wins (libsvm
takes the last); there is neither shrinking nor a kernel cache, and a kernel column is evaluated in float64 where libsvm
keeps float32.  The certificate needs no kernel evaluation, since t_i f_i = G_i + 1 + t_i b:

    al'Q al = sum al_i (G_i + 1),   primal = 1/2 al'Q al + sum c_i max(0, -G_i - t_i b),   dual = sum al_i - 1/2 al'Q al.

Two backends as in svm.py: "device" (csrc/pinn_ksvm.hip) and "host", the same state machine in float64 numpy, for machines
without a GPU and as the referee of the device tests.  Importing this module needs numpy only; scikit-learn is never imported.
"""
import warnings

import numpy as np

from ._classify import OneVsOneSVC, pairs_of, scaler_stats, slot_of
from ._device import _is_tensor, _pick_backend, _torch_lib, call
from .detection import DeviceStandardScaler
from .svm import SVCPipeline, SVMDiagnoser

# limits, status words and the 8-byte words of the state block: one copy, next to the bindings (include/pinn_hip.h)
from ._lib import (KSVM_MAX_CLASSES as MAX_CLASSES, KSVM_MAX_FEAT as MAX_FEAT, KSVM_NAN, KSVM_P_A as _P_A, KSVM_P_B as _P_B,
                   KSVM_P_CONVERGED as _P_CONV, KSVM_P_GAP as _P_GAP, KSVM_P_ITER as _P_ITER, KSVM_P_RHO as _P_RHO, KSVM_P_STATUS as _P_STATUS,
                   KSVM_P_VIOLATION as _P_VIOL, KSVM_PAIR_WORDS as _PW, KSVM_RANGE, KSVM_ST_HEADER as _HDR, KSVM_SV_TILE as SV_TILE)

TAU = 1e-12                              # stands for 2 - 2 K_ij where that is not positive (duplicate rows)
ITER_PER_ROW = 100                       # max_iter=-1: this many iterations per row of the largest pair
_STATUS_TEXT = {KSVM_NAN: "the rows hold values that are not finite", KSVM_RANGE: "a row index or a class index lies outside its range"}


def _check_limits(D, C):
    if not (1 <= D <= MAX_FEAT and 2 <= C <= MAX_CLASSES):
        raise NotImplementedError("the kernel SVC takes 1..%d features and 2..%d classes, got %d and %d" % (MAX_FEAT, MAX_CLASSES, D, C))


# ---------------------------------------------------------------------------------------------- host backend
def _kernel_column(Z, z, gamma):
    """exp(-gamma |Z_r - z|^2) of every row, the squared differences added in feature order as the kernel does."""
    d2 = np.zeros(Z.shape[0])
    for k in range(Z.shape[1]):
        d = Z[:, k] - z[k]
        d2 = d2 + d * d
    return np.exp(-(gamma * d2))


def _clipped_update(ai, aj, Gi, Gj, ci, cj, ti, tj, Kij):
    """libsvm's update of (alpha_i, alpha_j); Q_ii = Q_jj = 1, so both sign cases divide by 2 - 2 K_ij."""
    q = 2.0 - 2.0 * Kij
    if not q > 0.0:
        q = TAU
    if ti != tj:
        delta, diff = (-Gi - Gj) / q, ai - aj
        ai, aj = ai + delta, aj + delta
        if diff > 0.0:
            if aj < 0.0:
                aj, ai = 0.0, diff
        elif ai < 0.0:
            ai, aj = 0.0, -diff
        if diff > ci - cj:
            if ai > ci:
                ai, aj = ci, ci - diff
        elif aj > cj:
            aj, ai = cj, cj + diff
    else:
        delta, s = (Gi - Gj) / q, ai + aj
        ai, aj = ai - delta, aj + delta
        if s > ci:
            if ai > ci:
                ai, aj = ci, s - ci
        elif aj < 0.0:
            aj, ai = 0.0, s
        if s > cj:
            if aj > cj:
                aj, ai = cj, s - cj
        elif ai < 0.0:
            ai, aj = 0.0, s
    return ai, aj


def _margin(v, best):
    """Best value to second-best value of a selection by the largest entry of v."""
    if v.shape[0] < 2:
        return np.inf
    second = np.partition(v, -2)[-2]
    return float(best - second) if np.isfinite(second) else np.inf


def _sets(t, al, c):
    pos = t > 0
    return np.where(pos, al < c, al > 0.0), np.where(pos, al > 0.0, al < c)


def _host_smo(Z, t, c, gamma, tol, max_iter, pos=None, trace=None, abs_terms=None):
    """One pair on the host, rows in position order.  Returns alpha, G, n_iter, converged.  `abs_terms`: two arrays [m] that
    receive the sums of the absolute terms of alpha and of G (the latter starts at |-1|)."""
    m = len(t)
    al, G = np.zeros(m), -np.ones(m)
    it, conv = 0, False
    while True:
        up, low = _sets(t, al, c)
        v = -(t * G)
        vi = np.where(up, v, -np.inf)
        i = int(np.argmax(vi))                               # the first of equals
        gmax, gmin = vi[i], np.where(low, v, np.inf).min()
        if not gmax - gmin > tol:
            conv = True
            break
        if it >= max_iter:
            break
        Ki = _kernel_column(Z, Z[i], gamma)
        b = gmax + t * G
        q = 2.0 - 2.0 * Ki
        q = np.where(q > 0.0, q, TAU)
        key = np.where(low & (b > 0.0), (b * b) / q, -np.inf)          # libsvm minimises -b^2 / a
        j = int(np.argmax(key))
        if trace is not None:
            trace.append((int(pos[i]) if pos is not None else i, int(pos[j]) if pos is not None else j, float(gmax - gmin),
                          (_margin(vi, gmax), float(gmax)), (_margin(key, key[j]), float(key[j]))))
        Kj = _kernel_column(Z, Z[j], gamma)
        ai, aj = _clipped_update(al[i], al[j], G[i], G[j], c[i], c[j], t[i], t[j], Ki[j])
        di, dj = ai - al[i], aj - al[j]
        G = G + t * ((t[i] * Ki) * di + (t[j] * Kj) * dj)
        if abs_terms is not None:
            abs_terms[0][i] += abs(di)
            abs_terms[0][j] += abs(dj)
            abs_terms[1][:] += Ki * abs(di) + Kj * abs(dj)
        al[i], al[j] = ai, aj
        it += 1
    return al, G, it, conv


def _certificate(t, c, al, G):
    """libsvm's rho and the certificate at (alpha, G): dict with rho, primal, dual, gap, sum_alpha, t_alpha, n_free, violation."""
    pos = t > 0
    tG = t * G
    at_c, at_0 = al >= c, al <= 0.0
    free = ~at_c & ~at_0
    if free.any():
        rho = tG[free].sum() / free.sum()
    else:
        ub = np.where((at_c & ~pos) | (at_0 & ~at_c & pos), tG, np.inf).min()
        lb = np.where((at_c & pos) | (at_0 & ~at_c & ~pos), tG, -np.inf).max()
        rho = (ub + lb) / 2.0
    b = -rho
    quad = float(np.sum(al * (G + 1.0)))
    primal = 0.5 * quad + float(np.sum(c * np.maximum(0.0, -G - t * b)))
    dual = float(al.sum()) - 0.5 * quad
    up, low = _sets(t, al, c)
    v = -tG
    viol = np.where(up, v, -np.inf).max() - np.where(low, v, np.inf).min()
    return {"rho": float(rho), "primal": primal, "dual": dual, "gap": primal - dual, "sum_alpha": float(al.sum()),
            "t_alpha": float(np.sum(t * al)), "n_free": int(free.sum()), "violation": float(viol)}


def _host_values(Zx, sv, coef, sv_cls, rho, gamma, C):
    """Pairwise values [n, P]: the terms of a value added in the order of the support rows."""
    index = {ab: p for p, ab in enumerate(pairs_of(C))}
    acc = np.zeros((Zx.shape[0], len(index)))
    for s in range(sv.shape[0]):
        K = _kernel_column(Zx, sv[s], gamma)
        k = int(sv_cls[s])
        for o in range(C):
            if o != k:
                p = index[(min(o, k), max(o, k))]
                acc[:, p] = acc[:, p] + coef[s, slot_of(k, o)] * K
    return acc - rho[None, :]


def scale_gamma(Z):
    """scikit-learn's gamma="scale": 1 / (D var), var over all entries of Z by two-pass float64 sums."""
    Z = np.asarray(Z, dtype=np.float64)
    mean = Z.sum() / Z.size
    var = ((Z - mean) ** 2).sum() / Z.size
    return 1.0 / (Z.shape[1] * var) if var > 0 else 1.0


# ---------------------------------------------------------------------------------------------- the classifier
class DeviceKernelSVC(OneVsOneSVC):
    """One-vs-one RBF-kernel SVC with scikit-learn's SVC arguments; `kernel="rbf"` only.

    `tol` is libsvm's stopping rule, the largest violation gmax - gmin of a pair, and a real parameter here (DeviceLinearSVC
    only accepts it).  Its default is 1e-10 where scikit-learn's is 1e-3: at 1e-3 the iterate is no target (signs of
    borderline decision values differ between solvers), at 1e-10 the float64 iteration reaches a duality gap that libsvm,
    which keeps kernel values in float32, cannot.  `max_iter=-1` allows ITER_PER_ROW iterations per row of the largest pair.
    Working sets: the first of equal candidates wins, where libsvm takes the last.  `shrinking` and `random_state` are
    accepted and unused.

    Attributes: `classes_`, `class_weight_` [C], `gamma_`, `support_` (ascending row positions), `support_vectors_`
    (standardised coordinates when a scaler is attached), `dual_coef_` [C - 1, n_sv] and `intercept_` [P] in scikit-learn's
    layout and signs (row j of a support row: t alpha against its j-th other class in increasing order, positive for the
    pair's first class; both negated for two classes), `n_support_` [C], `alpha_` [n, C - 1], `n_iter_`, `violation_`,
    `dual_gap_` (primal - dual at the returned point) and `converged_` [P].  `pair_alpha(a, b)` as in svm.py.

    `fit`, `decision_function`, `predict` take X [n, D], or any array plus `columns` (and `row_index`): the device backend
    then reads the rows in place; `scaler=` (a fitted DeviceStandardScaler) standardises inside the row pass.  numpy in ->
    numpy out, device tensor in -> device tensors out."""

    def __init__(self, *, C=1.0, kernel="rbf", gamma="scale", class_weight=None, tol=1e-10, max_iter=-1, decision_function_shape="ovr",
                 shrinking=True, probability=False, break_ties=False, random_state=None, backend="auto", chunk=64):
        if kernel != "rbf":
            raise NotImplementedError("kernel=%r: only 'rbf' is implemented (svm.DeviceLinearSVC has 'linear')" % (kernel,))
        if probability:
            raise NotImplementedError("probability=True is not implemented")
        super().__init__(C, class_weight, max_iter, decision_function_shape, break_ties, random_state, backend, chunk, "tol", tol)
        if isinstance(gamma, str):
            if gamma not in ("scale", "auto"):
                raise ValueError("gamma must be 'scale', 'auto' or a positive number")
        elif not (float(gamma) > 0 and np.isfinite(float(gamma))):
            raise ValueError("gamma must be 'scale', 'auto' or a positive number")
        self.kernel, self.gamma, self.tol, self.shrinking, self.probability = kernel, gamma, float(tol), shrinking, False

    _FITTED, _NOT_FINITE, _LAYOUT = "dual_coef_", "the kernel SVC failed: %s" % _STATUS_TEXT[KSVM_NAN], (_HDR, _PW, _P_A, _P_B, 0)
    _check_limits = staticmethod(_check_limits)

    def _limit(self, count):
        if self.max_iter != -1:
            return self.max_iter
        top = np.sort(np.asarray(count))[-2:].sum()
        return ITER_PER_ROW * int(top)

    def _gamma_of(self, Z):
        if self.gamma == "auto":
            return 1.0 / Z.shape[1]
        return scale_gamma(Z) if self.gamma == "scale" else float(self.gamma)

    def _publish(self, classes, cw, gamma, Z_sup, support, alpha_sup, y_sup, rho, n_iter, viol, gap, conv, alpha, yi, count, as_tensor, dev=None):
        """Z_sup, alpha_sup [n_sv, C - 1], y_sup: the support rows (host arrays, ascending position)."""
        C = len(cw)
        if not np.all(conv):
            warnings.warn("SMO did not reach tol = %g in %d iterations (largest violation %.3e)" % (self.tol, self._limit(count), float(np.max(viol))))
        sign = np.ones_like(alpha_sup)
        for k in range(C):
            for o in range(C):
                if o > k:
                    sign[y_sup == k, slot_of(k, o)] = 1.0
                elif o < k:
                    sign[y_sup == k, slot_of(k, o)] = -1.0
        self._sv, self._coef = np.ascontiguousarray(Z_sup), np.ascontiguousarray(sign * alpha_sup)      # t alpha, slot layout
        self._sv_cls, self._rho, self._gamma = np.ascontiguousarray(y_sup, dtype=np.int64), np.ascontiguousarray(rho), float(gamma)
        flip = -1.0 if C == 2 else 1.0                                                  # scikit-learn negates the binary model
        out = [support.astype(np.int64), self._sv, np.ascontiguousarray(flip * self._coef.T), -flip * self._rho, np.asarray(cw, dtype=np.float64)]
        if as_tensor:
            import torch
            out = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in out]
        self.support_, self.support_vectors_, self.dual_coef_, self.intercept_, self.class_weight_ = out
        self.classes_, self.alpha_, self.gamma_ = classes, alpha, float(gamma)
        self.n_iter_, self.violation_ = np.asarray(n_iter, dtype=np.int64), np.asarray(viol, dtype=np.float64)
        self.dual_gap_, self.converged_ = np.asarray(gap, dtype=np.float64), np.asarray(conv, dtype=bool)
        self.n_support_ = np.bincount(y_sup, minlength=C).astype(np.int64)
        self.n_features_in_ = Z_sup.shape[1]
        self._yi = yi
        self._model = None

    # ---- fit
    def fit(self, X, y, sample_weight=None, columns=None, row_index=None, scaler=None, trace=None):
        """`scaler`: a fitted DeviceStandardScaler whose statistics standardise the rows.  `trace`: a list that receives one
        list per pair of (i, j, gmax - gmin, (margin, value) of the choice of i, (margin, value) of the choice of j) per
        iteration, i and j as row positions, a margin the best value minus the second best; host backend only."""
        if sample_weight is not None:
            raise NotImplementedError("sample_weight is not implemented (class_weight is)")
        if _pick_backend(self.backend, X) != "host":
            if trace is not None:
                raise NotImplementedError("trace= is kept by the host backend only (working_sets() reads the device's log)")
            return self._fit_device(X, y, columns, row_index, scaler)
        Z, yi, classes, cw, count = self._host_setup(X, y, columns, row_index, scaler)
        C = len(classes)
        gamma = self._gamma_of(Z)
        pairs = pairs_of(C)
        P, n = len(pairs), len(yi)
        alpha, rho = np.zeros((n, C - 1)), np.zeros(P)
        n_iter, viol, gap, conv = np.zeros(P, dtype=np.int64), np.zeros(P), np.zeros(P), np.zeros(P, dtype=bool)
        for p, (a, b) in enumerate(pairs):
            idx, t, c, sl = self._pair_rows(yi, cw, a, b)
            tr = [] if trace is not None else None
            al, G, n_iter[p], conv[p] = _host_smo(Z[idx], t, c, gamma, self.tol, self._limit(count), idx, tr)
            cert = _certificate(t, c, al, G)
            rho[p], viol[p], gap[p] = cert["rho"], cert["violation"], cert["gap"]
            alpha[idx, sl] = al
            if trace is not None:
                trace.append(tr)
        sup = np.nonzero((alpha > 0).any(axis=1))[0]
        self._publish(classes, cw, gamma, Z[sup], sup, alpha[sup], yi[sup], rho, n_iter, viol, gap, conv, alpha, yi, count, False)
        return self

    def _pair_rows(self, yi, cw, a, b):
        """Positions (ascending), t, c and the slot of every row of the pair (a, b)."""
        idx = np.nonzero((yi == a) | (yi == b))[0]
        first = yi[idx] == a
        return idx, np.where(first, 1.0, -1.0), self.C * cw[yi[idx]], np.where(first, slot_of(a, b), slot_of(b, a))

    def _dev_gamma(self, torch, Zp):
        """gamma from the packed z-scores [n, D] on the device: two-pass float64 sums."""
        if self.gamma == "auto":
            return 1.0 / Zp.shape[1]
        if self.gamma != "scale":
            return float(self.gamma)
        mean = Zp.sum() / Zp.numel()
        var = float((((Zp - mean) ** 2).sum() / Zp.numel()).item())
        return 1.0 / (Zp.shape[1] * var) if var > 0 and np.isfinite(var) else 1.0

    def _dev_state(self, torch, lib, rows, C, cw, mean, scale):
        n, D = rows.n, rows.D
        s0 = self._state0(n, C, D, self.C * cw, mean, scale)
        st = torch.zeros(lib.pinn_ksvm_state_bytes(n, C, D) // 8, dtype=torch.float64, device=rows.dev)
        st[:len(s0)] = torch.from_numpy(s0).to(rows.dev)
        wb = lib.pinn_ksvm_workspace_bytes(n, C, D)
        return st, len(s0), torch.empty(wb, dtype=torch.uint8, device=rows.dev), wb

    def _z_packed(self, torch, rows, mean, scale):
        """The z-scores [n, D] as a packed device tensor, for gamma="scale" and the support vectors.  A gather index outside
        the array reads the nearest row here: torch's indexing would fault on it, the kernels never read such a position and
        flag it, and the fit then raises before anything taken from this copy is used."""
        a = rows.arr
        if rows.ridx is not None:
            if a.shape[0] < 1:
                raise ValueError("X holds no rows")
            a = a[rows.ridx.clamp(0, a.shape[0] - 1)]
        return (a[:, rows.cols] - torch.from_numpy(mean).to(rows.dev)) / torch.from_numpy(scale).to(rows.dev)

    def _fit_device(self, X, y, columns, row_index, scaler):
        torch, _lib, lib = _torch_lib()
        rows, yi, classes, cls_h, count, cw, mean, scale = self._dev_setup(torch, X, y, columns, row_index, scaler)
        with torch.cuda.device(rows.dev):
            C, D, n = len(cw), rows.D, rows.n
            P = C * (C - 1) // 2
            Zp = self._z_packed(torch, rows, mean, scale)
            gamma = self._dev_gamma(torch, Zp)
            if not (gamma > 0 and np.isfinite(gamma)):
                raise ValueError("the kernel SVC failed: %s" % _STATUS_TEXT[KSVM_NAN])
            st, o, ws, wb = self._dev_state(torch, lib, rows, C, cw, mean, scale)
            stream = torch.cuda.current_stream().cuda_stream
            head = rows.head() + (yi, C)
            done, init, limit = 0, 1, self._limit(count)
            while True:
                step = min(self.chunk, limit - done)
                call("pinn_ksvm_smo", *head, gamma, init, step, self.tol, st, None, ws, wb, stream=stream)
                done, init = done + step, 0
                pi = st[_HDR:_HDR + P * _PW].cpu().numpy().view(np.int64).reshape(P, _PW)      # one read of the pair blocks per chunk
                if ((pi[:, _P_CONV] != 0) | (pi[:, _P_STATUS] != 0)).all() or done >= limit:
                    break
            status = int(np.bitwise_or.reduce(pi[:, _P_STATUS]))
            if status:
                raise ValueError("the kernel SVC failed: %s (status %d)" % (_STATUS_TEXT.get(status, "several failures"), status))
            call("pinn_ksvm_finish", *head, st, stream=stream)
            pb = st[_HDR:_HDR + P * _PW].cpu().numpy().reshape(P, _PW)
            pi = pb.view(np.int64)
            alpha = st[o:o + n * (C - 1)].reshape(n, C - 1).clone()
            sup = torch.nonzero((alpha > 0).any(dim=1)).reshape(-1)
            as_tensor = _is_tensor(X)
            self._publish(classes if as_tensor else cls_h, cw, gamma, Zp[sup].cpu().numpy(), sup.cpu().numpy(), alpha[sup].cpu().numpy(),
                          yi[sup].cpu().numpy(), pb[:, _P_RHO].copy(), pi[:, _P_ITER].copy(), pb[:, _P_VIOL].copy(), pb[:, _P_GAP].copy(),
                          (pi[:, _P_CONV] != 0) | ~(pb[:, _P_VIOL] > self.tol), alpha if as_tensor else alpha.cpu().numpy(), yi if as_tensor else yi.cpu().numpy(), count,
                          as_tensor, rows.dev)
        return self

    def working_sets(self, X, y, n_iters, columns=None, row_index=None, scaler=None):
        """The first `n_iters` iterations from alpha = 0, for tests and tools: dict with "log" [P, n_iters, 2] (i and j as row
        positions, -1 once a pair has stopped), "alpha" and "G" [n, C - 1] after them (host arrays), "gamma" and, from the
        host backend, "trace" (see `fit`) and "alpha_abs", "G_abs": the sums of the absolute terms of alpha and G."""
        n_iters = int(n_iters)
        if _pick_backend(self.backend, X) == "host":
            Z, yi, classes, cw, count = self._host_setup(X, y, columns, row_index, scaler)
            C = len(classes)
            gamma = self._gamma_of(Z)
            pairs = pairs_of(C)
            log = np.full((len(pairs), n_iters, 2), -1, dtype=np.int64)
            alpha, Gs, traces = np.zeros((len(yi), C - 1)), np.zeros((len(yi), C - 1)), []
            a_abs, g_abs = np.zeros((len(yi), C - 1)), np.zeros((len(yi), C - 1))
            for p, (a, b) in enumerate(pairs):
                idx, t, c, sl = self._pair_rows(yi, cw, a, b)
                tr, terms = [], (np.zeros(len(idx)), np.ones(len(idx)))
                alpha[idx, sl], Gs[idx, sl], _, _ = _host_smo(Z[idx], t, c, gamma, self.tol, n_iters, idx, tr, terms)
                a_abs[idx, sl], g_abs[idx, sl] = terms
                for k, e in enumerate(tr):
                    log[p, k] = e[0], e[1]
                traces.append(tr)
            return {"log": log, "alpha": alpha, "G": Gs, "gamma": gamma, "trace": traces, "alpha_abs": a_abs, "G_abs": g_abs}
        import torch
        q = self.device_problem(X, y, columns, row_index, scaler)
        st, o, n, C = q["state"], q["alpha_at"], q["n"], q["n_classes"]
        with torch.cuda.device(st.device):
            log = torch.full((C * (C - 1) // 2, n_iters, 2), -1, dtype=torch.int64, device=st.device)
            call("pinn_ksvm_smo", *q["head"], q["gamma"], 1, n_iters, self.tol, st, log, q["ws"], q["ws_bytes"])
            m = n * (C - 1)
            return {"log": log.cpu().numpy(), "alpha": st[o:o + m].reshape(n, C - 1).cpu().numpy(),
                    "G": st[o + m:o + 2 * m].reshape(n, C - 1).cpu().numpy(), "gamma": q["gamma"]}

    def device_problem(self, X, y, columns=None, row_index=None, scaler=None):
        """What a direct call of `pinn_ksvm_smo` needs, for tests and tools: dict with "head" (the entry point's arguments up to
        `n_classes`: the rows read in place, the class index of every row), "gamma", "state" (the state block as `fit` hands
        it to the first call: the pair blocks' classes, the scaler's statistics and the bounds C x class weight; a call with
        init = 1 writes the rest), "alpha_at" (the word at which alpha [n, C - 1] starts, G [n, C - 1] behind it), "ws",
        "ws_bytes", "n", "n_classes", and "rows", which owns the tensors that "head" points into.  Rows and classes are not checked here: the first launch does that."""
        torch, _lib, lib = _torch_lib()
        rows, yi, classes, cls_h, count, cw, mean, scale = self._dev_setup(torch, X, y, columns, row_index, scaler)
        with torch.cuda.device(rows.dev):
            gamma = self._dev_gamma(torch, self._z_packed(torch, rows, mean, scale))
            st, o, ws, wb = self._dev_state(torch, lib, rows, len(cw), cw, mean, scale)
        return {"head": rows.head() + (yi, len(cw)), "gamma": gamma, "state": st, "alpha_at": o, "ws": ws, "ws_bytes": wb,
                "n": rows.n, "n_classes": len(cw), "rows": rows}

    # ---- decision
    def _device_model(self, torch, dev, scaler):
        key = (str(dev), id(scaler))
        if self._model is None or self._model[0] != key:
            stats = None
            if scaler is not None:
                stats = torch.from_numpy(np.concatenate(scaler_stats(scaler, self.n_features_in_))).to(dev)
            self._model = (key, stats, torch.from_numpy(self._sv).to(dev), torch.from_numpy(self._coef).to(dev),
                           torch.from_numpy(self._sv_cls).to(dev), torch.from_numpy(self._rho).to(dev))
        return self._model[1:]

    def _host_values(self, Z):
        return _host_values(Z, self._sv, self._coef, self._sv_cls, self._rho, self._gamma, len(self.class_weight_))

    def _launch_decision(self, torch, rows, scaler, C, out):
        stats, sv, coef, sv_cls, rho = self._device_model(torch, rows.dev, scaler)
        call("pinn_ksvm_decision", *rows.head(), C, stats, sv, coef, sv_cls, sv.shape[0], rho, self._gamma,
             out["decision"], out["votes"], out["pred"])


def build_kernel_svm_classifier(backend="auto", **svc_args):
    """The pipeline script 05 names for Sup_SVM: StandardScaler, then SVC(kernel="rbf", C=0.05, gamma="scale",
    class_weight="balanced"); `named_steps["scaler"]` and `named_steps["svc"]` as svm.build_svm_classifier."""
    svc_args.setdefault("C", 0.05)
    svc_args.setdefault("class_weight", "balanced")
    return SVCPipeline(DeviceStandardScaler(backend=backend), DeviceKernelSVC(backend=backend, **svc_args))


def run_supervised_svm_kernel(X_tr, y_tr, X_te, C=0.05, gamma="scale", backend="auto", **svc_args):
    """Script 05's call of run_supervised_svm_rbf with the kernel its name promises: y_pred [n_te]."""
    return build_kernel_svm_classifier(backend, C=C, gamma=gamma, **svc_args).fit(X_tr, y_tr).predict(X_te)


class KernelSVMDiagnoser(SVMDiagnoser):
    """svm.SVMDiagnoser on a fitted pipeline of build_kernel_svm_classifier: predicted classes chunk by chunk."""
