"""Gaussian-mixture fault diagnosis with label-posterior mapping: the stage that names the fault (reference script 03).

A full-covariance mixture is fitted to the physics residual columns pV, pT, pH, pO of the results array, every component
is calibrated against the labels of the training rows (P(fault | component)), and each row then gets the probability of
flooding, oxygen starvation, membrane drying and hydrogen starvation.  The helpers keep script 03's names, arguments,
defaults and error types: `normalize_feature_spec`, `parse_features`, `parse_group_spec`, `build_label_mapper`,
`extract_X_y`, `fit_gmm_and_get_probabilities`.  Added: `DeviceGMM` (scikit-learn's GaussianMixture arguments and
attributes), `FaultDiagnoser` (online use, chunk by chunk, next to risk.RiskMonitor) and `classification_metrics`.

Two backends, as in risk.py.  "device": the HIP kernels of csrc/pinn_gmm.hip (float64; one EM iteration is a fused row
pass plus a one-workgroup M-step, iterations run without a host synchronisation between them).  "host": plain float64
numpy with scikit-learn's formulas, for machines without a GPU and as the referee of the device tests.  Importing this
module needs numpy only; scikit-learn is never imported.
"""
import re

import numpy as np

from ._device import (_DevRows, _as_numpy, _dev_f64_rows, _dev_vec, _host_rows, _is_tensor, _on_gpu, _pick_backend, _torch_lib,  # noqa: F401
                      call, columns_of)
from .risk import FAULT_ALIASES, INDEX

DEFAULT_GROUP_SPEC = "flooding:1,2,3,|oxygen_starvation:4,5,6,|membrane_drying:7,8,9,|hydrogen_starvation:10,11,12"
DEFAULT_FEATURES = "pV,pT,pH,pO"
TEST_SIZE = 0.25
RANDOM_STATE = 42
REQUIRED_MAX_INDEX = max(INDEX.values())
MAX_COMP, MAX_FEAT, MAX_CLASSES, TILE = 32, 8, 16, 128
EPS10 = 10.0 * np.finfo(np.float64).eps
_HDR = 8                                 # 8-byte words of the device state header (include/pinn_hip.h)


# ---------------------------------------------------------------------------------------------- script 03's helpers
def list_available_features():
    return sorted(INDEX, key=lambda k: INDEX[k])


def normalize_feature_spec(spec):
    """Any of the separators , ; | whitespace and their full-width forms become single commas; `1.2` reads as `1,2`."""
    s = re.sub(r"[，、；;|]+", ",", spec.strip())
    s = re.sub(r"(\d+)\.(\d+)", r"\1,\2", s)
    s = re.sub(r"\s+", ",", s)
    return re.sub(r",+", ",", s).strip(", ")


def parse_features(spec):
    """Column indices of a feature spec (names of INDEX or numbers), first occurrence kept.  KeyError for an unknown
    name, ValueError when the label column is asked for."""
    out = []
    for tok in normalize_feature_spec(spec).split(","):
        if tok == "":
            continue
        if tok.isdigit():
            idx = int(tok)
        elif tok in INDEX:
            idx = INDEX[tok]
        else:
            raise KeyError("unknown feature name %r; available: %s" % (tok, list_available_features()))
        if idx not in out:
            out.append(idx)
    if INDEX["label"] in out:
        raise ValueError("'label' is not allowed as an input feature")
    return out


def parse_group_spec(spec, translate=True):
    """`name:id,id,...|name:...` -> {name: [ids]} in the order given.  With translate=True the reference's Chinese class
    names become the English ones of risk.FAULT_ALIASES.  ValueError for a part without a colon, an id that is not an
    integer, a repeated name, or no group at all."""
    groups = {}
    for part in re.split(r"[|；;]\s*|\n+", spec.strip()):
        if not part.strip():
            continue
        if ":" not in part:
            raise ValueError("group %r has no colon" % part)
        name, ids = part.split(":", 1)
        name = name.strip()
        if translate:
            name = FAULT_ALIASES.get(name, name)
        det = []
        for tok in normalize_feature_spec(ids).split(","):
            if tok == "":
                continue
            if not re.match(r"^-?\d+$", tok):
                raise ValueError("label id %r is not an integer" % tok)
            det.append(int(tok))
        if name in groups:
            raise ValueError("group name %r is repeated" % name)
        groups[name] = det
    if not groups:
        raise ValueError("no group could be parsed")
    return groups


def build_label_mapper(groups):
    """({detailed label: class index}, [class names]); ValueError when a label sits in two groups."""
    names = list(groups)
    mapping = {}
    for ci, name in enumerate(names):
        for det in groups[name]:
            if det in mapping:
                raise ValueError("label %d is in two groups: %r and %r" % (det, names[mapping[det]], name))
            mapping[det] = ci
    return mapping, names


def extract_X_y(results, feature_indices, label_map, return_index=False, backend="auto"):
    """Rows whose label (column 17, truncated to an integer) is a key of `label_map` and whose features are all finite:
    X [n, D] float64 and y [n] class indices (int32 on the host as in the reference, int64 on the device).  A device
    array stays on the device.  With return_index=True also the kept row numbers, ready as a gather list."""
    if _pick_backend(backend, results) == "host":
        arr = _as_numpy(results)
        X_all = arr[:, feature_indices].astype(np.float64)
        with np.errstate(invalid="ignore"):
            det = arr[:, INDEX["label"]].astype(np.int32)
        keys = np.array(sorted(label_map), dtype=np.int64)
        keep = np.isin(det, keys)
        if not keep.any():
            raise ValueError("no rows are left: check the group definition")
        keep &= np.isfinite(X_all).all(axis=1)
        vals = np.array([label_map[int(k)] for k in keys], dtype=np.int32)
        y = vals[np.searchsorted(keys, det[keep])]
        out = (X_all[keep], y)
        return out + (np.flatnonzero(keep),) if return_index else out
    import torch
    arr = _dev_f64_rows(torch, results)
    lab = arr[:, INDEX["label"]]
    det = torch.where(torch.isfinite(lab), lab, torch.full_like(lab, -2.0 ** 31)).to(torch.int64)
    keys = torch.tensor(sorted(label_map), dtype=torch.int64, device=arr.device)
    keep = torch.isin(det, keys)
    if not bool(keep.any()):
        raise ValueError("no rows are left: check the group definition")
    X_all = arr[:, list(feature_indices)]
    keep &= torch.isfinite(X_all).all(dim=1)
    vals = torch.tensor([label_map[int(k)] for k in sorted(label_map)], dtype=torch.int64, device=arr.device)
    y = vals[torch.searchsorted(keys, det[keep])]
    X = X_all[keep].contiguous()
    if not _is_tensor(results):
        out = (X.cpu().numpy(), y.cpu().numpy().astype(np.int32))
        return out + (torch.nonzero(keep).reshape(-1).cpu().numpy(),) if return_index else out
    return (X, y, torch.nonzero(keep).reshape(-1)) if return_index else (X, y)


def classification_metrics(y_true, y_pred, n_classes):
    """Confusion matrix (rows = true class), accuracy and macro precision / recall / F1 with a zero division counted as 0.
    The macro averages run over the classes that occur in y_true or y_pred, as scikit-learn's do."""
    t, p = _as_numpy(y_true).astype(np.int64).reshape(-1), _as_numpy(y_pred).astype(np.int64).reshape(-1)
    if t.shape != p.shape:
        raise ValueError("y_true and y_pred differ in length")
    C = int(n_classes)
    ok = (t >= 0) & (t < C) & (p >= 0) & (p < C)
    cm = np.bincount(t[ok] * C + p[ok], minlength=C * C).reshape(C, C)
    tp = np.diag(cm).astype(float)
    pred_n, true_n = cm.sum(axis=0).astype(float), cm.sum(axis=1).astype(float)
    prec = np.divide(tp, pred_n, out=np.zeros(C), where=pred_n > 0)
    rec = np.divide(tp, true_n, out=np.zeros(C), where=true_n > 0)
    f1 = np.divide(2 * prec * rec, prec + rec, out=np.zeros(C), where=(prec + rec) > 0)
    present = (pred_n + true_n) > 0
    m = (lambda v: float(v[present].mean())) if present.any() else (lambda v: 0.0)
    return {"confusion_matrix": cm, "accuracy": float((t == p).mean()) if t.size else 0.0, "macro_precision": m(prec),
            "macro_recall": m(rec), "macro_f1": m(f1)}


# ---------------------------------------------------------------------------------------------- host backend
def _host_factor(cov):
    """precisions_cholesky (upper triangular, cov = L L^T, U = L^-T) of every covariance; ValueError when one is not
    positive definite."""
    K, D, _ = cov.shape
    out = np.empty_like(cov)
    for k in range(K):
        try:
            L = np.linalg.cholesky(cov[k])
        except np.linalg.LinAlgError:
            raise ValueError("the covariance of component %d is not positive definite: fewer components or a larger "
                             "reg_covar are needed" % k) from None
        out[k] = np.triu(np.linalg.solve(L, np.eye(D)).T)
    return out


def _host_mstep(X, resp, reg_covar):
    """n_k, means, covariances as scikit-learn's _estimate_gaussian_parameters (covariances from x - mean: two passes)."""
    nk = resp.sum(axis=0) + EPS10
    means = resp.T @ X / nk[:, None]
    K, D = means.shape
    cov = np.empty((K, D, D))
    for k in range(K):
        diff = X - means[k]
        cov[k] = (resp[:, k] * diff.T) @ diff / nk[k]
        cov[k].flat[:: D + 1] += reg_covar
    return nk, means, cov


def _host_estep(X, weights, means, pchol):
    """log_prob_norm [n] and responsibilities [n, K] (scikit-learn's formulas; logsumexp as max, sum, log)."""
    n, D = X.shape
    K = means.shape[0]
    lp = np.empty((n, K))
    for k in range(K):
        y = (X - means[k]) @ pchol[k]
        lp[:, k] = -0.5 * (D * np.log(2 * np.pi) + np.sum(y * y, axis=1)) + np.sum(np.log(np.diag(pchol[k])))
    with np.errstate(divide="ignore"):
        lp += np.log(weights)
    m = lp.max(axis=1)
    with np.errstate(invalid="ignore"):
        lpn = np.log(np.exp(lp - m[:, None]).sum(axis=1)) + m
        resp = np.exp(lp - lpn[:, None])
    return lpn, resp


def _n_moments(D):
    return 1 + D + D * (D + 1) // 2


def _host_moments(X, resp, shift):
    """The sums the device accumulates, [K, F] = (sum r, sum r d_i, sum r d_i d_j for i <= j by columns j) with
    d = x - shift_k, and the sums of the absolute terms (the scale of their rounding error)."""
    K, D = shift.shape
    S, A = np.zeros((K, _n_moments(D))), np.zeros((K, _n_moments(D)))
    for k in range(K):
        d, r = X - shift[k], resp[:, k]
        cols = [np.ones_like(r)] + [d[:, i] for i in range(D)] + [d[:, i] * d[:, j] for j in range(D) for i in range(j + 1)]
        for f, c in enumerate(cols):
            S[k, f] = (r * c).sum()
            A[k, f] = np.abs(r * c).sum()
    return S, A


def _host_kmeans(X, centres, n_iters):
    """Lloyd iterations with the device's rules: nearest centre (the first of equals), an empty cluster keeps its centre,
    stop when no centre moves.  Returns centres, labels of the final centres, iterations done."""
    centres = centres.copy()
    it = 0

    def assign(c):
        d2 = np.stack([((X - c[k]) ** 2).sum(axis=1) for k in range(c.shape[0])], axis=1)
        return d2.argmin(axis=1)
    for it in range(1, n_iters + 1):
        lab = assign(centres)
        new = centres.copy()
        for k in range(centres.shape[0]):
            sel = lab == k
            if sel.any():
                new[k] = centres[k] + (X[sel] - centres[k]).sum(axis=0) / sel.sum()
        moved = not np.array_equal(new, centres)
        centres = new
        if not moved:
            break
    return centres, assign(centres), it


def _upper_factor(P):
    """U upper triangular with U U^T = P: the density (x - mu) @ U is the one scikit-learn evaluates with the lower
    factor it takes of precisions_init."""
    try:
        return np.linalg.cholesky(P[::-1, ::-1])[::-1, ::-1]
    except np.linalg.LinAlgError:
        raise ValueError("precisions_init holds a matrix that is not positive definite") from None


# ---------------------------------------------------------------------------------------------- device backend
def _state_words(K, D):
    return _HDR + K * (2 + D + 2 * D * D)


def _pack_state(K, D, weights, means, cov, pchol, n_iter=0, lower=-np.inf):
    s = np.zeros(_state_words(K, D))
    hdr = s[:_HDR].view(np.int64)
    hdr[0], hdr[3], hdr[4] = n_iter, K, D
    s[5], s[6], s[7] = lower, -np.inf, np.inf
    o = _HDR
    for a, cnt in ((weights, K), (means, K * D), (cov, K * D * D), (pchol, K * D * D)):
        s[o:o + cnt] = 0.0 if a is None else np.asarray(a, dtype=np.float64).reshape(-1)
        o += cnt
    if pchol is not None:
        s[o:o + K] = np.log(np.diagonal(np.asarray(pchol, dtype=np.float64).reshape(K, D, D), axis1=1, axis2=2)).sum(axis=1)
    return s


def _unpack_state(s, K, D):
    """dict of views into a state vector (numpy array or tensor)."""
    hdr = s[:_HDR].view(np.int64) if isinstance(s, np.ndarray) else None
    o = _HDR
    out = {}
    for name, shape in (("weights", (K,)), ("means", (K, D)), ("covariances", (K, D, D)), ("precisions_cholesky", (K, D, D))):
        cnt = int(np.prod(shape))
        out[name] = s[o:o + cnt].reshape(shape)
        o += cnt
    if hdr is not None:
        out.update(n_iter=int(hdr[0]), converged=bool(hdr[1]), status=int(hdr[2]), lower_bound=float(s[5]), change=float(s[7]))
    return out


# ---------------------------------------------------------------------------------------------- the mixture
class DeviceGMM:
    """Full-covariance Gaussian mixture with scikit-learn's GaussianMixture arguments, defaults, stopping rule and
    attributes (`weights_, means_, covariances_, precisions_cholesky_, converged_, n_iter_, lower_bound_`).

    Initialisation, in this order of precedence: `resp_init` [n, K] or `labels_init` [n] (what scikit-learn's k-means
    step hands to its first M-step); `weights_init`, `means_init` and `precisions_init` all three; otherwise the package's
    own k-means (k-means++ seeds from a private generator seeded by `random_state`, then Lloyd iterations), whose result
    `weights_init` / `means_init` may override.  The own initialisation does not reproduce scikit-learn's draw for draw.
    `n_init` stays 1: several seeds, and several component counts, are fitted together by `selection.select_gmm`, whose
    criterion="lower_bound" over the seeds of one component count is scikit-learn's n_init rule.

    `fit`, `predict_proba`, `predict`, `score_samples`, `score` take X as a [n, D] array, or any array plus `columns`
    (and `row_index`): the device backend then reads the rows in place.  numpy in -> numpy out, device tensor in ->
    device tensors out."""

    def __init__(self, n_components=1, *, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1,
                 init_params="kmeans", weights_init=None, means_init=None, precisions_init=None, random_state=None,
                 warm_start=False, resp_init=None, labels_init=None, backend="auto", em_chunk=8, kmeans_iter=100):
        if covariance_type != "full":
            raise NotImplementedError("covariance_type=%r: only 'full' is implemented" % (covariance_type,))
        if n_init != 1:
            raise NotImplementedError("n_init > 1 is not implemented here: selection.select_gmm(X, (n_components,), seeds, "
                                      "criterion='lower_bound') fits the seeds in one batch and keeps the best")
        if warm_start:
            raise NotImplementedError("warm_start is not implemented")
        if init_params != "kmeans":
            raise NotImplementedError("init_params=%r: only 'kmeans' is implemented" % (init_params,))
        if backend not in ("auto", "device", "host"):
            raise ValueError("backend must be 'auto', 'device' or 'host'")
        if int(n_components) < 1 or tol < 0 or reg_covar < 0 or int(max_iter) < 0 or int(em_chunk) < 1:
            raise ValueError("n_components >= 1, tol >= 0, reg_covar >= 0, max_iter >= 0 and em_chunk >= 1 are required")
        self.n_components, self.covariance_type, self.tol, self.reg_covar = int(n_components), covariance_type, float(tol), float(reg_covar)
        self.max_iter, self.n_init, self.init_params, self.random_state, self.warm_start = int(max_iter), 1, init_params, random_state, False
        self.weights_init, self.means_init, self.precisions_init = weights_init, means_init, precisions_init
        self.resp_init, self.labels_init = resp_init, labels_init
        self.backend, self.em_chunk, self.kmeans_iter = backend, int(em_chunk), int(kmeans_iter)
        self._state = None               # device state block (device backend)
        self._as_tensor = False

    # ---- shared
    def _check_fitted(self):
        if not hasattr(self, "means_"):
            raise RuntimeError("this DeviceGMM is not fitted yet")

    def _seeds(self, n, first_d2, next_d2):
        """k-means++: `first_d2(i)` starts the running minimum of squared distances from row i, `next_d2(i)` lowers it;
        both return (cumulative sums, total) as host floats are drawn against them."""
        rng = np.random.default_rng(self.random_state)
        picks = [int(rng.integers(n))]
        pick = first_d2(picks[0])
        for _ in range(1, self.n_components):
            picks.append(pick(float(rng.random())))
            pick = next_d2(picks[-1])
        return picks

    def _set_attrs(self, p, n_iter, converged, lower):
        self.weights_, self.means_, self.covariances_ = p["weights"], p["means"], p["covariances"]
        self.precisions_cholesky_ = p["precisions_cholesky"]
        self.n_iter_, self.converged_, self.lower_bound_ = int(n_iter), bool(converged), float(lower)

    def _given(self):
        return self.weights_init is not None and self.means_init is not None and self.precisions_init is not None

    def _given_state(self, K, D):
        w = np.asarray(_as_numpy(self.weights_init), dtype=np.float64).reshape(K)
        mu = np.asarray(_as_numpy(self.means_init), dtype=np.float64).reshape(K, D)
        P = np.asarray(_as_numpy(self.precisions_init), dtype=np.float64).reshape(K, D, D)
        U = np.stack([_upper_factor(P[k]) for k in range(K)])
        return w, mu, np.stack([np.linalg.inv(P[k]) for k in range(K)]), U

    # ---- host
    def _fit_host(self, X):
        n, D = X.shape
        K = self.n_components
        if self.resp_init is not None or self.labels_init is not None or not self._given():
            if self.resp_init is not None:
                resp = np.asarray(_as_numpy(self.resp_init), dtype=np.float64).reshape(n, K)
            else:
                if self.labels_init is not None:
                    lab = _as_numpy(self.labels_init).astype(np.int64).reshape(n)
                else:
                    lab = self._host_own_labels(X)
                resp = np.zeros((n, K))
                ok = (lab >= 0) & (lab < K)
                resp[np.flatnonzero(ok), lab[ok]] = 1.0
            nk, mu, cov = _host_mstep(X, resp, self.reg_covar)
            w = nk / n
            pc = _host_factor(cov)
            if self.resp_init is None and self.labels_init is None:
                if self.weights_init is not None:
                    w = np.asarray(_as_numpy(self.weights_init), dtype=np.float64).reshape(K)
                if self.means_init is not None:
                    mu = np.asarray(_as_numpy(self.means_init), dtype=np.float64).reshape(K, D)
        else:
            w, mu, cov, pc = self._given_state(K, D)
        self._set_attrs({"weights": w, "means": mu, "covariances": cov, "precisions_cholesky": pc}, 0, False, -np.inf)
        self.lower_bound_changes_ = []
        self.em_iterations(X, self.max_iter)
        return self

    def _host_own_labels(self, X):
        n = X.shape[0]
        state = {}

        def start(i):
            state["d2"] = ((X - X[i]) ** 2).sum(axis=1)
            return draw

        def lower(i):
            state["d2"] = np.minimum(state["d2"], ((X - X[i]) ** 2).sum(axis=1))
            return draw

        def draw(u):
            c = np.cumsum(state["d2"])
            return int(min(np.searchsorted(c, u * c[-1], side="right"), n - 1))
        centres = X[self._seeds(n, start, lower)]
        return _host_kmeans(X, centres, self.kmeans_iter)[1]

    # ---- device
    def _ws(self, torch, lib, rows):
        wb = lib.pinn_gmm_workspace_bytes(rows.n, self.n_components, rows.D)
        return torch.empty(wb, dtype=torch.uint8, device=rows.dev), wb

    def _read_state(self, D):
        """One copy of the state block to the host; a set status word raises, as scikit-learn's Cholesky does."""
        s = self._state.cpu().numpy()
        p = _unpack_state(s, self.n_components, D)
        if p["status"] != 0:
            raise ValueError("a covariance is not positive definite (status %d): fewer components or a larger reg_covar "
                             "are needed" % p["status"])
        return p

    def _fit_device(self, X, columns, row_index):
        torch, _lib, lib = _torch_lib()
        rows = _DevRows(torch, X, columns, row_index)
        K, D, n = self.n_components, rows.D, rows.n
        if K > MAX_COMP:
            raise ValueError("the device backend takes at most %d components, got %d" % (MAX_COMP, K))
        if n < 1:
            raise ValueError("X holds no rows")
        with torch.cuda.device(rows.dev):
            stream = torch.cuda.current_stream().cuda_stream
            ws, wb = self._ws(torch, lib, rows)
            self._state = torch.zeros(_state_words(K, D), dtype=torch.float64, device=rows.dev)
            resp = lab = None
            if self.resp_init is not None:
                resp = _dev_vec(torch, self.resp_init, torch.float64, rows.dev)
                if resp.numel() != n * K:
                    raise ValueError("resp_init must be [n, n_components]")
            elif self.labels_init is not None:
                lab = _dev_vec(torch, self.labels_init, torch.int64, rows.dev)
                if lab.numel() != n:
                    raise ValueError("labels_init must hold one label per row")
            elif not self._given():
                lab = self._device_own_labels(torch, _lib, lib, rows, ws, wb, stream)
            if resp is not None or lab is not None:
                call("pinn_gmm_mstep_init", *rows.head(), K, resp, lab, self.reg_covar, self._state, ws, wb, stream=stream)
                if self.resp_init is None and self.labels_init is None and (self.weights_init is not None or self.means_init is not None):
                    p = self._read_state(D)
                    w = p["weights"] if self.weights_init is None else _as_numpy(self.weights_init)
                    mu = p["means"] if self.means_init is None else _as_numpy(self.means_init)
                    self._state = torch.from_numpy(_pack_state(K, D, w, mu, p["covariances"], p["precisions_cholesky"])).to(rows.dev)
            else:
                self._state = torch.from_numpy(_pack_state(K, D, *self._given_state(K, D))).to(rows.dev)
            self._as_tensor = _is_tensor(X)
            self._dims = (K, D)
            self.lower_bound_changes_ = []
            self._run_em(torch, _lib, lib, rows, ws, wb, stream, self.max_iter)
        return self

    def _device_own_labels(self, torch, _lib, lib, rows, ws, wb, stream):
        Xp = rows.packed(torch)
        n = rows.n
        state = {}

        def start(i):
            state["d2"] = ((Xp - Xp[i]) ** 2).sum(dim=1)
            return draw

        def lower(i):
            state["d2"] = torch.minimum(state["d2"], ((Xp - Xp[i]) ** 2).sum(dim=1))
            return draw

        def draw(u):
            c = torch.cumsum(state["d2"], dim=0)
            target = (c[-1] * u).reshape(1)
            return int(min(int(torch.searchsorted(c, target, right=True).item()), n - 1))
        picks = self._seeds(n, start, lower)
        K, D = self.n_components, rows.D
        centres = Xp[torch.tensor(picks, device=rows.dev)].cpu().numpy()
        km = torch.from_numpy(_pack_state(K, D, None, centres, None, None)).to(rows.dev)
        lab = torch.empty(n, dtype=torch.int64, device=rows.dev)
        call("pinn_gmm_kmeans", *rows.head(), K, self.kmeans_iter, km, lab, ws, wb, stream=stream)
        self.kmeans_centres_ = km[_HDR + K:_HDR + K + K * D].reshape(K, D)
        return lab

    def _run_em(self, torch, _lib, lib, rows, ws, wb, stream, n_iters):
        K, D = self._dims
        done, p = 0, None
        while True:
            step = min(self.em_chunk, n_iters - done)
            if step > 0:
                call("pinn_gmm_em", *rows.head(), K, step, self.tol, self.reg_covar, self._state, ws, wb, stream=stream)
                done += step
            p = self._read_state(D)
            if p["converged"] or done >= n_iters:
                break
        self._last_ws = ws
        self._publish(torch, p)

    def _publish(self, torch, p):
        K, D = self._dims
        if self._as_tensor:
            views = _unpack_state(self._state, K, D)
            views = {k: v.clone() for k, v in views.items()}
        else:
            views = {k: p[k].copy() for k in ("weights", "means", "covariances", "precisions_cholesky")}
        self._set_attrs(views, p["n_iter"], p["converged"], p["lower_bound"])

    def _device_state(self, torch, dev, D):
        """The state block on `dev`: the one a device fit left, or one packed from the attributes of a host fit."""
        K = self.n_components
        if self._state is None or self._state.device != dev:
            self._check_fitted()
            if self._state is not None:
                self._state = self._state.to(dev)
            else:
                self._state = torch.from_numpy(_pack_state(K, D, _as_numpy(self.weights_), _as_numpy(self.means_), _as_numpy(self.covariances_),
                                                           _as_numpy(self.precisions_cholesky_), self.n_iter_, self.lower_bound_)).to(dev)
                self._dims = (K, D)
        if self._dims[1] != D:
            raise ValueError("the mixture was fitted on %d features, got %d" % (self._dims[1], D))
        return self._state

    # ---- public
    def fit(self, X, y=None, columns=None, row_index=None):
        if _pick_backend(self.backend, X) == "host":
            self._state, self._as_tensor = None, False
            return self._fit_host(_host_rows(X, columns, row_index))
        return self._fit_device(X, columns, row_index)

    def em_iterations(self, X, n_iters, columns=None, row_index=None, return_moments=False):
        """`n_iters` more EM iterations from the current parameters, with the stopping rule (nothing happens once
        converged_).  With return_moments=True returns the moment sums of the last iteration's pass, [K, F] about the
        means it started from (the host backend returns the pair (sums, sums of absolute terms))."""
        self._check_fitted()
        if _pick_backend(self.backend, X) == "host":
            Xh = _host_rows(X, columns, row_index)
            w, mu, cov, pc = (_as_numpy(a) for a in (self.weights_, self.means_, self.covariances_, self.precisions_cholesky_))
            lower, it, conv, mom = self.lower_bound_, self.n_iter_, self.converged_, None
            for _ in range(n_iters):
                if conv:
                    break
                lpn, resp = _host_estep(Xh, w, mu, pc)
                if return_moments:
                    mom = _host_moments(Xh, resp, mu)
                nk, mu, cov = _host_mstep(Xh, resp, self.reg_covar)
                w = nk / nk.sum()
                pc = _host_factor(cov)
                prev, lower = lower, lpn.mean()
                it += 1
                self.lower_bound_changes_.append(lower - prev)
                conv = abs(lower - prev) < self.tol
            self._state = None
            self._set_attrs({"weights": w, "means": mu, "covariances": cov, "precisions_cholesky": pc}, it, conv, lower)
            return mom
        torch, _lib, lib = _torch_lib()
        rows = _DevRows(torch, X, columns, row_index)
        with torch.cuda.device(rows.dev):
            self._device_state(torch, rows.dev, rows.D)
            self._as_tensor = _is_tensor(X)
            ws, wb = self._ws(torch, lib, rows)
            self._run_em(torch, _lib, lib, rows, ws, wb, torch.cuda.current_stream().cuda_stream, n_iters)
            if return_moments:
                K, D = self._dims
                m = ws[:K * _n_moments(D) * 8].view(torch.float64).reshape(K, _n_moments(D)).clone()
                return m if self._as_tensor else m.cpu().numpy()
        return None

    def _posterior(self, X, columns=None, row_index=None, comp_map=None, want=("resp",)):
        """dict with the wanted of "log_prob_norm", "resp", "y_prob", "y_pred" (the last two need comp_map [K, C])."""
        self._check_fitted()
        K = self.n_components
        if _pick_backend(self.backend, X) == "host":
            Xh = _host_rows(X, columns, row_index)
            lpn, resp = _host_estep(Xh, *(_as_numpy(a) for a in (self.weights_, self.means_, self.precisions_cholesky_)))
            out = {"log_prob_norm": lpn, "resp": resp}
            if comp_map is not None:
                y = np.clip(resp @ _as_numpy(comp_map, np.float64), 1e-12, 1.0)
                y /= y.sum(axis=1, keepdims=True)
                out.update(y_prob=y, y_pred=y.argmax(axis=1))
            return {k: out[k] for k in want}
        torch, _lib, lib = _torch_lib()
        rows = _DevRows(torch, X, columns, row_index)
        with torch.cuda.device(rows.dev):
            st = self._device_state(torch, rows.dev, rows.D)
            cm, C = None, 0
            if comp_map is not None:
                cm = _dev_vec(torch, comp_map, torch.float64, rows.dev)
                C = cm.numel() // K
                if C < 1 or C > MAX_CLASSES or cm.numel() != K * C:
                    raise ValueError("comp_fault_prob must be [n_components, 1..%d classes]" % MAX_CLASSES)
            n = rows.n
            out = {"log_prob_norm": torch.empty(n, dtype=torch.float64, device=rows.dev) if "log_prob_norm" in want else None,
                   "resp": torch.empty(n, K, dtype=torch.float64, device=rows.dev) if "resp" in want else None,
                   "y_prob": torch.empty(n, C, dtype=torch.float64, device=rows.dev) if "y_prob" in want else None,
                   "y_pred": torch.empty(n, dtype=torch.int64, device=rows.dev) if "y_pred" in want else None}
            if (out["y_prob"] is not None or out["y_pred"] is not None) and cm is None:
                raise ValueError("y_prob and y_pred need comp_fault_prob")
            call("pinn_gmm_posterior", *rows.head(), K, st, cm, C, out["log_prob_norm"], out["resp"], out["y_prob"], out["y_pred"])
        if not _is_tensor(X):
            return {k: out[k].cpu().numpy() for k in want}
        return {k: out[k] for k in want}

    def predict_proba(self, X, columns=None, row_index=None):
        return self._posterior(X, columns, row_index, want=("resp",))["resp"]

    def predict(self, X, columns=None, row_index=None):
        return self.predict_proba(X, columns, row_index).argmax(1)

    def score_samples(self, X, columns=None, row_index=None):
        return self._posterior(X, columns, row_index, want=("log_prob_norm",))["log_prob_norm"]

    def score(self, X, y=None, columns=None, row_index=None):
        return float(self.score_samples(X, columns, row_index).mean())

    def label_map(self, X, y, n_classes, columns=None, row_index=None):
        """comp_fault_prob [K, n_classes]: P(fault | component) from the training rows and their classes, normalised per
        component; uniform for a component that no row (of a class in range) uses."""
        self._check_fitted()
        K, C = self.n_components, int(n_classes)
        if C < 1:
            raise ValueError("n_classes must be at least 1")
        if _pick_backend(self.backend, X) == "host":
            resp = self._posterior(X, columns, row_index)["resp"]
            yh = _as_numpy(y).astype(np.int64).reshape(-1)
            cfp = np.zeros((K, C))
            for c in range(C):
                cfp[:, c] = resp[yh == c].sum(axis=0)
            s = cfp.sum(axis=1, keepdims=True)
            return np.where(s > 0, cfp / np.where(s > 0, s, 1.0), 1.0 / C)
        torch, _lib, lib = _torch_lib()
        if C > MAX_CLASSES:
            raise ValueError("the device backend takes at most %d classes" % MAX_CLASSES)
        rows = _DevRows(torch, X, columns, row_index)
        with torch.cuda.device(rows.dev):
            st = self._device_state(torch, rows.dev, rows.D)
            cls = _dev_vec(torch, y, torch.int64, rows.dev)
            if cls.numel() != rows.n:
                raise ValueError("y must hold one class per row")
            ws, wb = self._ws(torch, lib, rows)
            out = torch.empty(K, C, dtype=torch.float64, device=rows.dev)
            call("pinn_gmm_label_map", *rows.head(), K, st, cls, C, out, ws, wb)
        return out if _is_tensor(X) else out.cpu().numpy()

    def diagnose(self, X, comp_fault_prob, columns=None, row_index=None):
        """(y_prob [n, C], y_pred [n]) of rows under a label map."""
        r = self._posterior(X, columns, row_index, comp_map=comp_fault_prob, want=("y_prob", "y_pred"))
        return r["y_prob"], r["y_pred"]


def fit_gmm_and_get_probabilities(X_tr, y_tr, X_te, n_classes, random_state=42, n_components=None, backend="auto", **gmm_args):
    """Fit the mixture on X_tr, calibrate every component against y_tr, diagnose X_te (03:360-426).
    Returns (y_prob [n_te, n_classes], y_pred [n_te], gmm, comp_fault_prob [n_components, n_classes]).
    `gmm_args`: further DeviceGMM arguments (labels_init, resp_init, means_init, tol, ...)."""
    if n_components is None:
        n_components = n_classes
    gmm = DeviceGMM(n_components=n_components, covariance_type="full", random_state=random_state, backend=backend, **gmm_args)
    gmm.fit(X_tr)
    comp_fault_prob = gmm.label_map(X_tr, y_tr, n_classes)
    y_prob, y_pred = gmm.diagnose(X_te, comp_fault_prob)
    return y_prob, y_pred, gmm, comp_fault_prob


class FaultDiagnoser:
    """Fault probabilities chunk by chunk: `update(rows)` takes the next rows of the results array [n, >= 17] (device
    tensor, or a host array) and returns (y_prob, y_pred) for them.  On the device a chunk is one kernel launch that reads
    the feature columns in place; it can run next to risk.RiskMonitor on the same chunk."""

    def __init__(self, gmm, comp_fault_prob, features=DEFAULT_FEATURES, backend="auto"):
        gmm._check_fitted()
        self.gmm, self.comp_fault_prob = gmm, comp_fault_prob
        self.columns = columns_of(features, parse_features)
        self.backend = backend
        self.n_seen = 0

    def update(self, rows):
        saved = self.gmm.backend
        self.gmm.backend = self.backend if self.backend != "auto" else saved
        try:
            if _on_gpu(rows) and not _is_tensor(self.comp_fault_prob):
                import torch
                self.comp_fault_prob = torch.from_numpy(np.ascontiguousarray(_as_numpy(self.comp_fault_prob, np.float64))).to(rows.device)
            out = self.gmm.diagnose(rows, self.comp_fault_prob, columns=self.columns)
        finally:
            self.gmm.backend = saved
        self.n_seen += int(rows.shape[0])
        return out
