"""Exact Shapley attributions: which residual made the diagnosis say "flooding, 0.93", which sensor moved the voltage.

f is a model with D <= 8 inputs and C <= 16 outputs, the background a set of B rows b.  The value of a coalition S of inputs
at a row x is the interventional (marginal) one,

    v(S; x) = (1 / B) sum over b of f(z),   z_i = x_i for i in S, b_i otherwise,

and the attribution of input j is phi_j(x) = sum over S without j of |S|! (D - |S| - 1)! / D! (v(S + j) - v(S)).  With at
most 2^8 coalitions all of them are enumerated: nothing is sampled.  base = v(none) is the mean prediction over the
background, fx = v(all) = f(x), and sum_j phi_j = fx - base (efficiency).  Written as phi_j = sum_S c_j(S) v(S) the absolute
coefficients sum to 2, so an error of at most delta in every model evaluation moves every phi by at most 2 delta.

`shapley_diagnosis` explains the fault probabilities of a fitted diagnosis.DeviceGMM with one fused kernel
(csrc/pinn_shap.hip: no hybrid row reaches memory); `shapley_values` explains any callable, in chunks of hybrid rows that
one kernel writes and another reduces, with the caller's model between them; `voltage_predictor` makes that callable from
a PhysicsInformedNN; `DiagnosisExplainer` is the online form next to diagnosis.FaultDiagnoser.  All return `Shapley(phi
[n, D, C], base [C], fx [n, C])` in float64.

Two backends, as in diagnosis.py: "device" (the HIP kernels) and "host" (float64 numpy, the subset formula, for machines
without a GPU); "auto" keeps a device tensor on the device.  A host array in gives numpy out.  Every sum has a fixed order:
the same call gives the same bytes, and a row's bytes do not depend on the other rows of the call or on the chunking.
Importing this module needs numpy only; neither scikit-learn nor an attribution library is imported.
"""
import collections
import math

import numpy as np

from ._device import _DevRows, _as_numpy, _dev_vec, _host_rows, _is_tensor, _on_gpu, _pick_backend, _torch_lib, call, columns_of
from .diagnosis import DEFAULT_FEATURES, parse_features

MAX_FEAT, MAX_CLASSES = 8, 16
TILE, BG_BLOCK, MAX_SPLIT = 128, 32, 32          # include/pinn_hip.h: PINN_SHAP_TILE, _BG_BLOCK, _MAX_SPLIT
MAX_WORKSPACE = 1 << 28                          # bytes of split sums one fused call may ask for; more rows go in several calls

Shapley = collections.namedtuple("Shapley", "phi base fx")


def coalition_weights(D):
    """c [D, 2^D]: phi_j = sum over S of c[j, S] v(S); bit i of S says whether input i is in the coalition."""
    f = math.factorial
    c = np.empty((D, 1 << D))
    for S in range(1 << D):
        s = bin(S).count("1")
        for j in range(D):
            c[j, S] = f(s - 1) * f(D - s) / f(D) if (S >> j) & 1 else -(f(s) * f(D - s - 1) / f(D))
    return c


def _check_dims(D, B):
    if not 1 <= D <= MAX_FEAT:
        raise ValueError("exact attributions take 1 to %d features, got %d" % (MAX_FEAT, D))
    if B < 1:
        raise ValueError("the background holds no rows")


def _check_outputs(F, m, where):
    """The model's outputs on m hybrid rows as [m, C]; ValueError for any other shape or more than 16 outputs."""
    shape = tuple(F.shape)
    if len(shape) == 1 and shape[0] == m:
        F = F.reshape(m, 1)
    elif len(shape) != 2 or shape[0] != m or shape[1] < 1:
        raise ValueError("predict returned shape %r for %d rows (%s): [m, C] or [m] is needed" % (shape, m, where))
    if F.shape[1] > MAX_CLASSES:
        raise ValueError("predict returned %d outputs, at most %d are taken" % (F.shape[1], MAX_CLASSES))
    return F


def _rows_per_chunk(D, B, max_hybrid_rows):
    return max(1, int(max_hybrid_rows) // ((1 << D) * B))


# ---------------------------------------------------------------------------------------------- host backend
def _host_shapley(predict, X, Bg, dtype, max_hybrid_rows):
    n, D = X.shape
    B, nS = Bg.shape[0], 1 << D
    coef = coalition_weights(D)
    masks = ((np.arange(nS)[:, None] >> np.arange(D)[None, :]) & 1).astype(bool)
    step = _rows_per_chunk(D, B, max_hybrid_rows)
    phi = base = fx = None
    for r0 in range(0, n, step):
        m = min(step, n - r0)
        H = np.where(masks[None, :, None, :], X[r0:r0 + m, None, None, :], Bg[None, None, :, :]).reshape(m * nS * B, D).astype(dtype)
        F = np.asarray(_check_outputs(_as_numpy(predict(H)), m * nS * B, "host backend"), dtype=np.float64)
        C = F.shape[1]
        F = F.reshape(m, nS, B, C)
        if phi is None:
            phi, fx = np.empty((n, D, C)), np.empty((n, C))
        v = np.zeros((m, nS, C))
        for b in range(B):                                   # background rows in order, as the device
            v += F[:, :, b, :]
        v /= B
        v[:, nS - 1, :] = F[:, nS - 1, 0, :]                 # the full coalition is the row itself: f(x), not a mean of B copies
        p = np.zeros((m, D, C))
        for S in range(nS):                                  # coalitions in order
            p += coef[None, :, S, None] * v[:, None, S, :]
        phi[r0:r0 + m], fx[r0:r0 + m] = p, v[:, nS - 1, :]
        if base is None:
            base = v[0, 0, :].copy()
    return Shapley(phi, base, fx)


def _finite_background(Bg):
    if not np.isfinite(Bg).all():
        raise ValueError("the background holds values that are not finite")


# ---------------------------------------------------------------------------------------------- device backend
def _dev_pair(torch, X, background, columns, row_index, background_index, background_columns):
    rows = _DevRows(torch, X, columns, row_index)
    bgr = _dev_background(torch, background, columns if background_columns is None else background_columns, background_index, rows.dev)
    if bgr.D != rows.D:
        raise ValueError("rows have %d features and the background %d" % (rows.D, bgr.D))
    return rows, bgr


def _dev_background(torch, background, columns, background_index, dev):
    """The background as rows read in place on `dev`, checked once: ValueError when a row read holds a value that is not
    finite or the gather list leaves the array."""
    if _is_tensor(background) and background.device != dev:
        background = background.to(dev)
    with torch.cuda.device(dev):
        bgr = _DevRows(torch, background, columns, background_index)
        if bgr.n < 1:
            raise ValueError("the background holds no rows")
        if bgr.ridx is not None and (int(bgr.ridx.min()) < 0 or int(bgr.ridx.max()) >= bgr.arr.shape[0]):
            raise ValueError("background_index leaves the background array")
        if not bool(torch.isfinite(bgr.packed(torch)).all()):
            raise ValueError("the background holds values that are not finite")
    return bgr


def _head_slice(rows, r0, m):
    """The row head of positions r0 .. r0 + m - 1 of `rows`."""
    arr, ld, n_arr, cols, D, ridx, _ = rows.head()
    if rows.ridx is not None:
        return (arr, ld, n_arr, cols, D, ridx + 8 * r0, m)
    return (arr + 8 * ld * r0, ld, n_arr - r0, cols, D, None, m)


def _device_shapley(torch, predict, rows, bgr, dtype, max_hybrid_rows):
    n, D, B = rows.n, rows.D, bgr.n
    nS = 1 << D
    tdt = torch.float64 if dtype == "float64" else torch.float32
    step = _rows_per_chunk(D, B, max_hybrid_rows)
    with torch.cuda.device(rows.dev):
        H = torch.empty(min(step, n) * nS * B, D, dtype=tdt, device=rows.dev)
        phi = base = fx = None
        for r0 in range(0, n, step):
            m = min(step, n - r0)
            Hc = H[:m * nS * B]
            call("pinn_shap_hybrid", *rows.head(), *bgr.head(), r0, m, int(tdt == torch.float64), Hc)
            F = predict(Hc)
            if not _is_tensor(F):
                F = torch.from_numpy(np.ascontiguousarray(_as_numpy(F))).to(rows.dev)
            F = _check_outputs(F.detach(), m * nS * B, "device backend")
            F = F.to(rows.dev, F.dtype if F.dtype in (torch.float32, torch.float64) else torch.float64).contiguous()
            C = F.shape[1]
            if phi is None:
                phi = torch.empty(n, D, C, dtype=torch.float64, device=rows.dev)
                fx = torch.empty(n, C, dtype=torch.float64, device=rows.dev)
                base = torch.empty(C, dtype=torch.float64, device=rows.dev)
            elif C != phi.shape[2]:
                raise ValueError("predict returned %d outputs, then %d" % (phi.shape[2], C))
            call("pinn_shap_reduce", F, int(F.dtype == torch.float64), m, D, B, C, phi[r0:], base if r0 == 0 else None, fx[r0:])
    return Shapley(phi, base, fx)


def _device_diagnosis(torch, lib, gmm, comp_fault_prob, rows, bgr):
    K, D, n, B = gmm.n_components, rows.D, rows.n, bgr.n
    with torch.cuda.device(rows.dev):
        st = gmm._device_state(torch, rows.dev, D)
        cm = _dev_vec(torch, comp_fault_prob, torch.float64, rows.dev)
        C = cm.numel() // K
        if C < 1 or C > MAX_CLASSES or cm.numel() != K * C:
            raise ValueError("comp_fault_prob must be [n_components, 1..%d classes]" % MAX_CLASSES)
        phi = torch.empty(n, D, C, dtype=torch.float64, device=rows.dev)
        fx = torch.empty(n, C, dtype=torch.float64, device=rows.dev)
        base = torch.empty(C, dtype=torch.float64, device=rows.dev)
        splits = min((B + BG_BLOCK - 1) // BG_BLOCK, MAX_SPLIT)
        step = max(TILE, MAX_WORKSPACE // (splits * D * C * 8) // TILE * TILE)
        wb = lib.pinn_shap_gmm_workspace_bytes(min(step, n), B, D, C)
        ws = torch.empty(wb, dtype=torch.uint8, device=rows.dev)
        for r0 in range(0, n, step):                         # one call, unless the split sums would pass MAX_WORKSPACE
            m = min(step, n - r0)
            call("pinn_shap_gmm", *_head_slice(rows, r0, m), *bgr.head(), K, st, cm, C, phi[r0:], base, fx[r0:], ws, wb)
    return Shapley(phi, base, fx)


def _to_host(r):
    return Shapley(*(a.cpu().numpy() for a in r))


# ---------------------------------------------------------------------------------------------- public
def shapley_values(predict, X, background, columns=None, row_index=None, background_index=None, dtype="float64",
                   max_hybrid_rows=1 << 22, backend="auto", background_columns=None):
    """Exact attributions of any model: `predict` maps hybrid rows [m, D] (`dtype`: "float64" or "float32"; a device tensor
    on the device backend, a numpy array on the host backend) to [m, C] or [m].  X and background are [n, D] and [B, D], or any
    arrays plus `columns` (and `row_index` / `background_index`, gather lists; `background_columns` when the background's
    columns differ): the device backend reads them in place.  Rows go in chunks of at most `max_hybrid_rows` hybrid rows
    (at least one row); the layout of a chunk is row-major over (row, coalition, background).  Returns Shapley(phi, base, fx).

    ValueError: more than 8 features, more than 16 outputs, an output shape other than [m, C] or [m], an empty background
    or one with a value that is not finite, a dtype other than the two."""
    if dtype not in ("float64", "float32"):
        raise ValueError("dtype must be 'float64' or 'float32'")
    if _pick_backend(backend, X) == "host":
        Xh = _host_rows(X, columns, row_index)
        Bg = _host_rows(background, columns if background_columns is None else background_columns, background_index)
        if Xh.shape[1] != Bg.shape[1]:
            raise ValueError("rows have %d features and the background %d" % (Xh.shape[1], Bg.shape[1]))
        _check_dims(Xh.shape[1], Bg.shape[0])
        _finite_background(Bg)
        return _host_shapley(predict, Xh, Bg, np.dtype(dtype), max_hybrid_rows)
    D = len(columns) if columns is not None else int(np.shape(X)[1])
    _check_dims(D, 1)
    torch, _lib, lib = _torch_lib()
    rows, bgr = _dev_pair(torch, X, background, columns, row_index, background_index, background_columns)
    if rows.n < 1:
        raise ValueError("X holds no rows")
    r = _device_shapley(torch, predict, rows, bgr, dtype, max_hybrid_rows)
    return r if _is_tensor(X) else _to_host(r)


def shapley_diagnosis(gmm, comp_fault_prob, X, background, columns=None, row_index=None, background_index=None, backend="auto",
                      background_columns=None):
    """Exact attributions of the fault probabilities `gmm.diagnose(., comp_fault_prob)` to the D residual columns: on the
    device one fused call (the coalitions are walked on-chip; fx is the y_prob of pinn_gmm_posterior), on the host
    `shapley_values` of the host diagnosis.  Arguments as `shapley_values`.  Returns Shapley(phi [n, D, C], base [C], fx [n, C]).
    ValueError as `shapley_values`, and for a comp_fault_prob that is not [n_components, 1..16]."""
    gmm._check_fitted()
    if _pick_backend(backend, X) == "host":
        return shapley_values(_host_diagnosis(gmm, comp_fault_prob), X, background, columns, row_index, background_index, "float64",
                              backend="host", background_columns=background_columns)
    D = len(columns) if columns is not None else int(np.shape(X)[1])
    _check_dims(D, 1)
    torch, _lib, lib = _torch_lib()
    rows, bgr = _dev_pair(torch, X, background, columns, row_index, background_index, background_columns)
    if rows.n < 1:
        raise ValueError("X holds no rows")
    r = _device_diagnosis(torch, lib, gmm, comp_fault_prob, rows, bgr)
    return r if _is_tensor(X) else _to_host(r)


def _host_diagnosis(gmm, comp_fault_prob):
    cfp = _as_numpy(comp_fault_prob, np.float64)

    def predict(Z):
        saved, gmm.backend = gmm.backend, "host"
        try:
            return gmm.diagnose(Z, cfp)[0]
        finally:
            gmm.backend = saved
    return predict


def voltage_predictor(model, outputs=("u", "logvar")):
    """A `predict` for `shapley_values` from a PhysicsInformedNN: float32 rows [m, 8] (normalised sensors) -> [m, len(outputs)]
    of `model.net_u` in eval mode (dropout off), for every kernel family of the forward; the network's train / eval mode is
    put back afterwards.  `outputs`: any of "u" (the voltage) and "logvar".  ValueError for another name or none."""
    outputs = tuple(outputs)
    if not outputs or any(o not in ("u", "logvar") for o in outputs):
        raise ValueError("outputs must name 'u' and / or 'logvar'")

    def predict(Z):
        import torch
        was = model.dnn.training
        model.dnn.eval()
        try:
            with torch.no_grad():
                u, lv = model.net_u(Z.to(torch.float32))
        finally:
            model.dnn.train(was)
        got = {"u": u.reshape(-1, 1), "logvar": lv.reshape(-1, 1)}
        return torch.cat([got[o] for o in outputs], dim=1)
    return predict


class DiagnosisExplainer:
    """Attributions chunk by chunk, next to diagnosis.FaultDiagnoser: `update(rows)` takes the next rows of the results array
    [n, >= 17] (device tensor, or a host array) and returns (phi [n, D, C], y_prob [n, C]) for them; y_prob is what
    FaultDiagnoser.update returns.  `background`: rows of a results array, or the feature columns alone [B, D].  It is checked
    and uploaded once; on the device a chunk is one library call that reads the feature columns in place.  `base` holds the mean
    prediction over the background after the first chunk."""

    def __init__(self, gmm, comp_fault_prob, background, features=DEFAULT_FEATURES, backend="auto"):
        gmm._check_fitted()
        if backend not in ("auto", "device", "host"):
            raise ValueError("backend must be 'auto', 'device' or 'host'")
        self.gmm, self.comp_fault_prob, self.backend = gmm, comp_fault_prob, backend
        self.columns = columns_of(features, parse_features)
        packed = int(np.shape(background)[1]) == len(self.columns)
        self._bg_columns = list(range(len(self.columns))) if packed else self.columns
        self._bg_host = _host_rows(background, self._bg_columns)
        _check_dims(len(self.columns), self._bg_host.shape[0])
        _finite_background(self._bg_host)
        self._bg_src = background if _on_gpu(background) else None
        self._bgr = None
        self.base, self.n_seen = None, 0

    def update(self, rows):
        if _pick_backend(self.backend, rows) == "host":
            r = shapley_diagnosis(self.gmm, self.comp_fault_prob, rows, self._bg_host, columns=self.columns, backend="host",
                                  background_columns=list(range(len(self.columns))))
        else:
            torch, _lib, lib = _torch_lib()
            dr = _DevRows(torch, rows, self.columns)
            if dr.n < 1:
                raise ValueError("the chunk holds no rows")
            if self._bgr is None or self._bgr.dev != dr.dev:
                if self._bg_src is not None:
                    self._bgr = _dev_background(torch, self._bg_src, self._bg_columns, None, dr.dev)
                else:
                    self._bgr = _dev_background(torch, torch.from_numpy(self._bg_host).to(dr.dev), None, None, dr.dev)
                self.comp_fault_prob = _dev_vec(torch, self.comp_fault_prob, torch.float64, dr.dev).reshape(self.gmm.n_components, -1)
            r = _device_diagnosis(torch, lib, self.gmm, self.comp_fault_prob, dr, self._bgr)
            if not _is_tensor(rows):
                r = _to_host(r)
        self.base = r.base
        self.n_seen += int(rows.shape[0])
        return r.phi, r.fx


def global_importance(phi):
    """The mean of |phi| over rows: [D, C]."""
    return phi.abs().mean(dim=0) if _is_tensor(phi) else np.abs(np.asarray(phi)).mean(axis=0)


def top_features(phi, feature_names, class_names, topn=3, verbose=False):
    """Per class the `topn` features by mean |phi| and, by the mean of phi itself, the most positive and most negative ones:
    [{"class", "importance", "positive", "negative"}] with (feature name, value) pairs, shaped as the lists of
    detection.explain_coefficients.  `phi`: [n, D, C]."""
    if topn <= 0:
        return []
    p = _as_numpy(phi, np.float64)
    if p.ndim != 3 or p.shape[1] != len(feature_names):
        raise ValueError("phi must be [n, %d, C]" % len(feature_names))
    imp, mean = np.abs(p).mean(axis=0), p.mean(axis=0)
    out = []
    for c in range(p.shape[2]):
        cname = class_names[c] if c < len(class_names) else str(c)
        top = [(feature_names[i], float(imp[i, c])) for i in np.argsort(-imp[:, c], kind="stable")[:topn]]
        pos = [(feature_names[i], float(mean[i, c])) for i in np.argsort(-mean[:, c], kind="stable")[:topn]]
        neg = [(feature_names[i], float(mean[i, c])) for i in np.argsort(mean[:, c], kind="stable")[:topn]]
        out.append({"class": cname, "importance": top, "positive": pos, "negative": neg})
        if verbose:
            print("- class[%d] %s:" % (c, cname))
            print("  top %d by mean |phi|: " % topn + ", ".join("%s(%.4f)" % t for t in top))
    return out
