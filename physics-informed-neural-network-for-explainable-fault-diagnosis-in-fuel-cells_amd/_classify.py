"""What the supervised classifiers share around their solvers: detection.DeviceLogisticRegression, svm.DeviceLinearSVC and
ksvm.DeviceKernelSVC.  Plain functions for all three (the scaler's statistics, the class set-up on the host and on the
device, the dict of wanted outputs, labels from class indices), and `OneVsOneSVC`, the base of the two SVCs: constructor
checks, class weights, pairs and slots, the state block's prefix, votes from pairwise values and the decision shell.  A
subclass supplies its solver, its model and two hooks: `_host_values` and `_launch_decision`.  Integers, indices and
plumbing only: every sum stays with its solver.  The device twin of the pair helpers is csrc/pinn_ovo.h.

Importing this module needs numpy only.
"""
import numpy as np

from ._device import _DevRows, _as_numpy, _dev_vec, _host_rows, _is_tensor, _pick_backend, _torch_lib


def scaler_stats(scaler, D):
    """(mean, scale) [D] of a fitted DeviceStandardScaler as host arrays; zeros and ones without one."""
    if scaler is None:
        return np.zeros(D), np.ones(D)
    mean, scale = _as_numpy(scaler.mean_, np.float64).reshape(-1), _as_numpy(scaler.scale_, np.float64).reshape(-1)
    if mean.size != D:
        raise ValueError("the scaler was fitted on %d features, got %d" % (mean.size, D))
    return mean, scale


def labels_of(classes, pred):
    """classes[pred]: class indices to labels, numpy or torch as `pred` is."""
    if _is_tensor(pred):
        import torch
        c = classes if _is_tensor(classes) else torch.from_numpy(np.asarray(classes))
        return (c if c.device == pred.device else c.to(pred.device))[pred]
    return _as_numpy(classes)[pred]


def host_classes(y, n_rows, too_few):
    """(classes, class index per row, rows per class) of the labels `y`, one per row.  `too_few(classes)` words the error for
    fewer than two classes."""
    yh = _as_numpy(y).reshape(-1)
    if yh.shape[0] != n_rows:
        raise ValueError("y must hold one class per row")
    classes, yi = np.unique(yh, return_inverse=True)
    if len(classes) < 2:
        raise ValueError(too_few(classes))
    return classes, yi, np.bincount(yi, minlength=len(classes))


def dev_classes(torch, y, rows, too_few):
    """host_classes on the device of `rows`: three device tensors; `too_few` gets the classes as a list."""
    yt = _dev_vec(torch, y, torch.int64, rows.dev)
    if yt.numel() != rows.n:
        raise ValueError("y must hold one class per row")
    classes = torch.unique(yt)
    if classes.numel() < 2:
        raise ValueError(too_few(classes.tolist()))
    yi = torch.searchsorted(classes, yt).contiguous()
    return classes, yi, torch.bincount(yi, minlength=int(classes.numel()))


def wanted_outputs(torch, X, dev, spec, want, launch, *args):
    """The entries `want` of a launch's optional outputs.  `spec`: {name: (shape, dtype)}; only the wanted are allocated,
    `launch(*args, out)` gets the dict with None for the others, and a host array `X` gets numpy back."""
    out = dict.fromkeys(spec)
    for k in want:
        out[k] = torch.empty(spec[k][0], dtype=spec[k][1], device=dev)
    launch(*args, out)
    return {k: out[k] if _is_tensor(X) else out[k].cpu().numpy() for k in want}


def pairs_of(C):
    """[(a, b)] with a < b in scikit-learn's order."""
    return [(a, b) for a in range(C) for b in range(a + 1, C)]


def slot_of(k, other):
    """The slot of class `other` in a row of class k: the other classes in increasing order."""
    return other if other < k else other - 1


def votes_of(dec, C):
    """(votes [n, C], prediction [n]) from pairwise values [n, P]: a vote for a where the value is > 0, else for b; the
    first maximum wins."""
    votes = np.zeros((dec.shape[0], C), dtype=np.int64)
    for p, (a, b) in enumerate(pairs_of(C)):
        pos = dec[:, p] > 0
        votes[:, a] += pos
        votes[:, b] += ~pos
    return votes, votes.argmax(axis=1).astype(np.int64)


def ovr_decision_function(dec_ovo, C):
    """scikit-learn's _ovr_decision_function as SVC calls it: per class the votes (a where the value is >= 0) plus the summed
    confidences squashed into (-1/3, 1/3).  numpy or torch."""
    cols = []
    for k in range(C):
        v = 0.0 * dec_ovo[:, 0]
        conf = 0.0 * dec_ovo[:, 0]
        for p, (a, b) in enumerate(pairs_of(C)):
            if a == k:
                v, conf = v + (dec_ovo[:, p] >= 0) * 1.0, conf + dec_ovo[:, p]
            elif b == k:
                v, conf = v + (dec_ovo[:, p] < 0) * 1.0, conf - dec_ovo[:, p]
        cols.append(v + conf / (3.0 * (abs(conf) + 1.0)))
    if _is_tensor(dec_ovo):
        import torch
        return torch.stack(cols, dim=1)
    return np.stack(cols, axis=1)


def _too_few_svc(classes):
    return "the number of classes has to be greater than one; got %d class" % len(classes)


class OneVsOneSVC:
    """Base of the one-vs-one SVCs.  A subclass sets `_FITTED` (the attribute that `fit` leaves), `_NOT_FINITE` (its message
    for rows that are not finite), `_LAYOUT` (its state block: header words, words of a pair block, the words of a and b in
    it, the header word of C; D, P and n follow C) and `_check_limits(D, C)`."""

    def __init__(self, C, class_weight, max_iter, decision_function_shape, break_ties, random_state, backend, chunk, tol_name, tol):
        if break_ties:
            raise NotImplementedError("break_ties=True is not implemented")
        if decision_function_shape not in ("ovr", "ovo"):
            raise ValueError("decision_function_shape must be 'ovr' or 'ovo'")
        if backend not in ("auto", "device", "host"):
            raise ValueError("backend must be 'auto', 'device' or 'host'")
        if not (isinstance(class_weight, dict) or class_weight in (None, "balanced")):
            raise ValueError("class_weight must be None, 'balanced' or a dict")
        if not C > 0 or not np.isfinite(C) or not tol > 0 or int(chunk) < 1 or (int(max_iter) < 1 and int(max_iter) != -1):
            raise ValueError("C > 0, %s > 0, chunk >= 1 and max_iter >= 1 (or -1) are required" % tol_name)
        self.C, self.class_weight, self.max_iter, self.decision_function_shape = float(C), class_weight, int(max_iter), decision_function_shape
        self.break_ties, self.random_state, self.backend, self.chunk = False, random_state, backend, int(chunk)
        self._model = None               # the model's device tensors, by device and scaler

    def _check_fitted(self):
        if not hasattr(self, self._FITTED):
            raise RuntimeError("this %s is not fitted yet" % type(self).__name__)

    def _weights(self, classes, count):
        C, n = len(classes), int(count.sum())
        if (count < 1).any():
            raise ValueError("a class without rows cannot be fitted")
        if self.class_weight is None:
            return np.ones(C)
        if isinstance(self.class_weight, dict):
            return np.array([float(self.class_weight.get(k.item() if hasattr(k, "item") else k, 1.0)) for k in classes])
        return n / (C * count.astype(np.float64))

    def pair_alpha(self, a, b):
        """(row positions, alpha) of the pair of class indices a < b, positions into the rows `fit` was given."""
        self._check_fitted()
        a, b = int(a), int(b)
        if not 0 <= a < b < len(self.class_weight_):
            raise ValueError("a < b must be class indices")
        yi, al = self._yi, self.alpha_
        if _is_tensor(al):
            import torch
            ia, ib = torch.nonzero(yi == a).reshape(-1), torch.nonzero(yi == b).reshape(-1)
            pos, order = torch.sort(torch.cat([ia, ib]))
            return pos, torch.cat([al[ia, slot_of(a, b)], al[ib, slot_of(b, a)]])[order]
        ia, ib = np.nonzero(yi == a)[0], np.nonzero(yi == b)[0]
        pos = np.concatenate([ia, ib])
        order = np.argsort(pos, kind="stable")
        return pos[order], np.concatenate([al[ia, slot_of(a, b)], al[ib, slot_of(b, a)]])[order]

    # ---- set-up
    def _host_setup(self, X, y, columns, row_index, scaler):
        """The z-scores [n, D], class indices, classes, class weights and rows per class."""
        Xh = _host_rows(X, columns, row_index)
        classes, yi, count = host_classes(y, Xh.shape[0], _too_few_svc)
        self._check_limits(Xh.shape[1], len(classes))
        mean, scale = scaler_stats(scaler, Xh.shape[1])
        cw = self._weights(classes, count)
        if not np.isfinite(Xh).all():
            raise ValueError(self._NOT_FINITE)
        return (Xh - mean) / scale, yi, classes, cw, count

    def _dev_setup(self, torch, X, y, columns, row_index, scaler):
        """The rows read in place, class indices, the classes (device and host), their counts and weights, the scaler's statistics."""
        rows = _DevRows.within(torch, X, columns, row_index, lambda D: self._check_limits(D, 2))
        if rows.n < 1:
            raise ValueError("X holds no rows")
        classes, yi, count = dev_classes(torch, y, rows, _too_few_svc)
        self._check_limits(rows.D, int(classes.numel()))
        count, cls_h = count.cpu().numpy(), classes.cpu().numpy()
        cw = self._weights(cls_h, count)
        mean, scale = scaler_stats(scaler, rows.D)
        return rows, yi, classes, cls_h, count, cw, mean, scale

    def _state0(self, n, C, D, bound, mean, scale):
        """What both state blocks start with: C, D, P, n in the header, (a, b) of every pair block, then mean [D], scale [D] and
        bound [C] (C x class weight)."""
        hdr, pw, p_a, p_b, st_c = self._LAYOUT
        pairs = pairs_of(C)
        o = hdr + len(pairs) * pw
        s0 = np.zeros(o + 2 * D + C)
        hi = s0.view(np.int64)
        hi[st_c:st_c + 4] = C, D, len(pairs), n
        for p, (a, b) in enumerate(pairs):
            hi[hdr + p * pw + p_a], hi[hdr + p * pw + p_b] = a, b
        s0[o:o + D], s0[o + D:o + 2 * D], s0[o + 2 * D:] = mean, scale, bound
        return s0

    # ---- decision
    def _decide(self, X, columns=None, row_index=None, scaler=None, want=("pred",)):
        """dict with the wanted of "decision" [n, P], "votes" [n, C] and "pred" (class indices)."""
        self._check_fitted()
        C, D = len(self.class_weight_), self.n_features_in_
        if _pick_backend(self.backend, X) == "host":
            Xh = _host_rows(X, columns, row_index)
            if Xh.shape[1] != D:
                raise ValueError("the model was fitted on %d features, got %d" % (D, Xh.shape[1]))
            mean, scale = scaler_stats(scaler, D)
            dec = self._host_values((Xh - mean) / scale)
            votes, pred = votes_of(dec, C)
            out = {"decision": dec, "votes": votes, "pred": pred}
            return {k: out[k] for k in want}
        torch, _lib, lib = _torch_lib()
        rows = _DevRows(torch, X, columns, row_index)
        if rows.D != D:
            raise ValueError("the model was fitted on %d features, got %d" % (D, rows.D))
        with torch.cuda.device(rows.dev):
            spec = {"decision": ((rows.n, C * (C - 1) // 2), torch.float64), "votes": ((rows.n, C), torch.int64), "pred": ((rows.n,), torch.int64)}
            return wanted_outputs(torch, X, rows.dev, spec, want, self._launch_decision, torch, rows, scaler, C)

    def decision_function(self, X, columns=None, row_index=None, scaler=None, shape=None):
        """[n, P] pairwise values for "ovo"; for "ovr" [n, C], scikit-learn's transform of votes and confidences ([n] for two
        classes, as scikit-learn: the negated value, positive for the second class).  `shape` overrides the constructor's."""
        shape = self.decision_function_shape if shape is None else shape
        if shape not in ("ovr", "ovo"):
            raise ValueError("shape must be 'ovr' or 'ovo'")
        dec = self._decide(X, columns, row_index, scaler, want=("decision",))["decision"]
        C = len(self.class_weight_)
        if C == 2:
            return -dec[:, 0]
        return dec if shape == "ovo" else ovr_decision_function(dec, C)

    def predict(self, X, columns=None, row_index=None, scaler=None):
        pred = self._decide(X, columns, row_index, scaler, want=("pred",))["pred"]
        return labels_of(self.classes_, pred)
