"""Script 02's feature group, chosen from the data: which columns of the results array separate faulty rows from normal
ones?  Every subset of a pool of columns (`feature_subsets`) is standardised, fitted and scored in one batch
(`feature_sweep`), the best one by validation AUC, accuracy, log-loss or training loss is kept (`select_features`), and
`forward_select` grows a set greedily, one sweep per round.

A candidate is, by definition, `detection.build_classifier(balanced=, backend=, **lr_args).fit(results, y_tr, columns=cols,
row_index=r_tr)` started from zeros: the same scaler, class weights, damped Newton iteration and stopping rule.  All
candidates of a sweep share ONE row set: the rows whose label is in `group_spec` and whose value is finite in every column
that any subset names (so a NaN in a column that a single subset uses drops the row for all of them, and the candidates are
compared on the same rows), and one split of it into training and validation rows.

Two backends, as in detection.py.  "device": the pinn_lr_batch_* entry points of csrc/pinn_lr.hip; the row passes run on a
grid of (row blocks, candidates) and the Newton steps with one workgroup per candidate, a candidate that has stopped is
skipped while the others go on, and the host reads the headers once per `chunk` passes.  A candidate's bytes are those of
the single device fit and do not depend on the rest of the batch.  "host": the loop of host fits, float64 numpy.
Importing this module needs numpy only.

Selection overfits.  The best of hundreds of candidates by a validation score is, on that split, better than it deserves:
the validation rows have been used to choose.  Report the chosen group's AUC on rows outside BOTH splits: split twice
(`stratified_split` for the held-out rows, again within the rest for training and validation), sweep on the inner split,
then `detection.evaluate_feature_groups(results, [chosen] + list(FEATURE_GROUPS), split=(inner rows, held-out rows))` and
`rocstat.compare_feature_groups` for the paired comparison with script 02's four groups.  examples/fault_detection.py
--select does exactly that.
"""
import copy
import ctypes
import itertools
import warnings

import numpy as np

from . import detection as _dt
from ._device import _DevRows, _as_numpy, _dev_f64_rows, _is_tensor, _pick_backend, _torch_lib, call
from .detection import (DEFAULT_GROUP_SPEC, DEFAULT_RANDOM_STATE, DEFAULT_TEST_SIZE, MAX_FEAT, build_classifier, build_label_mapper,
                        extract_X_y, parse_features, parse_group_spec, roc_counts, stratified_split)
from .risk import INDEX

MAX_BATCH = 4096                         # candidates of one device call (include/pinn_hip.h: PINN_LR_MAX_BATCH)
WS_BUDGET = 1 << 30                      # bytes of device memory one call or one scoring group may use, as selection.WS_BUDGET
SINGULAR, NAN, STALLED = 1, 2, 3         # a candidate's status (include/pinn_hip.h: PINN_LR_*)
CRITERIA = {"val_auc": 1.0, "val_accuracy": 1.0, "val_logloss": -1.0, "loss": -1.0}     # 1: the largest wins, -1: the smallest
_NAMES = {v: k for k, v in INDEX.items()}
_H = {k: _dt._dev_hdr(k) for k in ("ITER", "CONVERGED", "STATUS", "F", "PASSES", "GMAX", "MAXITER")}


def _columns(spec):
    """Column indices of a spec for detection.parse_features, or of a sequence of names and indices."""
    if not isinstance(spec, str):
        spec = ",".join(str(int(p)) if isinstance(p, (int, np.integer)) else str(p) for p in spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # y_true in a pool is the caller's business here
        return parse_features(spec)


def feature_subsets(pool, min_size=1, max_size=3, must_include=()):
    """Tuples of column indices: every subset of `pool` with min_size..max_size columns that contains all of
    `must_include`, size-major and lexicographic in pool order within a size.  `pool` and `must_include` take names or
    indices through detection.parse_features.  ValueError for a size above detection.MAX_FEAT."""
    cols = _columns(pool)
    must = _columns(must_include) if len(must_include) else []
    if int(max_size) > MAX_FEAT:
        raise ValueError("a subset holds at most %d columns, max_size = %d" % (MAX_FEAT, max_size))
    if int(min_size) < 1 or int(max_size) < int(min_size):
        raise ValueError("1 <= min_size <= max_size is required")
    if any(m not in cols for m in must):
        raise ValueError("must_include names a column outside the pool")
    out = []
    for size in range(int(min_size), int(max_size) + 1):
        for comb in itertools.combinations(cols, size):
            if all(m in comb for m in must):
                out.append(tuple(comb))
    return out


class FeatureSweep:
    """What `feature_sweep` found.  Per-candidate arrays in the order of the subsets: `features` (list of tuples),
    `n_features`, `n_iter`, `converged`, `status` (0, SINGULAR, NAN or STALLED), `n_passes`, `grad_max`, `loss` (F at the
    solution, on the training rows), `val_logloss` (mean of -log p[y] over the validation rows), `val_hits` (rows
    predicted right, an integer), `val_accuracy`, `val_U2`, `n_pos`, `n_neg` (integers of the ROC of p_fault against "not
    the normal class") and `val_auc` = U2 / (2 n_pos n_neg), NaN when a side is empty.  The numbers of a candidate whose
    status is SINGULAR or NAN are NaN.  Also `classes`, `class_names`, `normal`, `n_train`, `n_val`, `idx_train`,
    `idx_val`, `kept_rows`, `backend`."""

    def __init__(self, features, backend):
        self.features = [tuple(int(c) for c in f) for f in features]
        self.n_features = np.array([len(f) for f in self.features], dtype=np.int64)
        self.backend = backend
        B = len(self.features)
        self.n_iter, self.n_passes, self.status = (np.zeros(B, np.int64) for _ in range(3))
        self.converged = np.zeros(B, bool)
        self.val_hits, self.val_U2, self.n_pos, self.n_neg = (np.zeros(B, np.int64) for _ in range(4))
        self.grad_max, self.loss, self.val_logloss = (np.full(B, np.nan) for _ in range(3))
        self._states = self._models = None

    def __len__(self):
        return len(self.features)

    def _finish(self):
        bad = (self.status == SINGULAR) | (self.status == NAN)
        self.val_accuracy = self.val_hits / max(self.n_val, 1)
        den = 2.0 * self.n_pos * self.n_neg
        with np.errstate(invalid="ignore", divide="ignore"):
            self.val_auc = np.where(den > 0, self.val_U2 / np.where(den > 0, den, 1.0), np.nan)
        for a in (self.grad_max, self.loss, self.val_logloss, self.val_accuracy, self.val_auc):
            a[bad] = np.nan
        return self

    def names(self, i):
        return tuple(_NAMES.get(c, "col%d" % c) for c in self.features[int(i)])

    def model(self, i):
        """The fitted DetectionPipeline of candidate i, on a copy of its state.  ValueError, the one the single fit
        raises, for a candidate whose status is SINGULAR or NAN."""
        i = int(i)
        if self._models is not None:
            m = self._models[i]
            if isinstance(m, str):
                raise ValueError(m)
            return copy.deepcopy(m)
        C, D = len(self.classes), int(self.n_features[i])
        o = _dt._offsets(C, D)
        st = self._states[i, :o["end"]].clone()
        s = st.cpu().numpy()
        hdr = s[:_dt._HDR].view(np.int64)
        status = int(hdr[_H["STATUS"]])
        if status in _dt._STATUS_TEXT:
            raise ValueError("logistic regression failed: %s (status %d)" % (_dt._STATUS_TEXT[status], status))
        if status != 0:
            warnings.warn("the Newton direction gives no decrease: stopped at the last accepted point")
        clf = build_classifier(balanced=self.balanced, backend="device", **self.lr_args)
        stats = [st[o[k]:o[k] + D].clone() for k in ("mean", "var", "scale")]
        clf.named_steps["scaler"]._set(*(stats if self._as_tensor else [t.cpu().numpy() for t in stats]), self.n_train)
        lr = clf.named_steps["logreg"]
        lr._state = st
        P = C * (D + 1)
        lr._publish(s[o["prev"]:o["prev"] + P].reshape(C, D + 1), self.classes, hdr[_H["ITER"]], hdr[_H["CONVERGED"]], hdr[_H["PASSES"]],
                    s[_H["GMAX"]], s[_H["F"]], s[o["cw"]:o["cw"] + C], s[o["count"]:o["count"] + C].view(np.int64), self._as_tensor,
                    st.device)
        return clf

    def best(self, criterion="val_auc"):
        """Index of the best candidate: "val_auc", "val_accuracy" (largest) or "val_logloss", "loss" (smallest), among
        those with status 0 or STALLED; ties go to the first candidate, hence to the smaller subset."""
        if criterion not in CRITERIA:
            raise ValueError("criterion must be one of %s" % sorted(CRITERIA))
        v = CRITERIA[criterion] * getattr(self, criterion)
        ok = ((self.status == 0) | (self.status == STALLED)) & ~np.isnan(v)
        if not ok.any():
            raise ValueError("no candidate can be ranked by %r" % criterion)
        return int(np.argmax(np.where(ok, v, -np.inf)))

    def table(self, top=10, criterion="val_auc"):
        """The `top` best candidates by `criterion` (all with top=None), best first, as a list of dicts."""
        if criterion not in CRITERIA:
            raise ValueError("criterion must be one of %s" % sorted(CRITERIA))
        v = CRITERIA[criterion] * getattr(self, criterion)
        ok = ((self.status == 0) | (self.status == STALLED)) & ~np.isnan(v)
        order = [int(i) for i in np.argsort(-np.where(ok, v, -np.inf), kind="stable") if ok[i]]
        keys = ("n_iter", "converged", "status", "n_passes", "grad_max", "loss", "val_logloss", "val_hits", "val_accuracy", "val_U2", "n_pos",
                "n_neg", "val_auc")
        return [dict({"index": i, "features": self.features[i], "names": self.names(i)}, **{k: getattr(self, k)[i].item() for k in keys})
                for i in order[:top]]


def _lr_settings(lr_args):
    """(tol, l2, max_iter, fit_intercept) of the candidates, validated by the single model's constructor."""
    if lr_args.get("coef_init") is not None or lr_args.get("intercept_init") is not None:
        raise ValueError("the candidates of a sweep start from zeros: coef_init and intercept_init are not taken")
    lr = build_classifier(**lr_args).named_steps["logreg"]
    return lr.tol, 1.0 / lr.C, lr.max_iter, lr.fit_intercept


def _val_classes(classes, y_va):
    """Class index of every validation label among the training classes, -1 for a label that was not trained on."""
    idx = np.minimum(np.searchsorted(classes, y_va), len(classes) - 1)
    return np.where(classes[idx] == y_va, idx, -1).astype(np.int64)


def _sweep_host(sw, results, r_tr, y_tr, r_va, y_va):
    sw._models = []
    classes = np.unique(y_tr)
    sw.classes = classes
    nidx = int(np.searchsorted(classes, sw.normal))
    truth = y_va != sw.normal
    yi_va = _val_classes(classes, y_va)
    valid = yi_va >= 0
    for i, cols in enumerate(sw.features):
        clf = build_classifier(balanced=sw.balanced, backend="host", **sw.lr_args)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                clf.fit(results, y_tr, columns=list(cols), row_index=r_tr)
            except ValueError as e:
                if len(classes) < 2:
                    raise
                sw.status[i] = SINGULAR if _dt._STATUS_TEXT[SINGULAR] in str(e) else NAN
                sw._models.append(str(e))
                continue
        if any("gives no decrease" in str(w.message) for w in caught):
            sw.status[i] = STALLED
        sw._models.append(clf)
        lr = clf.named_steps["logreg"]
        sw.n_iter[i], sw.converged[i], sw.n_passes[i], sw.grad_max[i], sw.loss[i] = lr.n_iter_, lr.converged_, lr.n_passes_, lr.grad_max_, lr.loss_
        post = lr._posterior(results, list(cols), r_va, clf.named_steps["scaler"], nidx, ("proba", "pred", "p_fault"))
        with np.errstate(divide="ignore"):
            sw.val_logloss[i] = -np.log(post["proba"][valid, yi_va[valid]]).sum() / max(len(y_va), 1)
        sw.val_hits[i] = int((post["pred"][valid] == yi_va[valid]).sum())
        r = roc_counts(truth, post["p_fault"], pos_label=True, backend="host", curve=False)
        sw.val_U2[i], sw.n_pos[i], sw.n_neg[i] = r["U2"], r["n_pos"], r["n_neg"]
        if sw.val_p_fault is not None:
            sw.val_p_fault.append(post["p_fault"])
    if sw.val_p_fault is not None:
        sw.val_p_fault = np.stack(sw.val_p_fault) if len(sw.val_p_fault) == len(sw) else None
    return sw._finish()


def _sweep_device(sw, results, r_tr, y_tr, r_va, y_va, chunk, ws_budget, timings):
    torch, _lib, lib = _torch_lib()
    arr = _dev_f64_rows(torch, results)
    rows, vrows = _DevRows(torch, arr, [0], r_tr), _DevRows(torch, arr, [0], r_va)
    dev = rows.dev
    tol, l2, max_iter, fit_intercept = _lr_settings(sw.lr_args)
    B, Dmax = len(sw), int(sw.n_features.max())
    if rows.n < 1 or vrows.n < 1:
        raise ValueError("the training and the validation rows must not be empty")
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        yt = torch.from_numpy(np.ascontiguousarray(y_tr)).to(dev)
        classes = torch.unique(yt)
        if classes.numel() < 2:
            raise ValueError(_dt._too_few(classes.tolist()))
        C = int(classes.numel())
        _dt._check_limits(C, Dmax)
        cls_h = classes.cpu().numpy()
        sw.classes = classes if sw._as_tensor else cls_h
        yi = torch.searchsorted(classes, yt).contiguous()
        yi_va = torch.from_numpy(_val_classes(cls_h, y_va)).to(dev)
        truth = torch.from_numpy(np.ascontiguousarray((y_va != sw.normal).astype(np.int64))).to(dev)
        nidx = int(np.searchsorted(cls_h, sw.normal))
        if not 0 <= nidx < C:
            raise ValueError("normal must be one of the %d classes" % C)
        stride = lib.pinn_lr_batch_state_stride(C, Dmax) // 8
        n_ws = max(rows.n, vrows.n)
        per = lib.pinn_lr_batch_workspace_bytes(n_ws, 1, C, Dmax)
        bchunk = int(max(1, min(MAX_BATCH, B, int(ws_budget) // per)))
        group = int(max(1, min(bchunk, int(ws_budget) // (48 * vrows.n))))      # p_fault, its sorted copy, the order, the flags: 6 x 8 bytes
        states = torch.zeros(B, stride, dtype=torch.float64, device=dev)
        states.view(torch.int64)[:, _H["MAXITER"]] = max_iter
        ws = torch.empty(lib.pinn_lr_batch_workspace_bytes(n_ws, bchunk, C, Dmax), dtype=torch.uint8, device=dev)
        cols_h = np.zeros((B, Dmax), dtype=np.int32)
        for i, f in enumerate(sw.features):
            cols_h[i, :len(f)] = f
        nfeat_h = np.ascontiguousarray(sw.n_features.astype(np.int32))
        d_cols, d_nfeat = torch.from_numpy(cols_h).to(dev), torch.from_numpy(nfeat_h).to(dev)
        ip = ctypes.POINTER(ctypes.c_int)
        marks = []

        def mark(name):
            if timings is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append((name, e))

        def head(r, y, lo, hi):
            return (r.arr, r.ld, r.arr.shape[0], r.ridx, r.n, y, C, hi - lo, nfeat_h[lo:hi].ctypes.data_as(ip), cols_h[lo:hi].ctypes.data_as(ip),
                    Dmax, d_nfeat[lo:hi], d_cols[lo:hi])
        for lo in range(0, B, bchunk):
            hi = min(B, lo + bchunk)
            st = states[lo:hi]
            wb = lib.pinn_lr_batch_workspace_bytes(n_ws, hi - lo, C, Dmax)
            fit = head(rows, yi, lo, hi)
            mark("start")
            call("pinn_lr_batch_scaler", *fit, int(sw.balanced), st, ws, wb, stream=stream)
            mark("scaler")
            # every pass is a pair of launches for the whole batch; the headers are read once per `chunk` passes
            while True:
                call("pinn_lr_batch_newton", *fit, chunk, tol, l2, int(fit_intercept), st, ws, wb, stream=stream)
                hdr = st[:, :_dt._HDR].cpu().numpy()
                h = hdr.view(np.int64)
                if ((h[:, _H["CONVERGED"]] != 0) | (h[:, _H["STATUS"]] != 0) | (h[:, _H["ITER"]] >= max_iter)).all():
                    break
            mark("newton")
            sw.n_iter[lo:hi], sw.converged[lo:hi], sw.status[lo:hi] = h[:, _H["ITER"]], h[:, _H["CONVERGED"]] != 0, h[:, _H["STATUS"]]
            sw.n_passes[lo:hi], sw.grad_max[lo:hi], sw.loss[lo:hi] = h[:, _H["PASSES"]], hdr[:, _H["GMAX"]], hdr[:, _H["F"]]
            for glo in range(lo, hi, group):
                ghi = min(hi, glo + group)
                g = ghi - glo
                loss = torch.empty(g, dtype=torch.float64, device=dev)
                hits = torch.empty(g, dtype=torch.int64, device=dev)
                pf = torch.empty(g, vrows.n, dtype=torch.float64, device=dev)
                counts = torch.empty(g, _lib.LR_ROC_COUNTS, dtype=torch.int64, device=dev)
                mark("start")
                call("pinn_lr_batch_score", *head(vrows, yi_va, glo, ghi), states[glo:ghi], nidx, loss, hits, pf, ws,
                     lib.pinn_lr_batch_workspace_bytes(n_ws, g, C, Dmax), stream=stream)
                mark("score")
                # detection.roc_counts' order: a stable descending sort of the reversed scores, row by row
                s_sorted, order = torch.sort(pf.flip(1), dim=1, descending=True, stable=True)
                pos_sorted = truth.flip(0)[order].contiguous()
                call("pinn_lr_batch_auc", s_sorted, pos_sorted, vrows.n, g, counts, stream=stream)
                c = counts.cpu().numpy()
                mark("auc")
                sw.val_logloss[glo:ghi] = loss.cpu().numpy() / vrows.n
                sw.val_hits[glo:ghi] = hits.cpu().numpy()
                sw.n_pos[glo:ghi], sw.n_neg[glo:ghi], sw.val_U2[glo:ghi] = c[:, _lib.LR_ROC_POS], c[:, _lib.LR_ROC_N], c[:, _lib.LR_ROC_U2]
                if sw.val_p_fault is not None:
                    sw.val_p_fault.append(pf)
        if timings is not None:
            torch.cuda.synchronize()
            for (_, a), (name, b) in zip(marks[:-1], marks[1:]):
                if name != "start":
                    timings[name] = timings.get(name, 0.0) + a.elapsed_time(b)
    sw._states = states
    if sw.val_p_fault is not None:
        sw.val_p_fault = torch.cat(sw.val_p_fault)
    return sw._finish()


def feature_sweep(results, subsets, group_spec=DEFAULT_GROUP_SPEC, split=None, test_size=DEFAULT_TEST_SIZE,
                  random_state=DEFAULT_RANDOM_STATE, balanced=True, backend="auto", chunk=4, normal=None, ws_budget=WS_BUDGET, timings=None,
                  keep_p_fault=False, **lr_args):
    """Fit and score script 02's classifier on every column subset of `subsets` (tuples of column indices as
    `feature_subsets` returns them, or feature specs) and return a `FeatureSweep`.

    Rows.  Kept are the rows of `results` whose label is in `group_spec` and whose value is finite in EVERY column that ANY
    subset names: all candidates share this one row set.  `split = (idx_train, idx_val)` are positions among the kept rows;
    without it `stratified_split(y, test_size, random_state)` is used.  `normal`: the class index that counts as normal
    for p_fault and the AUC (by default the class named "normal", else class 0).

    A candidate is `build_classifier(balanced=balanced, backend=, **lr_args).fit(results, y_tr, columns=cols,
    row_index=r_tr)` started from zeros (`lr_args`: C, tol, max_iter, fit_intercept); a candidate whose fit fails gets its
    status set, the call does not raise for it.  Device backend: `chunk` passes run between two looks at the candidates'
    headers; batches above MAX_BATCH candidates or `ws_budget` bytes of workspace are split, and the validation scores are
    sorted and scored in groups that fit the budget, neither of which changes a byte.  `timings`: a dict that receives the
    device milliseconds of the phases (scaler, newton, score, auc = sort + AUC).  `keep_p_fault=True` keeps the validation
    scores as `sweep.val_p_fault` [candidates, n_val] (a device tensor on the device backend).

    The best candidate's validation score is optimistic: see the module's note on selection."""
    feats = [tuple(_columns(s)) if isinstance(s, str) else tuple(int(c) for c in s) for s in subsets]
    if not feats or min(len(f) for f in feats) < 1:
        raise ValueError("at least one subset is needed, and at least one column in each")
    if max(len(f) for f in feats) > MAX_FEAT:
        raise ValueError("a subset holds at most %d columns" % MAX_FEAT)
    if int(chunk) < 1 or int(ws_budget) < 1:
        raise ValueError("chunk >= 1 and ws_budget >= 1 are required")
    _lr_settings(lr_args)
    label_map, class_names = build_label_mapper(parse_group_spec(group_spec))
    if normal is None:
        normal = class_names.index("normal") if "normal" in class_names else 0
    union = sorted({c for f in feats for c in f})
    be = _pick_backend(backend, results)
    _, y, kept = extract_X_y(results, union, label_map, return_index=True, backend=be)
    yh = _as_numpy(y).astype(np.int64)
    idx_tr, idx_va = split if split is not None else stratified_split(yh, test_size, random_state)
    idx_tr, idx_va = np.asarray(_as_numpy(idx_tr), dtype=np.int64), np.asarray(_as_numpy(idx_va), dtype=np.int64)
    kept_h = _as_numpy(kept).astype(np.int64)
    sw = FeatureSweep(feats, be)
    sw.class_names, sw.normal, sw.balanced, sw.lr_args = class_names, int(normal), bool(balanced), dict(lr_args)
    sw.n_train, sw.n_val, sw.idx_train, sw.idx_val, sw.kept_rows = len(idx_tr), len(idx_va), idx_tr, idx_va, kept
    sw._as_tensor = _is_tensor(results)
    sw.val_p_fault = [] if keep_p_fault else None
    if be == "host":
        return _sweep_host(sw, results, kept_h[idx_tr], yh[idx_tr], kept_h[idx_va], yh[idx_va])
    return _sweep_device(sw, results, kept_h[idx_tr], yh[idx_tr], kept_h[idx_va], yh[idx_va], int(chunk), int(ws_budget), timings)


def select_features(results, subsets, criterion="val_auc", **sweep_args):
    """(the fitted DetectionPipeline of the best subset, the FeatureSweep): the best candidate by `criterion`, see
    `FeatureSweep.best`; its columns are `sweep.features[sweep.best(criterion)]`.  Further arguments as `feature_sweep`.
    Report its AUC on rows outside both splits: see the module's note on selection."""
    if criterion not in CRITERIA:
        raise ValueError("criterion must be one of %s" % sorted(CRITERIA))
    sweep = feature_sweep(results, subsets, **sweep_args)
    return sweep.model(sweep.best(criterion)), sweep


class ForwardPath:
    """What `forward_select` did: `sets[k]` the columns after round k + 1, `scores[k]` their score by `criterion`,
    `sweeps` one FeatureSweep per round run (the round that stopped the search included), `selected` = the last set."""

    def __init__(self, criterion):
        self.criterion, self.sets, self.scores, self.sweeps = criterion, [], [], []

    @property
    def selected(self):
        return self.sets[-1] if self.sets else ()


def forward_select(results, pool, max_size, criterion="val_auc", min_gain=0.0, **sweep_args):
    """Greedy forward selection, a host loop of sweeps: round k sweeps the current set plus each remaining column of
    `pool` and takes the best by `criterion`; the search stops when the gain over the previous round is <= min_gain
    (the candidate is then not taken) or the set holds `max_size` columns.  Every round names every pool column, so all
    rounds share one row set.  Returns a `ForwardPath`.  Further arguments as `feature_sweep`."""
    if criterion not in CRITERIA:
        raise ValueError("criterion must be one of %s" % sorted(CRITERIA))
    cols = _columns(pool)
    if not 1 <= int(max_size) <= MAX_FEAT:
        raise ValueError("1 <= max_size <= %d is required" % MAX_FEAT)
    path, current = ForwardPath(criterion), ()
    while len(current) < int(max_size):
        rest = [c for c in cols if c not in current]
        if not rest:
            break
        sw = feature_sweep(results, [current + (c,) for c in rest], **sweep_args)
        path.sweeps.append(sw)
        i = sw.best(criterion)
        score = float(getattr(sw, criterion)[i])
        if path.scores and CRITERIA[criterion] * (score - path.scores[-1]) <= min_gain:
            break
        current = sw.features[i]
        path.sets.append(current)
        path.scores.append(score)
    return path
