"""The mixture's size and seed, chosen from the data: every candidate (component count x seed) of a grid is seeded,
initialised, iterated and scored in one batch, and the best one by BIC, AIC, held-out likelihood or lower bound is kept.

`gmm_sweep` fits the candidates and returns a `GMMSweep` (per-candidate arrays, `.model(i)`, `.best(criterion)`);
`select_gmm` returns the chosen `DeviceGMM` with the sweep.  A candidate (K, seed) is, by definition,
`DeviceGMM(K, random_state=seed, tol=, reg_covar=, max_iter=, kmeans_iter=).fit(X)`: the same k-means++ draws
(`np.random.default_rng(seed)`: `integers(n)`, then K - 1 calls of `random()`), the same Lloyd iterations, the same
initial M-step, the same EM with the same stopping rule.

Two backends, as in diagnosis.py.  "device": the pinn_gmm_batch_* entry points of csrc/pinn_gmm.hip; the row passes run on
a grid of (row blocks, candidates) and the M-steps with one workgroup per candidate, a candidate that has converged is
skipped while the others go on, and the host reads the B headers once per `em_chunk` iterations.  A candidate's bytes are
those of the single device fit and do not depend on the rest of the batch.  "host": the loop of host fits, float64 numpy.
Importing this module needs numpy only.
"""
import copy
import ctypes
import itertools

import numpy as np

from ._device import _DevRows, _as_numpy, _host_rows, _is_tensor, _pick_backend, _torch_lib, call
from .diagnosis import _HDR, MAX_COMP, DeviceGMM, _state_words, classification_metrics

MAX_BATCH = 1024                         # candidates of one device call (include/pinn_hip.h: PINN_GMM_MAX_BATCH)
WS_BUDGET = 1 << 30                      # bytes of workspace one device call may use; larger batches are split
CRITERIA = {"bic": -1.0, "aic": -1.0, "val_score": 1.0, "lower_bound": 1.0}     # -1: the smallest wins, 1: the largest
_SINGULAR = "a covariance is not positive definite (status %d): fewer components or a larger reg_covar are needed"


def n_parameters(n_components, n_features):
    """Free parameters of a full-covariance mixture, as scikit-learn's `_n_parameters`: means, covariances, weights."""
    K, D = np.asarray(n_components, dtype=np.int64), int(n_features)
    return K * D + K * D * (D + 1) // 2 + K - 1


def _draws(n, K, seed):
    """The first row and the K - 1 uniforms of DeviceGMM._seeds, in its order."""
    rng = np.random.default_rng(seed)
    first = int(rng.integers(n))
    return first, [float(rng.random()) for _ in range(K - 1)]


class GMMSweep:
    """What `gmm_sweep` found.  Per-candidate arrays, in the order K-major, seed-minor: `n_components`, `seed`, `n_iter`,
    `converged`, `status` (0, or 1 when a covariance was not positive definite), `lower_bound`, `loglik` (the sum of
    log_prob_norm over the training rows under the final parameters), `n_parameters`, `aic`, `bic` (scikit-learn's
    formulas) and `val_score` (the mean held-out log_prob_norm; NaN without validation rows).  The numbers of a candidate
    whose status is set are NaN."""

    def __init__(self, n_components, seed, n_rows, n_features, params, backend):
        self.n_components, self.seed = np.asarray(n_components, dtype=np.int64), np.asarray(seed, dtype=np.int64)
        self.n_rows, self.n_features, self.params, self.backend = int(n_rows), int(n_features), dict(params), backend
        B = self.n_components.size
        self.n_iter, self.converged, self.status = np.zeros(B, np.int64), np.zeros(B, bool), np.zeros(B, np.int64)
        self.lower_bound, self.loglik, self.val_score = (np.full(B, np.nan) for _ in range(3))
        self.n_parameters = n_parameters(self.n_components, n_features)
        self._states, self._as_tensor, self._models = None, False, None

    def __len__(self):
        return self.n_components.size

    def _finish(self):
        bad = self.status != 0
        for a in (self.lower_bound, self.loglik, self.val_score):
            a[bad] = np.nan
        self.aic = -2.0 * self.loglik + 2.0 * self.n_parameters
        self.bic = -2.0 * self.loglik + self.n_parameters * np.log(self.n_rows)
        return self

    def model(self, i):
        """The fitted DeviceGMM of candidate i, on a copy of its state.  ValueError, the one a single fit raises, for a
        candidate whose status is set."""
        i = int(i)
        K, D = int(self.n_components[i]), self.n_features
        if self._models is not None:
            m = self._models[i]
            if isinstance(m, str):
                raise ValueError(m)
            return copy.deepcopy(m)
        import torch
        g = DeviceGMM(K, random_state=int(self.seed[i]), backend="device", **self.params)
        g._state = self._states[i, :_state_words(K, D)].clone()
        g._dims, g._as_tensor, g.lower_bound_changes_ = (K, D), self._as_tensor, []
        g._publish(torch, g._read_state(D))
        return g

    def best(self, criterion="bic"):
        """Index of the best candidate among those with status 0; ties go to the first.  Unconverged candidates take part
        (see `converged`)."""
        if criterion not in CRITERIA:
            raise ValueError("criterion must be one of %s" % sorted(CRITERIA))
        v = CRITERIA[criterion] * getattr(self, criterion)
        ok = (self.status == 0) & ~np.isnan(v)
        if not ok.any():
            raise ValueError("no candidate can be ranked by %r%s" % (criterion, " (no validation rows were given)"
                                                                     if criterion == "val_score" and (self.status == 0).any() else ""))
        return int(np.argmax(np.where(ok, v, -np.inf)))

    def table(self):
        """One line per candidate."""
        lines = ["%4s %6s %5s %4s %4s %14s %14s %14s %12s" % ("K", "seed", "iter", "conv", "stat", "lower_bound", "bic", "aic", "val_score")]
        for i in range(len(self)):
            lines.append("%4d %6d %5d %4d %4d %14.6f %14.3f %14.3f %12.6f" % (
                self.n_components[i], self.seed[i], self.n_iter[i], self.converged[i], self.status[i], self.lower_bound[i], self.bic[i],
                self.aic[i], self.val_score[i]))
        return "\n".join(lines)

    def diagnosis_metrics(self, X_tr, y_tr, X_te, y_te, n_classes):
        """`classification_metrics` of the label-posterior diagnosis per candidate (None where the status is set): every
        component is calibrated against y_tr on X_tr, then X_te is diagnosed."""
        out = []
        for i in range(len(self)):
            if self.status[i] != 0:
                out.append(None)
                continue
            m = self.model(i)
            _, pred = m.diagnose(X_te, m.label_map(X_tr, y_tr, n_classes))
            out.append(classification_metrics(y_te, pred, n_classes))
        return out


def _candidates(n_components, seeds, candidates):
    if candidates is not None:
        pairs = [(int(k), int(s)) for k, s in candidates]
    else:
        pairs = list(itertools.product([int(k) for k in np.atleast_1d(n_components)], [int(s) for s in np.atleast_1d(seeds)]))
    if not pairs or min(p[0] for p in pairs) < 1:
        raise ValueError("at least one candidate is needed, and n_components >= 1 for each")
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _sweep_host(sw, X, X_val):
    sw._models = []
    for i in range(len(sw)):
        g = DeviceGMM(int(sw.n_components[i]), random_state=int(sw.seed[i]), backend="host", **sw.params)
        try:
            g.fit(X)
        except ValueError as e:                      # a covariance that is not positive definite
            sw.status[i] = 1
            sw._models.append(str(e))
            continue
        sw._models.append(g)
        sw.n_iter[i], sw.converged[i], sw.lower_bound[i] = g.n_iter_, g.converged_, g.lower_bound_
        sw.loglik[i] = g.score_samples(X).sum()
        if X_val is not None:
            sw.val_score[i] = g.score_samples(X_val).mean()
    return sw._finish()


def _sweep_device(Ks, ss, params, X, columns, row_index, val_index, X_val, em_chunk, ws_budget, timings):
    torch, _lib, lib = _torch_lib()
    rows = _DevRows(torch, X, columns, row_index)
    vrows = None
    if val_index is not None:
        vrows = _DevRows(torch, X, columns, val_index)
    elif X_val is not None:
        vrows = _DevRows(torch, X_val, columns)
        if vrows.D != rows.D:
            raise ValueError("X_val must have the features of X")
    n, D, B = rows.n, rows.D, len(Ks)
    sw = GMMSweep(Ks, ss, n, D, params, "device")
    Kmax = max(Ks)
    if Kmax > MAX_COMP:
        raise ValueError("the device backend takes at most %d components, got %d" % (MAX_COMP, Kmax))
    if n < 1:
        raise ValueError("X holds no rows")
    p = params
    stride = lib.pinn_gmm_batch_state_stride(Kmax, D) // 8
    n_ws = max(n, vrows.n if vrows is not None else 0)
    per = lib.pinn_gmm_batch_workspace_bytes(n_ws, 1, Kmax, D)
    chunk = int(max(1, min(MAX_BATCH, int(ws_budget) // per)))
    draws = [_draws(n, int(K), int(s)) for K, s in zip(sw.n_components, sw.seed)]
    with torch.cuda.device(rows.dev):
        stream = torch.cuda.current_stream().cuda_stream
        states = torch.zeros(B, stride, dtype=torch.float64, device=rows.dev)
        ws = torch.empty(per * min(chunk, B), dtype=torch.uint8, device=rows.dev)
        marks = []

        def mark(name):
            if timings is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append((name, e))
        for lo in range(0, B, chunk):
            hi = min(B, lo + chunk)
            Bc = hi - lo
            ncomp = (ctypes.c_int * Bc)(*Ks[lo:hi])
            wb = lib.pinn_gmm_batch_workspace_bytes(n_ws, Bc, Kmax, D)
            first = torch.tensor([d[0] for d in draws[lo:hi]], dtype=torch.int64).to(rows.dev)
            u = np.zeros((Bc, max(Kmax - 1, 1)))
            for c, d in enumerate(draws[lo:hi]):
                u[c, :len(d[1])] = d[1]
            u = torch.from_numpy(u).to(rows.dev)
            st = states[lo:hi]
            labels = torch.empty(Bc, n, dtype=torch.int64, device=rows.dev)
            head = rows.head() + (Bc, ncomp, Kmax)
            mark("start")
            call("pinn_gmm_batch_seed", *head, first, u, st, None, ws, wb, stream=stream)
            mark("seed")
            call("pinn_gmm_batch_kmeans", *head, p["kmeans_iter"], st, labels, ws, wb, stream=stream)
            mark("kmeans")
            call("pinn_gmm_batch_mstep_init", *head, labels, p["reg_covar"], st, ws, wb, stream=stream)
            mark("init")
            done = 0
            while True:
                step = min(em_chunk, p["max_iter"] - done)
                if step > 0:
                    call("pinn_gmm_batch_em", *head, step, p["tol"], p["reg_covar"], st, ws, wb, stream=stream)
                    done += step
                hdr = st[:, :_HDR].cpu().numpy()                     # the B headers, one copy
                h = hdr.view(np.int64)
                if ((h[:, 1] != 0) | (h[:, 2] != 0)).all() or done >= p["max_iter"]:
                    break
            mark("em")
            sums = torch.empty(2, Bc, dtype=torch.float64, device=rows.dev)
            call("pinn_gmm_batch_score", *head, st, sums[0], ws, wb, stream=stream)
            if vrows is not None:
                call("pinn_gmm_batch_score", *(vrows.head() + (Bc, ncomp, Kmax)), st, sums[1], ws, wb, stream=stream)
            sums = sums.cpu().numpy()
            mark("score")
            sw.n_iter[lo:hi], sw.converged[lo:hi], sw.status[lo:hi] = h[:, 0], h[:, 1] != 0, h[:, 2]
            sw.lower_bound[lo:hi], sw.loglik[lo:hi] = hdr[:, 5], sums[0]
            if vrows is not None:
                sw.val_score[lo:hi] = sums[1] / vrows.n
        if timings is not None:
            torch.cuda.synchronize()
            for (_, a), (name, b) in zip(marks[:-1], marks[1:]):
                if name != "start":
                    timings[name] = timings.get(name, 0.0) + a.elapsed_time(b)
    sw._states, sw._as_tensor = states, _is_tensor(X)
    return sw._finish()


def gmm_sweep(X, n_components=(2, 4, 8, 12, 16, 20, 24, 32), seeds=(0, 1, 2), *, columns=None, row_index=None, val_index=None,
              X_val=None, tol=1e-3, reg_covar=1e-6, max_iter=100, kmeans_iter=100, em_chunk=8, backend="auto", ws_budget=WS_BUDGET,
              timings=None, candidates=None):
    """Fit the mixture for every (component count, seed) of the grid on the rows of X ([n, D], or any array plus `columns`
    and `row_index`, read in place on the device) and score each: see `GMMSweep`.  `candidates`: a list of (component
    count, seed) pairs to use instead of the grid, in that order.  Validation rows are a second gather list
    `val_index` into X, or an array `X_val` read with the same `columns`.  A candidate whose covariance is not positive
    definite gets its status set; the call does not raise for it.

    `em_chunk`: EM iterations between two looks at the candidates' headers.  `ws_budget`: bytes of device workspace one
    call may use; a larger batch is split into several calls, which changes no byte.  `timings`: a dict that receives the
    device milliseconds of the phases (seed, kmeans, init, em, score; device backend)."""
    if val_index is not None and X_val is not None:
        raise ValueError("give val_index or X_val, not both")
    if tol < 0 or reg_covar < 0 or int(max_iter) < 0 or int(em_chunk) < 1 or int(ws_budget) < 1:
        raise ValueError("tol >= 0, reg_covar >= 0, max_iter >= 0, em_chunk >= 1 and ws_budget >= 1 are required")
    Ks, ss = _candidates(n_components, seeds, candidates)
    params = {"tol": float(tol), "reg_covar": float(reg_covar), "max_iter": int(max_iter), "kmeans_iter": int(kmeans_iter),
              "em_chunk": int(em_chunk)}
    which = _pick_backend(backend, X)
    if which == "host":
        Xh = _host_rows(X, columns, row_index)
        Xv = _host_rows(X, columns, val_index) if val_index is not None else (None if X_val is None else _host_rows(X_val, columns))
        return _sweep_host(GMMSweep(Ks, ss, Xh.shape[0], Xh.shape[1], params, which), Xh, Xv)
    return _sweep_device(Ks, ss, params, X, columns, row_index, val_index, X_val, int(em_chunk), ws_budget, timings)


def select_gmm(X, n_components=(2, 4, 8, 12, 16, 20, 24, 32), seeds=(0, 1, 2), *, criterion="bic", **sweep_args):
    """(the chosen DeviceGMM, the GMMSweep): the candidate with status 0 that is best by `criterion` ("bic", "aic":
    smallest; "val_score", "lower_bound": largest), ties to the first.  Unconverged candidates take part and are flagged
    in the sweep's `converged`.  criterion="lower_bound" over several seeds of one component count is scikit-learn's
    n_init rule.  Further arguments as `gmm_sweep`."""
    if criterion not in CRITERIA:
        raise ValueError("criterion must be one of %s" % sorted(CRITERIA))
    sweep = gmm_sweep(X, n_components, seeds, **sweep_args)
    return sweep.model(sweep.best(criterion)), sweep
