"""Temporal diagnosis: a hidden Markov chain over the fault classes, the per-row class posteriors as emissions.

Every diagnosis of the package (DeviceGMM.diagnose, FaultDiagnoser, the logistic detector, the SVCs, the cluster diagnosers)
treats rows as exchangeable; the rows are a time series from a stack whose state persists.  `DeviceHMM` puts a Markov
chain with S <= 8 states over any of them:

  filter            P(class | rows so far)            the online diagnosis that does not flicker
  smooth            P(class | whole recording)        the curve script 03's per-sample figure wants
  viterbi           the single most probable fault history
  fit_transitions   Baum-Welch for the transition matrix (the analogue of calibrate_rf for this stage)

Emissions.  b_t(s) = y_prob[t, s] / prior[s] (the hybrid classifier-HMM rule: a posterior divided by the class prior is a
likelihood up to a factor); prior=None takes the columns as they stand.  A row whose emissions are all zero, or hold a
negative or non-finite value, is *missing*: b_t = 1 for every state.  Emissions are scale-free: a row may be multiplied by
any positive constant; posteriors and paths do not move and the log-likelihood moves by the constant's logarithm.

Segments.  `seg_starts` as in risk.rf_series: ascending positions, the first 0; a start discards everything to its left and
restarts from `init`.  A carry is an array [n_seg, 2 S + 1]: the filtered distribution, the log-likelihood so far and the
Viterbi scores of each segment's last row.  `filter` continues from the first S + 1 words of `carry_in` and `viterbi` from
the last S; each passes the other part through unchanged (NaN when there was none).

backend="auto" | "device" | "host" as everywhere (_device._pick_backend).  The device backend is csrc/pinn_hmm.hip: scans
over (flag, S x S matrix, exponent) elements.  The host backend is the plain sequential recursions in float64 numpy
(Rabiner's per-step normalisation, a log-domain Viterbi with the same tie rule: the lowest maximising state, -inf for
log 0); it serves machines without a GPU and is what the device is held to.  A tensor in gives tensors out, a numpy array
numpy.  Importing this module needs numpy only.
"""
import numpy as np

from ._device import _DevRows, _as_numpy, _dev_vec, _host_rows, _is_tensor, _pick_backend, _torch_lib, call

MAX_STATES = 8                          # include/pinn_hip.h: PINN_HMM_MAX_STATES
TILE = 1024                             # rows of a scan tile: a call of at most this many rows is one launch
ROWS_PER_THREAD = 16
_HEADER, _A, _P0, _IP = 96, 16, 80, 88  # words of the device model


# ---------------------------------------------------------------------------------------------- helpers
def sticky_transitions(S, stay=0.99):
    """S x S: `stay` on the diagonal, the rest spread evenly over the other states."""
    S = int(S)
    if S == 1:
        return np.ones((1, 1))
    A = np.full((S, S), (1.0 - stay) / (S - 1))
    np.fill_diagonal(A, stay)
    return A


def transitions_from_labels(y, n_states, seg_starts=None, pseudo_count=1.0):
    """Transition matrix from a label series: counts of (y[t], y[t+1]) inside each segment plus `pseudo_count`, rows
    normalised.  Runs on the host."""
    y = _as_numpy(y).astype(np.int64).reshape(-1)
    S = int(n_states)
    ok = np.ones(max(y.size - 1, 0), dtype=bool)
    if seg_starts is not None and len(seg_starts) > 0:
        starts = _as_numpy(seg_starts, np.int64).reshape(-1)
        ok[starts[starts > 0] - 1] = False
    counts = np.full((S, S), float(pseudo_count))
    if y.size > 1:
        np.add.at(counts, (y[:-1][ok], y[1:][ok]), 1.0)
    tot = counts.sum(axis=1, keepdims=True)
    return np.where(tot > 0, counts / np.where(tot > 0, tot, 1.0), 1.0 / S)


def scaled_likelihood(y_prob, prior):
    """y_prob / prior, the emission the chain uses (without the missing-row rule)."""
    if _is_tensor(y_prob):
        import torch
        return y_prob / torch.as_tensor(_as_numpy(prior, float), dtype=y_prob.dtype, device=y_prob.device).reshape(1, -1)
    return np.asarray(y_prob, dtype=float) / np.asarray(prior, dtype=float).reshape(1, -1)


def _bounds(seg_starts, n):
    if seg_starts is None or len(seg_starts) == 0:
        return None, [(0, n)]
    starts = _as_numpy(seg_starts, np.int64).reshape(-1)
    if starts[0] != 0 or np.any(np.diff(starts) <= 0) or starts[-1] >= max(n, 1):
        raise ValueError("seg_starts must begin with 0 and ascend strictly inside the %d positions" % n)
    edges = list(starts) + [n]
    return starts, [(int(edges[i]), int(edges[i + 1])) for i in range(len(starts))]


# ---------------------------------------------------------------------------------------------- host backend
def _host_emissions(P, inv_prior):
    with np.errstate(all="ignore"):
        b = P * inv_prior.reshape(1, -1)
        missing = ~np.all(np.isfinite(b) & (b >= 0.0), axis=1) | ~np.any(b > 0.0, axis=1)
    b[missing] = 1.0
    return b


def _host_forward(b, A, p0, bounds, carry):
    n, S = b.shape
    alpha, loglik = np.empty((n, S)), np.zeros(len(bounds))
    cout = np.full((len(bounds), 2 * S + 1), np.nan)
    if carry is not None:
        cout[:, S + 1:] = carry[:, S + 1:]
    with np.errstate(all="ignore"):
        for si, (lo, hi) in enumerate(bounds):
            scale = np.empty(hi - lo)
            a = p0 * b[lo] if carry is None else (carry[si, :S] @ A) * b[lo]
            for t in range(lo, hi):
                if t > lo:
                    a = (a @ A) * b[t]
                c = a.sum()
                a = a / c
                scale[t - lo] = c
                alpha[t] = a
            loglik[si] = np.log(scale).sum() + (0.0 if carry is None else carry[si, S])
            cout[si, :S], cout[si, S] = alpha[hi - 1], loglik[si]
    return alpha, loglik, cout


def _host_backward(b, A, alpha, bounds):
    """gamma [n, S], xi_sum [S, S], gamma_sum [S] (over rows with a successor in their segment)."""
    n, S = b.shape
    beta = np.empty((n, S))
    has_next = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for lo, hi in bounds:
            x = np.ones(S)
            beta[hi - 1] = x
            has_next[hi - 1] = False
            for t in range(hi - 2, lo - 1, -1):
                x = A @ (b[t + 1] * x)
                x = x / x.max()
                beta[t] = x
        g = alpha * beta
        gamma = g / g.sum(axis=1, keepdims=True)
        idx = np.flatnonzero(has_next)
        W = b[idx + 1] * beta[idx + 1]
        norm = (alpha[idx] * (W @ A.T)).sum(axis=1)
        xi = A * (alpha[idx].T @ (W / norm[:, None]))
        gsum = gamma[idx].sum(axis=0)
    return gamma, xi, gsum


def _host_viterbi(b, A, p0, bounds, carry):
    n, S = b.shape
    path, logprob = np.zeros(n, dtype=np.int64), np.zeros(len(bounds))
    cout = np.full((len(bounds), 2 * S + 1), np.nan)
    if carry is not None:
        cout[:, :S + 1] = carry[:, :S + 1]
    with np.errstate(divide="ignore"):
        lA, lb, lp0 = np.log(A), np.log(b), np.log(p0)
    psi = np.zeros((n, S), dtype=np.int64)
    for si, (lo, hi) in enumerate(bounds):
        d = lp0 + lb[lo] if carry is None else (carry[si, S + 1:][:, None] + lA).max(axis=0) + lb[lo]
        for t in range(lo + 1, hi):
            m = d[:, None] + lA
            psi[t] = m.argmax(axis=0)                   # the lowest maximising state
            d = m.max(axis=0) + lb[t]
        state = int(d.argmax())
        logprob[si], cout[si, S + 1:] = d[state], d
        path[hi - 1] = state
        for t in range(hi - 1, lo, -1):
            state = psi[t, state]
            path[t - 1] = state
    return path, logprob, cout


def _mstep(A, xi, pseudo):
    cnt = np.where(A > 0.0, xi + (0.0 if pseudo is None else pseudo), 0.0)
    tot = cnt.sum(axis=1, keepdims=True)
    return np.where(tot > 0.0, cnt / np.where(tot > 0.0, tot, 1.0), A)


# ---------------------------------------------------------------------------------------------- the model
class DeviceHMM:
    """A hidden Markov chain over S classes: row-stochastic `transitions` [S, S] (zeros allowed), initial distribution
    `init` [S] (uniform by default), class priors `prior` [S] or None (see the module's emission rule)."""

    def __init__(self, transitions, init=None, prior=None, backend="auto"):
        A = np.array(_as_numpy(transitions, float), dtype=float)
        if A.ndim != 2 or A.shape[0] != A.shape[1] or not 1 <= A.shape[0] <= MAX_STATES:
            raise ValueError("transitions must be S x S with 1 <= S <= %d" % MAX_STATES)
        S = A.shape[0]
        if not np.all(np.isfinite(A)) or np.any(A < 0) or np.any(np.abs(A.sum(axis=1) - 1.0) > 1e-9):
            raise ValueError("transitions must be row-stochastic")
        p0 = np.full(S, 1.0 / S) if init is None else np.array(_as_numpy(init, float), dtype=float).reshape(-1)
        if p0.shape != (S,) or np.any(p0 < 0) or abs(p0.sum() - 1.0) > 1e-9:
            raise ValueError("init must be a distribution over the %d states" % S)
        if prior is not None:
            prior = np.array(_as_numpy(prior, float), dtype=float).reshape(-1)
            if prior.shape != (S,) or not np.all(np.isfinite(prior)) or np.any(prior <= 0):
                raise ValueError("prior must hold %d positive values" % S)
        if backend not in ("auto", "device", "host"):
            raise ValueError("backend must be 'auto', 'device' or 'host'")
        self.n_states, self.backend = S, backend
        self.transitions_, self.init_, self.prior_ = A, p0, prior
        self.inv_prior_ = np.ones(S) if prior is None else 1.0 / prior
        self.n_iter_, self.converged_, self.loglik_history_ = 0, False, np.zeros(0)
        self._models = {}

    # ---- plumbing
    def _set_transitions(self, A):
        self.transitions_ = np.array(A, dtype=float)
        self._models = {}

    def _model_words(self, room=0):
        S = self.n_states
        m = np.zeros(_HEADER + room)
        m[2] = S
        m[_A:_A + 64].reshape(8, 8)[:S, :S] = self.transitions_
        m[_P0:_P0 + S] = self.init_
        m[_IP:_IP + S] = self.inv_prior_
        return m

    def _device_model(self, torch, dev):
        if dev not in self._models:
            self._models[dev] = torch.from_numpy(self._model_words()).to(dev)
        return self._models[dev]

    def _host_inputs(self, y_prob, columns, row_index, seg_starts, carry_in):
        P = _host_rows(y_prob, columns, row_index)
        if P.shape[1] != self.n_states:
            raise ValueError("the chain has %d states, the emissions %d columns" % (self.n_states, P.shape[1]))
        _, bounds = _bounds(None if seg_starts is None else _as_numpy(seg_starts), P.shape[0])
        carry = None if carry_in is None else _as_numpy(carry_in, float).reshape(len(bounds), 2 * self.n_states + 1)
        return _host_emissions(P, self.inv_prior_), bounds, carry

    def _device_inputs(self, y_prob, columns, row_index, seg_starts, carry_in):
        torch, _lib, lib = _torch_lib()
        rows = _DevRows(torch, y_prob, columns, row_index)
        if rows.D != self.n_states:
            raise ValueError("the chain has %d states, the emissions %d columns" % (self.n_states, rows.D))
        if seg_starts is not None and not _is_tensor(seg_starts):
            _bounds(seg_starts, rows.n)
        seg = _dev_vec(torch, seg_starts, torch.int64, rows.dev)
        if seg is not None and seg.numel() == 0:
            seg = None
        n_seg = 1 if seg is None else seg.numel()
        cs = 2 * self.n_states + 1
        cin = _dev_vec(torch, carry_in, torch.float64, rows.dev)
        if cin is not None and cin.numel() != n_seg * cs:
            raise ValueError("carry_in must hold 2 S + 1 words per segment")
        cout = torch.full((n_seg, cs), float("nan"), dtype=torch.float64, device=rows.dev) if cin is None else cin.reshape(n_seg, cs).clone()
        wb = lib.pinn_hmm_workspace_bytes(rows.n, self.n_states)
        ws = torch.empty(max(wb, 8), dtype=torch.uint8, device=rows.dev)
        return torch, rows, seg, n_seg, cin, cout, ws, wb

    def _forward_backward(self, y_prob, columns, row_index, seg_starts, carry_in, want):
        """One pinn_hmm_forward_backward call -> dict of device tensors (alpha, gamma, loglik, xi, gamma_sum, carry_out)."""
        torch, rows, seg, n_seg, cin, cout, ws, wb = self._device_inputs(y_prob, columns, row_index, seg_starts, carry_in)
        S, dev = self.n_states, rows.dev
        with torch.cuda.device(dev):
            out = {"alpha": torch.empty(rows.n, S, dtype=torch.float64, device=dev) if "alpha" in want else None,
                   "gamma": torch.empty(rows.n, S, dtype=torch.float64, device=dev) if "gamma" in want else None,
                   "loglik": torch.zeros(n_seg, dtype=torch.float64, device=dev),
                   "xi": torch.zeros(S, S, dtype=torch.float64, device=dev) if "xi" in want else None,
                   "gamma_sum": torch.zeros(S, dtype=torch.float64, device=dev) if "xi" in want else None}
            call("pinn_hmm_forward_backward", *rows.head(), self._device_model(torch, dev), seg, 0 if seg is None else n_seg, cin, 0, out["alpha"],
                 out["gamma"], out["loglik"], out["xi"], out["gamma_sum"], cout, ws, wb)
        out["carry_out"] = cout
        return out

    @staticmethod
    def _give(like, *values):
        return values if _is_tensor(like) else tuple(v.cpu().numpy() if _is_tensor(v) else v for v in values)

    # ---- inference
    def filter(self, y_prob, columns=None, row_index=None, seg_starts=None, carry_in=None):
        """Filtered P(class_t | rows up to t) -> (alpha [n, S], loglik [n_seg], carry_out [n_seg, 2 S + 1])."""
        if _pick_backend(self.backend, y_prob) == "host":
            b, bounds, carry = self._host_inputs(y_prob, columns, row_index, seg_starts, carry_in)
            return _host_forward(b, self.transitions_, self.init_, bounds, carry)
        r = self._forward_backward(y_prob, columns, row_index, seg_starts, carry_in, ("alpha",))
        return self._give(y_prob, r["alpha"], r["loglik"], r["carry_out"])

    def smooth(self, y_prob, columns=None, row_index=None, seg_starts=None, carry_in=None):
        """Smoothed P(class_t | every row of its segment) -> (gamma [n, S], loglik [n_seg])."""
        if _pick_backend(self.backend, y_prob) == "host":
            b, bounds, carry = self._host_inputs(y_prob, columns, row_index, seg_starts, carry_in)
            alpha, loglik, _ = _host_forward(b, self.transitions_, self.init_, bounds, carry)
            return _host_backward(b, self.transitions_, alpha, bounds)[0], loglik
        r = self._forward_backward(y_prob, columns, row_index, seg_starts, carry_in, ("gamma",))
        return self._give(y_prob, r["gamma"], r["loglik"])

    def expected_counts(self, y_prob, columns=None, row_index=None, seg_starts=None, carry_in=None):
        """The E-step -> (xi_sum [S, S], gamma_sum [S] over rows with a successor in their segment, loglik [n_seg])."""
        if _pick_backend(self.backend, y_prob) == "host":
            b, bounds, carry = self._host_inputs(y_prob, columns, row_index, seg_starts, carry_in)
            alpha, loglik, _ = _host_forward(b, self.transitions_, self.init_, bounds, carry)
            _, xi, gsum = _host_backward(b, self.transitions_, alpha, bounds)
            return xi, gsum, loglik
        r = self._forward_backward(y_prob, columns, row_index, seg_starts, carry_in, ("xi",))
        return self._give(y_prob, r["xi"], r["gamma_sum"], r["loglik"])

    def viterbi(self, y_prob, columns=None, row_index=None, seg_starts=None, carry_in=None, return_carry=False):
        """The most probable state path of each segment -> (path [n] int64, logprob [n_seg]), with return_carry also carry_out.

        Chunked use.  With `carry_in` the scores continue from the previous chunk, so `logprob` and the carried scores of
        the last chunk are those of the whole series.  The path returned for a chunk is the best path *ending in that
        chunk*: traced back from the lowest arg-max of the scores at the chunk's last row to its first row.  It is the
        decoder's current belief, not a re-decoded history: concatenated over chunks it need not be the path of the whole
        series (earlier chunks are never revised), and with chunks of one row it is the arg-max of the scores row by row."""
        if _pick_backend(self.backend, y_prob) == "host":
            b, bounds, carry = self._host_inputs(y_prob, columns, row_index, seg_starts, carry_in)
            path, logprob, cout = _host_viterbi(b, self.transitions_, self.init_, bounds, carry)
            return (path, logprob, cout) if return_carry else (path, logprob)
        torch, rows, seg, n_seg, cin, cout, ws, wb = self._device_inputs(y_prob, columns, row_index, seg_starts, carry_in)
        with torch.cuda.device(rows.dev):
            path = torch.empty(rows.n, dtype=torch.int64, device=rows.dev)
            logprob = torch.zeros(n_seg, dtype=torch.float64, device=rows.dev)
            call("pinn_hmm_viterbi", *rows.head(), self._device_model(torch, rows.dev), seg, 0 if seg is None else n_seg, cin, path,
                 logprob, cout, ws, wb)
        return self._give(y_prob, *((path, logprob, cout) if return_carry else (path, logprob)))

    # ---- fitting
    def fit_transitions(self, y_prob, columns=None, row_index=None, seg_starts=None, n_iter=50, tol=1e-6, pseudo_count=None):
        """Baum-Welch for the transitions: at most `n_iter` iterations of E-step and M-step, stopped after the iteration whose
        log-likelihood differs from the previous one's by less than `tol` (its M-step is still applied).  `pseudo_count`
        [S, S] or a number is added to the expected counts; a zero of the transitions stays zero.  Sets `transitions_`,
        `n_iter_`, `converged_` and `loglik_history_` (the log-likelihood under the transitions each iteration began with).
        On the device all `n_iter` iterations are queued without a host synchronisation: the launches after convergence
        return at once, and the model is read once at the end."""
        S, n_iter = self.n_states, int(n_iter)
        pc = None if pseudo_count is None else np.broadcast_to(np.asarray(pseudo_count, dtype=float), (S, S)).copy()
        if _pick_backend(self.backend, y_prob) == "host":
            b, bounds, _ = self._host_inputs(y_prob, columns, row_index, seg_starts, None)
            A, hist, prev, conv = self.transitions_, [], 0.0, False
            for it in range(n_iter):
                alpha, loglik, _ = _host_forward(b, A, self.init_, bounds, None)
                _, xi, _ = _host_backward(b, A, alpha, bounds)
                L = float(loglik.sum())
                hist.append(L)
                A = _mstep(A, xi, pc)
                if it > 0 and abs(L - prev) < tol:
                    conv = True
                    break
                prev = L
            self._set_transitions(A)
            self.n_iter_, self.converged_, self.loglik_history_ = len(hist), conv, np.array(hist)
            return self
        torch, rows, seg, n_seg, cin, cout, ws, wb = self._device_inputs(y_prob, columns, row_index, seg_starts, None)
        dev = rows.dev
        with torch.cuda.device(dev):
            model = torch.from_numpy(self._model_words(room=n_iter)).to(dev)
            xi = torch.zeros(S, S, dtype=torch.float64, device=dev)
            gsum = torch.zeros(S, dtype=torch.float64, device=dev)
            loglik = torch.zeros(n_seg, dtype=torch.float64, device=dev)
            pcd = None if pc is None else torch.from_numpy(pc).to(dev)
            for _ in range(n_iter):
                call("pinn_hmm_forward_backward", *rows.head(), model, seg, 0 if seg is None else n_seg, None, 1, None, None, loglik, xi,
                     gsum, None, ws, wb)
                call("pinn_hmm_mstep", model, S, xi, loglik, n_seg, pcd, float(tol), n_iter)
            words = model.cpu().numpy()             # the one host read
        self._set_transitions(words[_A:_A + 64].reshape(8, 8)[:S, :S])
        self.n_iter_, self.converged_ = int(words[0]), bool(words[1] != 0.0)
        self.loglik_history_ = words[_HEADER:_HEADER + self.n_iter_].copy()
        self._history_room = words[_HEADER:].copy()    # all n_iter slots: those past n_iter_ were never written
        return self

    def em_iterations(self, y_prob, n, columns=None, row_index=None, seg_starts=None, pseudo_count=None):
        """Exactly `n` iterations, never stopped: the form tests compare between backends."""
        return self.fit_transitions(y_prob, columns, row_index, seg_starts, n_iter=n, tol=-np.inf, pseudo_count=pseudo_count)


class TemporalDiagnoser:
    """The online form, next to FaultDiagnoser and RiskMonitor: `update(chunk)` returns the filtered class probabilities of
    the chunk's rows and their arg-max, the chain's state carried from chunk to chunk (one launch per chunk of up to TILE
    rows).  With `source`, an object whose update(rows) returns (y_prob, y_pred), `update` takes rows of the results array
    and diagnoses them per row first."""

    def __init__(self, hmm, source=None):
        self.hmm, self.source = hmm, source
        self.reset()

    def reset(self):
        self._carry, self._last, self.n_seen, self._switches = None, None, 0, 0

    @property
    def switches(self):
        """Changes of the filtered label so far."""
        self._switches = int(self._switches)
        return self._switches

    def update(self, chunk):
        y_prob = self.source.update(chunk)[0] if self.source is not None else chunk
        if len(y_prob) == 0:
            return y_prob, (y_prob[:, 0].long() if _is_tensor(y_prob) else np.zeros(0, dtype=np.int64))
        alpha, _, self._carry = self.hmm.filter(y_prob, carry_in=self._carry)
        labels = alpha.argmax(1) if _is_tensor(alpha) else alpha.argmax(axis=1)
        changes = (labels[1:] != labels[:-1]).sum()
        if self._last is not None:
            changes = changes + (labels[0] != self._last)
        self._switches = self._switches + changes       # stays on the device until it is read
        self._last = labels[-1]
        self.n_seen += len(labels)
        return alpha, labels
