"""Exact t-SNE: the two-dimensional embeddings behind the scatter figures of reference scripts 02 and 03.

Script 02 embeds the kept rows when more than two features are chosen (`plot_scatter_by_features`, `TSNE_PARAMS`:
perplexity 30, learning_rate "auto", init "pca"); script 03 embeds the test rows coloured by diagnosis
(`plot_tsne_of_test_samples`: perplexity 20, `n_iter=1000`, a spelling scikit-learn 1.7 no longer takes).  Here:
`DeviceTSNE` (scikit-learn's TSNE arguments and attributes, `method="exact"`), the pieces it is made of
(`joint_probabilities`, `kl_and_gradient`, `descend`), `trustworthiness`, and the two script-shaped helpers without
figures, `tsne_of_test_samples` and `scatter_by_features`.

The method is the exact O(n^2) one, which scikit-learn's default Barnes-Hut approximates.  What has a reproducible target:
P (the perplexity equation has one root per row), KL and its gradient at a given embedding, one update from a given
state, and the schedule as a state machine.  Trajectories and end points are no target: a float64 exact run moves by
percents of KL when P is perturbed by 1e-13.  Differences from scikit-learn 1.7:
  * beta_i is the root of the entropy equation to 1e-12 in float64 from float64 distances; scikit-learn bisects on float32
    distances to 1e-5.  P agrees to that tolerance.
  * a row whose m nearest rows lie at exactly the same distance with m >= perplexity (duplicated rows, as posterior columns
    that saturate to 0 or 1 produce them) has no root: its entropy stays above log m.  It gets the limit beta -> infinity,
    p = 1 / m on those rows (`beta` is inf and `entropy` log m for it); scikit-learn's bisection gives up after 100 steps at
    a large finite beta, which is the same distribution to rounding unless other rows lie very close.
  * the floor Q = max(w / Z, eps) is not applied.  It changes a term only where w_ij < eps Z, that is
    |y_i - y_j|^2 > 1 / (eps Z) - 1, of order 1 / (eps n^2) ~ 1e10 at the reference's size: no embedding gets there.
  * `kl_divergence_` is the KL at `embedding_`; scikit-learn reports the value from before the last update.
  * `max_iter=250` ends the run with the early-exaggeration phase (`n_iter_` 249).  scikit-learn 1.7.2 enters a second
    loop that does not iterate and reports `n_iter_` 250 with the largest float as KL.
  * `init="pca"` is an exact eigendecomposition of the D x D covariance with the sign rule of scikit-learn 1.7's PCA (the
    largest entry of every axis is positive; `svd_flip(..., u_based_decision=False)`), in float64; scikit-learn runs a
    randomized SVD and rounds to float32.  `init="random"` draws from a private generator seeded by `random_state`: not
    scikit-learn's draws.
There is no out-of-sample map (t-SNE has none), hence no `transform` and no online `update` form.

Two backends, as in comparison.py.  "device": the HIP kernels of csrc/pinn_tsne.hip (float64; an iteration is a pair pass
over all n^2 pairs and a one-workgroup update; 50 iterations are queued per call and the header is read once per chunk).
"host": float64 numpy, the same state machine step for step and the same sums in the same order, so an iteration gives the
device's embedding bit for bit.  exp and log are the libraries' own: P and the KL agree to rounding, and since the KL enters
the checks at every 50th iteration (best error, no progress) the two backends stop at the same iteration unless two errors
lie within rounding of each other.  The host backend is for machines without a GPU and the referee of the device tests: it
is O(n^2) numpy per iteration, minutes at a few thousand rows.
`backend="auto"` (the default) therefore uses the device for a device tensor, and for a host array of at least
AUTO_DEVICE_ROWS = 256 rows when a GPU is present; below that, or without a GPU, the host.  `DeviceTSNE.backend_` says which ran.
Importing this module needs numpy only; scikit-learn is never imported.
"""
import functools

import numpy as np

from . import _device
from ._device import _DevRows, _as_numpy, _dev_vec, _host_rows, _is_tensor, _torch_lib, call
from .diagnosis import extract_X_y

MAX_FEAT, MAX_ROWS = 8, 32768
AUTO_DEVICE_ROWS = 256                    # backend="auto" sends a host array of at least this many rows to a present GPU
EPS = 2.220446049250313e-16               # scikit-learn's MACHINE_EPSILON: the floor of P
EXPLORATION_ITER, N_ITER_CHECK = 250, 50  # scikit-learn's _EXPLORATION_MAX_ITER and _N_ITER_CHECK
TSNE_PARAMS = dict(n_components=2, perplexity=30, learning_rate="auto", init="pca", random_state=49)          # script 02
TSNE_TEST_PARAMS = dict(n_components=2, perplexity=20, learning_rate="auto", init="pca", random_state=42, n_iter=1000)   # script 03
STOP_NAMES = {0: None, 1: "max_iter", 2: "no_progress", 3: "min_grad_norm"}
_HDR = 16                                 # 8-byte words of the device state header (include/pinn_hip.h)
_SUMS = 8                                 # per-row sums: Z, Ax, Ay, Rx, Ry, sum P log P, sum P log(1 + d^2), sum P
_WAVE, _FIN = 64, 1024                    # lanes of the pair pass, threads of the one-workgroup launch
_BIG = float(np.finfo(np.float64).max)


_pick_backend = functools.partial(_device._pick_backend, threshold=AUTO_DEVICE_ROWS)      # an O(n^2) method: far fewer rows pay


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.shape(a)


def _n_rows(X, row_index):
    return int(_shape(X if row_index is None else row_index)[0])


def _check_limits(n, D):
    if not 1 <= D <= MAX_FEAT:
        raise NotImplementedError("t-SNE takes 1 to %d features, got %d" % (MAX_FEAT, D))
    if not 2 <= n <= MAX_ROWS:
        raise NotImplementedError("t-SNE takes 2 to %d rows (P is n x n float64), got %d" % (MAX_ROWS, n))


# ---------------------------------------------------------------------------------------------- host backend
def _tree(v):
    """The halving tree of the kernels' reductions over the last axis (a power of two long)."""
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


def _ordered_sum(T, width):
    """Sum over the last axis in the kernels' order: slot l adds the elements l, l + width, ... in turn, then the tree."""
    m = T.shape[-1]
    k = max(-(-m // width), 1)
    pad = np.zeros(T.shape[:-1] + (k * width,))
    pad[..., :m] = T
    pad = pad.reshape(T.shape[:-1] + (k, width))
    acc = pad[..., 0, :]
    for c in range(1, k):
        acc = acc + pad[..., c, :]
    return _tree(acc)


def _host_affinities(X, perplexity):
    """P [n, n], beta [n], entropy [n], status [n] with the kernel's rules: the root of H(beta) = log(perplexity) by Newton
    steps inside a bracket, to 1e-12 or 200 steps."""
    n, D = X.shape
    status = np.zeros(n, dtype=np.int64)
    if not np.isfinite(X).all():
        status[:] = 1
        return np.zeros((n, n)), np.full(n, np.nan), np.full(n, np.nan), status
    d = np.zeros((n, n))
    for k in range(D):
        e = X[:, k][:, None] - X[:, k][None, :]
        d += e * e
    if not np.isfinite(d).all():
        status[:] = 1
        return np.zeros((n, n)), np.full(n, np.nan), np.full(n, np.nan), status
    off = ~np.eye(n, dtype=bool)
    d = d - np.where(off, d, np.inf).min(axis=1)[:, None]
    target = np.log(perplexity)
    beta, lo, hi = np.ones(n), np.zeros(n), np.full(n, np.inf)
    H, S, conv, live = np.zeros(n), np.ones(n), np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
    m = ((d == 0.0) & off).sum(axis=1).astype(np.float64)
    dup = np.log(m) >= target                       # no root: the entropy stays above log m; the limit beta -> infinity
    live[dup] = False
    with np.errstate(all="ignore"):
        for _ in range(200):
            idx = np.flatnonzero(live)
            if idx.size == 0:
                break
            b, dd = beta[idx], d[idx]
            e = np.exp(-b[:, None] * dd) * off[idx]
            s = e.sum(axis=1)
            E = (dd * e).sum(axis=1) / s
            V = (dd * dd * e).sum(axis=1) / s - E * E
            h = np.log(s) + b * E
            H[idx], S[idx] = h, s
            diff = h - target
            ok = np.abs(diff) <= 1e-12
            conv[idx[ok]] = True
            l, u = np.where(diff > 0, b, lo[idx]), np.where(diff > 0, hi[idx], b)
            nb = b + diff / (b * V)
            inside = (nb > l) & (nb < u)
            nb = np.where(inside, nb, np.where(np.isinf(u), 2.0 * b, 0.5 * (l + u)))
            closed = nb == b
            move = ~ok & ~closed
            lo[idx], hi[idx] = np.where(ok, lo[idx], l), np.where(ok, hi[idx], u)
            beta[idx] = np.where(move, nb, b)
            live[idx[~move]] = False
    p = np.exp(-beta[:, None] * d) * off / S[:, None]
    status[~conv] = 2
    if dup.any():
        p[dup] = ((d[dup] == 0.0) & off[dup]) / m[dup][:, None]
        beta[dup], H[dup], status[dup] = np.inf, np.log(m[dup]), 4
    tot = max(2.0 * float(p.sum(axis=1).sum()), EPS)
    P = np.maximum((p + p.T) / tot, EPS)
    np.fill_diagonal(P, 0.0)
    return P, beta, H, status


def _host_pair_sums(P, Y, want_err=True, want_abs=False, block=2048):
    """The per-row sums of a pair pass [n, 8] in the kernel's arithmetic and order; with want_abs also the sums of the
    absolute terms (the scale of their rounding error)."""
    n = Y.shape[0]
    out = np.zeros((n, _SUMS))
    out_abs = np.zeros((n, _SUMS)) if want_abs else None
    idx = np.arange(n)
    for r0 in range(0, n, block):
        r1 = min(r0 + block, n)
        p = P[r0:r1]
        dx, dy = Y[r0:r1, 0][:, None] - Y[None, :, 0], Y[r0:r1, 1][:, None] - Y[None, :, 1]
        q = 1.0 + (dx * dx + dy * dy)
        w = 1.0 / q
        w[idx[r0:r1] - r0, idx[r0:r1]] = 0.0
        pw, w2 = p * w, w * w
        terms = [w, pw * dx, pw * dy, w2 * dx, w2 * dy]
        if want_err:
            pos = p > 0.0
            with np.errstate(divide="ignore", invalid="ignore"):
                terms += [np.where(pos, p * np.log(np.where(pos, p, 1.0)), 0.0), np.where(pos, p * np.log(q), 0.0), np.where(pos, p, 0.0)]
        for f, t in enumerate(terms):
            out[r0:r1, f] = _ordered_sum(t, _WAVE)
            if want_abs:
                out_abs[r0:r1, f] = np.abs(t).sum(axis=1)
    return (out, out_abs) if want_abs else out


def _host_reduce(rows, alpha, want_err=True):
    """Z, KL, the three sums behind it and the gradient [n, 2] from the per-row sums, in the kernel's order."""
    Z = _ordered_sum(rows[:, 0], _FIN)
    kl, plogp, plogq, sp = np.nan, 0.0, 0.0, 0.0
    if want_err:
        plogp, plogq, sp = (_ordered_sum(rows[:, f], _FIN) for f in (5, 6, 7))
        kl = alpha * (((plogp + np.log(alpha) * sp) + plogq) + sp * np.log(Z))
    grad = 4.0 * (alpha * rows[:, 1:3] - rows[:, 3:5] / Z)
    return float(Z), float(kl), float(plogp), float(plogq), float(sp), grad


def _wants_error(it, max_it):
    return (it + 1) % N_ITER_CHECK == 0 or it == max_it - 1


def new_state(Y, iteration=0, update=None, gains=None, best_error=_BIG, best_iteration=None, phase=None):
    """A descent state: the embedding [n, 2] with update (0) and gains (1), about to run `iteration`.  `phase`: 0 with
    early exaggeration and momentum 0.5, 1 after it; by default what `iteration` says."""
    Y = np.array(_as_numpy(Y, np.float64), dtype=np.float64).reshape(-1, 2)
    return {"Y": Y, "update": np.zeros_like(Y) if update is None else np.array(_as_numpy(update, np.float64)).reshape(-1, 2),
            "gains": np.ones_like(Y) if gains is None else np.array(_as_numpy(gains, np.float64)).reshape(-1, 2),
            "iteration": int(iteration), "phase": int(iteration >= EXPLORATION_ITER) if phase is None else int(phase),
            "best_error": float(best_error), "best_iteration": int(iteration if best_iteration is None else best_iteration),
            "done": 0, "status": 0, "error": _BIG, "grad_norm": 0.0, "n_iter": 0, "stop": 0, "stop1": 0, "Z": 0.0}


_HEADER_KEYS = ("iteration", "done", "status", "phase", "best_error", "best_iteration", "error", "grad_norm", "n_iter", "stop", "stop1", "Z")
HEADER_INTEGERS = ("iteration", "done", "status", "phase", "best_iteration", "n_iter", "stop", "stop1")


def _header_of(st):
    return {k: st[k] for k in _HEADER_KEYS}


def _host_iterate(P, st, max_iter, exaggeration, lr, no_progress, min_grad):
    """One iteration of the state machine on `st` in place: csrc/pinn_tsne.hip's pair pass and finish launch."""
    if st["done"] or st["status"]:
        return
    it, phase = st["iteration"], st["phase"]
    max_it = EXPLORATION_ITER if phase == 0 else max_iter
    err = _wants_error(it, max_it)
    alpha, mom = (exaggeration, 0.5) if phase == 0 else (1.0, 0.8)
    rows = _host_pair_sums(P, st["Y"], want_err=err)
    Z, kl, _, _, _, g = _host_reduce(rows, alpha, err)
    u, gn = st["update"], st["gains"]
    gn = np.where(u * g < 0.0, gn + 0.2, gn * 0.8)
    gn = np.where(gn < 0.01, 0.01, gn)
    g = g * gn
    un = mom * u - lr * g
    st["gains"], st["update"], st["Y"] = gn, un, st["Y"] + un
    gnorm = float(np.sqrt(_ordered_sum((g * g).reshape(-1), _FIN)))
    st["n_iter"], st["grad_norm"], st["Z"] = it, gnorm, Z
    if err:
        st["error"] = kl
    stop = 0
    if not np.isfinite(gnorm) or (err and not np.isfinite(kl)):
        st["status"], stop = 1, -1
    else:
        if (it + 1) % N_ITER_CHECK == 0:
            np_ = EXPLORATION_ITER if phase == 0 else no_progress
            if kl < st["best_error"]:
                st["best_error"], st["best_iteration"] = kl, it
            elif it - st["best_iteration"] > np_:
                stop = 2
            if not stop and gnorm <= min_grad:
                stop = 3
        if not stop and it + 1 >= max_it:
            stop = 1
    if stop > 0 and phase == 0 and not (stop == 1 and max_iter <= EXPLORATION_ITER):
        st.update(phase=1, iteration=it + 1, best_iteration=it + 1, best_error=_BIG, stop1=stop,
                  update=np.zeros_like(un), gains=np.ones_like(gn))
    elif stop != 0:
        st.update(done=1, stop=max(stop, 0))
    else:
        st["iteration"] = it + 1


def _host_pca(X):
    n, D = X.shape
    if D < 2:
        raise ValueError("init='pca' needs at least 2 features, got %d" % D)
    Xc = X - X.mean(axis=0)
    w, V = np.linalg.eigh(Xc.T @ Xc)
    V = V[:, ::-1][:, :2]
    V = V * np.sign(V[np.abs(V).argmax(axis=0), np.arange(2)])
    Y = Xc @ V
    return Y / np.std(Y[:, 0]) * 1e-4


# ---------------------------------------------------------------------------------------------- device backend
def _ws_offsets(n):
    a = lambda v: (v + 255) & ~255
    rows = a(n * n * 8)
    grad = rows + a(n * _SUMS * 8)
    scal = grad + a(n * 2 * 8)
    return rows, grad, scal


class _DevWork:
    """The workspace of n rows: P, per-row sums, gradient and scalars as views of one byte buffer."""

    def __init__(self, torch, lib, n, dev):
        self.n, self.bytes = n, lib.pinn_tsne_workspace_bytes(n)
        if self.bytes == 0:
            _check_limits(n, 1)
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=dev)
        r, g, s = _ws_offsets(n)
        self.P = self.buf[:n * n * 8].view(torch.float64).reshape(n, n)
        self.rows = self.buf[r:r + n * _SUMS * 8].view(torch.float64).reshape(n, _SUMS)
        self.grad = self.buf[g:g + n * 16].view(torch.float64).reshape(n, 2)
        self.scal = self.buf[s:s + 256].view(torch.float64)


def _dev_affinities(torch, _lib, lib, rows, perplexity):
    n = rows.n
    _check_limits(n, rows.D)
    ws = _DevWork(torch, lib, n, rows.dev)
    beta, ent = torch.empty(n, dtype=torch.float64, device=rows.dev), torch.empty(n, dtype=torch.float64, device=rows.dev)
    status = torch.empty(n, dtype=torch.int64, device=rows.dev)
    call("pinn_tsne_affinities", *rows.head(), float(perplexity), beta, ent, status, ws.buf, ws.bytes)
    return ws, beta, ent, status


def _raise_status(status):
    s = _as_numpy(status)
    if (s == 1).any():
        raise ValueError("the rows hold values that are not finite, or a row index lies outside the array")
    if (s == 2).any():
        raise ValueError("the perplexity equation was not solved to 1e-12 in 200 steps for %d rows (with perplexity above "
                         "n - 1 it has no root)" % int((s == 2).sum()))


def _dev_header(st):
    h = st[:_HDR].cpu().numpy()
    i = h.view(np.int64)
    return {"iteration": int(i[0]), "done": int(i[1]), "status": int(i[2]), "phase": int(i[4]), "best_error": float(h[5]),
            "best_iteration": int(i[6]), "error": float(h[7]), "grad_norm": float(h[8]), "n_iter": int(i[9]), "stop": int(i[10]),
            "stop1": int(i[11]), "Z": float(h[12])}


def _square(P):
    shape = _shape(P)
    if len(shape) != 2 or shape[0] != shape[1]:
        raise ValueError("P must be [n, n], got %s" % (shape,))
    return int(shape[0])


def _check_state(state, n):
    for k in ("Y", "update", "gains"):
        if np.shape(state[k]) != (n, 2):
            raise ValueError("state[%r] must be [%d, 2], got %s" % (k, n, np.shape(state[k])))


def _dev_state(torch, lib, state, dev):
    n = state["Y"].shape[0]
    h = np.zeros(_HDR)
    i = h.view(np.int64)
    i[0], i[1], i[2], i[3], i[4], i[6], i[9], i[10], i[11] = (state["iteration"], state["done"], state["status"], n, state["phase"],
                                                               state["best_iteration"], state["n_iter"], state["stop"], state["stop1"])
    h[5], h[7], h[8], h[12] = state["best_error"], state["error"], state["grad_norm"], state["Z"]
    flat = np.concatenate([h, state["Y"].reshape(-1), state["update"].reshape(-1), state["gains"].reshape(-1)])
    st = torch.from_numpy(flat).to(dev)
    assert st.numel() * 8 == lib.pinn_tsne_state_bytes(n)
    return st


# ---------------------------------------------------------------------------------------------- the pieces
def joint_probabilities(X, perplexity, columns=None, row_index=None, backend="auto"):
    """(P [n, n], beta [n], entropy [n]): P_ij = max((p_{j|i} + p_{i|j}) / sum, eps) with a zero diagonal, where
    p_{j|i} ~ exp(-beta_i |x_i - x_j|^2) has entropy log(perplexity) (in nats; `entropy` is what the root reached)."""
    if _pick_backend(backend, X, _n_rows(X, row_index)) == "host":
        Xh = _host_rows(X, columns, row_index)
        _check_limits(*Xh.shape)
        if perplexity >= Xh.shape[0]:
            raise ValueError("perplexity (%g) must be less than n_samples (%d)" % (perplexity, Xh.shape[0]))
        P, beta, H, status = _host_affinities(Xh, float(perplexity))
        _raise_status(status)
        return P, beta, H
    torch, _lib, lib = _torch_lib()
    D = len(columns) if columns is not None else int(X.shape[1])
    _check_limits(2, D)
    rows = _DevRows(torch, X, columns, row_index)
    if perplexity >= rows.n:
        raise ValueError("perplexity (%g) must be less than n_samples (%d)" % (perplexity, rows.n))
    with torch.cuda.device(rows.dev):
        ws, beta, ent, status = _dev_affinities(torch, _lib, lib, rows, perplexity)
        _raise_status(status)
        P = ws.P.clone()
    if not _is_tensor(X):
        return P.cpu().numpy(), beta.cpu().numpy(), ent.cpu().numpy()
    return P, beta, ent


def kl_and_gradient(P, Y, exaggeration=1.0, backend="auto"):
    """KL(alpha P || Q) and its gradient at the embedding Y [n, 2] with Q_ij = w_ij / Z, w = 1 / (1 + |y_i - y_j|^2).
    dict: kl, grad [n, 2], row_sums [n, 8] (Z_i, A_i [2], R_i [2], sum P log P, sum P log(1 + d^2), sum P per row), Z, sum_p,
    plogp, plogq, grad_norm; the host backend adds abs_row_sums, the sums of the absolute terms."""
    alpha = float(exaggeration)
    n = _square(P)
    if int(np.prod(_shape(Y))) != 2 * n:
        raise ValueError("Y must be [%d, 2], got %s" % (n, _shape(Y)))
    if _pick_backend(backend, P) == "host":
        Ph, Yh = _as_numpy(P, np.float64), np.ascontiguousarray(_as_numpy(Y, np.float64)).reshape(-1, 2)
        rows, rows_abs = _host_pair_sums(Ph, Yh, want_err=True, want_abs=True)
        Z, kl, plogp, plogq, sp, grad = _host_reduce(rows, alpha)
        return {"kl": kl, "grad": grad, "row_sums": rows, "abs_row_sums": rows_abs, "Z": Z, "sum_p": sp, "plogp": plogp, "plogq": plogq,
                "grad_norm": float(np.sqrt(_ordered_sum((grad * grad).reshape(-1), _FIN)))}
    torch, _lib, lib = _torch_lib()
    Pd = P if _is_tensor(P) and P.is_cuda else torch.from_numpy(np.ascontiguousarray(_as_numpy(P, np.float64))).cuda()
    _check_limits(n, 1)
    with torch.cuda.device(Pd.device):
        ws = _DevWork(torch, lib, n, Pd.device)
        ws.P.copy_(Pd.to(torch.float64))
        Yd = _dev_vec(torch, Y, torch.float64, Pd.device)
        call("pinn_tsne_kl_grad", n, Yd, alpha, ws.buf, ws.bytes)
        s = ws.scal.cpu().numpy()
        out = {"grad": ws.grad.clone(), "row_sums": ws.rows.clone()}
    if not _is_tensor(P):
        out = {k: v.cpu().numpy() for k, v in out.items()}
    out.update(kl=float(s[2]), Z=float(s[1]), sum_p=float(s[3]), plogp=float(s[4]), plogq=float(s[5]), grad_norm=float(s[6]))
    return out


def descend(P, state, n_iter, *, max_iter=1000, early_exaggeration=12.0, learning_rate=200.0, n_iter_without_progress=300,
            min_grad_norm=1e-7, backend="auto", chunk=N_ITER_CHECK):
    """Runs `n_iter` iterations of the state machine from `state` (see new_state; host arrays) and returns (new state,
    header): the header is the state's scalars (iteration: the one that runs next; n_iter: the last that ran; done; stop and
    stop1: why the run and its first phase ended, see STOP_NAMES).  After `done` further iterations change nothing."""
    if int(max_iter) < EXPLORATION_ITER:
        raise ValueError("max_iter must be at least %d" % EXPLORATION_ITER)
    args = (int(max_iter), float(early_exaggeration), float(learning_rate), int(n_iter_without_progress), float(min_grad_norm))
    n = _square(P)
    _check_state(state, n)
    if _pick_backend(backend, P) == "host":
        Ph = _as_numpy(P, np.float64)
        st = dict(state)
        for _ in range(int(n_iter)):
            if st["done"] or st["status"]:
                break
            _host_iterate(Ph, st, *args)
        return st, _header_of(st)
    torch, _lib, lib = _torch_lib()
    Pd = P if _is_tensor(P) and P.is_cuda else torch.from_numpy(np.ascontiguousarray(_as_numpy(P, np.float64))).cuda()
    _check_limits(n, 1)
    with torch.cuda.device(Pd.device):
        ws = _DevWork(torch, lib, n, Pd.device)
        ws.P.copy_(Pd.to(torch.float64))
        st = _dev_state(torch, lib, state, Pd.device)
        left = int(n_iter)
        while left > 0:
            step = min(int(chunk), left)
            call("pinn_tsne_descend", n, 0, step, args[0], args[1], args[2], args[3], args[4], st, ws.buf, ws.bytes)
            left -= step
        h = _dev_header(st)
        body = st[_HDR:].cpu().numpy().reshape(3, n, 2)
    out = dict(h, Y=body[0].copy(), update=body[1].copy(), gains=body[2].copy())
    return out, h


def trustworthiness(X, Y, n_neighbors=5):
    """scikit-learn's trustworthiness (Euclidean): 1 - 2 / (n k (2 n - 3 k - 1)) sum_i sum_{j in the k nearest of i in Y}
    max(0, rank of j among the neighbours of i in X - k)."""
    Xh, Yh = _as_numpy(X, np.float64), _as_numpy(Y, np.float64)
    Xh = Xh.reshape(Xh.shape[0], -1)
    n, k = Xh.shape[0], int(n_neighbors)
    if k >= n / 2:
        raise ValueError("n_neighbors (%d) should be less than n_samples / 2 (%g)" % (k, n / 2))

    def dist(A):
        d = np.zeros((n, n))
        for c in range(A.shape[1]):
            e = A[:, c][:, None] - A[:, c][None, :]
            d += e * e
        np.fill_diagonal(d, np.inf)
        return d
    ind_X = np.argsort(dist(Xh), axis=1, kind="stable")
    ind_Y = np.argsort(dist(Yh), axis=1, kind="stable")[:, :k]
    rank = np.zeros((n, n), dtype=np.int64)
    rank[np.arange(n)[:, None], ind_X] = np.arange(1, n + 1)
    r = rank[np.arange(n)[:, None], ind_Y] - k
    t = float(r[r > 0].sum())
    return 1.0 - t * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


# ---------------------------------------------------------------------------------------------- the estimator
class DeviceTSNE:
    """Exact t-SNE with scikit-learn's TSNE arguments, defaults, schedule and attributes (`embedding_, kl_divergence_, n_iter_,
    learning_rate_, n_features_in_`).  `n_iter` is the old name of `max_iter` (script 03 passes it); `verbose` is accepted and
    ignored.  `method="exact"` and two components only; the metric is Euclidean.

    `init`: "pca" (the two leading principal axes, scaled to std 1e-4 of the first), "random" (the package's own draws from a
    private generator seeded by `random_state`, times 1e-4: not scikit-learn's draw for draw), or an array [n, 2].
    `backend`: "device", "host", or "auto": the device for a device tensor and for a host array of at least AUTO_DEVICE_ROWS
    rows when a GPU is present, else the host; `backend_` says which ran.
    `fit` and `fit_transform` take X as a [n, D] array, or any array plus `columns` (and `row_index`): the device backend
    then reads the rows in place.  numpy in -> numpy out, device tensor in -> device tensors out.  See the module text for
    the differences from scikit-learn.  There is no `transform`: t-SNE has no out-of-sample map."""

    def __init__(self, n_components=2, *, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, metric="euclidean", init="pca", random_state=None, method="exact",
                 n_iter=None, verbose=0, backend="auto"):
        if method == "barnes_hut":
            raise NotImplementedError("method='barnes_hut' is not implemented: method='exact' is what it approximates, and is what runs here")
        if method != "exact":
            raise ValueError("method must be 'exact'")
        if int(n_components) != 2:
            raise NotImplementedError("n_components=%r: only 2 components are implemented" % (n_components,))
        if metric != "euclidean":
            raise NotImplementedError("metric=%r: only 'euclidean' is implemented" % (metric,))
        if isinstance(init, str) and init not in ("pca", "random"):
            raise ValueError("init must be 'pca', 'random' or an array [n, 2]")
        if backend not in ("auto", "device", "host"):
            raise ValueError("backend must be 'auto', 'device' or 'host'")
        if n_iter is not None:
            max_iter = n_iter
        if int(max_iter) < EXPLORATION_ITER:
            raise ValueError("max_iter must be at least %d, as in scikit-learn" % EXPLORATION_ITER)
        if not (isinstance(learning_rate, str) and learning_rate == "auto") and not float(learning_rate) > 0:
            raise ValueError("learning_rate must be 'auto' or positive")
        if not perplexity > 0 or not early_exaggeration >= 1 or min_grad_norm < 0 or int(n_iter_without_progress) < 0:
            raise ValueError("perplexity > 0, early_exaggeration >= 1, min_grad_norm >= 0 and n_iter_without_progress >= 0 are required")
        self.n_components, self.perplexity, self.early_exaggeration, self.learning_rate = 2, float(perplexity), float(early_exaggeration), learning_rate
        self.max_iter, self.n_iter_without_progress, self.min_grad_norm = int(max_iter), int(n_iter_without_progress), float(min_grad_norm)
        self.metric, self.init, self.random_state, self.method, self.verbose, self.backend = metric, init, random_state, method, verbose, backend

    def _lr(self, n):
        if isinstance(self.learning_rate, str):
            return max(n / self.early_exaggeration / 4.0, 50.0)
        return float(self.learning_rate)

    def _args(self, n):
        return (self.max_iter, self.early_exaggeration, self._lr(n), self.n_iter_without_progress, self.min_grad_norm)

    def _given_init(self, n):
        Y = np.ascontiguousarray(_as_numpy(self.init, np.float64))
        if Y.shape != (n, 2):
            raise ValueError("init must be [%d, 2], got %s" % (n, Y.shape))
        return Y

    def _random_init(self, n):
        return 1e-4 * np.random.default_rng(self.random_state).standard_normal((n, 2))

    def _check(self, n, D):
        _check_limits(n, D)
        if self.perplexity >= n:
            raise ValueError("perplexity (%g) must be less than n_samples (%d)" % (self.perplexity, n))

    def _fit_host(self, X):
        n, D = X.shape
        self._check(n, D)
        P, _, _, status = _host_affinities(X, self.perplexity)
        _raise_status(status)
        Y0 = _host_pca(X) if isinstance(self.init, str) and self.init == "pca" else (
            self._random_init(n) if isinstance(self.init, str) else self._given_init(n))
        st = new_state(Y0)
        args = self._args(n)
        while not (st["done"] or st["status"]):
            _host_iterate(P, st, *args)
        if st["status"]:
            raise ValueError("the embedding left the range of float64 (status %d)" % st["status"])
        rows = _host_pair_sums(P, st["Y"])
        self.embedding_, self.kl_divergence_, self.n_iter_ = st["Y"], _host_reduce(rows, 1.0)[1], st["n_iter"]
        self.learning_rate_, self.n_features_in_, self.header_ = args[2], D, _header_of(st)
        return self

    def _device_pca(self, torch, rows):
        if rows.D < 2:
            raise ValueError("init='pca' needs at least 2 features, got %d" % rows.D)
        Xp = rows.packed(torch)
        Xc = Xp - Xp.mean(dim=0)
        cov = (Xc[:, :, None] * Xc[:, None, :]).sum(dim=0).cpu().numpy()          # D x D; the eigenvectors come from the host
        w, V = np.linalg.eigh(cov)
        V = V[:, ::-1][:, :2]
        V = V * np.sign(V[np.abs(V).argmax(axis=0), np.arange(2)])
        Vd = torch.from_numpy(np.ascontiguousarray(V)).to(rows.dev)
        Y = torch.stack([(Xc * Vd[:, 0]).sum(dim=1), (Xc * Vd[:, 1]).sum(dim=1)], dim=1)
        return (Y / Y[:, 0].std(unbiased=False) * 1e-4).contiguous()

    def _fit_device(self, X, columns, row_index):
        torch, _lib, lib = _torch_lib()
        D = len(columns) if columns is not None else (int(X.shape[1]) if len(X.shape) == 2 else 1)
        _check_limits(2, D)
        rows = _DevRows(torch, X, columns, row_index)
        n = rows.n
        self._check(n, D)
        args = self._args(n)
        with torch.cuda.device(rows.dev):
            stream = torch.cuda.current_stream().cuda_stream
            ws, _, _, status = _dev_affinities(torch, _lib, lib, rows, self.perplexity)
            _raise_status(status)
            if isinstance(self.init, str) and self.init == "pca":
                Y0 = self._device_pca(torch, rows)
            else:
                Y0 = torch.from_numpy(self._random_init(n) if isinstance(self.init, str) else self._given_init(n)).to(rows.dev)
            st = torch.zeros(lib.pinn_tsne_state_bytes(n) // 8, dtype=torch.float64, device=rows.dev)
            st[_HDR:_HDR + 2 * n] = Y0.reshape(-1)
            queued, init = 0, 1
            while True:
                call("pinn_tsne_descend", n, init, N_ITER_CHECK, *args, st, ws.buf, ws.bytes, stream=stream)
                queued, init = queued + N_ITER_CHECK, 0
                h = _dev_header(st)                            # one read of the header per chunk
                if h["done"] or h["status"] or queued >= self.max_iter + N_ITER_CHECK:
                    break
            if h["status"]:
                raise ValueError("the embedding left the range of float64 (status %d)" % h["status"])
            if not h["done"]:
                raise RuntimeError("the schedule did not end within max_iter = %d iterations (header %r)" % (self.max_iter, h))
            Y = st[_HDR:_HDR + 2 * n].reshape(n, 2).clone()
            call("pinn_tsne_kl_grad", n, Y, 1.0, ws.buf, ws.bytes, stream=stream)
            kl = float(ws.scal[2].item())
        self.embedding_ = Y if _is_tensor(X) else Y.cpu().numpy()
        self.kl_divergence_, self.n_iter_, self.learning_rate_, self.n_features_in_, self.header_ = kl, h["n_iter"], args[2], D, h
        return self

    def fit(self, X, y=None, columns=None, row_index=None):
        self.backend_ = _pick_backend(self.backend, X, _n_rows(X, row_index))
        if self.backend_ == "host":
            return self._fit_host(_host_rows(X, columns, row_index))
        return self._fit_device(X, columns, row_index)

    def fit_transform(self, X, y=None, columns=None, row_index=None):
        return self.fit(X, columns=columns, row_index=row_index).embedding_


# ---------------------------------------------------------------------------------------------- the scripts' functions
def tsne_of_test_samples(X_te, y_pred=None, backend="auto", **tsne_args):
    """Script 03's plot_tsne_of_test_samples without the figure: the embedding [n, 2] of the test rows with its settings
    (TSNE_TEST_PARAMS; `tsne_args` override them), and with `y_pred` also {class: the rows predicted as it}."""
    emb = DeviceTSNE(backend=backend, **{**TSNE_TEST_PARAMS, **tsne_args}).fit_transform(X_te)
    if y_pred is None:
        return emb
    yp = _as_numpy(y_pred).astype(np.int64).reshape(-1)
    if yp.shape[0] != emb.shape[0]:
        raise ValueError("y_pred and X_te differ in length")
    return emb, {int(c): np.flatnonzero(yp == c) for c in np.unique(yp)}


def scatter_by_features(results, feature_indices, label_map, backend="auto", **tsne_args):
    """Script 02's plot_scatter_by_features without the figure: the rows of the results array whose label is a key of
    `label_map` and whose features are finite (extract_X_y); two features are returned as they are, more than two go through
    t-SNE with TSNE_PARAMS (`tsne_args` override them).  Returns (xy [n, 2], y [n], used_tsne)."""
    feature_indices = [int(c) for c in feature_indices]
    if len(feature_indices) < 2:
        raise ValueError("a scatter needs at least two features")
    X, y = extract_X_y(results, feature_indices, label_map, backend="device" if _is_tensor(results) and results.is_cuda else "host")
    if X.shape[1] == 2:
        return X, y, False
    return DeviceTSNE(backend=backend, **{**TSNE_PARAMS, **tsne_args}).fit_transform(X), y, True
