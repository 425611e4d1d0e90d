"""Comparison of fault-diagnosis methods: the clustering baselines and the driver of reference script 05.

Script 05 supports the claim that the Gaussian mixture with label-posterior mapping is the right diagnosis method: it runs
six methods on one stratified split of the fault rows and compares accuracy and macro precision / recall / F1.  Here:
`GMM` (diagnosis.fit_gmm_and_get_probabilities), `Sup_LR` (detection.build_classifier), and the two clustering baselines
with a well-defined answer: `KMeans` (k-means, 05:346-393) and `Agglo` (Ward agglomerative clustering with the nearest
cluster mean, 05:398-450), both with P(class | cluster) from the training labels.  `Sup_SVM` (05:323-341, a linear SVC) is
not one of the built-in four: libsvm's iterate stopped at 1e-3 is no target, but the optimum of its problem is, and svm.py
solves that; `device_extras()` hands it to `compare_methods` as `extra`.  `Spectral` (05:455-512: the eigenvectors of a kNN
graph, then ten k-means restarts) is not one of the built-in four either: its graph and the subspace of its embedding are
well-defined targets, spectral.py computes them, and `spectral_extras()` hands it over in the same way.

The helpers keep script 05's names, arguments and defaults: `fit_kmeans_posterior`, `fit_agglomerative_posterior`,
`fit_gmm_and_get_predictions`, `run_supervised_lr`, `compute_macro_metrics`, `load_data_for_fault_4class`,
`CLASS_NAMES_EN`, `N_CLASSES`.  Added: `DeviceKMeans` and `DeviceWard` (scikit-learn's arguments and attributes),
`compare_methods` (05:614-707 without figures) and `ClusterDiagnoser` (online use, next to diagnosis.FaultDiagnoser).

Two backends, as in risk.py.  "device": the HIP kernels of csrc/pinn_cluster.hip (float64; a Lloyd iteration is a row pass
plus a one-workgroup update, a Ward chain step a scan plus a one-workgroup decision; iterations and steps are queued
without a host synchronisation between them).  Ward runs on cluster means and sizes, O(n) memory, where scipy stores all
n (n - 1) / 2 distances.  "host": float64 numpy, the same state machines step for step, for machines without a GPU and as
the referee of the device tests.  Importing this module needs numpy only; scikit-learn is never imported.
"""
import functools
import heapq

import numpy as np

from .detection import compute_macro_metrics, run_supervised_lr, stratified_split  # noqa: F401
from ._device import _DevRows, _as_numpy, _dev_vec, _host_rows, _is_tensor, _on_gpu, _pick_backend, _torch_lib, call, columns_of
from .diagnosis import (DEFAULT_FEATURES, DEFAULT_GROUP_SPEC, RANDOM_STATE, REQUIRED_MAX_INDEX, TEST_SIZE, build_label_mapper,
                        classification_metrics, extract_X_y, fit_gmm_and_get_probabilities, parse_features, parse_group_spec)

CLASS_NAMES_EN = ["Flooding", "Oxygen starvation", "Membrane drying", "Hydrogen starvation"]
N_CLASSES = 4
MAX_CLUSTERS, MAX_FEAT, MAX_CLASSES = 32, 8, 16
METHODS = ("GMM", "Sup_LR", "KMeans", "Agglo")
NOT_BUILT = {"Sup_SVM": "it is not one of the built-in methods; comparison.device_extras() returns the package's linear SVC (svm.py) for it",
             "Spectral": "it is not one of the built-in methods; comparison.spectral_extras() returns the package's spectral clustering "
                         "(spectral.py) for it"}
_HDR = 16                                # 8-byte words of a device state header (include/pinn_hip.h)


def _check_limits(D, K=1, C=1):
    if not (1 <= D <= MAX_FEAT and 1 <= K <= MAX_CLUSTERS and 1 <= C <= MAX_CLASSES):
        raise NotImplementedError("the device backend takes up to %d features, %d clusters and %d classes, got %d, %d and %d"
                                  % (MAX_FEAT, MAX_CLUSTERS, MAX_CLASSES, D, K, C))


# ---------------------------------------------------------------------------------------------- host backend
def _host_d2(X, c):
    """sum_i (x_i - c_i)^2 of every row, added in column order as the kernels do."""
    s = np.zeros(X.shape[0])
    for i in range(X.shape[1]):
        d = X[:, i] - c[i]
        s += d * d
    return s


def _host_assign(X, centres):
    """(nearest centre, the first of equals; squared distance to it; margin to the second nearest)."""
    d2 = np.stack([_host_d2(X, centres[k]) for k in range(centres.shape[0])], axis=1)
    lab = d2.argmin(axis=1)
    best = d2[np.arange(X.shape[0]), lab]
    margin = np.inf
    if centres.shape[0] > 1 and X.shape[0] > 0:
        margin = float(np.min(np.partition(d2, 1, axis=1)[:, 1] - best))
    return lab.astype(np.int64), best, margin


def _host_sums(X, lab, centres):
    """What a row pass sums, [K, 1 + 2 D] = (count, sum d_i, sum d_i^2) with d = x - the cluster's centre, and the sums of
    the absolute terms (the scale of their rounding error)."""
    K, D = centres.shape
    S, A = np.zeros((K, 1 + 2 * D)), np.zeros((K, 1 + 2 * D))
    for k in range(K):
        d = X[lab == k] - centres[k]
        S[k, 0] = A[k, 0] = d.shape[0]
        S[k, 1:1 + D], A[k, 1:1 + D] = d.sum(axis=0), np.abs(d).sum(axis=0)
        S[k, 1 + D:] = A[k, 1 + D:] = (d * d).sum(axis=0)
    return S, A


def _host_step(X, centres):
    """One Lloyd iteration from `centres`: labels, sums, |sums|, new centres, sum |new - old|^2, assignment margin."""
    lab, _, margin = _host_assign(X, centres)
    S, A = _host_sums(X, lab, centres)
    D = centres.shape[1]
    cnt = S[:, :1]
    new = np.where(cnt > 0, centres + S[:, 1:1 + D] / np.where(cnt > 0, cnt, 1.0), centres)      # an empty cluster keeps its centre
    return lab, S, A, new, float(((new - centres) ** 2).sum()), margin


def host_tolerance(X, tol):
    """scikit-learn's KMeans._tolerance: tol x the mean over columns of the variance."""
    return float(tol) * float(np.mean(np.var(X, axis=0)))


def _host_lloyd(X, centres, max_iter, tol_abs, trace=None):
    """scikit-learn 1.7's _kmeans_single_lloyd.  Returns centres, labels, inertia, n_iter, strict.  `trace` (a list) gets
    one dict per iteration: margin, shift, empty."""
    centres = np.array(centres, dtype=np.float64)
    old, lab, strict, it = None, None, False, 0
    for it in range(1, max_iter + 1):
        lab, S, _, new, shift, margin = _host_step(X, centres)
        centres = new
        if trace is not None:
            trace.append({"margin": margin, "shift": shift, "empty": int((S[:, 0] == 0).sum())})
        if old is not None and np.array_equal(lab, old):
            strict = True
            break
        if shift <= tol_abs:
            break
        old = lab
    if not strict:
        lab, _, margin = _host_assign(X, centres)
        if trace is not None:
            trace.append({"margin": margin, "shift": np.inf, "empty": int(len(np.unique(lab)) < centres.shape[0])})
    inertia = float(_host_sums(X, lab, centres)[0][:, 1 + centres.shape[1]:].sum())
    return centres, lab, inertia, it, strict


def _host_ward(X):
    """The nearest-neighbour chain on means and sizes (scipy's rules).  Returns lo, hi, height in merge order and the number
    of chain steps."""
    n, D = X.shape
    mean, size = np.array(X, dtype=np.float64), np.ones(n)
    lo, hi, height = np.zeros(n - 1, dtype=np.int64), np.zeros(n - 1, dtype=np.int64), np.zeros(n - 1)
    chain, first, m, steps = [0], 0, 0, 0
    while m < n - 1:
        tip = chain[-1]
        with np.errstate(invalid="ignore", divide="ignore"):
            d = 2.0 * (size[tip] * size) / (size[tip] + size) * _host_d2(mean, mean[tip])
        d0 = d[chain[-2]] if len(chain) > 1 else np.inf
        d[size == 0] = np.inf
        d[tip] = np.inf
        j = int(np.argmin(d))
        steps += 1
        if d[j] < d0:
            chain.append(j)
            continue
        if len(chain) < 2:
            break
        pred = chain[-2]
        a, b = (tip, pred) if tip < pred else (pred, tip)
        lo[m], hi[m], height[m] = a, b, np.sqrt(d0)
        w = size[a] / (size[a] + size[b])
        mean[b] = mean[b] + w * (mean[a] - mean[b])
        size[b] += size[a]
        size[a] = 0
        del chain[-2:]
        m += 1
        if not chain and m < n - 1:
            while size[first] == 0:
                first += 1
            chain.append(first)
    return lo[:m], hi[:m], height[:m], steps


def tree_from_records(lo, hi, height, n):
    """(children_ [n - 1, 2], distances_ [n - 1]) in scikit-learn's numbering: merges in stable order of height, merge i
    makes node n + i, the smaller id first (scipy's sort and union-find relabelling)."""
    order = np.argsort(height, kind="stable")
    parent = np.arange(2 * n - 1)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    children = np.zeros((len(order), 2), dtype=np.int64)
    for i, o in enumerate(order):
        a, b = find(int(lo[o])), find(int(hi[o]))
        children[i] = (a, b) if a < b else (b, a)
        parent[a] = parent[b] = n + i
    return children, np.asarray(height, dtype=np.float64)[order]


def cut_tree(children, n, n_clusters):
    """labels [n] of the cut into n_clusters with the numbering of scikit-learn's _hc_cut."""
    if n_clusters > n:
        raise ValueError("cannot cut a tree of %d leaves into %d clusters" % (n, n_clusters))
    nodes = [-(int(max(children[-1])) + 1)] if len(children) else [0]
    for _ in range(n_clusters - 1):
        these = children[-nodes[0] - n]
        heapq.heappush(nodes, -int(these[0]))
        heapq.heappushpop(nodes, -int(these[1]))
    label = np.zeros(n, dtype=np.int64)
    for i, node in enumerate(nodes):
        stack = [-node]
        while stack:
            v = stack.pop()
            if v < n:
                label[v] = i
            else:
                stack.extend(int(c) for c in children[v - n])
    return label


def cluster_class_map(labels, y, n_clusters, n_classes):
    """P(class | cluster) [n_clusters, n_classes]: the class counts of every cluster normalised, 1 / n_classes for a cluster
    without rows (05:368-382).  Device tensors in -> device tensor out (an integer bincount, then one division)."""
    K, C = int(n_clusters), int(n_classes)
    if _on_gpu(labels):
        import torch
        lab, cls = labels.reshape(-1).to(torch.int64), _dev_vec(torch, y, torch.int64, labels.device)
        ok = (lab >= 0) & (lab < K) & (cls >= 0) & (cls < C)
        cnt = torch.bincount(lab[ok] * C + cls[ok], minlength=K * C).reshape(K, C).to(torch.float64)
        s = cnt.sum(dim=1, keepdim=True)
        return torch.where(s > 0, cnt / torch.where(s > 0, s, torch.ones_like(s)), torch.full_like(cnt, 1.0 / C))
    lab, cls = _as_numpy(labels).astype(np.int64).reshape(-1), _as_numpy(y).astype(np.int64).reshape(-1)
    ok = (lab >= 0) & (lab < K) & (cls >= 0) & (cls < C)
    cnt = np.bincount(lab[ok] * C + cls[ok], minlength=K * C).reshape(K, C).astype(np.float64)
    s = cnt.sum(axis=1, keepdims=True)
    return np.where(s > 0, cnt / np.where(s > 0, s, 1.0), 1.0 / C)


_rows = functools.partial(_DevRows.within, on_excess=_check_limits)


# ---------------------------------------------------------------------------------------------- assignment (both backends)
def assign_clusters(X, centres, cluster_class_prob=None, columns=None, row_index=None, backend="auto", want=("cluster",)):
    """dict with the wanted of "cluster" (nearest centre, the first of equals), "dist2", "y_prob" (the map's row of that
    cluster) and "y_pred" (its first maximum); the last two need cluster_class_prob [K, C].  One launch on the device."""
    if _pick_backend(backend, X) == "host":
        Xh, c = _host_rows(X, columns, row_index), _as_numpy(centres, np.float64)
        lab, d2, _ = _host_assign(Xh, c)
        out = {"cluster": lab, "dist2": d2}
        if cluster_class_prob is not None:
            y = _as_numpy(cluster_class_prob, np.float64)[lab]
            out.update(y_prob=y, y_pred=y.argmax(axis=1).astype(np.int64))
        return {k: out[k] for k in want}
    torch, _lib, lib = _torch_lib()
    rows = _rows(torch, X, columns, row_index)
    with torch.cuda.device(rows.dev):
        c = _dev_vec(torch, centres, torch.float64, rows.dev)
        K = c.numel() // rows.D
        if c.numel() != K * rows.D or K < 1:
            raise ValueError("the centres must be [n_clusters, %d]" % rows.D)
        cm, C = None, 1
        if cluster_class_prob is not None:
            cm = _dev_vec(torch, cluster_class_prob, torch.float64, rows.dev)
            C = cm.numel() // K
            if cm.numel() != K * C or C < 1:
                raise ValueError("cluster_class_prob must be [n_clusters, n_classes]")
        elif "y_prob" in want or "y_pred" in want:
            raise ValueError("y_prob and y_pred need cluster_class_prob")
        _check_limits(rows.D, K, C)
        n = rows.n
        out = {"cluster": torch.empty(n, dtype=torch.int64, device=rows.dev) if "cluster" in want else None,
               "dist2": torch.empty(n, dtype=torch.float64, device=rows.dev) if "dist2" in want else None,
               "y_prob": torch.empty(n, C, dtype=torch.float64, device=rows.dev) if "y_prob" in want else None,
               "y_pred": torch.empty(n, dtype=torch.int64, device=rows.dev) if "y_pred" in want else None}
        call("pinn_cluster_assign", *rows.head(), K, c, cm, C, out["cluster"], out["dist2"], out["y_prob"], out["y_pred"])
    if not _is_tensor(X):
        return {k: out[k].cpu().numpy() for k in want}
    return {k: out[k] for k in want}


# ---------------------------------------------------------------------------------------------- Lloyd on the device
def _km_header(st):
    h = st[:_HDR].cpu().numpy()
    i = h.view(np.int64)
    return {"n_iter": int(i[0]), "converged": bool(i[1]), "status": int(i[2]), "inertia": float(h[5]), "shift": float(h[6]),
            "tol_abs": float(h[7]), "strict": bool(i[8]), "changed": int(i[9]), "done": bool(i[10])}


class _Lloyd:
    """One of the two entry points of the Lloyd state machine (csrc/pinn_lloyd.h) with the rows it runs on: "pinn_km_lloyd"
    reads rows in place (`head` = rows.head(), up to 8 features), "pinn_sp_lloyd" packed rows (`head` = (E, n, Dm), up to 32
    columns).  The callers check their limits."""
    SIZES = {"pinn_km_lloyd": ("pinn_km_state_bytes", "pinn_km_workspace_bytes"),
             "pinn_sp_lloyd": ("pinn_sp_lloyd_state_bytes", "pinn_sp_lloyd_workspace_bytes")}

    def __init__(self, torch, lib, entry, head, n, D, dev):
        self.torch, self.entry, self.head, self.n, self.D, self.dev = torch, entry, head, n, D, dev
        self.state_bytes, self.workspace_bytes = (getattr(lib, name) for name in self.SIZES[entry])

    def state(self, K, centres):
        """A zeroed state block with `centres` written into it, and the workspace."""
        torch, D = self.torch, self.D
        st = torch.zeros(self.state_bytes(self.n, K, D) // 8, dtype=torch.float64, device=self.dev)
        c = _dev_vec(torch, centres, torch.float64, self.dev)
        if c.numel() != K * D:
            raise ValueError("the centres must be [%d, %d]" % (K, D))
        st[_HDR:_HDR + K * D] = c
        wb = self.workspace_bytes(self.n, K, D)
        return st, torch.empty(wb, dtype=torch.uint8, device=self.dev), wb

    def result(self, st, K):
        """(centres [K, D], labels [n]) copied out of a state block."""
        D = self.D
        return st[_HDR:_HDR + K * D].reshape(K, D).clone(), st[_HDR + K * D + K + D:].view(self.torch.int64).clone()

    def run(self, K, centres, max_iter, tol, chunk):
        """Iterations in chunks until converged, a status or max_iter, then the finishing call: (state, its header)."""
        stream = self.torch.cuda.current_stream().cuda_stream
        st, ws, wb = self.state(K, centres)
        done, init = 0, 1
        while True:
            step = min(chunk, max_iter - done)
            call(self.entry, *self.head, K, init, step, tol, 0, st, ws, wb, stream=stream)
            done, init = done + step, 0
            h = _km_header(st)                                 # one read of the header per chunk
            if h["converged"] or h["status"] or done >= max_iter:
                break
        if h["status"]:
            raise ValueError("the rows hold values that are not finite (status %d)" % h["status"])
        call(self.entry, *self.head, K, 0, 0, tol, 1, st, ws, wb, stream=stream)
        return st, _km_header(st)

    def probe(self, K, centres, tol, as_tensor):
        """One iteration from `centres`: the device dict of lloyd_iteration."""
        st, ws, wb = self.state(K, centres)
        call(self.entry, *self.head, K, 1, 1, float(tol), 0, st, ws, wb)
        h = _km_header(st)
        if h["status"]:
            raise ValueError("the rows hold values that are not finite")
        F = 1 + 2 * self.D
        new, labels = self.result(st, K)
        out = {"labels": labels, "sums": ws[:K * F * 8].view(self.torch.float64).reshape(K, F).clone(), "centres": new}
        if not as_tensor:
            out = {k: v.cpu().numpy() for k, v in out.items()}
        out.update(shift=h["shift"], inertia=h["inertia"], tol_abs=h["tol_abs"])
        return out


def _narrow(torch, lib, rows):
    return _Lloyd(torch, lib, "pinn_km_lloyd", rows.head(), rows.n, rows.D, rows.dev)


def lloyd_iteration(X, centres, columns=None, row_index=None, tol=1e-4, backend="auto"):
    """One Lloyd iteration from `centres`, for tests and timing.  dict: labels, sums [K, 1 + 2 D] = (count, sum d, sum d^2)
    with d = x - the centre the row went to, centres (the new ones), shift, inertia (to the old centres), tol_abs; the host
    backend adds abs_sums and margin."""
    c0 = _as_numpy(centres, np.float64)
    K = c0.shape[0]
    if _pick_backend(backend, X) == "host":
        Xh = _host_rows(X, columns, row_index)
        lab, S, A, new, shift, margin = _host_step(Xh, c0)
        return {"labels": lab, "sums": S, "abs_sums": A, "centres": new, "shift": shift, "inertia": float(S[:, 1 + c0.shape[1]:].sum()),
                "tol_abs": host_tolerance(Xh, tol), "margin": margin}
    torch, _lib, lib = _torch_lib()
    rows = _rows(torch, X, columns, row_index)
    _check_limits(rows.D, K)
    with torch.cuda.device(rows.dev):
        return _narrow(torch, lib, rows).probe(K, c0, tol, _is_tensor(X))


# ---------------------------------------------------------------------------------------------- k-means
class DeviceKMeans:
    """k-means with scikit-learn's KMeans arguments, defaults, stopping rule and attributes (`cluster_centers_, labels_,
    inertia_, n_iter_, n_features_in_`); `algorithm="lloyd"` only.

    `init`: an array [n_clusters, D] (then n_init is 1), or "k-means++": the package's own draws from a private generator
    seeded by `random_state` (as DeviceGMM's, with scikit-learn's greedy choice among 2 + log K candidates; they are not
    scikit-learn's draw for draw).  `n_init > 1` keeps the run with
    the lowest inertia.  Differences from scikit-learn: an empty cluster keeps its centre (scikit-learn moves it to the row
    farthest from its centre), and squared distances are sum (x - c)^2, not |x|^2 - 2 x.c + |c|^2.

    `fit`, `predict`, `fit_predict` take X as a [n, D] array, or any array plus `columns` (and `row_index`): the device
    backend then reads the rows in place.  numpy in -> numpy out, device tensor in -> device tensors out."""

    def __init__(self, n_clusters=8, *, init="k-means++", n_init="auto", max_iter=300, tol=1e-4, random_state=None, algorithm="lloyd",
                 backend="auto", chunk=16):
        if algorithm != "lloyd":
            raise NotImplementedError("algorithm=%r: only 'lloyd' is implemented" % (algorithm,))
        if isinstance(init, str) and init != "k-means++":
            raise NotImplementedError("init=%r: only 'k-means++' or an array of centres is implemented" % (init,))
        if backend not in ("auto", "device", "host"):
            raise ValueError("backend must be 'auto', 'device' or 'host'")
        if int(n_clusters) < 1 or int(max_iter) < 1 or tol < 0 or int(chunk) < 1 or (n_init != "auto" and int(n_init) < 1):
            raise ValueError("n_clusters >= 1, max_iter >= 1, tol >= 0, n_init >= 1 and chunk >= 1 are required")
        self.n_clusters, self.init, self.n_init, self.max_iter, self.tol = int(n_clusters), init, n_init, int(max_iter), float(tol)
        self.random_state, self.algorithm, self.backend, self.chunk = random_state, algorithm, backend, int(chunk)

    def _check_fitted(self):
        if not hasattr(self, "cluster_centers_"):
            raise RuntimeError("this DeviceKMeans is not fitted yet")

    def _runs(self):
        return 1 if (self.n_init == "auto" or not isinstance(self.init, str)) else int(self.n_init)

    def _picks(self, rng, n, d2_to, minimum, potential, search):
        """Greedy k-means++ (the variant scikit-learn uses): every new seed is the best of 2 + log K candidates drawn with
        probability proportional to the squared distance to the nearest seed so far, best meaning the lowest sum of those
        distances afterwards.  `d2_to(i)`: squared distances of all rows to row i; `search(d2, u)`: the row at fraction u of
        the cumulative sum."""
        trials = 2 + int(np.log(self.n_clusters))
        picks = [int(rng.integers(n))]
        d2 = d2_to(picks[0])
        for _ in range(1, self.n_clusters):
            best = None
            for u in rng.random(trials):
                i = search(d2, float(u))
                cand = minimum(d2, d2_to(i))
                pot = potential(cand)
                if best is None or pot < best[0]:
                    best = (pot, i, cand)
            picks.append(best[1])
            d2 = best[2]
        return picks

    def _host_seeds(self, rng, X):
        n = X.shape[0]

        def search(d2, u):
            c = np.cumsum(d2)
            return int(min(np.searchsorted(c, u * c[-1], side="right"), n - 1))
        return X[self._picks(rng, n, lambda i: _host_d2(X, X[i]), np.minimum, lambda v: float(v.sum()), search)]

    def _device_seeds(self, torch, rng, Xp):
        n = int(Xp.shape[0])

        def search(d2, u):
            c = torch.cumsum(d2, dim=0)
            return int(min(int(torch.searchsorted(c, (c[-1] * u).reshape(1), right=True).item()), n - 1))
        picks = self._picks(rng, n, lambda i: ((Xp - Xp[i]) ** 2).sum(dim=1), torch.minimum, lambda v: float(v.sum().item()), search)
        return Xp[torch.tensor(picks, device=Xp.device)]

    def _given_init(self, D):
        c = _as_numpy(self.init, np.float64)
        if c.shape != (self.n_clusters, D):
            raise ValueError("init must be [%d, %d], got %s" % (self.n_clusters, D, c.shape))
        return c

    def _fit_host(self, X):
        n, D = X.shape
        if n < self.n_clusters:
            raise ValueError("n_samples=%d should be >= n_clusters=%d" % (n, self.n_clusters))
        tol_abs = host_tolerance(X, self.tol)
        rng = np.random.default_rng(self.random_state)
        best = None
        for _ in range(self._runs()):
            c0 = self._host_seeds(rng, X) if isinstance(self.init, str) else self._given_init(D)
            run = _host_lloyd(X, c0, self.max_iter, tol_abs)
            if best is None or run[2] < best[2]:
                best = run
        self.cluster_centers_, self.labels_, self.inertia_, self.n_iter_, self.strict_ = best
        self.n_features_in_, self.tol_abs_ = D, tol_abs
        return self

    def _fit_device(self, X, columns, row_index):
        torch, _lib, lib = _torch_lib()
        rows = _rows(torch, X, columns, row_index)
        K, D, n = self.n_clusters, rows.D, rows.n
        _check_limits(D, K)
        if n < K:
            raise ValueError("n_samples=%d should be >= n_clusters=%d" % (n, K))
        rng = np.random.default_rng(self.random_state)
        best = None
        with torch.cuda.device(rows.dev):
            lloyd = _narrow(torch, lib, rows)
            for _ in range(self._runs()):
                c0 = self._device_seeds(torch, rng, rows.packed(torch)) if isinstance(self.init, str) else self._given_init(D)
                st, h = lloyd.run(K, c0, self.max_iter, self.tol, self.chunk)
                if best is None or h["inertia"] < best[1]["inertia"]:
                    best = (st, h)
            st, h = best
            centres, labels = lloyd.result(st, K)
        as_tensor = _is_tensor(X)
        self.cluster_centers_ = centres if as_tensor else centres.cpu().numpy()
        self.labels_ = labels if as_tensor else labels.cpu().numpy()
        self.inertia_, self.n_iter_, self.strict_, self.tol_abs_, self.n_features_in_ = h["inertia"], h["n_iter"], h["strict"], h["tol_abs"], D
        return self

    def fit(self, X, y=None, columns=None, row_index=None):
        if _pick_backend(self.backend, X) == "host":
            return self._fit_host(_host_rows(X, columns, row_index))
        return self._fit_device(X, columns, row_index)

    def predict(self, X, columns=None, row_index=None):
        self._check_fitted()
        return assign_clusters(X, self.cluster_centers_, None, columns, row_index, self.backend)["cluster"]

    def fit_predict(self, X, y=None, columns=None, row_index=None):
        return self.fit(X, columns=columns, row_index=row_index).labels_


# ---------------------------------------------------------------------------------------------- Ward
class DeviceWard:
    """Ward agglomerative clustering with the attributes of scikit-learn's AgglomerativeClustering(linkage="ward"):
    `children_` (merges in stable order of height, merge i makes node n + i, the smaller id first), `distances_` (always
    kept; compute_distances is accepted for compatibility), `labels_` (the numbering of scikit-learn's cut), `n_leaves_`,
    `n_clusters_`, and `cluster_means_` [n_clusters, D], the mean of every cluster's rows, which `predict` assigns new rows
    to (05:418-425, 442-444).  `n_steps_` counts the chain steps (at most 3 (n - 1)).

    The dendrogram comes from the nearest-neighbour chain on cluster means and sizes (O(n) memory); sorting the n - 1
    records, relabelling them and cutting the tree run on the host.  With exact ties in the distances the tree is a valid
    Ward tree but need not be scipy's."""

    def __init__(self, n_clusters=2, *, linkage="ward", compute_distances=False, backend="auto", chunk=1024):
        if linkage != "ward":
            raise NotImplementedError("linkage=%r: only 'ward' is implemented" % (linkage,))
        if backend not in ("auto", "device", "host"):
            raise ValueError("backend must be 'auto', 'device' or 'host'")
        if int(n_clusters) < 1 or int(chunk) < 1:
            raise ValueError("n_clusters >= 1 and chunk >= 1 are required")
        self.n_clusters, self.linkage, self.compute_distances, self.backend, self.chunk = int(n_clusters), linkage, compute_distances, backend, int(chunk)

    def _check_fitted(self):
        if not hasattr(self, "children_"):
            raise RuntimeError("this DeviceWard is not fitted yet")

    def _finish(self, lo, hi, height, n, steps):
        if len(height) != n - 1:
            raise ValueError("only %d of %d merges could be made: the rows hold values that are not finite or lie outside the array"
                             % (len(height), n - 1))
        self.records_ = (lo, hi, height)
        self.children_, self.distances_ = tree_from_records(lo, hi, height, n)
        self.n_leaves_, self.n_clusters_, self.n_steps_ = n, self.n_clusters, int(steps)
        return cut_tree(self.children_, n, self.n_clusters)

    def cut(self, n_clusters):
        """labels of another cut of the fitted tree (host array)."""
        self._check_fitted()
        return cut_tree(self.children_, self.n_leaves_, int(n_clusters))

    def fit(self, X, y=None, columns=None, row_index=None):
        if _pick_backend(self.backend, X) == "host":
            Xh = _host_rows(X, columns, row_index)
            n, D = Xh.shape
            if n < 2:
                raise ValueError("Ward clustering needs at least 2 rows")
            lo, hi, height, steps = _host_ward(Xh)
            lab = self._finish(lo, hi, height, n, steps)
            self.labels_ = lab
            self.cluster_means_ = np.stack([Xh[lab == c].mean(axis=0) for c in range(self.n_clusters)])
            self.n_features_in_ = D
            return self
        torch, _lib, lib = _torch_lib()
        rows = _rows(torch, X, columns, row_index)
        n, D = rows.n, rows.D
        _check_limits(D)
        if n < 2:
            raise ValueError("Ward clustering needs at least 2 rows")
        with torch.cuda.device(rows.dev):
            stream = torch.cuda.current_stream().cuda_stream
            st = torch.zeros(lib.pinn_ward_state_bytes(n, D) // 8, dtype=torch.float64, device=rows.dev)
            wb = lib.pinn_ward_workspace_bytes(n, D)
            ws = torch.empty(wb, dtype=torch.uint8, device=rows.dev)
            queued, init, limit = 0, 1, 3 * (n - 1)
            while True:
                step = min(self.chunk, limit - queued)
                call("pinn_ward_tree", *rows.head(), init, step, st, ws, wb, stream=stream)
                queued, init = queued + step, 0
                hdr = st[:_HDR].cpu().numpy().view(np.int64)        # one read of the header per chunk
                if hdr[1] or hdr[2] or queued >= limit:
                    break
            m = int(hdr[5])
            o = _HDR + n * D + 2 * n
            rec = st[o:o + 3 * n].cpu().numpy()
            lo, hi, height = rec[:n].view(np.int64)[:m].copy(), rec[n:2 * n].view(np.int64)[:m].copy(), rec[2 * n:][:m].copy()
            lab = self._finish(lo, hi, height, n, int(hdr[0]))
            lab_d = torch.from_numpy(lab).to(rows.dev)
            self.cluster_means_ = None
            if self.n_clusters <= MAX_CLUSTERS:
                kwb = lib.pinn_km_workspace_bytes(n, self.n_clusters, D)
                kws = torch.empty(kwb, dtype=torch.uint8, device=rows.dev)
                means = torch.zeros(self.n_clusters, D, dtype=torch.float64, device=rows.dev)
                for _ in range(2):                                # the second pass sums x - mean: exact to rounding at any offset
                    call("pinn_cluster_means", *rows.head(), self.n_clusters, lab_d, means, None, kws, kwb, stream=stream)
                self.cluster_means_ = means if _is_tensor(X) else means.cpu().numpy()
        self.labels_ = lab_d if _is_tensor(X) else lab
        self.n_features_in_ = D
        return self

    def predict(self, X, columns=None, row_index=None):
        self._check_fitted()
        if self.cluster_means_ is None:
            raise NotImplementedError("the device backend assigns rows to at most %d clusters" % MAX_CLUSTERS)
        return assign_clusters(X, self.cluster_means_, None, columns, row_index, self.backend)["cluster"]

    def fit_predict(self, X, y=None, columns=None, row_index=None):
        return self.fit(X, columns=columns, row_index=row_index).labels_


# ---------------------------------------------------------------------------------------------- script 05's functions
def _posterior_from(model, centres, labels_tr, y_tr, X_te, n_clusters, n_classes, backend, return_details):
    cmap = cluster_class_map(labels_tr, y_tr if _on_gpu(labels_tr) else _as_numpy(y_tr), n_clusters, n_classes)
    r = assign_clusters(X_te, centres, cmap, backend=backend, want=("cluster", "y_prob", "y_pred"))
    if return_details:
        return {"y_pred": r["y_pred"], "y_prob": r["y_prob"], "cluster": r["cluster"], "model": model, "cluster_class_prob": cmap}
    return r["y_pred"]


def fit_kmeans_posterior(X_tr, y_tr, X_te, n_classes, random_state=42, n_clusters=None, backend="auto", return_details=False, **km_args):
    """k-means on X_tr, P(class | cluster) from y_tr, every row of X_te gets the distribution of its nearest centre
    (05:346-393).  Returns y_pred [n_te]; with return_details=True a dict (y_pred, y_prob, cluster, model,
    cluster_class_prob).  `km_args`: further DeviceKMeans arguments (init, n_init, max_iter, tol, ...)."""
    if n_clusters is None:
        n_clusters = n_classes
    km = DeviceKMeans(n_clusters=n_clusters, random_state=random_state, backend=backend, **km_args).fit(X_tr)
    return _posterior_from(km, km.cluster_centers_, km.labels_, y_tr, X_te, n_clusters, n_classes, backend, return_details)


def fit_agglomerative_posterior(X_tr, y_tr, X_te, n_classes, n_clusters=None, backend="auto", return_details=False):
    """Ward clustering of X_tr, the mean of every cluster as its centre, then as fit_kmeans_posterior (05:398-450)."""
    if n_clusters is None:
        n_clusters = n_classes
    ward = DeviceWard(n_clusters=n_clusters, backend=backend).fit(X_tr)
    if ward.cluster_means_ is None:
        raise NotImplementedError("the device backend assigns rows to at most %d clusters" % MAX_CLUSTERS)
    return _posterior_from(ward, ward.cluster_means_, ward.labels_, y_tr, X_te, n_clusters, n_classes, backend, return_details)


def fit_gmm_and_get_predictions(X_tr, y_tr, X_te, n_classes, random_state=42, n_components_factor=5, backend="auto", **gmm_args):
    """The mixture with label-posterior mapping on n_components_factor x n_classes components (05:229-279): y_pred [n_te]."""
    return fit_gmm_and_get_probabilities(X_tr, y_tr, X_te, n_classes, random_state=random_state, n_components=n_components_factor * n_classes,
                                         backend=backend, **gmm_args)[1]


def load_data_for_fault_4class(results_or_path, features=DEFAULT_FEATURES, group_spec=DEFAULT_GROUP_SPEC, backend="auto"):
    """(X [n, D] float64, y [n] class indices, class names) of the fault rows (05:196-222).  `results_or_path`: the results
    array (numpy, or a device tensor, which stays on the device) or the path of a MAT file holding `comprehensive_results`."""
    results = results_or_path
    if isinstance(results_or_path, (str, bytes)) or hasattr(results_or_path, "__fspath__"):
        from .ingest import _loadmat
        data = _loadmat(results_or_path)
        if "comprehensive_results" not in data:
            raise KeyError("the MAT file holds no variable 'comprehensive_results'")
        results = np.array(data["comprehensive_results"])
    if results.shape[1] <= REQUIRED_MAX_INDEX:
        raise ValueError("the results array has %d columns, more than %d are needed" % (results.shape[1], REQUIRED_MAX_INDEX))
    label_map, names = build_label_mapper(parse_group_spec(group_spec))
    X, y = extract_X_y(results, parse_features(features), label_map, backend=backend)
    return X, y, names


def _take(a, idx):
    if _is_tensor(a):
        import torch
        return a[torch.from_numpy(idx).to(a.device)]
    return np.asarray(a)[idx]


def compare_methods(X, y, methods=METHODS, split=None, extra=None, n_classes=N_CLASSES, test_size=TEST_SIZE, random_state=RANDOM_STATE,
                    backend="auto", method_args=None):
    """Script 05's main loop without figures (05:614-707): one stratified split of (X, y) (or `split = (idx_tr, idx_te)`,
    gather lists into X), every method fitted on the training rows, and on the test rows y_pred, the confusion matrix
    (rows = true class), accuracy and macro precision / recall / F1.

    Built in: "GMM" (5 n_classes components), "Sup_LR", "KMeans" (5 n_classes clusters), "Agglo" (4 n_classes clusters), the
    counts of 05:648-662.  `extra` maps a name to a callable (X_tr, y_tr, X_te) -> y_pred, which takes precedence; that is
    the way to run "Sup_SVM" (`extra=device_extras()`) and "Spectral" (`extra=spectral_extras()`), which raise NotImplementedError
    without one; all six methods: `methods=METHODS + ("Sup_SVM", "Spectral"), extra={**device_extras(), **spectral_extras()}`.
    `method_args` maps a built-in name to further keyword arguments of its function.
    Returns {name: {"y_pred", "confusion_matrix", "accuracy", "macro_precision", "macro_recall", "macro_f1"}}, in the order
    of `methods`; "y_test", "idx_train" and "idx_test" sit next to the names under the key "split"."""
    extra, method_args = dict(extra or {}), dict(method_args or {})
    C = int(n_classes)
    built_in = {
        "GMM": lambda a, b, c: fit_gmm_and_get_predictions(a, b, c, n_classes=C, random_state=random_state, n_components_factor=5,
                                                           backend=backend, **method_args.get("GMM", {})),
        "Sup_LR": lambda a, b, c: run_supervised_lr(a, b, c, backend=backend, **method_args.get("Sup_LR", {})),
        "KMeans": lambda a, b, c: fit_kmeans_posterior(a, b, c, n_classes=C, random_state=random_state, n_clusters=5 * C, backend=backend,
                                                       **method_args.get("KMeans", {})),
        "Agglo": lambda a, b, c: fit_agglomerative_posterior(a, b, c, n_classes=C, n_clusters=4 * C, backend=backend,
                                                             **method_args.get("Agglo", {})),
    }
    funcs = []
    for name in methods:
        if name in extra:
            funcs.append((name, extra[name]))
        elif name in built_in:
            funcs.append((name, built_in[name]))
        elif name in NOT_BUILT:
            raise NotImplementedError("%s is not built here: %s.  Pass a callable (X_tr, y_tr, X_te) -> y_pred as extra[%r]"
                                      % (name, NOT_BUILT[name], name))
        else:
            raise ValueError("unknown method %r; built in: %s" % (name, list(built_in)))
    yh = _as_numpy(y).astype(np.int64).reshape(-1)
    idx_tr, idx_te = split if split is not None else stratified_split(yh, test_size, random_state)
    idx_tr, idx_te = np.asarray(_as_numpy(idx_tr), dtype=np.int64), np.asarray(_as_numpy(idx_te), dtype=np.int64)
    X_tr, X_te, y_tr, y_te = _take(X, idx_tr), _take(X, idx_te), _take(y, idx_tr), yh[idx_te]
    out = {"split": {"y_test": y_te, "idx_train": idx_tr, "idx_test": idx_te}}
    for name, fn in funcs:
        y_pred = _as_numpy(fn(X_tr, y_tr, X_te)).astype(np.int64).reshape(-1)
        m = classification_metrics(y_te, y_pred, C)
        out[name] = {"y_pred": y_pred, **m}
    return out


def device_extras(backend="auto", **svc_args):
    """{"Sup_SVM": callable} for `compare_methods(..., methods=METHODS + ("Sup_SVM",), extra=device_extras())`: script 05's
    run_supervised_svm_rbf (svm.py).  `svc_args`: further DeviceLinearSVC arguments."""
    from .svm import run_supervised_svm_rbf
    return {"Sup_SVM": lambda X_tr, y_tr, X_te: run_supervised_svm_rbf(X_tr, y_tr, X_te, backend=backend, **svc_args)}


def kernel_extras(backend="auto", **svc_args):
    """{"Sup_SVM_RBF": callable} for `compare_methods(..., methods=METHODS + ("Sup_SVM", "Sup_SVM_RBF"),
    extra={**device_extras(), **kernel_extras()})`: script 05's Sup_SVM with the RBF kernel its name promises
    (ksvm.run_supervised_svm_kernel).  `svc_args`: further DeviceKernelSVC arguments."""
    from .ksvm import run_supervised_svm_kernel
    return {"Sup_SVM_RBF": lambda X_tr, y_tr, X_te: run_supervised_svm_kernel(X_tr, y_tr, X_te, backend=backend, **svc_args)}


def spectral_extras(backend="auto", n_classes=N_CLASSES, **sc_args):
    """{"Spectral": callable} for `compare_methods(..., methods=METHODS + ("Spectral",), extra=spectral_extras())`: script 05's
    fit_spectral_posterior (spectral.py) on 4 n_classes clusters with random_state = RANDOM_STATE (05:663-670).  `sc_args`:
    further DeviceSpectralClustering arguments."""
    from .spectral import fit_spectral_posterior
    C = int(n_classes)
    return {"Spectral": lambda X_tr, y_tr, X_te: fit_spectral_posterior(X_tr, y_tr, X_te, n_classes=C, random_state=RANDOM_STATE,
                                                                         n_clusters=4 * C, backend=backend, **sc_args)}


class ClusterDiagnoser:
    """Class distributions chunk by chunk from a fitted DeviceKMeans, DeviceWard or DeviceSpectralClustering and its P(class | cluster):
    `update(rows)` takes the next rows of the results array [n, >= 17] (device tensor, or a host array) and returns
    (y_prob, y_pred) for them.  On the device a chunk is one kernel launch that reads the feature columns in place; it can
    run next to diagnosis.FaultDiagnoser on the same chunk."""

    def __init__(self, model, cluster_class_prob, features=DEFAULT_FEATURES, backend="auto"):
        model._check_fitted()
        self.centres = model.cluster_centers_ if hasattr(model, "cluster_centers_") else model.cluster_means_
        if self.centres is None:
            raise NotImplementedError("the device backend assigns rows to at most %d clusters" % MAX_CLUSTERS)
        self.model, self.cluster_class_prob, self.backend = model, cluster_class_prob, backend
        self.columns = columns_of(features, parse_features)
        self.n_seen = 0

    def update(self, rows):
        r = assign_clusters(rows, self.centres, self.cluster_class_prob, columns=self.columns, backend=self.backend, want=("y_prob", "y_pred"))
        self.n_seen += int(rows.shape[0])
        return r["y_prob"], r["y_pred"]
