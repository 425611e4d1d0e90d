"""Unsupervised anomaly detection: the isolation forest of reference script 02 (02:571-596), the one detector there that
needs no fault labels.

`DeviceIsolationForest` has scikit-learn's IsolationForest arguments, defaults and attributes.  The target splits in two.

Scoring a given forest is exact.  `score_samples` restates scikit-learn's: the row is cast to float32 and descends every
tree by `x32 <= threshold`; the leaf value is `(depth + 1) + c(n_node_samples) - 1` with c(n) = 2 (ln(n - 1) + gamma) -
2 (n - 1) / n for n > 2, c(2) = 1, c(n <= 1) = 0; the leaf values are added in tree order in float64; the score is
`-2 ** (-sum / (T c(max_samples)))`.  The host backend is these numpy expressions and equals scikit-learn bit for bit; the
device backend (csrc/pinn_iforest.hip) forms the same sum bit for bit and differs in the last places of the power only.
`from_sklearn` and `from_arrays` import a fitted forest (duck-typed: scikit-learn is never imported here).

Fitting is the package's own counter-based construction with scikit-learn's rules, not its draws: per tree `max_samples_`
distinct rows (a Feistel permutation of the positions keyed by (seed, tree)), rows as float32, a node splits while depth <
ceil(log2(max_samples_)) and it holds more than one row and some feature is not constant on it, the feature uniform among
the non-constant ones, the threshold uniform in [lo, hi) (Philox4x32-10 at counter (tree, node)), rows with x <= t to the
left.  Both backends run the same state machine on the same draws and give the same trees bit for bit.

Two backends as in detection.py: "device" reads the rows in place (`columns=`, `row_index=`), "host" is numpy.
Also here: `AnomalyMonitor` (online use, next to detection.FaultDetector).  Importing this module needs numpy only.
"""
import functools
import warnings

import numpy as np

from .detection import FEAT_GRP1, parse_features
from ._device import _DevRows, _as_numpy, _is_tensor, _pick_backend, _torch_lib, call, columns_of

# include/pinn_hip.h: PINN_IF_*
MAX_TREES, MAX_SAMPLES, MAX_FEAT, MAX_NODES, MAX_LEAF_VALUES, LDS_NODES = 1024, 1024, 8, 2047, 16384, 4096
_MAGIC, _HDR = 0x49464f52, 16
_H_MAGIC, _H_TREES, _H_NODES, _H_FEAT, _H_LEAF_VALUES, _H_TOTAL_NODES, _H_GROUPS, _H_DEN = range(8)
_OFF_LEAF = _HDR
_OFF_TREE = _OFF_LEAF + MAX_LEAF_VALUES
_OFF_GROUP = _OFF_TREE + (MAX_TREES + 2) // 2
_OFF_NODES = _OFF_GROUP + (MAX_TREES + 2) // 2
_LEAF_BIT = 0x80000000
_DRAW_SPLIT, _DRAW_PERM = 0, 1
_M32 = np.uint64(0xFFFFFFFF)


def _check_limits(T=1, m=1, D=1, nodes=1):
    if not (1 <= T <= MAX_TREES and 1 <= m <= MAX_SAMPLES and 1 <= D <= MAX_FEAT and 1 <= nodes <= MAX_NODES):
        raise NotImplementedError("the isolation forest takes up to %d trees, %d rows per tree, %d features and %d nodes per tree, "
                                  "got %d, %d, %d and %d" % (MAX_TREES, MAX_SAMPLES, MAX_FEAT, MAX_NODES, T, m, D, nodes))


# ---------------------------------------------------------------------------------------------- shared arithmetic
def average_path_length(n):
    """c(n) of scikit-learn's _average_path_length, the same numpy expressions."""
    n = np.asarray(n)
    out = np.zeros(n.shape)
    big = n > 2
    out[n == 2] = 1.0
    nb = n[big]
    out[big] = 2.0 * (np.log(nb - 1.0) + np.euler_gamma) - 2.0 * (nb - 1.0) / nb
    return out


def floor32(t):
    """The largest float32 <= t (float64).  For a float32 x: x <= t exactly when x <= floor32(t), because no float32 lies
    strictly between floor32(t) and t."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(over="ignore"):
        f = t.astype(np.float32)
    up = f.astype(np.float64) > t
    return np.where(up, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 as csrc/pinn_mlp_core.h states it; counters may be arrays.  Returns four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3)])
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for r in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64((k0 + r * 0x9E3779B9) & 0xFFFFFFFF)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64((k1 + r * 0xBB67AE85) & 0xFFFFFFFF)
        c1, c3, c0, c2 = p1 & _M32, p0 & _M32, n0, n2
    return c0, c1, c2, c3


def _mix32(h):
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85ebca6b)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xc2b2ae35)) & _M32
    return h ^ (h >> np.uint64(16))


def subsample_positions(seed, tree, m, n):
    """The m distinct positions of [0, n) that tree `tree` trains on: i = 0..m-1 sent through a four-round Feistel
    permutation of [0, 4^k) (the smallest such range that holds n), walked until it falls below n."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = [np.uint64(int(w)) for w in philox4x32_10(tree, 0, _DRAW_PERM, 0, seed & 0xFFFFFFFF, seed >> 32)]
    bits = max(int(n - 1).bit_length(), 1)
    k = np.uint64((bits + 1) // 2)
    mask = np.uint64((1 << int(k)) - 1)
    v = np.arange(m, dtype=np.uint64)
    todo = np.ones(m, dtype=bool)
    while todo.any():
        w = v[todo]
        L, R = w >> k, w & mask
        for r in range(4):
            L, R = R, L ^ (_mix32(R ^ key[r]) & mask)
        w = (L << k) | R
        v[todo] = w
        todo[todo] = w >= np.uint64(n)
    return v.astype(np.int64)


def max_depth_of(max_samples):
    """ceil(log2(max(max_samples, 2))), in integers."""
    return max(int(max_samples) - 1, 1).bit_length()


# ---------------------------------------------------------------------------------------------- host backend
def _host_fit_tree(Xs, seed, tree, max_depth):
    """One tree on the float32 subsample Xs [m, D]: the state machine of if_fit_kernel.  Returns the five arrays."""
    m, D = Xs.shape
    M = 2 * m - 1
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r0, r1, _, _ = philox4x32_10(tree, np.arange(M), _DRAW_SPLIT, 0, seed & 0xFFFFFFFF, seed >> 32)
    feature, threshold = np.full(M, -2, dtype=np.int64), np.full(M, -2.0)
    left, right, n_node = np.full(M, -1, dtype=np.int64), np.full(M, -1, dtype=np.int64), np.zeros(M, dtype=np.int64)
    stack, count = [(np.arange(m), 0, -1, 0)], 0
    while stack:
        idx, depth, parent, is_right = stack.pop()
        node, count = count, count + 1
        n_node[node] = idx.size
        if parent >= 0:
            (right if is_right else left)[parent] = node
        if idx.size <= 1 or depth >= max_depth:
            continue
        sub = Xs[idx]
        lo, hi = sub.min(axis=0), sub.max(axis=0)
        free = np.flatnonzero(lo < hi)
        if free.size == 0:
            continue
        f = int(free[(int(r0[node]) * free.size) >> 32])
        dlo, dhi = float(lo[f]), float(hi[f])
        t = dlo + (int(r1[node]) * 2.0 ** -32) * (dhi - dlo)
        if t >= dhi:
            t = dlo
        feature[node], threshold[node] = f, t
        goes_left = sub[:, f].astype(np.float64) <= t
        stack.append((idx[~goes_left], depth + 1, node, 1))
        stack.append((idx[goes_left], depth + 1, node, 0))
    return feature[:count], threshold[:count], left[:count], right[:count], n_node[:count]


def tree_depths(left, right):
    """Depth of every node of a tree given as children arrays (any numbering with parents before children or not)."""
    depth = np.zeros(len(left), dtype=np.int64)
    cur = np.array([0])
    d = 0
    while cur.size:
        depth[cur] = d
        inner = cur[left[cur] >= 0]
        cur = np.concatenate([left[inner], right[inner]])
        d += 1
        if d > len(left):
            raise ValueError("the children arrays do not describe a tree")
    return depth


def leaf_values(tree):
    """(depth + 1) + c(n_node_samples) - 1.0 of every node, the float64 numbers scikit-learn adds."""
    _, _, left, right, n_node = tree
    return (tree_depths(left, right) + 1) + average_path_length(n_node) - 1.0


def _host_rows_ok(X, columns, row_index):
    """(rows [n, D] float64, ok [n]): a gather index outside the array reads nothing."""
    a = _as_numpy(X)
    if a.ndim != 2:
        raise ValueError("X must be a 2-D array")
    ok = np.ones(a.shape[0] if row_index is None else np.size(_as_numpy(row_index)), dtype=bool)
    if row_index is not None:
        idx = _as_numpy(row_index, np.int64).reshape(-1)
        ok = (idx >= 0) & (idx < a.shape[0])
        a = a[np.where(ok, idx, 0)] if a.shape[0] else np.zeros((idx.size, a.shape[1]))
    if columns is not None:
        a = a[:, list(columns)]
    return np.ascontiguousarray(a, dtype=np.float64), ok


def _host_depth_sums(trees, values, X, ok):
    """Sum over the trees, in tree order, of the leaf value each row of X (cast to float32) lands on; NaN for a row that was
    not read or is not finite as float32."""
    with np.errstate(over="ignore", invalid="ignore"):
        X32 = X.astype(np.float32)
    ok = ok & np.isfinite(X32).all(axis=1)
    X32 = np.where(ok[:, None], X32, np.float32(0))
    total = np.zeros(X.shape[0])
    rows = np.arange(X.shape[0])
    for (feature, threshold, left, right, _), val in zip(trees, values):
        node = np.zeros(X.shape[0], dtype=np.int64)
        live = rows[feature[node] >= 0]
        while live.size:
            nd = node[live]
            goes_left = X32[live, feature[nd]] <= threshold[nd]            # float32 against float64: compared in float64
            node[live] = np.where(goes_left, left[nd], right[nd])
            live = live[feature[node[live]] >= 0]
        total += val[node]
    total[~ok] = np.nan
    return total


def _scores_from_sums(sums, den):
    ratio = np.divide(sums, den, out=np.ones_like(sums), where=den != 0)
    ratio[np.isnan(sums)] = np.nan
    return -(2 ** (-ratio))


# ---------------------------------------------------------------------------------------------- the forest block
def _bfs_order(feature, left, right):
    """Renumbering with the two children of a node adjacent: (old ids in new order, new left child of every new node,
    depth of every new node)."""
    order, new_left, depth = [np.array([0])], [], []
    nxt, d = 1, 0
    while order[-1].size:
        cur = order[-1]
        inner = feature[cur] >= 0
        nl = np.zeros(cur.size, dtype=np.int64)
        nl[inner] = nxt + 2 * np.arange(int(inner.sum()))
        new_left.append(nl)
        depth.append(np.full(cur.size, d))
        kids = np.stack([left[cur[inner]], right[cur[inner]]], axis=1).reshape(-1)
        nxt += kids.size
        d += 1
        order.append(kids)
        if d > feature.size:
            raise ValueError("the children arrays do not describe a tree")
    return np.concatenate(order), np.concatenate(new_left), np.concatenate(depth)


def pack_forest(trees, max_samples, n_features):
    """The device block of include/pinn_hip.h as a uint64 array, and the per-tree leaf values the host backend adds."""
    T = len(trees)
    _check_limits(T=T, D=n_features, nodes=max(len(t[0]) for t in trees))
    values = [leaf_values(t) for t in trees]
    leaf_all = np.concatenate([v[t[0] < 0] for v, t in zip(values, trees)])
    table, inverse = np.unique(leaf_all, return_inverse=True)
    if table.size > MAX_LEAF_VALUES:
        raise NotImplementedError("the isolation forest takes up to %d distinct leaf values, got %d" % (MAX_LEAF_VALUES, table.size))
    counts = np.array([len(t[0]) for t in trees], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    block = np.zeros(_OFF_NODES + int(off[-1]), dtype=np.uint64)
    groups, used = [0], 0
    for t in range(T):
        if used + counts[t] > LDS_NODES:
            groups.append(t)
            used = 0
        used += int(counts[t])
    groups.append(T)
    hdr = block[:_HDR].view(np.int64)
    hdr[_H_MAGIC], hdr[_H_TREES], hdr[_H_NODES], hdr[_H_FEAT] = _MAGIC, T, int(counts.max()), int(n_features)
    hdr[_H_LEAF_VALUES], hdr[_H_TOTAL_NODES], hdr[_H_GROUPS] = table.size, int(off[-1]), len(groups) - 1
    den = T * average_path_length(np.array([max_samples]))
    block[:_HDR].view(np.float64)[_H_DEN] = den[0]
    block[_OFF_LEAF:_OFF_LEAF + table.size] = table.view(np.uint64)
    block[_OFF_TREE:_OFF_GROUP].view(np.int32)[:T + 1] = off
    block[_OFF_GROUP:_OFF_NODES].view(np.int32)[:len(groups)] = groups
    seen = 0
    for t, (feature, threshold, left, right, _) in enumerate(trees):
        if feature.max(initial=-2) >= n_features:
            raise ValueError("tree %d splits on feature %d, the forest has %d" % (t, feature.max(), n_features))
        order, new_left, _ = _bfs_order(feature, left, right)
        if order.size != feature.size or np.unique(order).size != order.size:
            raise ValueError("the children arrays of tree %d do not describe a tree" % t)
        f = feature[order]
        inner = f >= 0
        n_leaf = int((~inner).sum())
        leaf_idx = np.zeros(order.size, dtype=np.int64)
        pos = np.empty(feature.size, dtype=np.int64)                         # leaf number of an old node, in old order
        pos[np.flatnonzero(feature < 0)] = np.arange(n_leaf)
        leaf_idx[~inner] = inverse[seen + pos[order[~inner]]]
        seen += n_leaf
        w0 = np.where(inner, floor32(threshold[order]).view(np.uint32).astype(np.uint64), leaf_idx.astype(np.uint64))
        w1 = np.where(inner, (new_left | (np.where(inner, f, 0) << 16)).astype(np.uint64), np.uint64(_LEAF_BIT))
        block[_OFF_NODES + off[t]:_OFF_NODES + off[t + 1]] = w0 | (w1 << np.uint64(32))
    return block, values, den


def block_depth_sums(block, X):
    """What if_score_kernel computes from a forest block, in numpy: the float64 depth sums of the rows of X [n, D] (cast to
    float32), from the packed nodes, the float32 thresholds and the leaf table.  For tests of the packing."""
    hdr = block[:_HDR].view(np.int64)
    T = int(hdr[_H_TREES])
    table = block[_OFF_LEAF:_OFF_LEAF + int(hdr[_H_LEAF_VALUES])].view(np.float64)
    off = block[_OFF_TREE:_OFF_GROUP].view(np.int32)[:T + 1]
    X32 = np.asarray(X, dtype=np.float64).astype(np.float32)
    total = np.zeros(X32.shape[0])
    for t in range(T):
        nodes = block[_OFF_NODES + off[t]:_OFF_NODES + off[t + 1]]
        w0, w1 = (nodes & _M32).astype(np.uint32), (nodes >> np.uint64(32)).astype(np.uint32)
        node = np.zeros(X32.shape[0], dtype=np.int64)
        live = np.flatnonzero((w1[node] & _LEAF_BIT) == 0)
        while live.size:
            nd = node[live]
            goes_left = X32[live, (w1[nd] >> 16) & 7] <= w0[nd].view(np.float32)
            node[live] = (w1[nd] & 0xFFFF).astype(np.int64) + np.where(goes_left, 0, 1)
            live = live[(w1[node[live]] & _LEAF_BIT) == 0]
        total += table[w0[node]]
    return total


def _as_tree(t):
    feature, threshold, left, right, n_node = t
    out = (np.ascontiguousarray(feature, dtype=np.int64).reshape(-1), np.ascontiguousarray(threshold, dtype=np.float64).reshape(-1),
           np.ascontiguousarray(left, dtype=np.int64).reshape(-1), np.ascontiguousarray(right, dtype=np.int64).reshape(-1),
           np.ascontiguousarray(n_node, dtype=np.int64).reshape(-1))
    if len({a.size for a in out}) != 1 or out[0].size < 1:
        raise ValueError("the five arrays of a tree must have one length of at least 1")
    return out


_rows = functools.partial(_DevRows.within, on_excess=lambda D: _check_limits(D=D))


# ---------------------------------------------------------------------------------------------- the estimator
class DeviceIsolationForest:
    """Isolation forest with scikit-learn's IsolationForest arguments, defaults and attributes (`max_samples_`, `offset_`,
    `n_features_in_`), plus `trees_` (per tree the five arrays feature, threshold, children_left, children_right,
    n_node_samples in scikit-learn's shape: nodes in pre-order, leaves carry -2, -2.0, -1, -1), `samples_` [n_estimators,
    max_samples_] (the positions every tree was trained on) and `seed_`.  `max_features != 1.0` and `bootstrap=True` are
    not implemented.  `random_state`: an integer seed (None draws one); the trees are the package's own, not scikit-learn's
    draw for draw, and the first k trees of a forest are the forest of k trees.

    `fit`, `score_samples`, `decision_function`, `predict`, `fit_predict`, `depth_sums` take X [n, D], or any array plus
    `columns` (and `row_index`): the device backend then reads the rows in place.  numpy in -> numpy out, device tensor in
    -> device tensors out.  A row that is not finite, or a gather index outside the array, scores NaN (prediction -1)."""

    def __init__(self, n_estimators=100, *, max_samples="auto", contamination="auto", max_features=1.0, bootstrap=False,
                 random_state=None, backend="auto"):
        if max_features != 1.0:
            raise NotImplementedError("max_features=%r: only 1.0 is implemented" % (max_features,))
        if bootstrap:
            raise NotImplementedError("bootstrap=True is not implemented: every tree draws distinct rows")
        if backend not in ("auto", "device", "host"):
            raise ValueError("backend must be 'auto', 'device' or 'host'")
        if int(n_estimators) < 1:
            raise ValueError("n_estimators >= 1 is required")
        if contamination != "auto" and not 0.0 < float(contamination) <= 0.5:
            raise ValueError("contamination must be 'auto' or lie in (0, 0.5]")
        self.n_estimators, self.max_samples, self.contamination = int(n_estimators), max_samples, contamination
        self.max_features, self.bootstrap, self.random_state, self.backend = max_features, bootstrap, random_state, backend
        self._blocks = {}

    # ---- import
    @classmethod
    def from_arrays(cls, trees, max_samples, offset=-0.5, n_features=None, backend="auto"):
        """A forest from per-tree arrays (feature, threshold, children_left, children_right, n_node_samples)."""
        self = cls(n_estimators=len(trees), backend=backend)
        trees = [_as_tree(t) for t in trees]
        if n_features is None:
            n_features = max(1, 1 + max(int(t[0].max()) for t in trees))
        self._set_forest(trees, int(max_samples), int(n_features))
        self.offset_ = float(offset)
        return self

    @classmethod
    def from_sklearn(cls, est, backend="auto"):
        """A fitted scikit-learn IsolationForest (anything with estimators_[i].tree_, max_samples_ and offset_)."""
        trees = []
        for e in est.estimators_:
            t = e.tree_
            trees.append((t.feature, t.threshold, t.children_left, t.children_right, t.n_node_samples))
        feats = getattr(est, "estimators_features_", None)
        n_features = int(getattr(est, "n_features_in_", 0)) or None
        if feats is not None and n_features is not None and any(not np.array_equal(f, np.arange(n_features)) for f in feats):
            raise NotImplementedError("a forest fitted with max_features < 1.0 is not implemented")
        return cls.from_arrays(trees, int(est.max_samples_), float(est.offset_), n_features, backend)

    def _set_forest(self, trees, max_samples, n_features):
        self._block, self._values, self._den = pack_forest(trees, max_samples, n_features)
        self.trees_, self.max_samples_, self.n_features_in_ = trees, int(max_samples), int(n_features)
        self._blocks = {}

    def _check_fitted(self):
        if not hasattr(self, "trees_"):
            raise RuntimeError("this DeviceIsolationForest is not fitted yet")

    # ---- fit
    def _resolve_max_samples(self, n):
        ms = self.max_samples
        if isinstance(ms, str):
            if ms != "auto":
                raise ValueError("max_samples must be 'auto', an int or a float")
            return min(256, n)
        if isinstance(ms, (int, np.integer)):
            if ms < 1:
                raise ValueError("max_samples >= 1 is required")
            if ms > n:
                warnings.warn("max_samples (%d) is greater than the total number of samples (%d): max_samples is set to n_samples" % (ms, n))
                return n
            return int(ms)
        if not 0.0 < float(ms) <= 1.0:
            raise ValueError("a float max_samples must lie in (0, 1]")
        return max(int(float(ms) * n), 1)

    def fit(self, X, y=None, columns=None, row_index=None):
        be = _pick_backend(self.backend, X)
        seed = self.random_state
        if seed is None:
            seed = int(np.random.default_rng().integers(1 << 62))
        if not isinstance(seed, (int, np.integer)):
            raise NotImplementedError("random_state must be an integer or None")
        self.seed_ = int(seed) & 0xFFFFFFFFFFFFFFFF
        if be == "host":
            Xh, ok = _host_rows_ok(X, columns, row_index)
            n, D = Xh.shape
            if n < 1:
                raise ValueError("X holds no rows")
            m = self._resolve_max_samples(n)
            _check_limits(T=self.n_estimators, m=m, D=D)
            depth = max_depth_of(m)
            samples = np.stack([subsample_positions(self.seed_, t, m, n) for t in range(self.n_estimators)])
            trees = []
            for t in range(self.n_estimators):
                with np.errstate(over="ignore", invalid="ignore"):
                    Xs = Xh[samples[t]].astype(np.float32)
                if not (ok[samples[t]].all() and np.isfinite(Xs).all()):
                    raise ValueError("the training rows hold values that are not finite or lie outside the array")
                trees.append(_host_fit_tree(Xs, self.seed_, t, depth))
        else:
            trees, samples, m, D = self._fit_device(X, columns, row_index)
        self._set_forest(trees, m, D)
        self.samples_ = samples
        self.offset_ = -0.5
        if self.contamination != "auto":
            s = _as_numpy(self.score_samples(X, columns=columns, row_index=row_index))
            self.offset_ = float(np.percentile(s, 100.0 * float(self.contamination)))
        return self

    def _fit_device(self, X, columns, row_index):
        torch, _lib, lib = _torch_lib()
        rows = _rows(torch, X, columns, row_index)
        n, D, T = rows.n, rows.D, self.n_estimators
        if n < 1:
            raise ValueError("X holds no rows")
        if n >= 1 << 31:
            raise NotImplementedError("the isolation forest is fitted on fewer than 2^31 positions, got %d" % n)
        m = self._resolve_max_samples(n)
        _check_limits(T=T, m=m, D=D)
        M = 2 * m - 1
        with torch.cuda.device(rows.dev):
            i32 = dict(dtype=torch.int32, device=rows.dev)
            feature, left, right, n_node = (torch.empty(T * M, **i32) for _ in range(4))
            threshold = torch.empty(T * M, dtype=torch.float64, device=rows.dev)
            count, status = torch.empty(T, **i32), torch.empty(T, **i32)
            samples = torch.empty(T * m, dtype=torch.int64, device=rows.dev)
            call("pinn_if_fit", *rows.head(), T, m, max_depth_of(m), self.seed_, feature, threshold, left, right, n_node, count, samples, status)
            count, status = count.cpu().numpy(), status.cpu().numpy()                # the one host read of a fit
            if status.any():
                raise ValueError("the training rows hold values that are not finite or lie outside the array")
            arrs = [a.cpu().numpy().reshape(T, M) for a in (feature, threshold, left, right, n_node)]
            samples = samples.cpu().numpy().reshape(T, m)
        trees = [_as_tree(tuple(a[t, :count[t]] for a in arrs)) for t in range(T)]
        return trees, samples, m, D

    # ---- scoring
    def _device_block(self, torch, dev):
        key = str(dev)
        if key not in self._blocks:
            self._blocks[key] = torch.from_numpy(self._block.view(np.int64)).to(dev)
        return self._blocks[key]

    def _evaluate(self, X, columns, row_index, want, variant=0):
        """dict with the wanted of "sum", "score", "pred"."""
        self._check_fitted()
        if _pick_backend(self.backend, X) == "host":
            Xh, ok = _host_rows_ok(X, columns, row_index)
            if Xh.shape[1] != self.n_features_in_:
                raise ValueError("the forest was fitted on %d features, got %d" % (self.n_features_in_, Xh.shape[1]))
            sums = _host_depth_sums(self.trees_, self._values, Xh, ok)
            score = _scores_from_sums(sums, self._den)
            with np.errstate(invalid="ignore"):
                pred = np.where(score - self.offset_ >= 0, 1, -1).astype(np.int64)
            out = {"sum": sums, "score": score, "pred": pred}
            return {k: out[k] for k in want}
        torch, _lib, lib = _torch_lib()
        rows = _rows(torch, X, columns, row_index)
        if rows.D != self.n_features_in_:
            raise ValueError("the forest was fitted on %d features, got %d" % (self.n_features_in_, rows.D))
        with torch.cuda.device(rows.dev):
            block = self._device_block(torch, rows.dev)
            n = rows.n
            out = {"sum": torch.empty(n, dtype=torch.float64, device=rows.dev) if "sum" in want else None,
                   "score": torch.empty(n, dtype=torch.float64, device=rows.dev) if "score" in want else None,
                   "pred": torch.empty(n, dtype=torch.int64, device=rows.dev) if "pred" in want else None}
            call("pinn_if_score", *rows.head(), block, float(self.offset_), out["sum"], out["score"], out["pred"], int(variant))
        if not _is_tensor(X):
            return {k: out[k].cpu().numpy() for k in want}
        return {k: out[k] for k in want}

    def depth_sums(self, X, columns=None, row_index=None, variant=0):
        """The float64 sum over the trees, in tree order, of the leaf values (for tests and timing)."""
        return self._evaluate(X, columns, row_index, ("sum",), variant)["sum"]

    def score_samples(self, X, columns=None, row_index=None):
        return self._evaluate(X, columns, row_index, ("score",))["score"]

    def decision_function(self, X, columns=None, row_index=None):
        return self.score_samples(X, columns, row_index) - self.offset_

    def predict(self, X, columns=None, row_index=None):
        return self._evaluate(X, columns, row_index, ("pred",))["pred"]

    def fit_predict(self, X, y=None, columns=None, row_index=None):
        return self.fit(X, columns=columns, row_index=row_index).predict(X, columns=columns, row_index=row_index)


class AnomalyMonitor:
    """Anomaly score chunk by chunk: `update(rows)` takes the next rows of the results array [n, >= 17] (device tensor, or
    a host array) and returns (anomaly_score, pred): -score_samples (larger = more anomalous, 02:591) and +1 / -1.  On the
    device a chunk is one kernel launch that reads the feature columns in place; it can run next to detection.FaultDetector."""

    def __init__(self, forest, features=FEAT_GRP1, backend="auto"):
        forest._check_fitted()
        self.forest, self.backend = forest, backend
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            self.columns = columns_of(features, parse_features)
        self.n_seen = 0

    def update(self, rows):
        saved = self.forest.backend
        self.forest.backend = self.backend if self.backend != "auto" else saved
        try:
            r = self.forest._evaluate(rows, self.columns, None, ("score", "pred"))
        finally:
            self.forest.backend = saved
        self.n_seen += int(rows.shape[0])
        return -r["score"], r["pred"]
