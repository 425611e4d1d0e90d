"""Spectral clustering with label-posterior mapping: the `Spectral` baseline of reference script 05 (05:455-512).

scikit-learn's SpectralClustering(affinity="nearest_neighbors", assign_labels="kmeans") is three well-defined pieces, and
each is built here:

  the graph      kneighbors_graph(X, n_neighbors, include_self=True), made symmetric as 0.5 (C + C^T): `knn_graph`,
                 `knn_affinity`.  Neighbours are ordered by (squared distance added in column order, position), so the
                 graph is determined whenever no row has a tie at its last neighbour.
  the embedding  D^{-1/2} times the eigenvectors of the K largest eigenvalues of S = D^{-1/2} A D^{-1/2} (A without its
                 diagonal, D its row sums), every column with scikit-learn's sign: `spectral_embedding`.  k-means on the
                 rows sees Euclidean distances only, which a rotation inside the subspace does not change: the target is
                 the invariant subspace, defined whenever theta_K > theta_{K+1}.  It is found by Chebyshev-filtered
                 subspace iteration on a block of min(n, K + 16) columns from a start block drawn on the host.
  the labels     k-means on the rows of the embedding: k-means++ seeds by the package's own draws (DeviceKMeans._picks),
                 `n_init` restarts, the lowest inertia kept.  As for `KMeans`, these are not scikit-learn's draws.

`DeviceSpectralClustering` carries scikit-learn's argument names and attributes, `fit_spectral_posterior` is script 05's
function, and `comparison.spectral_extras()` hands it to `compare_methods`.

Two backends, as in comparison.py.  "device": the HIP kernels of csrc/pinn_spectral.hip (float64, fixed summation order,
launches queued without a host synchronisation; the header of the eigen state is read once per chunk of outer
iterations).  "host": float64 numpy running the same steps (the small dense eigenproblems by numpy.linalg.eigh), for
machines without a GPU and as the referee of the device tests.  numpy in -> numpy out, device tensor in -> device tensors
out.  Importing this module needs numpy only; neither scipy nor scikit-learn is imported.
"""
import math
import warnings

import numpy as np

from ._device import _DevRows, _as_numpy, _dev_vec, _host_rows, _is_tensor, _on_gpu, _pick_backend, _torch_lib, call
from .comparison import _HDR, DeviceKMeans, _Lloyd, _host_lloyd, _host_step, _posterior_from, host_tolerance

MAX_FEAT, MAX_NEIGHBORS, MAX_COMPONENTS, MAX_CLUSTERS, MAX_DIM, MAX_ROWS = 8, 32, 32, 32, 32, 1 << 24
GUARD, MAX_DEGREE, GROWTH = 16, 40, 1e8          # block columns beyond K; Chebyshev steps of a filter; its largest growth
KM_MAX_ITER, KM_TOL = 300, 1e-4                  # scikit-learn's k_means defaults, which SpectralClustering does not change


def _check_limits(D=1, k=1, K=1, n_clusters=1, n=1):
    if not (1 <= D <= MAX_FEAT and 1 <= k <= MAX_NEIGHBORS and 1 <= K <= MAX_COMPONENTS and 1 <= n_clusters <= MAX_CLUSTERS and n <= MAX_ROWS):
        raise NotImplementedError("the device backend takes up to %d features, %d neighbours, %d components, %d clusters and %d rows, got %d, "
                                  "%d, %d, %d and %d" % (MAX_FEAT, MAX_NEIGHBORS, MAX_COMPONENTS, MAX_CLUSTERS, MAX_ROWS, D, k, K, n_clusters, n))


def _rows(torch, X, columns, row_index):
    return _DevRows.within(torch, X, columns, row_index, on_excess=lambda D: _check_limits(D=D))


def block_columns(n, K):
    return min(int(n), int(K) + GUARD)


def filter_degree(a):
    """(c, e, degree) of the Chebyshev filter that damps [-1, a]: the largest degree <= 40 whose growth at 1 stays <= 1e8."""
    a = max(float(a), -0.99)
    c, e = (a - 1.0) / 2.0, (a + 1.0) / 2.0
    r = (1.0 - c) / e
    deg = MAX_DEGREE
    while deg > 1 and not (r >= 1.0 and math.cosh(deg * math.acosh(r)) <= GROWTH):
        deg -= 1
    return c, e, deg


# ---------------------------------------------------------------------------------------------- host backend
def _host_valid_rows(X, columns, row_index):
    """(rows [n, D], valid [n]): a gather index outside the array reads nothing."""
    if row_index is None:
        Xh = _host_rows(X, columns, None)
        return Xh, np.ones(Xh.shape[0], dtype=bool)
    a = _as_numpy(X)
    if a.ndim != 2:
        raise ValueError("X must be a 2-D array")
    r = _as_numpy(row_index, np.int64).reshape(-1)
    valid = (r >= 0) & (r < a.shape[0])
    a = a[np.where(valid, r, 0)]
    if columns is not None:
        a = a[:, list(columns)]
    a = np.ascontiguousarray(a, dtype=np.float64)
    a[~valid] = 0.0
    return a, valid


def _host_knn(X, valid, k, include_self, rows_per_pass=512):
    n, D = X.shape
    idx, dist = np.full((n, k), -1, dtype=np.int64), np.full((n, k), np.nan)
    for lo in range(0, n, rows_per_pass):
        hi = min(n, lo + rows_per_pass)
        d2 = np.zeros((hi - lo, n))
        for c in range(D):                                   # added in column order, as the kernel does
            d = X[lo:hi, c][:, None] - X[None, :, c]
            d2 += d * d
        d2[:, ~valid] = np.inf
        if not include_self:
            d2[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
        order = np.argsort(d2, axis=1, kind="stable")[:, :k]               # stable: equal distances by position
        dd = np.take_along_axis(d2, order, axis=1)
        found = np.isfinite(dd) | np.isnan(dd)
        idx[lo:hi, :order.shape[1]] = np.where(found, order, -1)
        dist[lo:hi, :order.shape[1]] = np.where(found, dd, np.nan)
    idx[~valid], dist[~valid] = -1, np.nan
    return idx, dist


def _host_affinity(knn, n):
    """CSR of 0.5 (C + C^T) without its diagonal, columns ascending: indptr, indices, data, degree."""
    knn = np.asarray(knn, dtype=np.int64).reshape(n, -1)
    i = np.repeat(np.arange(n, dtype=np.int64), knn.shape[1])
    j = knn.reshape(-1)
    ok = (j >= 0) & (j < n) & (j != i)
    directed = np.unique(i[ok] * n + j[ok])
    key, counts = np.unique(np.concatenate([directed, (directed % n) * n + directed // n]), return_counts=True)
    rows, cols, data = key // n, key % n, 0.5 * counts
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    degree = np.bincount(rows, weights=data, minlength=n).astype(np.float64)
    return indptr, cols.astype(np.int64), data.astype(np.float64), degree


def _inverse_roots(dd):
    return np.where(dd > 0, 1.0 / np.where(dd > 0, dd, 1.0), 0.0)


def _host_spmm(indptr, indices, data, rdd, Z):
    """S Z with S = D^{-1/2} A D^{-1/2}; a row without an edge has S_ii = 1."""
    out = np.zeros_like(Z)
    if len(indices):
        prod = data[:, None] * (Z * rdd[:, None])[indices]
        some = indptr[1:] > indptr[:-1]
        out[some] = np.add.reduceat(prod, indptr[:-1][some], axis=0)
    out *= rdd[:, None]
    lone = ~(rdd > 0)
    out[lone] = Z[lone]
    return out


def _host_ortho(Y):
    """Y diag(G)^{-1/2} U Lambda^{-1/2} with G = Y^T Y scaled to unit diagonal, Lambda floored at 1e-15 of its largest."""
    g = np.einsum("ij,ij->j", Y, Y)
    s = np.where(g > 0, 1.0 / np.sqrt(np.where(g > 0, g, 1.0)), 0.0)
    G = (Y.T @ Y) * np.outer(s, s)
    lam, U = np.linalg.eigh(0.5 * (G + G.T))
    lam, U = lam[::-1], U[:, ::-1]
    lam = np.maximum(lam, 1e-15 * lam[0])
    return Y @ (s[:, None] * U / np.sqrt(lam))


def _host_eigs(indptr, indices, data, dd, K, Q0, tol, max_iter):
    rdd = _inverse_roots(dd)
    Q = _host_ortho(_host_ortho(np.array(Q0, dtype=np.float64)))
    m = Q.shape[1]
    n_iter, n_matvec, degree, converged = 0, 0, 0, False
    theta, res = np.full(m, np.nan), np.full(m, np.inf)
    while n_iter < max_iter:
        SQ = _host_spmm(indptr, indices, data, rdd, Q)
        H = Q.T @ SQ
        theta, V = np.linalg.eigh(0.5 * (H + H.T))
        theta, V = theta[::-1], V[:, ::-1]
        Q, SQ = Q @ V, SQ @ V
        res = np.sqrt(np.einsum("ij,ij->j", SQ - Q * theta, SQ - Q * theta))
        n_iter, n_matvec = n_iter + 1, n_matvec + 1
        if not np.all(np.isfinite(res)) or not np.all(np.isfinite(theta)):
            raise ValueError("the affinity matrix or the start block holds values that are not finite")
        if res[:K].max() <= tol:
            converged = True
            break
        c, e, degree = filter_degree(theta[-1])
        n_matvec += degree
        Y0, Y1 = Q, (SQ - c * Q) / e
        for _ in range(1, degree):
            Y0, Y1 = Y1, 2.0 * (_host_spmm(indptr, indices, data, rdd, Y1) - c * Y1) / e - Y0
        Q = _host_ortho(_host_ortho(Y1))
    return {"Q": Q, "theta": theta, "res": res, "n_iter": n_iter, "n_matvec": n_matvec, "degree": degree, "converged": converged}


def _host_embed(Q, dd, K):
    E = Q[:, :K] / np.where(dd > 0, dd, 1.0)[:, None]
    top = np.argmax(np.abs(E), axis=0)                      # the first of equals, scikit-learn's _deterministic_vector_sign_flip
    return E * np.where(E[top, np.arange(K)] < 0, -1.0, 1.0)


# ---------------------------------------------------------------------------------------------- the graph
def _check_graph_args(n, k):
    if int(k) < 1:
        raise ValueError("n_neighbors >= 1 is required")
    if int(k) > n:
        raise ValueError("Expected n_neighbors <= n_samples, got n_neighbors = %d, n_samples = %d" % (k, n))


def knn_graph(X, n_neighbors=10, include_self=True, columns=None, row_index=None, backend="auto"):
    """The `n_neighbors` nearest rows of every row by (sum (x_i - y_i)^2 added in column order, position), the row itself
    among them when include_self.  dict: `indices` [n, k] (64-bit), `dist2` [n, k], `status` (0, or 2 when a gather index
    lay outside the array: such a position has no neighbours, (-1, NaN), and is nobody's neighbour)."""
    k = int(n_neighbors)
    if _pick_backend(backend, X) == "host":
        Xh, valid = _host_valid_rows(X, columns, row_index)
        _check_graph_args(Xh.shape[0], k)
        idx, dist = _host_knn(Xh, valid, k, bool(include_self))
        return {"indices": idx, "dist2": dist, "status": 0 if valid.all() else 2}
    torch, _lib, lib = _torch_lib()
    rows = _rows(torch, X, columns, row_index)
    _check_graph_args(rows.n, k)
    _check_limits(D=rows.D, k=k, n=rows.n)
    with torch.cuda.device(rows.dev):
        idx = torch.empty(rows.n, k, dtype=torch.int64, device=rows.dev)
        dist = torch.empty(rows.n, k, dtype=torch.float64, device=rows.dev)
        status = torch.zeros(1, dtype=torch.int64, device=rows.dev)
        call("pinn_sp_knn", *rows.head(), k, 1 if include_self else 0, idx, dist, status)
    if not _is_tensor(X):
        return {"indices": idx.cpu().numpy(), "dist2": dist.cpu().numpy(), "status": int(status.item())}
    return {"indices": idx, "dist2": dist, "status": status}


def knn_affinity(X=None, n_neighbors=10, include_self=True, columns=None, row_index=None, backend="auto", knn=None):
    """The affinity scikit-learn's SpectralClustering(affinity="nearest_neighbors") builds, 0.5 (C + C^T) of the
    connectivity C of `knn_graph`, as CSR without its diagonal (the Laplacian ignores it) and with ascending columns.
    dict: `indptr` [n + 1], `indices`, `data` (0.5 or 1.0), `degree` [n] = A 1.  `knn`: neighbour lists [n, k] to start from
    instead of X (entries outside [0, n) are skipped)."""
    if knn is None:
        knn = knn_graph(X, n_neighbors, include_self, columns, row_index, backend)["indices"]
        as_tensor = _is_tensor(X)
    else:
        as_tensor = _is_tensor(knn)
    if _pick_backend(backend, knn) == "host":
        lists = _as_numpy(knn, np.int64)
        indptr, indices, data, degree = _host_affinity(lists, lists.shape[0])
        return {"indptr": indptr, "indices": indices, "data": data, "degree": degree}
    torch, _lib, lib = _torch_lib()
    lists = knn if _on_gpu(knn) else torch.from_numpy(np.ascontiguousarray(_as_numpy(knn, np.int64))).cuda()
    lists = lists.to(torch.int64).contiguous()
    n, k = int(lists.shape[0]), int(lists.shape[1])
    _check_limits(k=k, n=n)
    dev = lists.device
    with torch.cuda.device(dev):
        indptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        indices = torch.empty(2 * n * k, dtype=torch.int64, device=dev)
        data = torch.empty(2 * n * k, dtype=torch.float64, device=dev)
        degree, dd = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
        wb = lib.pinn_sp_affinity_workspace_bytes(n, k)
        ws = torch.empty(wb, dtype=torch.uint8, device=dev)
        call("pinn_sp_affinity", n, k, lists, indptr, indices, data, degree, dd, ws, wb)
        nnz = int(indptr[-1].item())
        out = {"indptr": indptr, "indices": indices[:nnz].clone(), "data": data[:nnz].clone(), "degree": degree}
    if not as_tensor:
        out = {key: v.cpu().numpy() for key, v in out.items()}
    return out


# ---------------------------------------------------------------------------------------------- the embedding
def _eig_header(st):
    h = st[:_HDR].cpu().numpy()
    i = h.view(np.int64)
    return {"n_iter": int(i[0]), "converged": bool(i[1]), "status": int(i[2]), "n_matvec": int(i[6]), "degree": int(i[7]), "max_residual": float(h[8])}


def spectral_embedding(affinity, n_components, tol=1e-10, max_iter=100, random_state=None, backend="auto", chunk=4):
    """scikit-learn's spectral_embedding(..., drop_first=False) of the CSR `affinity` (the dict of `knn_affinity`): the rows
    of D^{-1/2} [q_1 .. q_K], q_j the eigenvectors of the K = n_components largest eigenvalues of S = D^{-1/2} A D^{-1/2},
    by Chebyshev-filtered subspace iteration from `default_rng(random_state).normal(size=(n, m))`, m = min(n, K + 16), drawn
    on the host in both backends.  The columns span scikit-learn's subspace; inside a cluster of eigenvalues they need not
    be its vectors.  dict: `embedding` [n, K], `eigenvalues` [K] (of S, descending; the Laplacian's are 1 - theta),
    `residuals` [K] = |S q - theta q|, `eigengap` = theta_K - theta_{K+1} from the block (inf when the block has no further
    column), `n_iter` (outer iterations), `n_matvec` (products of S with the block), `converged` (every residual <= tol;
    it stays False after max_iter iterations, which happens when more than K eigenvalues equal 1: a graph of more than K
    components has no defined subspace), and `vectors` [n, K] (the orthonormal q_j).  `chunk`: outer iterations queued
    between two reads of the state's header."""
    K = int(n_components)
    indptr = affinity["indptr"]
    n = int(indptr.shape[0]) - 1
    if K < 1 or K > n:
        raise ValueError("1 <= n_components <= n_samples is required, got %d and %d" % (K, n))
    if int(max_iter) < 1 or int(chunk) < 1 or not tol >= 0:
        raise ValueError("max_iter >= 1, chunk >= 1 and tol >= 0 are required")
    m = block_columns(n, K)
    Q0 = np.random.default_rng(random_state).normal(size=(n, m))
    as_tensor = _is_tensor(indptr)
    if _pick_backend(backend, indptr) == "host":
        ip, ix, da = _as_numpy(indptr, np.int64), _as_numpy(affinity["indices"], np.int64), _as_numpy(affinity["data"], np.float64)
        dd = np.sqrt(_as_numpy(affinity["degree"], np.float64))
        r = _host_eigs(ip, ix, da, dd, K, Q0, float(tol), int(max_iter))
        theta, res = r["theta"], r["res"]
        out = {"embedding": _host_embed(r["Q"], dd, K), "vectors": r["Q"][:, :K].copy(), "eigenvalues": theta[:K].copy(), "residuals": res[:K].copy()}
        h = r
    else:
        torch, _lib, lib = _torch_lib()
        _check_limits(K=K, n=n)
        dev = indptr.device if _on_gpu(indptr) else torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(dev):
            ip, ix = _dev_vec(torch, indptr, torch.int64, dev), _dev_vec(torch, affinity["indices"], torch.int64, dev)
            da = _dev_vec(torch, affinity["data"], torch.float64, dev)
            dd = torch.sqrt(_dev_vec(torch, affinity["degree"], torch.float64, dev))
            nnz = int(ix.numel())
            if int(da.numel()) != nnz or int(dd.numel()) != n:
                raise ValueError("indices and data must have one length, degree one entry per row")
            st = torch.zeros(lib.pinn_sp_eigs_state_bytes(n, K) // 8, dtype=torch.float64, device=dev)
            st[_HDR + 2 * m:] = torch.from_numpy(Q0.reshape(-1)).to(dev)
            wb = lib.pinn_sp_eigs_workspace_bytes(n, K)
            ws = torch.empty(wb, dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream().cuda_stream
            done, init = 0, 1
            while True:
                step = min(int(chunk), int(max_iter) - done)
                call("pinn_sp_eigs", n, ip, ix, da, nnz, dd, K, init, step, float(tol), st, ws, wb, stream=stream)
                done, init = done + step, 0
                h = _eig_header(st)                              # one read of the header per chunk
                if h["converged"] or h["status"] or done >= int(max_iter):
                    break
            if h["status"]:
                raise ValueError("the affinity matrix or the start block holds values that are not finite (status %d)" % h["status"])
            E = torch.empty(n, K, dtype=torch.float64, device=dev)
            call("pinn_sp_embed", n, K, dd, st, E, ws, wb, stream=stream)
            theta, res = st[_HDR:_HDR + m].cpu().numpy(), st[_HDR + m:_HDR + 2 * m].cpu().numpy()
            out = {"embedding": E, "vectors": st[_HDR + 2 * m:].reshape(n, m)[:, :K].clone(), "eigenvalues": torch.from_numpy(theta[:K].copy()).to(dev),
                   "residuals": torch.from_numpy(res[:K].copy()).to(dev)}
        if not as_tensor:
            out = {key: v.cpu().numpy() for key, v in out.items()}
    out.update(eigengap=float(theta[K - 1] - theta[K]) if m > K else float("inf"), n_iter=h["n_iter"], n_matvec=h["n_matvec"],
               converged=bool(h["converged"]), degree=h["degree"])
    return out


# ---------------------------------------------------------------------------------------------- k-means on wide rows
def _wide(E, K):
    """(_Lloyd on the packed rows E as a float64 device block, that block's device)."""
    torch, _lib, lib = _torch_lib()
    Ed = E if _on_gpu(E) else torch.from_numpy(np.ascontiguousarray(_as_numpy(E, np.float64))).cuda()
    if Ed.dim() != 2:
        raise ValueError("the rows must be a 2-D array")
    Ed = Ed.detach().to(torch.float64).contiguous()
    n, Dm = int(Ed.shape[0]), int(Ed.shape[1])
    if not (1 <= Dm <= MAX_DIM):
        raise NotImplementedError("the device backend takes rows of up to %d columns, got %d" % (MAX_DIM, Dm))
    _check_limits(n_clusters=K, n=n)
    return _Lloyd(torch, lib, "pinn_sp_lloyd", (Ed, n, Dm), n, Dm, Ed.device), torch.cuda.device(Ed.device)


def wide_lloyd_iteration(E, centres, tol=KM_TOL, backend="auto"):
    """One Lloyd iteration on the packed rows E [n, Dm <= 32] from `centres` [K <= 32, Dm], for tests and timing: the dict
    of comparison.lloyd_iteration."""
    c0 = _as_numpy(centres, np.float64)
    K = c0.shape[0]
    if _pick_backend(backend, E) == "host":
        Eh = np.ascontiguousarray(_as_numpy(E, np.float64))
        lab, S, A, new, shift, margin = _host_step(Eh, c0)
        return {"labels": lab, "sums": S, "abs_sums": A, "centres": new, "shift": shift, "inertia": float(S[:, 1 + c0.shape[1]:].sum()),
                "tol_abs": host_tolerance(Eh, tol), "margin": margin}
    lloyd, device = _wide(E, K)
    with device:
        return lloyd.probe(K, c0, tol, _is_tensor(E))


def wide_lloyd(E, centres, max_iter=KM_MAX_ITER, tol=KM_TOL, backend="auto", chunk=16):
    """Lloyd's k-means on the packed rows E [n, Dm] from `centres` with scikit-learn's stopping rule (DeviceKMeans's, an
    empty cluster keeps its centre).  dict: centres, labels, inertia, n_iter, strict."""
    c0 = _as_numpy(centres, np.float64)
    K = c0.shape[0]
    if _pick_backend(backend, E) == "host":
        Eh = np.ascontiguousarray(_as_numpy(E, np.float64))
        cen, lab, inertia, n_iter, strict = _host_lloyd(Eh, c0, int(max_iter), host_tolerance(Eh, tol))
        return {"centres": cen, "labels": lab, "inertia": inertia, "n_iter": n_iter, "strict": strict}
    lloyd, device = _wide(E, K)
    with device:
        st, h = lloyd.run(K, c0, int(max_iter), float(tol), int(chunk))
        out = dict(zip(("centres", "labels"), lloyd.result(st, K)))
    if not _is_tensor(E):
        out = {key: v.cpu().numpy() for key, v in out.items()}
    out.update(inertia=h["inertia"], n_iter=h["n_iter"], strict=h["strict"])
    return out


def _kmeans_restarts(E, n_clusters, n_init, rng, backend):
    """k-means on the rows of E: k-means++ seeds by DeviceKMeans._picks from the generator `rng`, the lowest inertia kept."""
    seeder = DeviceKMeans(n_clusters=n_clusters, backend=backend)
    best = None
    for _ in range(int(n_init)):
        if _on_gpu(E):
            import torch
            c0 = seeder._device_seeds(torch, rng, E)
        else:
            c0 = seeder._host_seeds(rng, E)
        run = wide_lloyd(E, c0, backend=backend)
        if best is None or run["inertia"] < best["inertia"]:
            best = run
    return best


# ---------------------------------------------------------------------------------------------- the estimator
def label_means(X, labels, n_clusters, columns=None, row_index=None, backend="auto"):
    """[n_clusters, D]: the mean of the rows of every label in feature space, zero for a label without rows (05:483-489)."""
    K = int(n_clusters)
    if _pick_backend(backend, X) == "host":
        Xh, lab = _host_rows(X, columns, row_index), _as_numpy(labels)
        return np.stack([Xh[lab == c].mean(axis=0) if np.any(lab == c) else np.zeros(Xh.shape[1]) for c in range(K)])
    torch, _lib, lib = _torch_lib()
    rows = _rows(torch, X, columns, row_index)
    _check_limits(D=rows.D, n_clusters=K)
    with torch.cuda.device(rows.dev):
        lab = _dev_vec(torch, labels, torch.int64, rows.dev)
        wb = lib.pinn_km_workspace_bytes(rows.n, K, rows.D)
        ws = torch.empty(wb, dtype=torch.uint8, device=rows.dev)
        means = torch.zeros(K, rows.D, dtype=torch.float64, device=rows.dev)
        for _ in range(2):                                    # the second pass sums x - mean: exact to rounding at any offset
            call("pinn_cluster_means", *rows.head(), K, lab, means, None, ws, wb)
    return means if _is_tensor(X) else means.cpu().numpy()


class DeviceSpectralClustering:
    """Spectral clustering with scikit-learn's SpectralClustering argument names, for the configuration script 05 uses.

    Built: `affinity="nearest_neighbors"` (the default here; scikit-learn's is "rbf"), `assign_labels="kmeans"`,
    `eigen_solver=None` (the package's own solver; scikit-learn's default means ARPACK, which finds the same subspace).
    `affinity="rbf"`, `"precomputed"` and the other kernels, `assign_labels="discretize"` or `"cluster_qr"` and
    `eigen_solver="arpack"`, `"lobpcg"` or `"amg"` raise NotImplementedError.  `n_components` defaults to `n_clusters`;
    `eigen_tol` is the residual |S q - theta q| every kept eigenvector reaches (default 1e-10); `eigen_max_iter` bounds the
    outer iterations.  k-means on the embedding draws its k-means++ seeds from the package's own generator seeded by
    `random_state` (they are not scikit-learn's draws; the one generator first gives the eigen stage its start block, as
    scikit-learn threads one RandomState through both stages), runs `n_init` times and keeps the lowest inertia.

    Attributes: `labels_`, `affinity_matrix_` (the CSR dict of knn_affinity), `embedding_` [n, n_components],
    `eigenvalues_` (of S, descending), `eigengap_`, `converged_`, `n_iter_`, `n_matvec_`, `n_features_in_`, `inertia_` (of
    the kept restart) and `cluster_means_` [n_clusters, D]: the mean of every cluster's rows in feature space, zero for a
    cluster without rows (05:483-489), which `predict` assigns new rows to.  An eigen stage that did not converge, or
    `eigengap_ <= eigen_tol` (zero to the accuracy of the eigenvalues), warns once and goes on: the subspace is not defined
    then, and scikit-learn's answer is as arbitrary.

    `fit`, `fit_predict` and `predict` take X as a [n, D] array, or any array plus `columns` (and `row_index`).  numpy in ->
    numpy out, device tensor in -> device tensors out."""

    def __init__(self, n_clusters=8, *, eigen_solver=None, n_components=None, random_state=None, n_init=10, gamma=1.0,
                 affinity="nearest_neighbors", n_neighbors=10, eigen_tol=1e-10, assign_labels="kmeans", degree=3, coef0=1, kernel_params=None,
                 n_jobs=None, verbose=False, backend="auto", eigen_max_iter=100, chunk=4):
        if affinity != "nearest_neighbors":
            raise NotImplementedError("affinity=%r: only 'nearest_neighbors' is implemented" % (affinity,))
        if assign_labels != "kmeans":
            raise NotImplementedError("assign_labels=%r: only 'kmeans' is implemented" % (assign_labels,))
        if eigen_solver is not None:
            raise NotImplementedError("eigen_solver=%r: only None (the package's subspace iteration) is implemented" % (eigen_solver,))
        if backend not in ("auto", "device", "host"):
            raise ValueError("backend must be 'auto', 'device' or 'host'")
        if eigen_tol == "auto":
            eigen_tol = 1e-10
        if int(n_clusters) < 1 or int(n_init) < 1 or int(n_neighbors) < 1 or (n_components is not None and int(n_components) < 1):
            raise ValueError("n_clusters >= 1, n_init >= 1, n_neighbors >= 1 and n_components >= 1 are required")
        self.n_clusters, self.n_components, self.random_state, self.n_init = int(n_clusters), n_components, random_state, int(n_init)
        self.affinity, self.n_neighbors, self.eigen_tol, self.assign_labels = affinity, int(n_neighbors), float(eigen_tol), assign_labels
        self.eigen_solver, self.backend, self.eigen_max_iter, self.chunk = eigen_solver, backend, int(eigen_max_iter), int(chunk)

    def _check_fitted(self):
        if not hasattr(self, "cluster_means_"):
            raise RuntimeError("this DeviceSpectralClustering is not fitted yet")

    def fit(self, X, y=None, columns=None, row_index=None):
        backend = _pick_backend(self.backend, X)
        K = self.n_clusters if self.n_components is None else int(self.n_components)
        D = len(columns) if columns is not None else int(X.shape[1])
        n = int(X.shape[0]) if row_index is None else int(np.prod(row_index.shape))
        if n < self.n_clusters:
            raise ValueError("n_samples=%d should be >= n_clusters=%d" % (n, self.n_clusters))
        if backend == "device":
            _check_limits(D=D, k=self.n_neighbors, K=K, n_clusters=self.n_clusters, n=n)
            if not _is_tensor(X):
                import torch
                X = torch.from_numpy(np.ascontiguousarray(_as_numpy(X, np.float64))).cuda()      # one copy; every stage then stays on the device
                back = True
            else:
                back = False
        else:
            back = False
        rng = np.random.default_rng(self.random_state)       # one generator through both stages, as scikit-learn threads its RandomState
        A = knn_affinity(X, self.n_neighbors, True, columns, row_index, backend)
        emb = spectral_embedding(A, K, tol=self.eigen_tol, max_iter=self.eigen_max_iter, random_state=rng, backend=backend, chunk=self.chunk)
        if not emb["converged"] or not emb["eigengap"] > self.eigen_tol:
            warnings.warn("the eigen stage %s (eigengap %.3e, largest residual %.3e after %d iterations): the subspace of the %d largest "
                          "eigenvalues is not well defined, as when the graph has more than %d components; the labels are one of many answers"
                          % ("converged" if emb["converged"] else "did not converge", emb["eigengap"], float(_as_numpy(emb["residuals"]).max()),
                             emb["n_iter"], K, K), RuntimeWarning, stacklevel=2)
        run = _kmeans_restarts(emb["embedding"], self.n_clusters, self.n_init, rng, backend)
        means = label_means(X, run["labels"], self.n_clusters, columns, row_index, backend)

        def out(v):
            return v.cpu().numpy() if back else v
        self.labels_, self.embedding_, self.eigenvalues_ = out(run["labels"]), out(emb["embedding"]), out(emb["eigenvalues"])
        self.affinity_matrix_ = {key: out(v) for key, v in A.items()}
        self.cluster_means_ = out(means)
        self.eigengap_, self.converged_, self.n_iter_, self.n_matvec_ = emb["eigengap"], emb["converged"], emb["n_iter"], emb["n_matvec"]
        self.inertia_, self.n_features_in_ = run["inertia"], D
        return self

    def predict(self, X, columns=None, row_index=None):
        """The cluster whose mean in feature space is nearest (05:505-506), as DeviceWard.predict."""
        from .comparison import assign_clusters
        self._check_fitted()
        return assign_clusters(X, self.cluster_means_, None, columns, row_index, self.backend)["cluster"]

    def fit_predict(self, X, y=None, columns=None, row_index=None):
        return self.fit(X, columns=columns, row_index=row_index).labels_


def fit_spectral_posterior(X_tr, y_tr, X_te, n_classes, random_state=42, n_clusters=None, backend="auto", return_details=False, **sc_args):
    """Spectral clustering of X_tr (10 neighbours, 10 k-means restarts), the mean of every cluster's rows as its centre,
    P(class | cluster) from y_tr, every row of X_te gets the distribution of its nearest centre (05:455-512).  Returns
    y_pred [n_te]; with return_details=True a dict (y_pred, y_prob, cluster, model, cluster_class_prob).  `sc_args`:
    further DeviceSpectralClustering arguments."""
    if n_clusters is None:
        n_clusters = n_classes
    args = {"n_neighbors": 10, "n_init": 10}
    args.update(sc_args)
    sc = DeviceSpectralClustering(n_clusters=n_clusters, random_state=random_state, affinity="nearest_neighbors", assign_labels="kmeans",
                                  backend=backend, **args).fit(X_tr)
    return _posterior_from(sc, sc.cluster_means_, sc.labels_, y_tr, X_te, n_clusters, n_classes, backend, return_details)
