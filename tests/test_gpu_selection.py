"""GPU: the batched sweep of pinn_amd.selection (the pinn_gmm_batch_* entry points of csrc/pinn_gmm.hip) against the single
device fit, bit for bit, and against the host referee.

A candidate (K, seed) is DeviceGMM(K, random_state=seed).fit(X).  Gates: a candidate's state block equals the single device
fit's byte for byte whatever else is in the batch (same code, same order of every sum; the k-means++ picks are compared
only where the host finds a pick margin of 1e-9 x total, far above what the order of a sum of n <= 2e5 float64 terms can
move, n x 1.1e-16); against the host, as DESIGN 3g gates a full fit: n_iter equal and parameters within 10 x the
sensitivity of the referee to 1e-13 relative input noise (not below 1e-13), moment sums within 1e-12 x the sum of their
absolute terms, log-likelihood sums within 1e-12 x the sum of |log_prob_norm|.  Every comparison prints its maxima before
it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import selection_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    from pinn_amd import selection
    return selection


@pytest.fixture(scope="module")
def D():
    from pinn_amd import diagnosis
    return diagnosis


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def state_bytes(sw, i):
    from pinn_amd.diagnosis import _state_words
    return sw._states[i, :_state_words(int(sw.n_components[i]), sw.n_features)].cpu().numpy().tobytes()


def assert_margin(X, K, seed):
    picks, margin = SC.host_picks(X, K, seed)
    assert margin >= 1e-9, "the host's k-means++ draws for K=%d seed %d come within %.1e of a boundary" % (K, seed, margin)
    return picks


def one(S, X, K, seed, **kw):
    return S.gmm_sweep(X, (K,), (seed,), backend="device", **kw)


def seed_picks(X, cands):
    """pinn_gmm_batch_seed alone: the positions it picks, [B][Kmax] (unused slots -1), and the centres it writes."""
    from pinn_amd import _device, _lib, selection
    lib = _lib.load()
    rows = _device._DevRows(torch, X)
    B, Kmax = len(cands), max(K for K, _ in cands)
    stride = lib.pinn_gmm_batch_state_stride(Kmax, rows.D) // 8
    wb = lib.pinn_gmm_batch_workspace_bytes(rows.n, B, Kmax, rows.D)
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    st = torch.zeros(B, stride, dtype=torch.float64, device="cuda")
    draws = [selection._draws(rows.n, K, s) for K, s in cands]
    u = np.zeros((B, max(Kmax - 1, 1)))
    for c, d in enumerate(draws):
        u[c, :len(d[1])] = d[1]
    picks = torch.full((B, Kmax), -1, dtype=torch.int64, device="cuda")
    ncomp = (ctypes.c_int * B)(*[K for K, _ in cands])
    _device.call("pinn_gmm_batch_seed", *rows.head(), B, ncomp, Kmax, dev(np.array([d[0] for d in draws], dtype=np.int64)), dev(u), st, picks, ws, wb)
    torch.cuda.synchronize()
    return picks.cpu().numpy(), st.cpu().numpy()


def test_seed_kernel_picks_what_the_host_picks():
    G = SC.fixture()
    dup = np.repeat(SC.clustered(40, 3, 2, seed=1), 3, axis=0)            # every row three times
    same = np.ones((10, 2))                                               # total 0: every draw picks n - 1
    for name, X, cands in (("fixture", G["X_tr"], [(20, 42), (1, 3), (32, 0), (8, 2)]), ("duplicate rows", dup, [(6, 0), (6, 1), (2, 2)]),
                           ("identical rows", same, [(3, 0), (1, 1)]), ("one row", np.array([[2.5]]), [(1, 0)])):
        want = [assert_margin(X, K, s) for K, s in cands]
        got, st = seed_picks(X, cands)
        print(name, "host picks", want, "device picks", [list(got[c, :K]) for c, (K, _) in enumerate(cands)])
        for c, (K, _) in enumerate(cands):
            assert list(got[c, :K]) == want[c] and (got[c, K:] == -1).all()
            assert st[c, 8 + K:8 + K + K * X.shape[1]].tobytes() == X[want[c]].tobytes()      # the centres are those rows
            hdr = st[c, :8].view(np.int64)
            assert list(hdr[:5]) == [0, 0, 0, K, X.shape[1]] and st[c, 5] == -np.inf
    assert list(seed_picks(same, [(3, 0)])[0][0, 1:]) == [9, 9]


BATCH_OF_ONE = [(1, 1, 1, 0), (129, 3, 2, 1), (1349, 20, 4, 42), (2049, 32, 8, 0)]


@pytest.mark.parametrize("n,K,Dm,seed", BATCH_OF_ONE)
def test_batch_of_one_is_the_single_device_fit(S, D, n, K, Dm, seed):
    X = SC.fixture()["X_tr"] if n == 1349 else SC.clustered(n, K, Dm, seed=n + K + Dm)
    assert X.shape == (n, Dm)
    assert_margin(X, K, seed)
    ref = D.DeviceGMM(K, random_state=seed, backend="device").fit(X)
    sw = one(S, X, K, seed)
    m = sw.model(0)
    print("n=%d K=%d D=%d: n_iter single %d batch %d, lower bound %.15g / %.15g" % (n, K, Dm, ref.n_iter_, sw.n_iter[0], ref.lower_bound_,
                                                                                   sw.lower_bound[0]))
    assert sw.status[0] == 0 and sw.n_iter[0] == m.n_iter_ == ref.n_iter_ and bool(sw.converged[0]) == ref.converged_
    assert state_bytes(sw, 0) == ref._state.cpu().numpy().tobytes()
    for name in ("weights_", "means_", "covariances_", "precisions_cholesky_"):
        assert getattr(m, name).tobytes() == getattr(ref, name).tobytes(), name
    assert m.lower_bound_ == ref.lower_bound_ == sw.lower_bound[0]


MIXED = [(1, 3), (5, 1), (20, 42), (32, 0), (8, 2)]


def test_a_candidate_does_not_depend_on_its_batch(S):
    from pinn_amd import _lib
    X = SC.fixture()["X_tr"]
    for K, s in MIXED:
        assert_margin(X, K, s)
    alone = {c: one(S, X, *c) for c in MIXED}
    want = {c: state_bytes(sw, 0) for c, sw in alone.items()}
    iters = {c: int(sw.n_iter[0]) for c, sw in alone.items()}
    print("n_iter alone:", iters)
    assert len(set(iters.values())) >= 3 and max(iters.values()) >= 2 * min(iters.values())     # some stop while others run
    per = _lib.load().pinn_gmm_batch_workspace_bytes(X.shape[0], 1, 32, 4)
    padded = (MIXED * 8)[:37]
    runs = {"B=5": (MIXED, {}), "B=5 permuted": ([MIXED[i] for i in (3, 0, 4, 2, 1)], {}), "B=5 in two calls": (MIXED, dict(ws_budget=3 * per)),
            "B=37": (padded, {}), "B=37 permuted": (padded[::-1], {}), "B=37 in two calls": (padded, dict(ws_budget=20 * per))}
    for name, (cands, kw) in runs.items():
        sw = S.gmm_sweep(X, candidates=cands, backend="device", **kw)
        differ = [i for i, c in enumerate(cands) if state_bytes(sw, i) != want[c]]
        print("%-18s candidates whose bytes differ from their batch of one: %s" % (name, differ))
        assert not differ
        assert [int(v) for v in sw.n_iter] == [iters[c] for c in cands]
        assert sw.loglik.tobytes() == np.array([alone[c].loglik[0] for c in cands]).tobytes()


def test_more_than_1024_tiles(S, D):
    """131 073 rows are 1025 tiles: the first workgroup takes two of them.  The full-fit gate is test_gpu_diagnosis.py's: 10 x
    the referee's sensitivity over 5 draws, not below 1e-13.  On rows whose clusters overlap (selection_cases.clustered, 7
    centres, seed 7) that sensitivity is 5e-15 to 1e-14, the gate is its floor, and the device's covariances came to 1.4e-13
    of the largest entry (means 9.9e-14, weights 1.8e-14, lower bound 2.3e-14): five EM iterations that have not converged
    carry the rounding of the 131 073-term sums forward, which independent input noise of 1e-13 does not show because it
    averages out over the rows.  The rows used here (selection_cases.nested) are separated well enough for an iteration not
    to amplify; the moment sums are gated by the arithmetic alone either way."""
    n, Dm, seed, kw = 131073, 4, 1, dict(max_iter=5, kmeans_iter=5)
    X = SC.nested(n, seed=7)
    Ks = (4, 7)
    for K in Ks:
        assert_margin(X, K, seed)
    ref = S.gmm_sweep(X, Ks, (seed,), backend="host", **kw)
    margins = [float(np.min(np.abs(np.abs(np.array(ref.model(i).lower_bound_changes_)) - 1e-3))) for i in range(len(Ks))]
    print("host: n_iter %s, convergence margins %s" % (ref.n_iter, margins))
    assert min(margins) >= 1e-8

    def dist(g, h):
        return np.array([np.abs(g.weights_ - h.weights_).max(), np.abs(g.means_ - h.means_).max() / np.abs(h.means_).max(),
                         (np.abs(g.covariances_ - h.covariances_) / np.abs(h.covariances_).max(axis=(1, 2), keepdims=True)).max(),
                         abs(g.lower_bound_ - h.lower_bound_)])
    sens = [np.zeros(4) for _ in Ks]
    prng = np.random.default_rng(999)
    for _ in range(5):
        p = S.gmm_sweep(X * (1.0 + 1e-13 * prng.uniform(-1.0, 1.0, X.shape)), Ks, (seed,), backend="host", **kw)
        assert np.array_equal(p.n_iter, ref.n_iter)
        sens = [np.maximum(s, dist(p.model(i), ref.model(i))) for i, s in enumerate(sens)]
    Xd = dev(X)
    got = S.gmm_sweep(X, Ks, (seed,), backend="device", **kw)
    print("n_iter host %s device %s" % (ref.n_iter, got.n_iter))
    assert np.array_equal(got.n_iter, ref.n_iter) and (got.status == 0).all()
    for i, K in enumerate(Ks):
        err, gate = dist(got.model(i), ref.model(i)), np.maximum(10.0 * sens[i], 1e-13)
        for name, e, g_ in zip(("weights", "means", "covariances", "lower_bound"), err, gate):
            print("K=%d %-12s err %.3e  gate %.3e" % (K, name, e, g_))
        assert np.all(err <= gate)
        assert state_bytes(got, i) == state_bytes(S.gmm_sweep(Xd, (K,), (seed,), **kw), 0)
    # one EM iteration of the batch from the referee's parameters: every moment sum of every candidate
    from pinn_amd import _device, _lib
    lib = _lib.load()
    rows = _device._DevRows(torch, Xd)
    Kmax = max(Ks)
    stride = lib.pinn_gmm_batch_state_stride(Kmax, Dm) // 8
    block = lib.pinn_gmm_batch_workspace_bytes(n, 1, Kmax, Dm)
    ws = torch.zeros(2 * block, dtype=torch.uint8, device="cuda")
    st = torch.zeros(2, stride, dtype=torch.float64, device="cuda")
    hosts = [ref.model(i) for i in range(2)]
    for i, h in enumerate(hosts):
        packed = D._pack_state(Ks[i], Dm, h.weights_, h.means_, h.covariances_, h.precisions_cholesky_)
        st[i, :packed.size] = dev(packed)
    _device.call("pinn_gmm_batch_em", *rows.head(), 2, (ctypes.c_int * 2)(*Ks), Kmax, 1, 0.0, 1e-6, st, ws, 2 * block)
    for i, h in enumerate(hosts):
        h.converged_ = False
        mom_h, abs_h = h.em_iterations(X, 1, return_moments=True)
        mom_d = ws[i * block:i * block + mom_h.size * 8].view(torch.float64).cpu().numpy().reshape(mom_h.shape)
        ratio = (np.abs(mom_d - mom_h) / np.maximum(abs_h, 1e-300)).max()
        print("K=%d moments: %.3e of sum|terms| (gate 1e-12)" % (Ks[i], ratio))
        assert np.all(np.abs(mom_d - mom_h) <= 1e-12 * abs_h)


def test_a_singular_candidate_stays_alone(S):
    X = SC.duplicated_rows()
    cands = [(1, 1), (2, 1), (1, 2), (3, 4)]
    for K, s in cands:
        assert_margin(X, K, s)
    sw = S.gmm_sweep(X, candidates=cands, reg_covar=0.0, backend="device")             # does not raise
    print("status", sw.status, "n_iter", sw.n_iter, "bic", sw.bic)
    assert list(sw.status) == [0, 1, 0, 1]
    without = S.gmm_sweep(X, candidates=[cands[0], cands[2]], reg_covar=0.0, backend="device")
    assert state_bytes(sw, 0) == state_bytes(without, 0) and state_bytes(sw, 2) == state_bytes(without, 1)
    assert np.isfinite(sw._states.cpu().numpy()[:, 8:]).all()                         # the last good parameters stay
    for i in (1, 3):
        with pytest.raises(ValueError, match="positive definite"):
            sw.model(i)
    g, sw2 = S.select_gmm(X, candidates=cands[1:], reg_covar=0.0, backend="device")
    assert g.n_components == 1 and g.random_state == 2 and sw2.best("bic") == 1
    ok = S.gmm_sweep(X, candidates=cands, backend="device")                           # the same rows with the default regularisation
    assert (ok.status == 0).all() and np.isfinite(ok.bic).all()


def test_scores(S, D):
    G = SC.fixture()
    Xtr, Xte = G["X_tr"], G["X_te"]
    kw = dict(n_components=(4, 20), seeds=(1,), backend="device")
    sw = S.gmm_sweep(Xtr, X_val=Xte, **kw)
    for i in range(len(sw)):
        m = sw.model(i)
        for what, X, got in (("loglik", Xtr, sw.loglik[i]), ("val_score", Xte, sw.val_score[i] * Xte.shape[0])):
            lpn, _ = D._host_estep(X, m.weights_, m.means_, m.precisions_cholesky_)
            print("K=%d %-9s device %.12f host %.12f, difference %.3e, gate %.3e" % (sw.n_components[i], what, got, lpn.sum(),
                                                                                 abs(got - lpn.sum()), 1e-12 * np.abs(lpn).sum()))
            assert abs(got - lpn.sum()) <= 1e-12 * np.abs(lpn).sum()
    assert np.array_equal(sw.bic, -2.0 * sw.loglik + sw.n_parameters * np.log(1349))
    # rows read in place: 22 columns, the features scattered among them, training and held-out rows by gather lists
    rng = np.random.default_rng(3)
    wide = rng.normal(size=(2700, 22))
    cols, tr, te = [13, 2, 21, 7], rng.permutation(2700)[:1349], rng.permutation(2700)[:450]
    wide[np.ix_(tr, cols)] = Xtr
    Xv = wide[np.ix_(te, cols)]
    packed = S.gmm_sweep(Xtr, X_val=Xv, **kw)
    assert packed._states.cpu().numpy().tobytes() == sw._states.cpu().numpy().tobytes()
    for X in (wide, dev(wide)):
        inplace = S.gmm_sweep(X, columns=cols, row_index=tr, val_index=te, **kw)
        for name in ("loglik", "val_score", "lower_bound", "n_iter", "bic"):
            assert getattr(inplace, name).tobytes() == getattr(packed, name).tobytes(), name
        assert inplace._states.cpu().numpy().tobytes() == packed._states.cpu().numpy().tobytes()
    again = S.gmm_sweep(Xtr, X_val=Xv, **kw)                                           # two identical calls
    assert again._states.cpu().numpy().tobytes() == packed._states.cpu().numpy().tobytes()
    assert again.loglik.tobytes() == packed.loglik.tobytes() and again.val_score.tobytes() == packed.val_score.tobytes()
    assert isinstance(S.gmm_sweep(dev(Xtr), **kw).model(0).means_, torch.Tensor)


@pytest.fixture(scope="module")
def device_sweep(S):
    G = SC.fixture()
    for K in SC.GRID_K:
        for s in SC.SEEDS:
            assert_margin(G["X_tr"], K, s)
    return S.gmm_sweep(G["X_tr"], SC.GRID_K, SC.SEEDS, X_val=G["X_te"], backend="device")


def test_fixture_sweep_selects_as_the_host(S, device_sweep):
    G, ref = SC.fixture(), SC.host_sweep()
    print(device_sweep.table())
    SC.check_conditions(ref, SC.host_margins())
    SC.check_conditions(device_sweep, SC.host_margins())
    assert np.array_equal(device_sweep.n_iter, ref.n_iter)
    SC.check_selections(device_sweep, G)
    g, _ = S.select_gmm(G["X_tr"], (20,), SC.SEEDS, criterion="lower_bound", backend="device")
    assert g.random_state == 1 and g.n_components == 20


@pytest.mark.parametrize("K", SC.GRID_K)
def test_fixture_sweep_against_the_host(D, device_sweep, K):
    G, ref = SC.fixture(), SC.host_sweep()
    X = G["X_tr"]

    def dist(g, h):
        return np.array([np.abs(g.weights_ - h.weights_).max(), np.abs(g.means_ - h.means_).max() / np.abs(h.means_).max(),
                         (np.abs(g.covariances_ - h.covariances_) / np.abs(h.covariances_).max(axis=(1, 2), keepdims=True)).max(),
                         abs(g.lower_bound_ - h.lower_bound_)])
    prng = np.random.default_rng(999 + K)
    for i in np.flatnonzero(ref.n_components == K):
        h, sens = ref.model(i), np.zeros(4)
        for _ in range(5):
            p = D.DeviceGMM(K, random_state=int(ref.seed[i]), backend="host").fit(X * (1.0 + 1e-13 * prng.uniform(-1.0, 1.0, X.shape)))
            assert p.n_iter_ == h.n_iter_
            sens = np.maximum(sens, dist(p, h))
        err, gate = dist(device_sweep.model(i), h), np.maximum(10.0 * sens, 1e-13)
        print("K=%d seed %d: n_iter host %d device %d; err %s; gate %s" % (K, ref.seed[i], h.n_iter_, device_sweep.n_iter[i], err, gate))
        assert device_sweep.n_iter[i] == h.n_iter_ and device_sweep.converged[i]
        assert np.all(err <= gate)
