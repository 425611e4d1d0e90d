"""GPU: the device backend of pinn_amd.embedding (csrc/pinn_tsne.hip) against tests/golden/g_tsne.npz and against the
package's host backend (float64 numpy, the same state machine and the same order of every sum).

Gates: those of tests/test_embedding_host.py through its checkers, with the device as the backend; and the device
against the host: P of both within 1e-9 max P of each other (both are roots to 1e-12), raw sums within 1e-12 x the sum of the
absolute terms at n in {5, 64, 65, 257, 600} (the last wave and the last tile one row and one column long at 65 and 257), and
the schedule's cases with equal header integers.  The embedding depends on +, -, x, / and comparisons only, which both
backends round alike and add in the same order, so it is compared bit for bit as well.  Repeated fits, in-place and
gathered reads and tensor inputs are compared bit for bit.  Every comparison prints its maxima before it asserts."""
import numpy as np
import pytest
import torch

from test_embedding_host import (SHAPES, case_boundary, case_max_iter_250, case_no_progress, case_stationary, check_affinities_fixture,
                                 check_affinities_shape, check_duplicates, check_end_to_end, check_helpers, check_one_iteration, check_raw_sums,
                                 check_stored_states, full, host, ints, kl_tolerance, run, same_state, small_problem, stationary_start)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(golden):
    return golden("g_tsne.npz")


@pytest.fixture(scope="module")
def E():
    from pinn_amd import embedding
    return embedding


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("sfx", ["", "1", "8"])
def test_device_affinities_against_root_and_reference(G, E, sfx):
    P = check_affinities_fixture(G, E, "device", sfx)
    Pt = check_affinities_fixture(G, E, "device", sfx, dev)
    assert P.tobytes() == Pt.tobytes()                                          # numpy in and tensor in: the same bytes
    out = E.joint_probabilities(dev(G["X" + sfx]), float(G["perplexity"]), backend="device")
    assert all(isinstance(a, torch.Tensor) and a.is_cuda for a in out)


@pytest.mark.parametrize("n,D,perplexity", SHAPES)
def test_device_affinities_and_raw_sums_against_host(E, n, D, perplexity):
    X, P = check_affinities_shape(E, "device", n, D, perplexity)
    Ph, _, _ = E.joint_probabilities(X, perplexity, backend="host")
    d = np.abs(P - Ph).max() / Ph.max()
    print("n = %d: max |P_device - P_host| / max P = %.3e (bound 1e-9)" % (n, d))
    assert d <= 1e-9
    rng = np.random.default_rng(n)
    for scale, alpha in ((1e-4, 12.0), (3.0, 1.0)):                             # a start and a spread-out embedding
        check_raw_sums(E, "device", Ph, scale * rng.standard_normal((n, 2)), alpha, "n = %d, scale %g" % (n, scale))


def test_device_kl_and_gradient_at_stored_states(G, E):
    check_stored_states(G, E, "device")
    r = E.kl_and_gradient(dev(full(G["P_sk"])), dev(G["s260_Y"]), 1.0, backend="device")
    assert r["grad"].is_cuda and r["row_sums"].is_cuda
    again = E.kl_and_gradient(full(G["P_sk"]), G["s260_Y"], 1.0, backend="device")
    assert host(r["grad"]).tobytes() == again["grad"].tobytes() and host(r["row_sums"]).tobytes() == again["row_sums"].tobytes()
    assert r["kl"] == again["kl"]


def test_device_one_iteration_from_stored_states(G, E):
    check_one_iteration(G, E, "device")


def compare(E, tag, dev_out, dev_h, host_out, host_h):
    """Header integers equal, and the state bit for bit (the trajectory takes no exp or log)."""
    dy = np.abs(dev_out["Y"] - host_out["Y"]).max()
    print("%s: device %s\n  host   %s\n  max |Y_device - Y_host| = %.3e, error %.12f / %.12f" % (tag, ints(E, dev_h), ints(E, host_h), dy,
                                                                                        dev_h["error"], host_h["error"]))
    assert ints(E, dev_h) == ints(E, host_h)
    assert same_state(dev_out, host_out)


def test_device_state_machine_against_host(G, E):
    P, Y0 = small_problem(G, E)
    out, h = case_max_iter_250(E, "device", P, Y0)
    compare(E, "max_iter 250", out, h, *case_max_iter_250(E, "host", P, Y0))
    assert h["done"] and h["n_iter"] == 249 and h["phase"] == 0
    more, h2 = run(E, "device", P, out, 100, max_iter=250, learning_rate=50.0)
    assert same_state(out, more) and h2 == h                                    # after done queued chunks change nothing

    d = case_boundary(E, "device", P, Y0)
    hst = case_boundary(E, "host", P, Y0)
    compare(E, "max_iter 300 at 250", d[0], d[1], hst[0], hst[1])
    compare(E, "max_iter 300 at the end", d[2], d[3], hst[2], hst[3])
    assert d[1]["iteration"] == 250 and d[1]["phase"] == 1 and np.all(d[0]["update"] == 0.0) and np.all(d[0]["gains"] == 1.0)
    assert d[3]["done"] and d[3]["n_iter"] == 299

    Ps, Ys = stationary_start(E)
    out, h = case_stationary(E, "device", Ps, Ys)
    compare(E, "stationary start", out, h, *case_stationary(E, "host", Ps, Ys))
    assert h["done"] and h["n_iter"] == 299 and E.STOP_NAMES[h["stop"]] == "min_grad_norm"

    h0, out, h = case_no_progress(E, "device", P, Y0)
    g0, gout, gh = case_no_progress(E, "host", P, Y0)
    compare(E, "no progress", out, h, gout, gh)
    assert ints(E, h0) == ints(E, g0) and h["done"] and E.STOP_NAMES[h["stop"]] == "no_progress" and h["n_iter"] == gh["n_iter"]


def test_device_plumbing(G, E):
    X = G["X"][:65]
    kw = dict(perplexity=20, n_iter=250, random_state=5, backend="device")
    for init in ("pca", "random"):
        a = E.DeviceTSNE(init=init, **kw).fit(X)
        b = E.DeviceTSNE(init=init, **kw).fit(X)
        assert a.max_iter == 250 and a.n_iter_ == 249 and a.learning_rate_ == 50.0 and a.n_features_in_ == 4
        assert isinstance(a.embedding_, np.ndarray) and a.embedding_.tobytes() == b.embedding_.tobytes()      # two fits: the same bytes
        assert a.kl_divergence_ == b.kl_divergence_
        wide = np.full((90, 22), np.nan)
        perm = np.random.default_rng(0).permutation(90)[:65]
        wide[perm[:, None], np.array([13, 14, 15, 16])[None, :]] = X
        c = E.DeviceTSNE(init=init, **kw).fit(wide, columns=[13, 14, 15, 16], row_index=perm)
        t = E.DeviceTSNE(init=init, **kw).fit(dev(wide), columns=[13, 14, 15, 16], row_index=dev(perm))
        p = E.DeviceTSNE(init=init, **kw).fit(dev(X))
        assert isinstance(t.embedding_, torch.Tensor) and t.embedding_.is_cuda and isinstance(c.embedding_, np.ndarray)
        for o in (c, t, p):
            assert host(o.embedding_).tobytes() == a.embedding_.tobytes() and o.kl_divergence_ == a.kl_divergence_
        P, _, _ = E.joint_probabilities(X, 20, backend="device")
        ref = E.kl_and_gradient(P, a.embedding_, backend="host")
        got = E.kl_and_gradient(P, a.embedding_, backend="device")
        print("init %s: kl_divergence_ %.12f, kl_and_gradient %.12f (device) %.12f (host)" % (init, a.kl_divergence_, got["kl"], ref["kl"]))
        assert abs(a.kl_divergence_ - got["kl"]) <= kl_tolerance(ref, 1.0) and abs(a.kl_divergence_ - ref["kl"]) <= kl_tolerance(ref, 1.0)
    hst = E.DeviceTSNE(init="random", **{**kw, "backend": "host"}).fit(X)
    dy = np.abs(hst.embedding_ - a.embedding_).max()
    print("host fit against device fit (random start): max |Y diff| = %.3e, n_iter_ %d / %d" % (dy, hst.n_iter_, a.n_iter_))
    assert hst.n_iter_ == a.n_iter_
    bad = X.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        E.DeviceTSNE(**kw).fit(bad)
    with pytest.raises(ValueError):
        E.DeviceTSNE(**kw).fit(X, row_index=np.array([0, 1, 2, 900] + list(range(4, 65))))       # a gather index outside the array
    with pytest.raises(ValueError):
        E.DeviceTSNE(perplexity=65, backend="device").fit(X)
    with pytest.raises(NotImplementedError, match="approximates"):
        E.DeviceTSNE(method="barnes_hut", backend="device")
    with pytest.raises(NotImplementedError):
        E.DeviceTSNE(n_components=3, backend="device")
    with pytest.raises(NotImplementedError):
        E.DeviceTSNE(**kw).fit(np.random.default_rng(0).random((65, 9)))


def test_device_argument_errors(E):
    """NULL, misaligned and out-of-limit arguments are PINN_E_ARG, a short workspace PINN_E_WORKSPACE, before any launch."""
    import ctypes
    from pinn_amd import _lib
    lib = _lib.load()
    n = 64
    assert lib.pinn_tsne_state_bytes(n) == (16 + 6 * n) * 8 and lib.pinn_tsne_state_bytes(1) == 0
    assert lib.pinn_tsne_workspace_bytes(_lib.TSNE_MAX_ROWS + 1) == 0 and lib.pinn_tsne_workspace_bytes(_lib.TSNE_MAX_ROWS) > 8 * 32768 ** 2
    wb = lib.pinn_tsne_workspace_bytes(n)
    ws, st = torch.zeros(wb, dtype=torch.uint8, device="cuda"), torch.zeros(16 + 6 * n, dtype=torch.float64, device="cuda")
    X, v, s = torch.rand(n, 4, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    cols = (ctypes.c_int * 4)(0, 1, 2, 3)
    p = lambda t: t.data_ptr()
    aff = lambda **k: lib.pinn_tsne_affinities(*[k.get(a, d) for a, d in (("arr", p(X)), ("ld", 4), ("n_arr", n), ("cols", cols), ("D", 4), ("ridx", None),
                                               ("n", n), ("perp", 20.0), ("beta", p(v)), ("ent", p(v)), ("status", p(s)), ("ws", p(ws)), ("wb", wb),
                                               ("stream", None))])
    for bad in (dict(arr=None), dict(beta=None), dict(status=None), dict(ws=None), dict(ws=p(ws) + 4), dict(perp=64.0), dict(perp=0.0), dict(n=1),
                dict(n=_lib.TSNE_MAX_ROWS + 1), dict(D=9), dict(D=0)):
        assert aff(**bad) == -1, bad
    assert aff(wb=wb - 1) == -3
    assert lib.pinn_tsne_kl_grad(n, None, 1.0, p(ws), wb, None) == -1 and lib.pinn_tsne_kl_grad(n, p(st) + 4, 1.0, p(ws), wb, None) == -1
    assert lib.pinn_tsne_kl_grad(n, p(st), 0.0, p(ws), wb, None) == -1 and lib.pinn_tsne_kl_grad(n, p(st), 1.0, p(ws), wb - 1, None) == -3
    good = (n, 1, 1, 250, 12.0, 50.0, 300, 1e-7, p(st), p(ws), wb, None)
    for i, val in ((0, 1), (2, -1), (3, 249), (4, 0.0), (5, 0.0), (6, -1), (7, -1.0), (8, None), (8, p(st) + 4), (9, None)):
        a = list(good)
        a[i] = val
        assert lib.pinn_tsne_descend(*a) == -1, (i, val)
    assert lib.pinn_tsne_descend(*good[:10], wb - 1, None) == -3


def test_device_duplicated_rows(G, E):
    P = check_duplicates(G, E, "device")
    Ph = check_duplicates(G, E, "host")
    d = np.abs(P - Ph).max() / Ph.max()
    print("duplicated rows: max |P_device - P_host| / max P = %.3e (bound 1e-9)" % d)
    assert d <= 1e-9
    assert check_duplicates(G, E, "device", dev).tobytes() == P.tobytes()


def test_auto_backend_runs_the_device(G, E, monkeypatch):
    """A numpy array of at least AUTO_DEVICE_ROWS rows and the default backend: the device runs (the host backend is made to
    fail), numpy comes back, and the bytes are those of backend="device"."""
    X = G["X"]
    assert X.shape[0] >= E.AUTO_DEVICE_ROWS

    def no_host(*a, **k):
        raise AssertionError("the host backend ran")
    monkeypatch.setattr(E, "_host_affinities", no_host)
    monkeypatch.setattr(E, "_host_iterate", no_host)
    kw = dict(perplexity=20, n_iter=250, init="pca")
    m = E.DeviceTSNE(**kw).fit(X)
    ref = E.DeviceTSNE(backend="device", **kw).fit(X)
    assert m.backend_ == "device" and isinstance(m.embedding_, np.ndarray) and m.embedding_.tobytes() == ref.embedding_.tobytes()
    wide = np.zeros((300, 22))
    wide[:257, 13:17] = X
    assert E.DeviceTSNE(**kw).fit(wide, columns=[13, 14, 15, 16], row_index=np.arange(257)).embedding_.tobytes() == ref.embedding_.tobytes()
    emb = E.tsne_of_test_samples(X, n_iter=250)
    assert isinstance(emb, np.ndarray) and emb.tobytes() == E.DeviceTSNE(backend="device", **{**E.TSNE_TEST_PARAMS, "n_iter": 250}).fit_transform(X).tobytes()
    P, _, _ = E.joint_probabilities(X, 20.0)
    assert isinstance(P, np.ndarray)
    small = E.DeviceTSNE(perplexity=20, n_iter=250, init="random", random_state=0)
    monkeypatch.undo()
    assert small.fit(X[:65]).backend_ == "host"                                 # below the threshold the host backend serves


def test_device_end_to_end_band(G, E):
    m = check_end_to_end(G, E, "device")
    assert isinstance(m.embedding_, np.ndarray) and m.embedding_.shape == (257, 2)


def test_device_script_helpers(G, E):
    check_helpers(G, E, "device")
    check_helpers(G, E, "device", dev)
