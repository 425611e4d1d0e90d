"""GPU: the device backend of pinn_amd.ksvm (csrc/pinn_ksvm.hip) against tests/golden/g_ksvm.npz and against the package's host
backend (float64 numpy, the same state machine).

Gates (from the problem's convexity and the number format, not from what the kernels give): gates 1-4 of
tests/test_ksvm_host.py through backend="device"; the working sets of the first 32 iterations equal the host's up to the
first iteration at which the host's selection margin (best to second-best value) falls below 1e-9 max(1, |value|), and alpha
and G after them agree to 1e-12 x the sum of their absolute terms; device and host decision values of converged fits within
sqrt(2 g_dev) + sqrt(2 g_host) plus the two violations; the decision kernel on the host's model within 1e-12 x the sum of the
absolute terms per value.  Repeated fits, in-place and gathered reads, chunk sizes, calls after convergence and chunked
diagnosis are compared bit for bit.  Every comparison prints its maxima before it asserts."""
import copy

import numpy as np
import pytest
import torch

from test_ksvm_host import (NAMED, blobs, check_all_at_bound, check_arguments, check_decision, check_duplicates, check_fixture, check_model,
                            check_named, fixture_fit, host, one_row_class_case, own_decision)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(golden):
    g = golden("g_cluster.npz")
    g.update({"k_" + k: v for k, v in golden("g_ksvm.npz").items()})
    return g


@pytest.fixture(scope="module")
def K():
    from pinn_amd import ksvm
    return ksvm


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 8. working sets
SETS = [(m, D, C) for m in (127, 128, 129, 257, 2049) for D in (1, 4, 8) for C in (2, 4)]


@pytest.mark.parametrize("m,D,C", SETS)
def test_working_sets_against_the_host(K, m, D, C):
    n_it = 32
    X, y = blobs(m, C, D, 100 * m + 10 * D + C)
    sc = K.DeviceStandardScaler("host").fit(X)
    h = K.DeviceKernelSVC(C=1.0, class_weight="balanced", backend="host").working_sets(X, y, n_it, scaler=sc)
    d = K.DeviceKernelSVC(C=1.0, class_weight="balanced", backend="device").working_sets(X, y, n_it, scaler=sc)
    assert abs(d["gamma"] - h["gamma"]) <= 1e-14 * h["gamma"]
    P = C * (C - 1) // 2
    pairs = [(a, b) for a in range(C) for b in range(a + 1, C)]
    stops = []
    for p, (a, b) in enumerate(pairs):
        tr = h["trace"][p]
        stop = len(tr)
        for k, (_, _, _, (mi, vi), (mj, vj)) in enumerate(tr):
            if k > 0 and (mi < 1e-9 * max(1.0, abs(vi)) or mj < 1e-9 * max(1.0, abs(vj))):      # iteration 0 is an exact tie on both sides
                stop = k
                break
        assert stop >= 1 and np.array_equal(d["log"][p, :stop], h["log"][p, :stop]), (p, stop, d["log"][p, :stop + 1], h["log"][p, :stop + 1])
        assert tuple(d["log"][p, 0]) == (np.nonzero(y == a)[0][0], h["log"][p, 0, 1])
        stops.append(stop if stop < len(tr) else n_it)

    def state_errors(dd, hh, which):
        e_a, e_g = 0.0, 0.0
        for p in which:
            a, b = pairs[p]
            rows = np.nonzero((y == a) | (y == b))[0]
            sl = np.where(y[rows] == a, b - 1, a)
            e_a = max(e_a, float(np.max(np.abs(dd["alpha"][rows, sl] - hh["alpha"][rows, sl]) / np.maximum(hh["alpha_abs"][rows, sl], 1e-300))))
            e_g = max(e_g, float(np.max(np.abs(dd["G"][rows, sl] - hh["G"][rows, sl]) / hh["G_abs"][rows, sl])))
        return e_a, e_g

    # alpha and G where the working sets are the same: after the whole chunk for the pairs that went through it, and for every
    # pair after the shortest stretch that all pairs share
    whole = [p for p in range(P) if stops[p] == n_it]
    e_a, e_g = state_errors(d, h, whole)
    n_cmp = min(stops)
    if n_cmp < n_it:
        h2 = K.DeviceKernelSVC(C=1.0, class_weight="balanced", backend="host").working_sets(X, y, n_cmp, scaler=sc)
        d2 = K.DeviceKernelSVC(C=1.0, class_weight="balanced", backend="device").working_sets(X, y, n_cmp, scaler=sc)
        assert np.array_equal(d2["log"], h2["log"]) and np.array_equal(d2["log"], d["log"][:, :n_cmp])
        e2 = state_errors(d2, h2, range(P))
        e_a, e_g = max(e_a, e2[0]), max(e_g, e2[1])
    print("working sets %d rows per class x %d, %d classes: %d of %d pairs compared after %d iterations, all after %d; alpha off by %.3e, "
          "G by %.3e of their absolute terms (gate 1e-12)" % (m, D, C, len(whole), P, n_it, n_cmp, e_a, e_g))
    assert e_a <= 1e-12 and e_g <= 1e-12


# ---- 9. end points
@pytest.mark.parametrize("ci", [0, 1])
def test_device_matches_reference_fixture(G, K, ci):
    pipe = check_fixture(K, G, "device", ci)
    m = pipe.named_steps["svc"]
    for a in (m.support_, m.support_vectors_, m.dual_coef_, m.intercept_, m.alpha_, m.class_weight_, pipe.predict(G["X_te"])):
        assert isinstance(a, np.ndarray)
    tp = check_fixture(K, G, "device", ci, dev)
    tm = tp.named_steps["svc"]
    for a in (tm.support_, tm.support_vectors_, tm.dual_coef_, tm.intercept_, tm.alpha_, tm.class_weight_, tp.predict(dev(G["X_te"])),
              tp.decision_function(dev(G["X_te"]))):
        assert isinstance(a, torch.Tensor) and a.is_cuda
    for name in ("support_", "dual_coef_", "intercept_", "alpha_"):
        assert host(getattr(tm, name)).tobytes() == getattr(m, name).tobytes(), name        # numpy in and tensor in: the same bytes
    assert host(tp.decision_function(dev(G["X_te"]), shape="ovo")).tobytes() == pipe.decision_function(G["X_te"], shape="ovo").tobytes()
    # device against host: sqrt(2 g_dev) + sqrt(2 g_host) on the values without intercept, plus the two violations
    hp = fixture_fit(K, G, "host", ci)
    hm = hp.named_steps["svc"]
    bound = np.sqrt(2.0 * np.maximum(m.dual_gap_, 0.0)) + np.sqrt(2.0 * np.maximum(hm.dual_gap_, 0.0)) + m.violation_ + hm.violation_
    diff = np.abs(pipe.decision_function(G["X_te"], shape="ovo") - hp.decision_function(G["X_te"], shape="ovo")).max(axis=0)
    print("fixture, C = %g: device and host decision values differ by %s (bounds %s); iterations %s and %s"
          % (G["k_C"][ci], diff, bound, list(m.n_iter_), list(hm.n_iter_)))
    assert (diff <= bound).all()


@pytest.mark.parametrize("name", list(NAMED))
def test_named_cases_on_the_device(K, name):
    check_named(K, name, "device")
    check_named(K, name, "device", dev)


def test_special_cases_on_the_device(K):
    X, y = one_row_class_case()
    pipe, _, _ = check_model(K, X, y, "device", "a class of one row, device", C=1.0)
    assert pipe.named_steps["svc"].n_support_[1] == 1
    check_duplicates(K, "device")
    m = check_all_at_bound(K, "device")
    h = check_all_at_bound(K, "host")
    assert abs(m.intercept_[0] - h.intercept_[0]) <= 1e-14
    Xb, yb = blobs(40, 3, 2, 13)
    with pytest.warns(UserWarning, match="did not reach tol"):
        w = K.DeviceKernelSVC(max_iter=3, backend="device").fit(Xb, yb)
    assert not w.converged_.any() and (w.n_iter_ == 3).all() and (w.violation_ > w.tol).all()


# ---- 10. the decision kernel alone
@pytest.mark.parametrize("n_sv", [1, 128, 129])
def test_decision_kernel_on_the_host_model(G, K, n_sv):
    from pinn_amd import _lib
    assert _lib.KSVM_SV_TILE == 128
    hp = fixture_fit(K, G, "host", 0)
    hm, sc = hp.named_steps["svc"], hp.named_steps["scaler"]
    assert len(hm.support_) > 129
    yi = np.searchsorted(np.unique(G["y_tr"]), G["y_tr"])
    cut = copy.copy(hm)                                   # the model cut to its first n_sv support rows, for both backends
    cut._sv, cut._coef, cut._sv_cls = hm._sv[:n_sv].copy(), hm._coef[:n_sv].copy(), hm._sv_cls[:n_sv].copy()
    cut.support_, cut.support_vectors_, cut.dual_coef_ = hm.support_[:n_sv], hm.support_vectors_[:n_sv], hm.dual_coef_[:, :n_sv]
    on_dev = copy.copy(cut)
    on_dev.backend, on_dev._model = "device", None
    rng = np.random.default_rng(n_sv)
    for n in (1, 127, 129, 2049):
        X = G["X_te"][rng.integers(0, len(G["X_te"]), n)] + rng.normal(0.0, 0.05, (n, 4)) * sc.scale_
        Z = (X - sc.mean_) / sc.scale_
        dec, keep = check_decision(cut, on_dev, X, Z, yi, "decision kernel, %d rows x %d support rows" % (n, n_sv), scaler=sc)
        dec_h = cut.decision_function(X, scaler=sc, shape="ovo")
        _, mag = own_decision(cut, Z, yi)
        assert (np.abs(on_dev.decision_function(X, scaler=sc, shape="ovo") - dec_h) <= 1e-12 * mag).all()
        r = on_dev._decide(dev(X), scaler=sc, want=("decision", "votes", "pred"))
        votes = host(r["votes"])
        assert votes.shape == (n, 4) and (votes.sum(axis=1) == 6).all()
        assert np.array_equal(host(r["pred"])[keep], votes.argmax(axis=1)[keep])
        assert np.array_equal(host(r["pred"])[keep], cut.predict(X, scaler=sc)[keep])


# ---- 11. the same bytes
def test_same_bytes(G, K):
    n_tr, n_te = len(G["y_tr"]), len(G["y_te"])
    rng = np.random.default_rng(5)
    res = rng.normal(size=(n_tr + n_te + 40, 22))
    where = rng.permutation(n_tr + n_te + 40)[:n_tr + n_te]
    res[where[:n_tr], 13:17], res[where[n_tr:], 13:17] = G["X_tr"], G["X_te"]
    res_d, cols = dev(res), [13, 14, 15, 16]
    build = lambda **kw: K.build_kernel_svm_classifier("device", C=1.0, **kw)
    packed = build().fit(dev(G["X_tr"]), dev(G["y_tr"]))
    placed = build().fit(res_d, dev(G["y_tr"]), columns=cols, row_index=dev(where[:n_tr]))
    again = build().fit(dev(G["X_tr"]), dev(G["y_tr"]))
    single = build(chunk=1).fit(dev(G["X_tr"]), dev(G["y_tr"]))
    a = packed.named_steps["svc"]
    for other in (placed, again, single):
        b = other.named_steps["svc"]
        for name in ("support_", "support_vectors_", "dual_coef_", "intercept_", "alpha_"):
            assert host(getattr(a, name)).tobytes() == host(getattr(b, name)).tobytes(), name
        assert np.array_equal(a.n_iter_, b.n_iter_) and a.dual_gap_.tobytes() == b.dual_gap_.tobytes() and a.gamma_ == b.gamma_
    one = packed.predict(dev(G["X_te"]))
    assert torch.equal(placed.predict(res_d, columns=cols, row_index=dev(where[n_tr:])), one)
    assert torch.equal(placed.decision_function(res_d, columns=cols, row_index=dev(where[n_tr:]), shape="ovo"),
                       packed.decision_function(dev(G["X_te"]), shape="ovo"))
    rows = dev(res[where[n_tr:]])
    d = K.KernelSVMDiagnoser(placed)
    got = torch.cat([d.update(rows[i:i + 128]) for i in range(0, n_te, 128)])
    assert d.n_seen == n_te and torch.equal(got, one) and torch.equal(K.KernelSVMDiagnoser(placed).update(rows), one)


def raw_fit(K, X, y, n_calls, n_iters, extra_calls=0, row_index=None, C=1.0):
    """The state block after n_calls calls of pinn_ksvm_smo with n_iters iterations each (the first with init = 1)."""
    from pinn_amd._device import call
    q = K.DeviceKernelSVC(C=C, backend="device").device_problem(dev(X), dev(y), row_index=row_index)
    st, states = q["state"], []
    for k in range(n_calls + extra_calls):
        call("pinn_ksvm_smo", *q["head"], 0.5, int(k == 0), n_iters, 1e-10, st, None, q["ws"], q["ws_bytes"])
        if k >= n_calls - 1:
            states.append(st.clone())
    torch.cuda.synchronize()
    return states, q["alpha_at"]


def test_calls_after_convergence_change_nothing(K):
    from pinn_amd import _lib
    X, y = blobs(70, 3, 2, 21)
    states, o = raw_fit(K, X, y, 1, 2000, extra_calls=2)
    pi = host(states[0])[_lib.KSVM_ST_HEADER:o - 2 * 2 - 3].view(np.int64).reshape(3, _lib.KSVM_PAIR_WORDS)
    assert (pi[:, _lib.KSVM_P_CONVERGED] == 1).all() and (pi[:, _lib.KSVM_P_STATUS] == 0).all() and (pi[:, _lib.KSVM_P_ITER] < 1999).all()
    for s in states[1:]:
        assert host(s).tobytes() == host(states[0]).tobytes()


# ---- 12. the C side
def test_limits_and_bad_rows_on_the_device(G, K):
    from pinn_amd import _lib
    lib = _lib.load()
    assert lib.pinn_ksvm_state_bytes(100, 9, 4) == 0 and lib.pinn_ksvm_state_bytes(100, 4, 9) == 0 and lib.pinn_ksvm_workspace_bytes(100, 1, 4) == 0
    assert lib.pinn_ksvm_state_bytes(100, 8, 8) > 0 and lib.pinn_ksvm_workspace_bytes(100, 8, 8) > 0 and lib.pinn_ksvm_state_bytes(-1, 4, 4) == 0
    one = torch.zeros(64, dtype=torch.float64, device="cuda")
    p, cols = one.data_ptr(), (_lib.c_int * 9)(*range(9))
    big = 1 << 30
    smo = lambda **kw: lib.pinn_ksvm_smo(*[kw.get(k, v) for k, v in (
        ("arr", p), ("ld", 4), ("n_arr", 1), ("cols", cols), ("D", 4), ("ridx", None), ("n", 1), ("y", p), ("C", 3), ("gamma", 0.5), ("init", 1),
        ("n_iters", 1), ("tol", 1e-10), ("st", p), ("log", None), ("ws", p), ("wb", big), ("stream", None))])
    assert smo(C=9) == -1 and smo(D=9, ld=9) == -1 and smo(st=None) == -1 and smo(ws=None) == -1 and smo(y=None) == -1 and smo(arr=None) == -1
    assert smo(st=p + 4) == -1 and smo(ws=p + 4) == -1 and smo(log=p + 4) == -1 and smo(gamma=0.0) == -1 and smo(tol=0.0) == -1 and smo(n_iters=-1) == -1
    need = lib.pinn_ksvm_workspace_bytes(1, 3, 4)
    assert smo(wb=need - 1) == -3 and smo(wb=8) == -3
    fin = lambda **kw: lib.pinn_ksvm_finish(*[kw.get(k, v) for k, v in (
        ("arr", p), ("ld", 4), ("n_arr", 1), ("cols", cols), ("D", 4), ("ridx", None), ("n", 1), ("y", p), ("C", 3), ("st", p), ("stream", None))])
    assert fin(C=9) == -1 and fin(D=9, ld=9) == -1 and fin(st=None) == -1 and fin(y=None) == -1 and fin(st=p + 4) == -1 and fin(n=0) == -1
    dec = lambda **kw: lib.pinn_ksvm_decision(*[kw.get(k, v) for k, v in (
        ("arr", p), ("ld", 4), ("n_arr", 1), ("cols", cols), ("D", 4), ("ridx", None), ("n", 1), ("C", 3), ("scaler", None), ("sv", p), ("coef", p),
        ("cls", p), ("n_sv", 1), ("rho", p), ("gamma", 0.5), ("dec", None), ("votes", None), ("pred", None), ("stream", None))])
    assert dec(C=9) == -1 and dec(D=9, ld=9) == -1 and dec(sv=None) == -1 and dec(rho=None) == -1 and dec(gamma=-1.0) == -1 and dec(dec=p + 4) == -1
    assert dec(n_sv=-1) == -1 and dec(scaler=p + 4) == -1
    check_arguments(K, "device", dev)
    m = K.DeviceKernelSVC(backend="device")
    with pytest.raises(NotImplementedError):
        m.fit(dev(G["X_tr"][:50]), dev(G["y_tr"][:50]), trace=[])
    # a gather index behind the array and an inf in a row: the status word on exactly the pairs of that row's class, and the
    # rest of the state as the launch that checks the rows left it
    X, y = G["X_tr"][:300].copy(), G["y_tr"][:300]
    pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)]

    def stopped_pairs(X, row_index, bad_row, word):
        states, o = raw_fit(K, X, y, 1, 0, row_index=row_index)
        after, _ = raw_fit(K, X, y, 1, 3, row_index=row_index)
        s0, s1 = host(states[0]).copy(), host(after[0]).copy()
        P, W = 6, _lib.KSVM_PAIR_WORDS
        pi = s1[_lib.KSVM_ST_HEADER:_lib.KSVM_ST_HEADER + P * W].view(np.int64).reshape(P, W)
        hit = pi[:, _lib.KSVM_P_STATUS] == word
        assert list(hit) == [int(y[bad_row]) in ab for ab in pairs] and (pi[~hit, _lib.KSVM_P_STATUS] == 0).all()
        assert (pi[:, _lib.KSVM_P_CONVERGED] == 0).all() and (pi[hit, _lib.KSVM_P_ITER] == 0).all() and (pi[~hit, _lib.KSVM_P_ITER] == 3).all()
        a0, a1 = s0[o:].reshape(2, 300, 3), s1[o:].reshape(2, 300, 3)
        for pr, (ca, cb) in enumerate(pairs):
            ra, rb = np.nonzero(y == ca)[0], np.nonzero(y == cb)[0]
            same = np.array_equal(a1[:, ra, cb - 1], a0[:, ra, cb - 1]) and np.array_equal(a1[:, rb, ca], a0[:, rb, ca])
            assert same == bool(hit[pr]), (pr, same)          # a stopped pair keeps alpha = 0, G = -1; the others moved

    where = np.arange(300)
    where[41] = 300
    with pytest.raises(ValueError, match="outside its range"):
        m.fit(dev(X), dev(y), row_index=dev(where))
    stopped_pairs(X, dev(where), 41, _lib.KSVM_RANGE)
    X[17, 2] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        m.fit(dev(X), dev(y))
    stopped_pairs(X, None, 17, _lib.KSVM_NAN)
