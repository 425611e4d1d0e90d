"""CPU: what pinn_amd._classify states once for the logistic regression and the two one-vs-one SVCs: the class-weight rule,
labels from class indices, votes from pairwise values, and the base class itself.  Also the hand-made models of
tests/test_gpu_classify.py, with the properties their draws must have checked here, on the host alone.

The models have one feature and no scaler, and every sign is exact.  Linear: w[p] and x drawn from {-1, 0, +1}, b = 0, so a
value is exactly -1, 0 or +1.  Kernel: one support row at z = 0 with coefficients from {-1, 0, +1}, rho = 0, gamma = 0.5, so a
value is +-K with K = exp(-x^2 / 2) >= e^-0.5, or exactly 0."""
import numpy as np
import pytest

KINDS, CLASSES, ROWS = ("linear", "kernel"), (2, 3, 8), (1, 127, 129)
SEEDS = {("linear", 2): 0, ("linear", 3): 7, ("linear", 8): 2, ("kernel", 2): 0, ("kernel", 3): 7, ("kernel", 8): 4}


def hand_model(kind, C):
    """A fitted-looking classifier (backend="host") with the drawn model, and the generator its rows come from."""
    from pinn_amd import ksvm, svm
    rng = np.random.default_rng(SEEDS[kind, C])
    P = C * (C - 1) // 2
    if kind == "linear":
        m = svm.DeviceLinearSVC(backend="host")
        m._w, m._b = rng.integers(-1, 2, (P, 1)).astype(np.float64), np.zeros(P)
        m.coef_, m.intercept_ = m._w, m._b
    else:
        m = ksvm.DeviceKernelSVC(backend="host")
        m._sv, m._coef = np.zeros((1, 1)), rng.integers(-1, 2, (1, C - 1)).astype(np.float64)
        m._sv_cls, m._rho, m._gamma = rng.integers(0, C, 1).astype(np.int64), np.zeros(P), 0.5
        m.dual_coef_ = m._coef.T
    m.class_weight_, m.classes_, m.n_features_in_ = np.ones(C), np.arange(C), 1
    return m, rng


def drawn_rows(rng, n):
    return rng.integers(-1, 2, (n, 1)).astype(np.float64)


def ties_and_zeros(out):
    """Per row: the top vote count is shared by two classes; a pairwise value is exactly zero."""
    top = out["votes"].max(axis=1)
    return (out["votes"] == top[:, None]).sum(axis=1) >= 2, (out["decision"] == 0.0).any(axis=1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", CLASSES)
def test_hand_models_hold_ties_and_zeros(kind, C):
    """What the device test relies on: beyond one row, every draw holds a value that is not zero and, from three classes on, an
    exactly-zero value and a row whose top vote count is shared.  (One pair cannot tie, and the kernel model's only pair has
    one coefficient: it is not zero, so that the sign of K is tested.)"""
    m, rng = hand_model(kind, C)
    for n in ROWS:
        X = drawn_rows(rng, n)
        out = m._decide(X, want=("decision", "votes", "pred"))
        tie, zero = ties_and_zeros(out)
        mag = np.abs(out["decision"])
        assert out["decision"].shape == (n, C * (C - 1) // 2) and ((mag == 0.0) | (mag >= np.exp(-0.5))).all()
        assert (out["votes"].sum(axis=1) == C * (C - 1) // 2).all() and np.array_equal(out["pred"], out["votes"].argmax(axis=1))
        if n > 1:
            assert (mag > 0.0).any() and (C == 2 or (zero.any() and tie.any())), (kind, C, n)


def test_votes_on_a_cycle_and_on_an_exact_zero():
    from pinn_amd import _classify as K
    # 0 beats 1, 2 beats 0, 1 beats 2: one vote each, the first maximum wins
    votes, pred = K.votes_of(np.array([[1.0, -1.0, 1.0]] * 2), 3)
    assert np.array_equal(votes, [[1, 1, 1]] * 2) and np.array_equal(pred, [0, 0]) and votes.dtype == pred.dtype == np.int64
    # 1 beats 0, 2 beats 0, and a value of exactly 0 is a vote for the pair's second class
    votes, pred = K.votes_of(np.array([[-1.0, -1.0, 0.0]]), 3)
    assert np.array_equal(votes, [[0, 1, 2]]) and np.array_equal(pred, [2])


def test_class_weights_labels_and_the_base_class():
    import torch
    from pinn_amd import _classify as K, ksvm, svm
    assert issubclass(svm.DeviceLinearSVC, K.OneVsOneSVC) and issubclass(ksvm.DeviceKernelSVC, K.OneVsOneSVC)
    assert issubclass(ksvm.KernelSVMDiagnoser, svm.SVMDiagnoser) and svm.pairs_of is K.pairs_of and svm.slot_of is K.slot_of
    classes, count = np.array([5, 7, 9]), np.array([2, 6, 4])
    for cls in (svm.DeviceLinearSVC, ksvm.DeviceKernelSVC):
        assert np.array_equal(cls(backend="host")._weights(classes, count), np.ones(3))
        assert np.array_equal(cls(class_weight="balanced", backend="host")._weights(classes, count), 12 / (3 * count.astype(np.float64)))
        by_dict = cls(class_weight={5: 2.0, 9: 0.5}, backend="host")        # no entry for 7; the classes are numpy scalars
        assert np.array_equal(by_dict._weights(classes, count), [2.0, 1.0, 0.5])
        for cw in (None, "balanced", {5: 2.0}):
            with pytest.raises(ValueError, match="a class without rows"):
                cls(class_weight=cw, backend="host")._weights(classes, np.array([2, 0, 4]))
    pred = np.array([2, 0, 0, 1])
    assert np.array_equal(K.labels_of(classes, pred), [9, 5, 5, 7])
    for cl in (classes, torch.from_numpy(classes)):
        got = K.labels_of(cl, torch.from_numpy(pred))
        assert isinstance(got, torch.Tensor) and got.tolist() == [9, 5, 5, 7]
    mean, scale = K.scaler_stats(None, 3)
    assert np.array_equal(mean, np.zeros(3)) and np.array_equal(scale, np.ones(3))
