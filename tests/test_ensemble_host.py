"""CPU: the float64 referee of the ensemble's combine rules against hand-computed cases, the case lists, and what the Python
layer promises without a GPU (the module imports, the constructor raises, the results keyword exists)."""
import inspect
import math

import numpy as np
import pytest

import ensemble_cases as EC


def test_referee_hand_computed_two_members():
    # u = (1, 3): mean 2, mean of squares 5, variance 1.  logvar = (0, ln 4): rule 0 sqrt(exp(ln 2)) = sqrt 2; rule 1 sqrt((1 + 4) / 2)
    u = np.array([[1.0], [3.0]], np.float32)
    lv = np.array([[0.0], [math.log(4.0)]], np.float32)
    lv64 = lv.astype(np.float64)
    pm, au, eu = EC.combine_referee(u, lv, 0)
    assert pm[0] == 2.0 and eu[0] == 1.0
    assert au[0] == math.sqrt(math.exp((lv64[0, 0] + lv64[1, 0]) / 2))
    assert abs(au[0] - math.sqrt(2.0)) < 1e-7          # (ln 4 was rounded to float32 on the way in)
    pm, au, eu = EC.combine_referee(u, lv, 1)
    assert pm[0] == 2.0 and eu[0] == 1.0
    assert abs(au[0] - math.sqrt(2.5)) < 1e-7


def test_referee_hand_computed_three_members_two_rows():
    u = np.array([[0.0, -1.0], [3.0, -1.0], [6.0, 2.0]], np.float32)
    lv = np.zeros((3, 2), np.float32)
    for rule in (0, 1):
        pm, au, eu = EC.combine_referee(u, lv, rule)
        assert pm.tolist() == [3.0, 0.0]
        assert eu[0] == math.sqrt(15.0 - 9.0) and eu[1] == math.sqrt(2.0)
        assert au.tolist() == [1.0, 1.0]                 # unit variances under both rules


def test_referee_one_member_has_no_spread():
    rng = np.random.default_rng(0)
    u = rng.standard_normal((1, 257)).astype(np.float32)
    lv = rng.standard_normal((1, 257)).astype(np.float32)
    for rule in (0, 1):
        pm, au, eu = EC.combine_referee(u, lv, rule)
        assert np.array_equal(pm, u[0].astype(np.float64))
        assert np.array_equal(eu, np.zeros(257))         # exactly 0: u^2 - u^2 in one precision
        assert np.allclose(au, np.exp(0.5 * lv[0].astype(np.float64)), rtol=1e-14, atol=0)


@pytest.mark.parametrize("e", [2, 3, 5, 32])
def test_referee_equal_members_have_no_spread(e):
    """k u and k u^2 are exact in float64 for a float32 u and k <= 32 (24 + 5 and 48 + 5 bits), so the variance is exactly 0."""
    rng = np.random.default_rng(e)
    u1 = rng.standard_normal(300).astype(np.float32)
    lv1 = rng.standard_normal(300).astype(np.float32)
    u, lv = np.tile(u1, (e, 1)), np.tile(lv1, (e, 1))
    for rule in (0, 1):
        pm, au, eu = EC.combine_referee(u, lv, rule)
        assert np.array_equal(pm, u1.astype(np.float64))
        assert np.array_equal(eu, np.zeros(300))
        assert np.allclose(au, np.exp(0.5 * lv1.astype(np.float64)), rtol=1e-14, atol=0)


def test_referee_rules_order():
    """Jensen: the mixture variance is never below the geometric one, and they differ once the members' variances do."""
    rng = np.random.default_rng(3)
    u = rng.standard_normal((5, 100)).astype(np.float32)
    lv = rng.standard_normal((5, 100)).astype(np.float32)
    a0 = EC.combine_referee(u, lv, 0)[1]
    a1 = EC.combine_referee(u, lv, 1)[1]
    assert np.all(a1 >= a0) and np.any(a1 > a0 * 1.01)
    assert np.array_equal(EC.combine_referee(u, lv, 0)[2], EC.combine_referee(u, lv, 1)[2])


def test_case_lists_are_what_the_kernels_need():
    assert EC.LAYERS == [[8, 4, 1], [8, 33, 12, 1], [8, 64, 64, 1]]
    assert EC.ROWS == [1, 63, 65, 200, 4200] and EC.MEMBERS == [1, 2, 3, 5, 32]
    assert len(EC.CASES) == 75 and len({EC.case_id(c) for c in EC.CASES}) == 75
    assert (EC.SEED + 1) & EC.MASK64 == EC.MASK64 and (EC.SEED + 2) & EC.MASK64 == 0          # the seed wraps at member 2


def test_module_imports_without_gpu():
    import pinn_amd
    from pinn_amd import ensemble
    assert pinn_amd.DeepEnsemble is ensemble.DeepEnsemble
    assert ensemble.RULES == {"mc": 0, "mixture": 1}
    for word in ("bagging", "different layers", "MC-dropout inside", "autograd", "data parallelism", "fused and wide"):
        assert word in ensemble.__doc__, word


def test_constructor_fails_loudly_without_gpu():
    import torch
    from pinn_amd import ensemble
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(Exception) as e:
        ensemble.DeepEnsemble([8, 32, 32, 1], 4, p=0.2)
    assert "GPU" in str(e.value)


def test_results_array_takes_an_ensemble_keyword():
    from pinn_amd import results
    sig = inspect.signature(results.create_comprehensive_results_array_v2)
    assert sig.parameters["ensemble"].default is None
    assert list(sig.parameters)[:5] == ["model", "dataset", "mc_times", "dropout", "device_output"]
