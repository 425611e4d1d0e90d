"""CPU: the float64 referee of the physics-stage optimizer (tests/stage_optimizer.py).  It is torch's Adam, its list of parameters
without a gradient is autograd's, and a numpy float32 twin of the kernel's operation order stays inside the referee's three bounds."""
import numpy as np
import pytest
import torch

import pinn_oracle as O
import stage_optimizer as so


def _synthetic_sums(rng):
    s = np.zeros(so.NSUMS)
    s[:len(so.SUM_NAMES)] = rng.normal(size=len(so.SUM_NAMES)) * 10.0 ** rng.uniform(-2, 3, size=len(so.SUM_NAMES))
    for k in ("FV2", "YV2", "YU2", "FT2", "FH2", "FO2"):
        s[so.S[k]] = abs(s[so.S[k]]) + 1e-3
    return s


def test_tables_agree_with_the_binding_and_the_oracle():
    from pinn_amd import _lib
    assert so.S == _lib.S and so.NSUMS == _lib.NSUMS and so.NLAMBDA == _lib.NLAMBDA == len(O.LAMBDA_NAMES)
    assert so.STAGE_IDS == (_lib.STAGE_LAMBDA_PM, _lib.STAGE_LAMBDA_F, _lib.STAGE_THERMAL, _lib.STAGE_HYDROGEN, _lib.STAGE_OXYGEN)
    seen = []
    for stage in so.STAGE_IDS[1:]:
        idx = so.stage_index(stage)
        assert idx == list(range(idx[0], idx[0] + len(idx)))          # a stage's parameters are one contiguous run of slots
        seen += idx
    assert sorted(seen) == list(range(so.NLAMBDA))                    # and the four runs tile the 17 slots
    assert sum(len(so.stage_bounds(s)) for s in so.STAGE_IDS[1:]) * 2 == 34
    for stage in so.STAGE_IDS:
        for lo, hi in so.stage_bounds(stage):
            assert lo.dtype == np.float32 and hi.dtype == np.float32 and lo < hi


@pytest.mark.parametrize("stage", so.STAGE_IDS)
def test_referee_is_torch_adam(stage):
    """With torch's double constants the referee's step is O.AdamState's on float64 tensors, to 1e-15 relative: the parameter, both
    moments, a skipped parameter and the clamp.  Steps 1, 2 and 1000 with carried moments of both signs."""
    rng = np.random.default_rng(100 + stage)
    names, idx = so.stage_names(stage), so.stage_index(stage)
    bounds = O.STAGES[so.STAGE_KEY[stage]][3]
    for step in (1, 2, 1000):
        sums = _synthetic_sums(rng)
        n, vn_scale, lr = 2049, np.float32(0.0123), np.float32(so.stage_rate(stage)[0] * 0.8)
        lam = np.array([O.LAMBDA_INIT[k] for k in O.LAMBDA_NAMES], dtype=np.float32)
        adam = np.zeros(2 * so.NLAMBDA, dtype=np.float32)
        g, _ = so.gradients(stage, sums, n, vn_scale)
        if step > 1:
            for name, i in zip(names, idx):
                if name in g:
                    adam[i] = np.float32(g[name] * rng.choice([-0.7, 0.4, 1.3]))
                    adam[so.NLAMBDA + i] = np.float32(g[name] ** 2 * rng.uniform(0.5, 2.0))
        r = so.referee_step(stage, sums, n, vn_scale, lr, step, lam, adam, consts=so.TORCH)
        ps = [torch.tensor([float(lam[i])], dtype=torch.float64) for i in idx]
        st = O.AdamState(ps)
        for k, i in enumerate(idx):
            st.m[k].fill_(float(adam[i])); st.v[k].fill_(float(adam[so.NLAMBDA + i])); st.t[k] = step - 1
        grads = [torch.tensor([g[name]], dtype=torch.float64) if name in g else None for name in names]
        st.step(ps, grads, float(lr))
        for k, (i, (lo, hi)) in enumerate(zip(idx, bounds)):
            want_step = ps[k].item()
            want = float(torch.clamp(ps[k], float(np.float32(lo)), float(np.float32(hi))).item())
            assert abs(r["lam_step"][i] - want_step) <= 1e-15 * abs(want_step), (step, names[k])
            assert abs(r["lam"][i] - want) <= 1e-15 * abs(want), (step, names[k])
            assert abs(r["m"][i] - st.m[k].item()) <= 1e-15 * abs(st.m[k].item()), (step, names[k])
            assert abs(r["v"][i] - st.v[k].item()) <= 1e-15 * abs(st.v[k].item()), (step, names[k])
            if not r["has_grad"][k]:
                assert r["lam_step"][i] == float(lam[i]) and r["m"][i] == float(adam[i]) and r["v"][i] == float(adam[so.NLAMBDA + i])
        other = [i for i in range(so.NLAMBDA) if i not in idx]
        assert np.array_equal(r["lam"][other], lam[other].astype(np.float64))
    # the losses are the means the reference prints
    g, (total, physics) = so.gradients(stage, sums, n, vn_scale)
    assert physics == sums[so.S[so.PHYSICS_SUM[stage]]] / n
    assert total == (physics + sums[so.S["YU2"]] / n if so.STAGE_KIND[stage] == "V" else physics)


@pytest.mark.parametrize("stage", so.STAGE_IDS)
def test_gradients_and_no_gradient_list_are_autograd(stage):
    """On synthetic rows: the parameters for which torch.autograd.grad(O.stage_loss) returns None are exactly the referee's list (every
    stage, both voltage variants), and every other gradient is finite and non-zero."""
    from pinn_amd import synth
    ds = synth.make_dataset(257, (), seed=6)
    real = torch.from_numpy(O.denorm(ds[0].numpy(), *O.scaler_affine(ds[4])))
    names = so.stage_names(stage)
    lam = O.init_lambdas()
    ps = [lam[n].clone().requires_grad_(True) for n in names]
    for n, p in zip(names, ps):
        lam[n] = p
    kw = {}
    if so.STAGE_KIND[stage] == "V":
        ymn, ysc = O.scaler_affine(ds[5])
        kw = dict(y=ds[1].reshape(-1, 1), u_eval=(ds[1] + 0.01).reshape(-1, 1), y_min=ymn, y_scale=ysc, u_scal=ds[5],
                  dnn_para=stage == so.STAGE_LAMBDA_F)
    total, _ = O.stage_loss(so.STAGE_KEY[stage], real, lam, **kw)
    grads = torch.autograd.grad(total, ps, allow_unused=True)
    none = [n for n, g in zip(names, grads) if g is None]
    print("stage %d without a gradient: %s" % (stage, none))
    assert none == so.no_grad_names(stage)
    assert all(torch.isfinite(g).all() and float(g.abs()) > 0.0 for g in grads if g is not None)


def test_no_gradient_list_names_five_parameters():
    got = sorted(set(n for s in so.STAGE_IDS for n in so.no_grad_names(s)))
    assert got == sorted(["lambda_4", "lambda_T2", "lambda_T4", "lambda_H4", "lambda_O4"])


def _draw(rng, n_cases):
    """Steps, StepLR rates of every stage after 0..4 edges, gradients over ten decades, moments of both signs relative to the gradient."""
    step = rng.choice([1, 2, 3, 10, 1000, 46007], size=n_cases)
    rates = np.array([np.float32(O.steplr(lr0, gamma, 1, k)) for _, lr0, gamma, _ in O.STAGES.values() for k in range(5)], dtype=np.float32)
    lr = rng.choice(rates, size=n_cases)
    g = rng.choice([-1.0, 1.0], size=n_cases) * 10.0 ** rng.uniform(-6, 4, size=n_cases)
    m = (g * rng.choice([-1.0, 1.0], size=n_cases) * 10.0 ** rng.uniform(-3, 1, size=n_cases)).astype(np.float32)
    m[rng.random(n_cases) < 0.1] = 0.0
    v = (g * g * 10.0 ** rng.uniform(-2, 2, size=n_cases)).astype(np.float32)
    v[rng.random(n_cases) < 0.1] = 0.0
    p = (rng.choice([-1.0, 1.0], size=n_cases) * 10.0 ** rng.uniform(-6, 4, size=n_cases)).astype(np.float32)
    return g, p, m, v, lr, step


def test_float32_twin_stays_inside_the_bounds():
    """200 000 drawn steps: the numpy float32 restatement of the kernel's operation order against the referee, as fractions of the
    units each bound allows (16, 3 and 5).  Second moments below 1e-40 are subnormal in float32 and excluded."""
    rng = np.random.default_rng(7)
    g, p, m, v, lr, step = _draw(rng, 200000)
    r = so.adam_core(g, p, m, v, lr, step)
    p1, m1, v1 = so.mirror_core(g, p, m, v, lr, step)
    keep = r["v"] >= 1e-40
    assert keep.sum() > 190000
    with np.errstate(divide="ignore", invalid="ignore"):
        err_p = np.abs(p1.astype(np.float64) - r["p"])
        ep = err_p / r["bound_p"]
        # the step's share in its own units: what is left of the error after the final subtraction's u |p'|
        es = np.where(r["unit_step"] > 0, np.maximum(err_p - so.U * np.abs(r["p"]), 0.0) / r["unit_step"], 0.0)
        em = np.where(r["bound_m"] > 0, np.abs(m1.astype(np.float64) - r["m"]) / (so.U * r["S_m"]), 0.0)
        ev = np.abs(v1.astype(np.float64) - r["v"]) / (so.U * r["v"])
    worst = (es[keep].max(), em[keep].max(), ev[keep].max())
    print("float32 twin, largest error in units u: step %.2f of %g, first moment %.2f of %g, second moment %.2f of %g; "
          "parameter error / bound %.3f" % (worst[0], so.P_UNITS, worst[1], so.M_UNITS, worst[2], so.V_UNITS, ep[keep].max()))
    assert np.all(np.isfinite(ep[keep])) and np.all(np.isfinite(ev[keep]))
    assert ep[keep].max() <= 1.0
    assert worst[0] <= so.P_UNITS and worst[1] <= so.M_UNITS and worst[2] <= so.V_UNITS
    # the bounds are not slack by orders of magnitude either: the twin uses a fair share of each
    assert worst[0] >= 1.0 and worst[1] >= 1.0 and worst[2] >= 1.0


def test_ulps():
    a = np.array([1.0, -1.0, 0.0, 1.0], dtype=np.float32)
    b = np.array([np.nextafter(np.float32(1.0), np.float32(2.0)), -1.0, -0.0, 1.0], dtype=np.float32)
    assert so.ulps(a, b).tolist() == [1, 0, 0, 0]
