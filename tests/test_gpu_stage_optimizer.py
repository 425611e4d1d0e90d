"""The physics-stage optimizer on the device against the float64 referee of tests/stage_optimizer.py.

pinn_lambda_step reads nothing but d_sums, so the first half feeds it synthetic sums that give every gradient a chosen sign and size:
every clamp bound of every parameter, interior steps at the referee's rounding bounds, the parameters without a gradient, the slots
of the other stages and NaN sums.  The second half runs the persistent kernel behind pinn_lambda_stage_run on synthetic rows with a
short StepLR schedule (an edge every 3 epochs): against the referee from non-zero first epochs, resumed in two calls, its log rows,
and the row counts around its two- and four-row trips.  Bounds come from the rounding count in stage_optimizer's docstring; the two
route gates (rtol 2e-5 / atol 1e-9 on parameters, rtol 2e-6 on sums) are test_gpu_model's and test_gpu_stage_pass's."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pinn_oracle as O
import stage_optimizer as so

E_ARG = -1
STEPS = [1, 2, 10, 1000, 46007]
N_ROWS, LR_STEP, N_ITERS = 2049, 3, 7
ROW_COUNTS = [1, 1023, 1024, 1025, 2047, 2049, 4095, 4097, 65536]
VN_SCALE = np.float32(0.37)
N_SYNTH = 4099


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _lam_init():
    return np.array([O.LAMBDA_INIT[n] for n in O.LAMBDA_NAMES], dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# pinn_lambda_step on synthetic sums
# ------------------------------------------------------------------------------------------------------------------------
def _sums_for(stage, grads, n, rng):
    """32 sums whose gradients of `stage` are `grads` (name -> value); every other sum a distinct finite number, the sums of squares
    positive."""
    s = np.zeros(so.NSUMS)
    k = len(so.SUM_NAMES)
    s[:k] = rng.choice([-1.0, 1.0], size=k) * 10.0 ** rng.uniform(-1, 3, size=k)
    for name in ("FV2", "YV2", "YU2", "FT2", "FH2", "FO2"):
        s[so.S[name]] = abs(s[so.S[name]])
    for name, g in grads.items():
        src = so.S[so.GRAD_SUM[stage][name]]
        s[src] = -g * n / (10.0 * float(VN_SCALE)) if stage == so.STAGE_LAMBDA_PM else g * n / 2.0
    got, _ = so.gradients(stage, s, n, VN_SCALE)
    assert all(abs(got[name] - g) <= 1e-12 * abs(g) for name, g in grads.items())
    return s


def _prefill(rng):
    """Distinct values in all 17 parameter and 34 moment slots: interior parameters, moments no optimizer would leave."""
    lam = (_lam_init().astype(np.float64) * (1.0 + 0.01 * rng.uniform(-1, 1, size=so.NLAMBDA))).astype(np.float32)
    adam = np.concatenate([100.0 + np.arange(so.NLAMBDA) + rng.uniform(0.1, 0.9, size=so.NLAMBDA),
                           300.0 + np.arange(so.NLAMBDA) + rng.uniform(0.1, 0.9, size=so.NLAMBDA)]).astype(np.float32)
    assert len(set(adam.tolist())) == 2 * so.NLAMBDA and len(set(lam.tolist())) == so.NLAMBDA
    return lam, adam


def _step(lib, stage, sums, n, lr, step, lam, adam):
    """One pinn_lambda_step; returns (lam, adam, loss) and checks that no slot of another stage changed a bit."""
    import hip_helpers as hh
    from pinn_amd import _lib
    d_sums = torch.from_numpy(np.asarray(sums, dtype=np.float64)).to(hh.dev())
    d_lam, d_adam = torch.from_numpy(lam.copy()).to(hh.dev()), torch.from_numpy(adam.copy()).to(hh.dev())
    d_loss = torch.full((2,), float("nan"), device=hh.dev())
    _lib.check(lib.pinn_lambda_step(stage, hh.ptr(d_sums), n, float(VN_SCALE), float(lr), int(step), hh.ptr(d_lam), hh.ptr(d_adam),
                                    hh.ptr(d_loss), hh.stream()), "pinn_lambda_step")
    lam1, adam1, loss = d_lam.cpu().numpy(), d_adam.cpu().numpy(), d_loss.cpu().numpy()
    other = np.array([i not in so.stage_index(stage) for i in range(so.NLAMBDA)])
    assert np.array_equal(_bits(lam1)[other], _bits(lam)[other]), "a parameter of another stage changed"
    assert np.array_equal(_bits(adam1)[np.tile(other, 2)], _bits(adam)[np.tile(other, 2)]), "a moment of another stage changed"
    return lam1, adam1, loss


def _ratios(r, lam1, adam1, idx):
    """Error / bound of the parameters with a gradient: (parameter, first moment, second moment), each the largest over idx."""
    n = so.NLAMBDA
    out = []
    for got, want, bound in ((lam1, r["lam"], r["bound_p"]), (adam1[:n], r["m"], r["bound_m"]), (adam1[n:], r["v"], r["bound_v"])):
        e = np.abs(got[idx].astype(np.float64) - want[idx])
        assert np.all(bound[idx] > 0.0)
        out.append(float((e / bound[idx]).max()))
    return out


@pytest.mark.parametrize("stage", so.STAGE_IDS)
def test_step_clamps_at_every_bound(lib, stage):
    """Step 1 from zero moments moves a parameter by lr sign(g) (up to eps): started half a step inside a bound it crosses it and comes
    out at the float32 bound, bit for bit, with the moments of the unclamped step."""
    rng = np.random.default_rng(10 + stage)
    names, idx, bounds = so.stage_names(stage), so.stage_index(stage), so.stage_bounds(stage)
    lr = np.float32(so.stage_rate(stage)[0])
    live = [(k, i) for k, (name, i) in enumerate(zip(names, idx)) if name in so.GRAD_SUM[stage]]
    worst = [0.0, 0.0]
    for side in (0, 1):
        lam, adam = _prefill(rng)
        grads = {}
        for k, i in live:
            adam[i] = adam[so.NLAMBDA + i] = 0.0
            mag = 10.0 ** rng.uniform(-2, 2)
            grads[names[k]] = mag if side == 0 else -mag
            lam[i] = np.float32(float(bounds[k][side]) + (0.5 if side == 0 else -0.5) * float(lr))
            # (lambda_2's range is a two-hundredth of its rate: its start lies beyond the other bound, which the step crosses back)
        sums = _sums_for(stage, grads, N_SYNTH, rng)
        r = so.referee_step(stage, sums, N_SYNTH, VN_SCALE, lr, 1, lam, adam)
        lam1, adam1, _ = _step(lib, stage, sums, N_SYNTH, lr, 1, lam, adam)
        for k, i in live:
            crossed = r["lam_step"][i] < float(bounds[k][0]) if side == 0 else r["lam_step"][i] > float(bounds[k][1])
            assert crossed and r["lam"][i] == float(bounds[k][side])
            assert _bits(lam1[i]) == _bits(bounds[k][side]), (names[k], "lo" if side == 0 else "hi", lam1[i], bounds[k][side])
        live_idx = [i for _, i in live]
        _, em, ev = _ratios(r, lam1, adam1, live_idx)
        worst = [max(worst[0], em), max(worst[1], ev)]
    print("stage %d at its %d bounds: moment error / bound %.3f (first), %.3f (second)" % (stage, 2 * len(live), worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0


def _interior_case(stage, step, sign, rng):
    """Sums, parameters and moments of one interior step: moments of sign `sign` relative to the gradient, the second moment raised
    until the referee's step stays a tenth of the way from either bound (lambda_2's range is a thousandth of its rate)."""
    names, idx, bounds = so.stage_names(stage), so.stage_index(stage), so.stage_bounds(stage)
    lr0, gamma = so.stage_rate(stage)
    lr = np.float32(O.steplr(lr0, gamma, 1000, step - 1))
    lam, adam = _prefill(rng)
    grads = {n: float(rng.choice([-1.0, 1.0])) * 10.0 ** rng.uniform(-3, 2) for n in so.GRAD_SUM[stage]}
    sums = _sums_for(stage, grads, N_SYNTH, rng)
    for k, (name, i) in enumerate(zip(names, idx)):
        if name not in grads:
            continue
        g = grads[name]
        adam[i] = np.float32(sign * g * 10.0 ** rng.uniform(-1, 1))
        v = g * g * 10.0 ** rng.uniform(-1, 1)
        room = 0.1 * min(float(lam[i]) - float(bounds[k][0]), float(bounds[k][1]) - float(lam[i]))
        assert room > 0.0
        for _ in range(40):
            adam[so.NLAMBDA + i] = np.float32(v)
            c = so.adam_core(g, lam[i], adam[i], adam[so.NLAMBDA + i], lr, step)
            if abs(float(c["p"]) - float(lam[i])) <= room:
                break
            v *= 100.0
        else:
            raise AssertionError("no interior step for %s" % name)
    return sums, lr, lam, adam


@pytest.mark.parametrize("stage", so.STAGE_IDS)
def test_interior_steps_within_rounding_bounds(lib, stage):
    """Steps 1, 2, 10, 1000 and 46007 with prior moments of both signs relative to the gradient: parameters and both moments inside the
    referee's forward error bounds, both losses within 2 u.  PINN_STAGE_LAMBDA_PM's gradient is -(2 / N) 5 vn_scale sum, its data term
    YU2; the bias corrections at step 46007 are 1 to the last bit, at step 1 they are 0.1 and 0.001."""
    rng = np.random.default_rng(20 + stage)
    idx = so.stage_index(stage)
    live = [i for n, i in zip(so.stage_names(stage), idx) if n in so.GRAD_SUM[stage]]
    worst, worst_loss = [0.0, 0.0, 0.0], 0.0
    for step in STEPS:
        for sign in (1.0, -1.0):
            sums, lr, lam, adam = _interior_case(stage, step, sign, rng)
            r = so.referee_step(stage, sums, N_SYNTH, VN_SCALE, lr, step, lam, adam)
            assert np.array_equal(r["lam"], r["lam_step"])                       # interior: the clamp does nothing
            lam1, adam1, loss = _step(lib, stage, sums, N_SYNTH, lr, step, lam, adam)
            worst = [max(a, b) for a, b in zip(worst, _ratios(r, lam1, adam1, live))]
            assert not np.array_equal(_bits(lam1[live]), _bits(lam[live]))
            for got, want in zip(loss, r["loss"]):
                assert want > 0.0
                worst_loss = max(worst_loss, abs(float(got) - want) / (so.U * want))
    print("stage %d interior steps, error / bound: parameter %.3f, first moment %.3f, second moment %.3f; loss %.2f u of %g"
          % (stage, worst[0], worst[1], worst[2], worst_loss, so.LOSS_UNITS))
    assert max(worst) <= 1.0
    assert worst_loss <= so.LOSS_UNITS


@pytest.mark.parametrize("stage", so.STAGE_IDS)
def test_parameters_without_gradient_are_only_clamped(lib, stage):
    """lambda_4, lambda_T2, lambda_T4, lambda_H4, lambda_O4: above hi -> hi, below lo -> lo, inside -> unchanged, bit for bit, and their
    moment slots keep what was in them."""
    rng = np.random.default_rng(30 + stage)
    names, idx, bounds = so.stage_names(stage), so.stage_index(stage), so.stage_bounds(stage)
    dead = [(k, i) for k, (name, i) in enumerate(zip(names, idx)) if name not in so.GRAD_SUM[stage]]
    assert dead
    for where in ("above", "below", "inside"):
        sums, lr, lam, adam = _interior_case(stage, 3, 1.0, rng)
        want = {}
        for k, i in dead:
            lo, hi = float(bounds[k][0]), float(bounds[k][1])
            lam[i] = np.float32({"above": hi + 1.0 + abs(hi), "below": lo - 1.0 - abs(lo), "inside": lo + 0.3137 * (hi - lo)}[where])
            want[i] = {"above": bounds[k][1], "below": bounds[k][0], "inside": lam[i]}[where]
        lam1, adam1, _ = _step(lib, stage, sums, N_SYNTH, lr, 3, lam, adam)
        r = so.referee_step(stage, sums, N_SYNTH, VN_SCALE, lr, 3, lam, adam)
        for k, i in dead:
            assert _bits(lam1[i]) == _bits(want[i]), (names[k], where, lam1[i], want[i])
            assert r["lam"][i] == float(want[i])
            assert _bits(adam1[i]) == _bits(adam[i]) and _bits(adam1[so.NLAMBDA + i]) == _bits(adam[so.NLAMBDA + i]), (names[k], where)


@pytest.mark.parametrize("stage", so.STAGE_IDS)
def test_slots_of_other_stages_keep_their_bits(lib, stage):
    """Every parameter and moment slot that belongs to another stage, pre-filled with distinct values, is unchanged (_step asserts it
    on every call of this file; here on its own, with the stage's parameters moving)."""
    rng = np.random.default_rng(40 + stage)
    sums, lr, lam, adam = _interior_case(stage, 2, -1.0, rng)
    idx = so.stage_index(stage)
    lam1, adam1, _ = _step(lib, stage, sums, N_SYNTH, lr, 2, lam, adam)
    mine = np.zeros(so.NLAMBDA, dtype=bool)
    mine[idx] = True
    assert mine.sum() in (4, 5) and np.array_equal(_bits(lam1)[~mine], _bits(lam)[~mine])
    assert np.array_equal(_bits(adam1)[np.tile(~mine, 2)], _bits(adam)[np.tile(~mine, 2)])
    assert not np.array_equal(_bits(lam1)[mine], _bits(lam)[mine])


@pytest.mark.parametrize("stage", [so.STAGE_THERMAL, so.STAGE_HYDROGEN, so.STAGE_OXYGEN])
def test_nan_sum_reaches_what_it_feeds(lib, stage):
    """Each sum of the stage's range in turn is NaN: exactly the parameters it feeds (and their moments) become NaN and the clamp does
    not bring them back; the parameters without a gradient stay finite; the losses are NaN iff it is the sum of squares."""
    rng = np.random.default_rng(50 + stage)
    names, idx = so.stage_names(stage), so.stage_index(stage)
    lo, hi = so.LIVE[so.STAGE_KIND[stage]]
    for s in range(so.S[lo], so.S[hi] + 1):
        sums, lr, lam, adam = _interior_case(stage, 2, 1.0, rng)
        sums[s] = float("nan")
        feeds = [so.GRAD_SUM[stage].get(n) == so.SUM_NAMES[s] for n in names]
        lam1, adam1, loss = _step(lib, stage, sums, N_SYNTH, lr, 2, lam, adam)
        r = so.referee_step(stage, sums, N_SYNTH, VN_SCALE, lr, 2, lam, adam)
        assert np.isnan(lam1[idx]).tolist() == feeds, (so.SUM_NAMES[s], lam1[idx])
        assert np.isnan(r["lam"][idx]).tolist() == feeds
        assert np.isnan(adam1[idx]).tolist() == feeds and np.isnan(adam1[so.NLAMBDA + np.array(idx)]).tolist() == feeds
        for n, i in zip(names, idx):
            if n not in so.GRAD_SUM[stage]:
                assert np.isfinite(lam1[i]) and _bits(lam1[i]) == _bits(lam[i])
        assert np.isnan(loss).tolist() == [so.SUM_NAMES[s] == so.PHYSICS_SUM[stage]] * 2, (so.SUM_NAMES[s], loss)
    assert sum(len(v) for v in so.GRAD_SUM[stage].values()) > 0


# ------------------------------------------------------------------------------------------------------------------------
# the persistent kernel: schedule, resume, log, row counts
# ------------------------------------------------------------------------------------------------------------------------
def _flag(stage):
    from pinn_amd import _lib
    return getattr(_lib, "RES_" + so.STAGE_KIND[stage])


@functools.lru_cache(maxsize=None)
def _rows(N):
    """The first N synthetic rows of a series of at least 256 (the scalers of a single row would be degenerate: a target scale of 2e12,
    with which the squared voltage gradient overflows float32 and Adam's step is 0 on the device and in torch alike)."""
    import hip_helpers as hh
    from pinn_amd import synth
    ds = synth.make_dataset(max(N, 256), (), seed=6)
    x, y = ds[0][:N].contiguous().to(hh.dev()), ds[1].reshape(-1)[:N].contiguous().to(hh.dev())
    u = (y + 0.01).contiguous()
    return x, u, y, hh.affine_struct(ds[4], ds[5])


@functools.lru_cache(maxsize=None)
def _stage_work(lib, N):
    import hip_helpers as hh
    wb = lib.pinn_lambda_stage_workspace_bytes(N)
    return torch.empty(wb, dtype=torch.uint8, device=hh.dev()), wb


@functools.lru_cache(maxsize=None)
def _res_work(lib):
    import hip_helpers as hh
    wb = lib.pinn_residuals_workspace_bytes()
    return torch.empty(wb, dtype=torch.uint8, device=hh.dev()), wb


def _stage_run(lib, stage, N, first_epoch, n_iters, lam, adam, log_rows=0, log_every=0, flags=None, expect=0):
    """pinn_lambda_stage_run on the rows of _rows(N) with the stage's own lr0 and gamma and an edge every LR_STEP epochs.
    Returns (lam, adam, loss, sums, log); the log pre-filled with NaN."""
    import hip_helpers as hh
    x, u, y, aff = _rows(N if N <= max(ROW_COUNTS) else max(ROW_COUNTS))
    lr0, gamma = so.stage_rate(stage)
    work, wb = _stage_work(lib, N)
    d_lam, d_adam = torch.from_numpy(np.asarray(lam, dtype=np.float32).copy()).to(hh.dev()), torch.from_numpy(np.asarray(adam, dtype=np.float32).copy()).to(hh.dev())
    d_loss = torch.full((2,), float("nan"), device=hh.dev())
    d_sums = torch.full((so.NSUMS,), float("nan"), dtype=torch.float64, device=hh.dev())
    from pinn_amd import _lib
    d_log = torch.full((log_rows, _lib.STAGE_LOG_FLOATS), float("nan"), device=hh.dev()) if log_rows else None
    rc = lib.pinn_lambda_stage_run(stage, _flag(stage) if flags is None else flags, hh.ptr(x), hh.ptr(u), hh.ptr(y), ctypes.byref(aff), N, lr0,
                                   gamma, LR_STEP, first_epoch, n_iters, hh.ptr(d_lam), hh.ptr(d_adam), hh.ptr(d_loss), hh.ptr(d_log), log_every,
                                   hh.ptr(d_sums), hh.ptr(work), wb, hh.stream())
    assert rc == expect, (rc, expect)
    return (d_lam.cpu().numpy(), d_adam.cpu().numpy(), d_loss.cpu().numpy(), d_sums.cpu().numpy(),
            d_log.cpu().numpy() if log_rows else None)


@functools.lru_cache(maxsize=None)
def _cache(lib, stage_kind, N):
    """The parameter-independent half of the rows (pinn_residuals_prepare), once per stage kind."""
    import hip_helpers as hh
    from pinn_amd import _lib
    x, u, y, aff = _rows(N)
    cache = torch.empty(6 * N, dtype=torch.float32, device=hh.dev())
    lam = torch.from_numpy(_lam_init()).to(hh.dev())
    _lib.check(lib.pinn_residuals_prepare(hh.ptr(x), hh.ptr(u), hh.ptr(y), ctypes.byref(aff), hh.ptr(lam), getattr(_lib, "RES_" + stage_kind), N,
                                          hh.ptr(cache), hh.stream()), "prepare")
    return cache


def _cached_sums(lib, stage, N, lam):
    import hip_helpers as hh
    from pinn_amd import _lib
    cache, (work, wb) = _cache(lib, so.STAGE_KIND[stage], N), _res_work(lib)
    d_lam = torch.from_numpy(np.asarray(lam, dtype=np.float32)).to(hh.dev())
    sums = torch.full((so.NSUMS,), float("nan"), dtype=torch.float64, device=hh.dev())
    _lib.check(lib.pinn_residuals_cached(hh.ptr(cache), ctypes.byref(_rows(N)[3]), hh.ptr(d_lam), _flag(stage), N, hh.ptr(sums), hh.ptr(work), wb,
                                         hh.stream()), "cached")
    return sums.cpu().numpy()


def _referee_run(lib, stage, N, first_epoch, n_iters, lam, adam):
    """n_iters referee steps from epoch first_epoch: sums from pinn_residuals_cached at the current float32 parameters, one float64
    step with step = epoch + 1 and rate O.steplr(lr0, gamma, LR_STEP, epoch), parameters and moments rounded to float32."""
    lr0, gamma = so.stage_rate(stage)
    vn_scale = _rows(N)[3].vn_scale
    lam, adam = np.asarray(lam, dtype=np.float32).copy(), np.asarray(adam, dtype=np.float32).copy()
    for epoch in range(first_epoch, first_epoch + n_iters):
        sums = _cached_sums(lib, stage, N, lam)
        r = so.referee_step(stage, sums, N, vn_scale, np.float32(O.steplr(lr0, gamma, LR_STEP, epoch)), epoch + 1, lam, adam)
        lam = r["lam"].astype(np.float32)
        adam = np.concatenate([r["m"], r["v"]]).astype(np.float32)
    return lam, adam


@functools.lru_cache(maxsize=None)
def _state_at(lib, stage, epoch):
    """Parameters and moments a stage has after `epoch` referee epochs from the initial values: what a resumed call starts from."""
    return _referee_run(lib, stage, N_ROWS, 0, epoch, _lam_init(), np.zeros(2 * so.NLAMBDA, dtype=np.float32))


@pytest.mark.parametrize("first_epoch", [0, 2, 3, 4])
@pytest.mark.parametrize("stage", so.STAGE_IDS)
def test_stage_run_against_referee(lib, stage, first_epoch):
    """7 iterations from epoch 0, 2, 3 and 4 (an edge every 3 epochs, so the first rate is lr0 gamma^0 or gamma^1 and the first bias
    corrections 1 - beta^(first_epoch + 1)) against the referee stepping on the device's own sums."""
    lam0, adam0 = _state_at(lib, stage, first_epoch)
    want, want_adam = _referee_run(lib, stage, N_ROWS, first_epoch, N_ITERS, lam0, adam0)
    got, got_adam, _, _, _ = _stage_run(lib, stage, N_ROWS, first_epoch, N_ITERS, lam0, adam0)
    idx = so.stage_index(stage)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(got[idx].astype(np.float64) - want[idx]) / np.abs(want[idx])
    print("stage %d from epoch %d: largest relative distance to the referee %.3g, parameters %s" % (stage, first_epoch, rel.max(), got[idx].tolist()))
    assert np.all(np.isfinite(got)) and not np.array_equal(got[idx], lam0[idx])
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-9, err_msg="stage %d first_epoch %d" % (stage, first_epoch))
    other = [i for i in range(so.NLAMBDA) if i not in idx]
    assert np.array_equal(_bits(got)[other], _bits(lam0)[other])


@pytest.mark.parametrize("stage", so.STAGE_IDS)
def test_stage_run_resumes(lib, stage):
    """7 iterations in one call and as k + (7 - k), k in {1, 3, 4}, carrying d_lambda and d_adam with first_epoch = k in the second."""
    lam0, adam0 = _lam_init(), np.zeros(2 * so.NLAMBDA, dtype=np.float32)
    one, one_adam, _, _, _ = _stage_run(lib, stage, N_ROWS, 0, N_ITERS, lam0, adam0)
    for k in (1, 3, 4):
        a, a_adam, _, _, _ = _stage_run(lib, stage, N_ROWS, 0, k, lam0, adam0)
        b, b_adam, _, _, _ = _stage_run(lib, stage, N_ROWS, k, N_ITERS - k, a, a_adam)
        print("stage %d resumed at %d: %d units in the last place (parameters), %d (moments)"
              % (stage, k, so.ulps(one, b).max(), so.ulps(one_adam, b_adam).max()))
        np.testing.assert_allclose(b, one, rtol=2e-5, atol=1e-9, err_msg="stage %d split at %d" % (stage, k))


@pytest.mark.parametrize("first_epoch", [0, 2, 4])
@pytest.mark.parametrize("stage", so.STAGE_IDS)
def test_stage_run_log_rows(lib, stage, first_epoch):
    """log_every = 2: one row per even epoch of the range and no other; a row holds, bit for bit, what a call that stops after that
    epoch leaves in d_loss, d_lambda and d_sums, and the rate of the following epoch."""
    lr0, gamma = so.stage_rate(stage)
    lam0, adam0 = _state_at(lib, stage, first_epoch)
    n_log = 6
    _, _, _, _, log = _stage_run(lib, stage, N_ROWS, first_epoch, N_ITERS, lam0, adam0, log_rows=n_log, log_every=2)
    epochs = [e for e in range(first_epoch, first_epoch + N_ITERS) if e % 2 == 0]
    assert len(epochs) == 4
    for r, e in enumerate(epochs):
        lam_e, _, loss_e, sums_e, _ = _stage_run(lib, stage, N_ROWS, first_epoch, e - first_epoch + 1, lam0, adam0)
        assert np.array_equal(_bits(log[r, 0:2]), _bits(loss_e)), (r, e)
        assert np.array_equal(_bits(log[r, 3:20]), _bits(lam_e)), (r, e)
        assert np.array_equal(_bits(log[r, 20:52]), _bits(sums_e.astype(np.float32))), (r, e)
        want_lr = np.float32(lr0 * gamma ** ((e + 1) // LR_STEP))
        assert so.ulps(log[r, 2], want_lr) <= 1, (r, e, log[r, 2], want_lr)
        assert np.all(np.isnan(log[r, 52:]))
    assert np.all(np.isnan(log[len(epochs):]))
    assert np.all(np.isfinite(log[:len(epochs), :52]))


def test_stage_run_log_needs_an_aligned_first_epoch(lib):
    lam0, adam0 = _lam_init(), np.zeros(2 * so.NLAMBDA, dtype=np.float32)
    for first_epoch in (1, 3):
        lam, adam, _, _, log = _stage_run(lib, so.STAGE_THERMAL, N_ROWS, first_epoch, N_ITERS, lam0, adam0, log_rows=6, log_every=2, expect=E_ARG)
        assert np.array_equal(_bits(lam), _bits(lam0)) and np.all(np.isnan(log))


@pytest.mark.parametrize("N", ROW_COUNTS)
def test_stage_run_row_counts(lib, N):
    """One iteration of every stage at one row, around the edges of the 1024-thread trips (2 rows per thread in the voltage stage, 4 in
    the others) and at PINN_STAGE_RUN_MAX_ROWS: d_sums against pinn_residuals at the same flag (the stage's range; the rest exactly 0),
    the parameters against one pinn_lambda_step on those sums."""
    import hip_helpers as hh
    from pinn_amd import _lib
    x, u, y, aff = _rows(N)
    work, wb = _res_work(lib)
    lam0, adam0 = _lam_init(), np.zeros(2 * so.NLAMBDA, dtype=np.float32)
    d_lam0 = torch.from_numpy(lam0).to(hh.dev())
    for stage in so.STAGE_IDS:
        lam_p, adam_p, loss_p, sums_p, _ = _stage_run(lib, stage, N, 0, 1, lam0, adam0)
        ref = torch.full((_lib.NSUMS,), float("nan"), dtype=torch.float64, device=hh.dev())
        _lib.check(lib.pinn_residuals(hh.ptr(x), hh.ptr(u), hh.ptr(y), ctypes.byref(aff), hh.ptr(d_lam0), _flag(stage), N, None, 0, hh.ptr(ref),
                                      hh.ptr(work), wb, hh.stream()), "residuals")
        ref = ref.cpu().numpy()
        live = so.live_mask(so.STAGE_KIND[stage])
        assert np.all(sums_p[~live] == 0.0) and np.all(ref[~live] == 0.0)
        assert np.all(np.isfinite(ref[live])) and ref[live][0] > 0.0
        np.testing.assert_allclose(sums_p[live], ref[live], rtol=2e-6, atol=1e-6 * max(1.0, np.abs(ref).max()) * 1e-3,
                                   err_msg="stage %d N=%d" % (stage, N))
        lam_i, adam_i, loss_i = _step_on(lib, stage, sums_p, N, aff.vn_scale, so.stage_rate(stage)[0], lam0, adam0)
        print("stage %d N %d: %d units in the last place between the persistent kernel and pinn_lambda_step on its sums"
              % (stage, N, so.ulps(lam_p, lam_i).max()))
        np.testing.assert_allclose(lam_p, lam_i, rtol=2e-5, atol=1e-9, err_msg="stage %d N=%d" % (stage, N))
        assert not np.array_equal(lam_p, lam0)
        assert np.all(np.abs(loss_p - loss_i) <= 1e-5 * np.abs(loss_i))


def _step_on(lib, stage, sums, n, vn_scale, lr, lam, adam):
    import hip_helpers as hh
    from pinn_amd import _lib
    d_sums = torch.from_numpy(np.asarray(sums, dtype=np.float64)).to(hh.dev())
    d_lam, d_adam = torch.from_numpy(lam.copy()).to(hh.dev()), torch.from_numpy(adam.copy()).to(hh.dev())
    d_loss = torch.full((2,), float("nan"), device=hh.dev())
    _lib.check(lib.pinn_lambda_step(stage, hh.ptr(d_sums), n, vn_scale, lr, 1, hh.ptr(d_lam), hh.ptr(d_adam), hh.ptr(d_loss), hh.stream()),
               "pinn_lambda_step")
    return d_lam.cpu().numpy(), d_adam.cpu().numpy(), d_loss.cpu().numpy()


def test_stage_run_refuses_more_than_max_rows(lib):
    from pinn_amd import _lib
    assert max(ROW_COUNTS) == _lib.STAGE_RUN_MAX_ROWS
    lam0, adam0 = _lam_init(), np.zeros(2 * so.NLAMBDA, dtype=np.float32)
    lam, _, _, _, _ = _stage_run(lib, so.STAGE_HYDROGEN, _lib.STAGE_RUN_MAX_ROWS + 1, 0, 1, lam0, adam0, expect=E_ARG)
    assert np.array_equal(_bits(lam), _bits(lam0))


# ------------------------------------------------------------------------------------------------------------------------
# stage / flags pairs and what model.py hands over
# ------------------------------------------------------------------------------------------------------------------------
def test_stage_and_flags_must_agree(lib):
    """All 5 x 4 pairs: the voltage stages go with PINN_RES_V, every other stage with its own flag; anything else is PINN_E_ARG and
    touches nothing."""
    from pinn_amd import _lib
    lam0, adam0 = _lam_init(), np.zeros(2 * so.NLAMBDA, dtype=np.float32)
    for stage in so.STAGE_IDS:
        for flags in (_lib.RES_V, _lib.RES_T, _lib.RES_H, _lib.RES_O):
            ok = flags == _flag(stage)
            lam, adam, _, _, _ = _stage_run(lib, stage, 1025, 0, 1, lam0, adam0, flags=flags, expect=0 if ok else E_ARG)
            assert np.array_equal(_bits(lam), _bits(lam0)) != ok, (stage, flags)
            if not ok:
                assert np.array_equal(_bits(adam), _bits(adam0))


class _LibSpy:
    """Forwards every call to the library and keeps the arguments of the two stage entry points."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ("pinn_lambda_stage_run", "pinn_lambda_step"):
            return fn

        def spy(*args):
            self.calls.append((name, args))
            return fn(*args)
        return spy


@pytest.mark.parametrize("persistent", [True, False])
def test_trainers_hand_over_the_oracle_rates(lib, persistent, monkeypatch):
    """train_lambda (both variants), train_thermal, train_hydrogen and train_oxygen pass the lr0 and gamma of O.STAGES to
    _run_lambda_stage, with a stage and a flag that agree, and the library sees them: the persistent route as (lr0, gamma, 1000, 0),
    the iterated route as the float32 rate of epoch 0."""
    import pinn_amd
    from pinn_amd import synth
    seen = []
    inner = pinn_amd.PhysicsInformedNN._run_lambda_stage

    def wrapper(self, stage, nIter, flags, lr0, gamma, need_u, log_fn):
        seen.append((stage, nIter, flags, lr0, gamma, need_u))
        return inner(self, stage, nIter, flags, lr0, gamma, need_u, log_fn)
    monkeypatch.setattr(pinn_amd.PhysicsInformedNN, "_run_lambda_stage", wrapper)
    ds = synth.make_dataset(300, (), seed=4)
    torch.manual_seed(0)
    m = pinn_amd.PhysicsInformedNN(ds[0], ds[1], [8, 128, 128, 1], ds[4], ds[5], p=0.2, logvar=True, seed=2)
    m.verbose = False
    if not persistent:
        m.stage_run_max_rows = 0
    spy = _LibSpy(m._lib)
    m._lib = spy
    m.train_lambda(2, False); m.train_lambda(2, True); m.train_thermal(2); m.train_hydrogen(2); m.train_oxygen(2)
    assert [s[0] for s in seen] == list(so.STAGE_IDS) and all(s[1] == 2 for s in seen)
    for stage, _, flags, lr0, gamma, need_u in seen:
        assert (lr0, gamma) == so.stage_rate(stage), (stage, lr0, gamma)
        assert flags == _flag(stage) and need_u == (so.STAGE_KIND[stage] == "V")
    if persistent:
        assert [c[0] for c in spy.calls] == ["pinn_lambda_stage_run"] * 5
        for stage, (_, a) in zip(so.STAGE_IDS, spy.calls):
            assert (a[0], a[1]) == (stage, _flag(stage))
            assert (a[7], a[8], a[9], a[10], a[11]) == so.stage_rate(stage) + (1000, 0, 2)
    else:
        assert [c[0] for c in spy.calls] == ["pinn_lambda_step"] * 10
        for k, (_, a) in enumerate(spy.calls):
            stage = so.STAGE_IDS[k // 2]
            assert a[0] == stage and a[5] == k % 2 + 1
            assert np.float32(a[4]) == np.float32(so.stage_rate(stage)[0])
    assert np.all(np.isfinite(m._lambda.cpu().numpy()))
