"""GPU: deep ensembles on the any-width kernels (pinn_gens_*, pinn_amd.ensemble).

Bitwise part: member m of a batched call equals the single-network pinn_gnet_* call on member m's slices of the same buffers with
dropout seed + m -- torch.equal on the raw bytes, no tolerance.  Whatever pins the single-network path (golden vectors, the
float64 referee, the regimes) then pins the ensemble.  Then the combine against its float64 referee, and the Python layer."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ensemble_cases as EC
import gnet_helpers as G
from ensemble_cases import same_bytes
from hip_helpers import dev


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _rows(n):
    """x [n, 8], y [n] on the device: computed once per row count, shared by every test, never written."""
    x, y = G.data(n, seed=n, with_y=True)
    return x.to(dev()).contiguous(), y.to(dev()).contiguous()


@functools.lru_cache(maxsize=None)
def _params(layers, e):
    return EC.member_params(list(layers), e, seed=e + sum(layers)).to(dev())


def _case(layers, n, e):
    return _params(tuple(layers), e), _rows(n)


# ---------------------------------------------------------------------------------------------------------------------------
# bitwise: batched against E single calls
@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_forward_is_the_single_call_per_member(lib, case):
    layers, n, e = case
    fp, (x, _) = _case(*case)
    u, lv = EC.gens_forward(lib, layers, fp, x)
    for m in range(e):
        us, ls = G.forward(lib, layers, fp[m], x)
        assert same_bytes(u[m], us) and same_bytes(lv[m], ls), ("eval", m)
    stream = 0x80000001
    from pinn_amd import _lib
    u, lv = EC.gens_forward(lib, layers, fp, x, G.drop(_lib.DROP_PHILOX, layers, p=0.2, seed=EC.SEED, stream=stream))
    for m in range(e):
        us, ls = G.forward(lib, layers, fp[m], x, EC.member_drop(layers, m, stream))
        assert same_bytes(u[m], us) and same_bytes(lv[m], ls), ("philox", m)
    assert not torch.isnan(u).any() and not torch.isnan(lv).any()


@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_train_grads_are_the_single_call_per_member(lib, case):
    layers, n, e = case
    fp, (x, y) = _case(*case)
    from pinn_amd import _lib
    g, loss = EC.gens_train_grads(lib, layers, fp, x, y, G.drop(_lib.DROP_PHILOX, layers, p=0.2, seed=EC.SEED, stream=3))
    assert not torch.isnan(g).any() and not torch.isnan(loss).any()
    for m in range(e):
        gs, ls = G.train_grads(lib, layers, fp[m], x, y, EC.member_drop(layers, m, 3))
        assert same_bytes(g[m], gs), ("grads", m)
        assert same_bytes(loss[m], ls), ("loss sums", m, loss[m].tolist(), ls.tolist())


@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_three_train_steps_are_the_single_calls_per_member(lib, case):
    layers, n, e = case
    fp, (x, y) = _case(*case)
    from pinn_amd import _lib
    drops = [G.drop(_lib.DROP_PHILOX, layers, p=0.2, seed=EC.SEED, stream=k + 1) for k in range(3)]
    par, mo, vo = EC.gens_train_steps(lib, layers, fp, x, y, drops)
    assert not same_bytes(par, fp.cpu())
    for m in range(e):
        ps, ms, vs = EC.gnet_train_steps(lib, layers, fp[m], x, y, [EC.member_drop(layers, m, k + 1) for k in range(3)])
        assert same_bytes(par[m], ps) and same_bytes(mo[m], ms) and same_bytes(vo[m], vs), m


def test_second_chunk_accumulates_per_member(lib):
    """Two members of a wide net on a few rows more than one training chunk holds (the capacity comes from the library): the second
    chunk adds to each member's own acc and writes each member's own loss partials."""
    layers, e = EC.WIDE, 2
    cap, _ = EC.train_plan(lib, layers, 1 << 20)
    n = cap + 37
    assert EC.train_plan(lib, layers, n)[0] == cap and n > cap          # two chunks
    fp, (x, y) = _case(layers, n, e)
    from pinn_amd import _lib
    g, loss = EC.gens_train_grads(lib, layers, fp, x, y, G.drop(_lib.DROP_PHILOX, layers, p=0.2, seed=EC.SEED, stream=9))
    for m in range(e):
        gs, ls = G.train_grads(lib, layers, fp[m], x, y, EC.member_drop(layers, m, 9))
        assert same_bytes(g[m], gs) and same_bytes(loss[m], ls), m
    assert not same_bytes(g[0], g[1])


def test_most_slices_times_most_members(lib):
    """The grid limit.  gemm_kernel<kWgrad> counts slices in the grid's z (limit 65 535).  No legal shape makes slices * 32 reach it:
    a training chunk holds at most 131 072 rows (kMaxChunkRows) and slice_plan gives a slice at least 128 of them, so a chunk has at
    most 1024 slices whatever the 2048 of its tile rule, and 1024 * 32 = 32 768.  The member does not ride in z anyway: it is
    folded into the weight-gradient grid's x (member * tiles + tile, limit 2^31 - 1; at most 32 * 33 here), so there are no groups of
    members and nothing for a result to depend on.  This runs the extreme the planner can produce -- 1024 slices, 32 members --
    and asserts the bytes."""
    layers, e, n = [8, 4, 1], 32, 131072
    rows, slices = EC.train_plan(lib, layers, n)
    assert (rows, slices) == (131072, 1024) and slices * e < 65535
    assert max(EC.train_plan(lib, layers, k)[1] for k in (n + 64, 4 * n, 1 << 24)) == 1024          # more rows: more chunks, not more slices
    fp, (x, y) = _case(layers, n, e)
    from pinn_amd import _lib
    g, loss = EC.gens_train_grads(lib, layers, fp, x, y, G.drop(_lib.DROP_PHILOX, layers, p=0.2, seed=EC.SEED, stream=2))
    for m in range(e):
        gs, ls = G.train_grads(lib, layers, fp[m], x, y, EC.member_drop(layers, m, 2))
        assert same_bytes(g[m], gs) and same_bytes(loss[m], ls), m


@pytest.mark.parametrize("layers", EC.LAYERS, ids=lambda l: "x".join(map(str, l)))
def test_two_identical_batched_calls_are_byte_equal(lib, layers):
    fp, (x, y) = _case(layers, 200, 5)
    from pinn_amd import _lib
    d = G.drop(_lib.DROP_PHILOX, layers, p=0.2, seed=EC.SEED, stream=4)
    a, b = EC.gens_forward(lib, layers, fp, x, d), EC.gens_forward(lib, layers, fp, x, d)
    assert same_bytes(a[0], b[0]) and same_bytes(a[1], b[1])
    a, b = EC.gens_train_grads(lib, layers, fp, x, y, d), EC.gens_train_grads(lib, layers, fp, x, y, d)
    assert same_bytes(a[0], b[0]) and same_bytes(a[1], b[1])


@pytest.mark.parametrize("layers", EC.LAYERS, ids=lambda l: "x".join(map(str, l)))
def test_identical_members_give_identical_outputs(lib, layers):
    """A member stride applied to a shared pointer (the input rows, the targets) would show here.  The members' parameters are
    set equal by hand; their Philox seeds are seed + m by the ABI and cannot be, so the seeds are made equal the one way the ABI
    allows -- dropout off, in the forward and in the training call -- and the stochastic call must then differ."""
    e, n = 5, 200
    fp = EC.member_params(layers, e, seed=1, identical=True).to(dev())
    x, y = _rows(n)
    u, lv = EC.gens_forward(lib, layers, fp, x)
    g, loss = EC.gens_train_grads(lib, layers, fp, x, y)
    for m in range(1, e):
        assert same_bytes(u[m], u[0]) and same_bytes(lv[m], lv[0]), m
        assert same_bytes(g[m], g[0]) and same_bytes(loss[m], loss[0]), m
    from pinn_amd import _lib
    u, _ = EC.gens_forward(lib, layers, fp, x, G.drop(_lib.DROP_PHILOX, layers, p=0.5, seed=EC.SEED, stream=1))
    assert all(not same_bytes(u[m], u[0]) for m in range(1, e))


@pytest.mark.parametrize("layers", EC.LAYERS, ids=lambda l: "x".join(map(str, l)))
def test_members_leave_each_other_alone(lib, layers):
    """A member run alone (a batch of one, its seed set by hand) and the same member among different ones: the same bytes."""
    e, n = 5, 200
    fp, (x, y) = _case(layers, n, e)
    from pinn_amd import _lib
    d = G.drop(_lib.DROP_PHILOX, layers, p=0.2, seed=EC.SEED, stream=6)
    u, lv = EC.gens_forward(lib, layers, fp, x, d)
    g, loss = EC.gens_train_grads(lib, layers, fp, x, y, d)
    for m in range(e):
        one = fp[m:m + 1]
        u1, lv1 = EC.gens_forward(lib, layers, one, x, EC.member_drop(layers, m, 6))
        g1, loss1 = EC.gens_train_grads(lib, layers, one, x, y, EC.member_drop(layers, m, 6))
        assert same_bytes(u[m], u1[0]) and same_bytes(lv[m], lv1[0]), m
        assert same_bytes(g[m], g1[0]) and same_bytes(loss[m], loss1[0]), m
    # and another member's parameters do not reach it: change member 0, members 1.. keep their bytes
    fp2 = fp.clone()
    fp2[0] = fp[1]
    u2, lv2 = EC.gens_forward(lib, layers, fp2, x, d)
    assert same_bytes(u2[1:], u[1:]) and same_bytes(lv2[1:], lv[1:]) and not same_bytes(u2[0], u[0])


# ---------------------------------------------------------------------------------------------------------------------------
# combine
@pytest.mark.parametrize("e", [1, 2, 5, 32])
def test_combine_against_the_float64_referee(lib, e):
    """On the device's own u and logvar.  Bound: one float32 spacing of the referee's value -- the device rounds a double result
    once, and that can differ from numpy's only where the two double exp / sqrt differ in their last place across a float32
    rounding boundary."""
    layers, n = [8, 33, 12, 1], 4200
    fp, (x, _) = _case(layers, n, e)
    u, lv = EC.gens_forward(lib, layers, fp, x)
    ud, lvd = u.to(dev()), lv.to(dev())
    for rule in (0, 1):
        got = EC.gens_combine(lib, ud, lvd, rule)
        want = EC.combine_referee(u.numpy(), lv.numpy(), rule)
        for name, gv, wv in zip(("pred_mean", "a_u", "e_u"), got, want):
            w32 = wv.astype(np.float32)
            err = np.abs(gv.astype(np.float64) - w32.astype(np.float64))
            bound = np.spacing(np.abs(w32)).astype(np.float64)
            print("combine E=%d rule=%d %s: max err / spacing %.3f" % (e, rule, name, float(np.max(err / bound))))
            assert np.all(err <= bound), (rule, name, float(np.max(err / bound)))
        if e == 1:
            assert np.array_equal(got[2], np.zeros(n, np.float32))          # one member: no spread, exactly
            assert np.array_equal(got[0], u.numpy()[0])
    same = torch.cat([ud[:1]] * e), torch.cat([lvd[:1]] * e)
    for rule in (0, 1):
        got = EC.gens_combine(lib, same[0], same[1], rule)
        assert np.array_equal(got[2], np.zeros(n, np.float32)) and np.array_equal(got[0], u.numpy()[0])          # equal members


# ---------------------------------------------------------------------------------------------------------------------------
# the Python layer
LAYERS_PY, E_PY, SEED_PY, N_PY = [8, 33, 12, 1], 3, 7, 200


def _single_models(n):
    import pinn_amd
    from pinn_amd import synth
    ds = synth.make_dataset(n, (), seed=0)
    torch.manual_seed(5)
    models = []
    for m in range(E_PY):
        mod = pinn_amd.PhysicsInformedNN(ds[0], ds[1], LAYERS_PY, ds[4], ds[5], p=0.2, logvar=True, seed=SEED_PY + m, kernels="general")
        mod.verbose = False
        models.append(mod)
    return models, ds


def _ensemble():
    import pinn_amd
    torch.manual_seed(5)
    ens = pinn_amd.DeepEnsemble(LAYERS_PY, E_PY, p=0.2, logvar=True, seed=SEED_PY)
    ens.verbose = False
    return ens


def test_members_are_the_single_models_before_training():
    import pinn_amd
    ens = _ensemble()
    torch.manual_seed(5)
    for m in range(E_PY):
        dnn = pinn_amd.DNN(0.2, True, LAYERS_PY, seed=SEED_PY + m, kernels="general")
        mem = ens.member(m)
        assert same_bytes(mem.flat_params().cpu(), dnn.flat_params().cpu()), m
        assert same_bytes(ens._flat[m].cpu(), dnn.flat_params().cpu()), m
        assert mem.seed == dnn.seed and mem.kernels == "general" and mem.layer_sizes == LAYERS_PY
        a, b = mem.dropout_struct(3), dnn.dropout_struct(3)
        assert (a.seed, a.stream, list(a.p)) == (b.seed, b.stream, list(b.p))
    assert not same_bytes(ens._flat[0].cpu(), ens._flat[1].cpu())


def test_fit_is_train_dnn_of_every_member():
    """Seeds, dropout-stream positions and the schedule of the Python layer: five steps, then three more in a second call (a fresh
    optimizer, the stream continuing), against train_dnn of the single models."""
    models, ds = _single_models(N_PY)
    ens = _ensemble()
    for steps in (5, 3):
        ens.fit(ds[0], ds[1], steps)
        for m, mod in enumerate(models):
            mod.train_dnn(steps)
            assert same_bytes(ens._flat[m].cpu(), mod.dnn.flat_params().cpu()), (steps, m)
            assert same_bytes(ens._adam_m[m].cpu(), mod._adam_m.cpu()) and same_bytes(ens._adam_v[m].cpu(), mod._adam_v.cpu()), (steps, m)
            assert ens.last_loss[m] == mod.last_loss, (steps, m)          # the same doubles through the same expression
            assert ens._step_counter == mod._step_counter
    assert ens.losses.shape == (4, E_PY) and ens.loss_epochs == [0, 4, 0, 2]
    # from_models takes the trained models back; state_dict round-trips through a weights_only load
    back = type(ens).from_models(models)
    assert same_bytes(back._flat.cpu(), ens._flat.cpu()) and back.seed == SEED_PY and back.layers == LAYERS_PY


def test_state_dict_round_trip(tmp_path):
    ens = _ensemble()
    x, y = _rows(N_PY)
    ens.fit(x, y, 2)
    path = str(tmp_path / "ens.pt")
    torch.save(ens.state_dict(), path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    torch.manual_seed(99)
    other = type(ens)(LAYERS_PY, E_PY, p=0.5, logvar=True, seed=0)
    other.verbose = False
    other.load_state_dict(sd)
    assert same_bytes(other._flat.cpu(), ens._flat.cpu()) and (other.p, other.seed, other._step_counter) == (ens.p, ens.seed, ens._step_counter)
    ens.fit(x, y, 1); other.fit(x, y, 1)
    assert same_bytes(other._flat.cpu(), ens._flat.cpu())
    with pytest.raises(ValueError):
        type(ens)(LAYERS_PY, E_PY + 1, p=0.2).load_state_dict(sd)


@pytest.fixture(scope="module")
def trained():
    """512 synthetic rows + two fault segments, [8, 32, 32, 1]: an MC-dropout model and an ensemble of 4, 300 steps each."""
    import pinn_amd
    from pinn_amd import synth
    layers = [8, 32, 32, 1]
    ds = synth.make_dataset(512, (96, 64), seed=3)
    torch.manual_seed(1)
    model = pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=True, seed=1, kernels="general")
    model.verbose = False
    model.train_dnn(300)
    ens = pinn_amd.DeepEnsemble(layers, 4, p=0.2, seed=100)
    ens.verbose = False
    ens.fit(ds[0], ds[1], 300)
    return model, ens, ds


def test_ensemble_trains_and_members_differ(trained):
    _, ens, ds = trained
    assert ens.losses.shape == (2, 4) and ens.loss_epochs == [0, 299]
    assert np.all(ens.losses[-1] < ens.losses[0]), ens.losses
    u, lv = ens.forward(ds[2])
    assert u.shape == (4, ds[2].shape[0]) and lv.shape == u.shape and u.is_cuda
    for a in range(4):
        for b in range(a + 1, 4):
            assert not torch.equal(u[a], u[b]) and not torch.equal(lv[a], lv[b])
    pm, au, eu = ens.predict(ds[2])
    assert pm.dtype == np.float32 and pm.shape == (ds[2].shape[0],) and au.shape == pm.shape and eu.shape == pm.shape
    assert np.all(eu > 0) and np.all(au > 0) and np.all(np.isfinite(pm))
    for rule in ("mc", "mixture"):
        want = ens.combine(u, lv, rule=rule)
        got = ens.predict(ds[2], rule=rule, device_output=True)
        assert all(g.is_cuda and torch.equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(ens.predict(ds[2], rule="mc")[0], ens.predict(ds[2], rule="mixture")[0])
    assert np.all(ens.predict(ds[2], rule="mixture")[1] >= au)
    with pytest.raises(ValueError):
        ens.predict(ds[2], rule="median")


def test_results_array_with_an_ensemble(trained):
    import pinn_amd
    model, ens, ds = trained
    model._mc_calls = 0
    plain = pinn_amd.create_comprehensive_results_array_v2(model, ds, mc_times=8)
    model._mc_calls = 0
    none = pinn_amd.create_comprehensive_results_array_v2(model, ds, mc_times=8, ensemble=None)
    assert plain.dtype == np.float64 and plain.tobytes() == none.tobytes()
    arr = pinn_amd.create_comprehensive_results_array_v2(model, ds, mc_times=8, ensemble=ens)
    assert arr.shape == plain.shape == (ds[2].shape[0], 22)
    other = [c for c in range(22) if c not in (9, 10, 11, 12)]
    assert arr[:, other].tobytes() == plain[:, other].tobytes()
    for c in (9, 10, 11, 12):
        assert not np.array_equal(arr[:, c], plain[:, c]), c
    assert np.array_equal(arr[:, 12], arr[:, 8] - arr[:, 9])          # res follows the ensemble's prediction
    assert np.all(arr[:, 11] > 0)
    dev_arr = pinn_amd.create_comprehensive_results_array_v2(model, ds, ensemble=ens, device_output=True)
    assert dev_arr.is_cuda and dev_arr.cpu().numpy().tobytes() == arr.tobytes()
