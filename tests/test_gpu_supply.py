"""GPU: the device backend of pinn_amd.supply (csrc/pinn_breakpoint.hip, pinn_bp_fit) against the brute force of
supply_cases.py and against the package's host backend (itself held to the brute force in test_supply_host.py).

Gates, as in the host file: G on the objective (brute force up to 257 rows; above, the host backend's direct SSE and the best of
64 grid values of c); on the well-separated windows host and device theta agree to 1e-9 relative and cov to 1e-7 relative;
integer words equal; bytes equal where the design promises them.  Every comparison prints its worst figure before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

import supply_cases as C
from pinn_amd import identify as I
from pinn_amd import supply as S

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

pytestmark = pytest.mark.gpu

LENGTHS = (4, 5, 255, 256, 257, 511, 1024, 4096)
INTS = slice(10, 15)                                                    # kind, k, n_used, distinct currents, status


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_fit(table, start, length, **kw):
    return S.fit_breakpoints(table if torch.is_tensor(table) else dev(table), start, length, backend="device", **kw)


def host_fit(table, start, length, **kw):
    return S.fit_breakpoints(table, start, length, backend="numpy", **kw)


def referee_sse(rows, host_theta):
    used = int(np.isfinite(rows).all(axis=1).sum())
    return C.brute_sse(rows) if used <= 257 else min(C.direct_sse(rows, host_theta), C.grid_sse(rows))


def rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(a - b) / np.abs(b)
    return float(np.nanmax(np.where(a == b, 0.0, r)))


@pytest.mark.parametrize("quantised", (False, True))
@pytest.mark.parametrize("m", LENGTHS)
def test_gate_G_and_host_parity(m, quantised):
    if m >= 255:
        rows, _, _ = C.separated(m, quantised)
    else:                                                               # 4 and 5 rows: no separation to speak of, gate G and the integers only
        rows = C.draw(np.random.default_rng(m + int(quantised)), m, quantised, 0.02, (1.5, 0.8, 150.0), lo=100.0, hi=200.0)
    rng = np.random.default_rng(7 * m + int(quantised))
    holes = rows.copy()                                                 # 5 % missing rows (at least one from 20 rows on)
    holes[rng.permutation(m)[:(m + 19) // 20 if m >= 20 else 0], rng.integers(0, 2)] = np.nan
    # packed in a wider array (columns 2 and 0), and the same rows scattered over a larger table behind a gather list
    wide = np.full((m, 3), -1.0)
    wide[:, 2], wide[:, 0] = rows[:, 0], rows[:, 1]
    perm = rng.permutation(2 * m + 3)[:m]
    scattered = np.full((2 * m + 3, 2), np.nan)
    scattered[perm] = rows
    d = device_fit(rows, [0], [m])
    h = host_fit(rows, [0], [m])
    sse, bound = C.gate_G(rows, d.theta[0], referee_sse(rows, h.theta[0]))
    print("m=%d quantised=%s: device sse %.12g, bound %.12g; kind %d k %d; host kind %d k %d" % (m, quantised, sse, bound, d.kind[0], d.k[0], h.kind[0], h.k[0]))
    assert sse <= bound and d.status[0] == h.status[0] and d.n_used[0] == m
    assert device_fit(wide, [0], [m], cols=(2, 0)).raw.tobytes() == d.raw.tobytes()
    assert device_fit(scattered, [0], [m], row_index=perm).raw.tobytes() == d.raw.tobytes()
    if m >= 255:
        r_theta, r_cov = rel(d.theta[0], h.theta[0]), rel(d.cov[0], h.cov[0])
        r_rest = rel(d.raw[0, 15:21], h.raw[0, 15:21])
        print("    against the host: theta %.3g (gate 1e-9), cov %.3g (gate 1e-7), sse_line .. x_max %.3g" % (r_theta, r_cov, r_rest))
        assert np.array_equal(d.raw[0, INTS], h.raw[0, INTS])
        assert r_theta <= 1e-9 and r_cov <= 1e-7
        assert np.array_equal(d.c_interval, h.c_interval) and np.array_equal(d.x_range, h.x_range)
    dh, hh = device_fit(holes, [0], [m]), host_fit(holes, [0], [m])
    assert dh.n_used[0] == hh.n_used[0] == int(np.isfinite(holes).all(axis=1).sum()) and dh.status[0] == hh.status[0]
    if dh.status[0] in (0, 5):
        sse, bound = C.gate_G(holes, dh.theta[0], referee_sse(holes, hh.theta[0]))
        print("    with %d rows missing: device sse %.12g, bound %.12g" % (m - dh.n_used[0], sse, bound))
        assert sse <= bound


_stride = {}


def stride_case():
    """700 windows of 64 rows every 16: more windows than workgroups."""
    if not _stride:
        rng = np.random.default_rng(700)
        table = dev(C.draw(rng, 699 * 16 + 64, True, 0.05))
        start, length = I.sliding_windows(table.shape[0], 64, 16)
        _stride["case"] = (table, start, length, device_fit(table, start, length))
    return _stride["case"]


def test_grid_stride_windows_equal_windows_alone():
    table, start, length, f = stride_case()
    assert len(start) == 700 and np.all(f.n_used == 64)
    for w in range(700):
        alone = device_fit(table, [start[w]], [64])
        assert alone.raw[0].tobytes() == f.raw[w].tobytes(), w
    h = host_fit(table.cpu().numpy(), start, length)
    assert np.array_equal(f.status, h.status)


def test_kinds_and_statuses_match_the_host():
    table, names, d = C.check_kinds_and_statuses(device_fit)
    _, _, h = C.check_kinds_and_statuses(host_fit)
    assert np.array_equal(d.raw[:, INTS], h.raw[:, INTS]), (d.raw[:, INTS], h.raw[:, INTS])
    for i, n in enumerate(names):
        assert np.allclose(d.theta[i], h.theta[i], rtol=1e-9, atol=0, equal_nan=True), (n, d.theta[i], h.theta[i])


def test_determinism():
    table, start, length, f = stride_case()
    assert device_fit(table, start, length).raw.tobytes() == f.raw.tobytes()
    rows, _, _ = C.separated(4096, True)
    a, b = device_fit(rows, [0, 0, 1000], [4096, 300, 2048]), device_fit(rows, [0, 0, 1000], [4096, 300, 2048])
    assert a.raw.tobytes() == b.raw.tobytes()
    # a window's bytes depend neither on the other windows of the call (which size the LDS) nor on the gather list
    assert device_fit(rows, [0], [300]).raw[0].tobytes() == a.raw[1].tobytes()
    assert device_fit(rows, [0], [2048], row_index=np.arange(1000, 3048)).raw[0].tobytes() == a.raw[2].tobytes()


@pytest.mark.parametrize("gas", S.GASES)
def test_flow_table_from_a_model(gas):
    import pinn_amd
    from pinn_amd import synth
    ds = synth.make_dataset(512, (), seed=0)
    torch.manual_seed(0)
    m = pinn_amd.PhysicsInformedNN(ds[0], ds[1], [8, 128, 128, 1], ds[4], ds[5], p=0.2, logvar=True, seed=11)
    m.verbose = False
    t = pinn_amd.flow_table(m, ds[0], gas, ds[4])
    assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (512, 2)
    mn, sc = np.asarray(ds[4].min_, dtype=np.float64), np.asarray(ds[4].scale_, dtype=np.float64)
    phys = (ds[0].numpy().astype(np.float64) - mn) / sc                 # the de-normalised rows
    want = S.flow_table(None, phys, gas)
    err = np.max(np.abs(t.cpu().numpy() - want) / np.abs(want), axis=0)
    print("%s table against float64: worst relative difference per column %s (gate 4 * 2^-23)" % (gas, err))
    assert np.all(err <= 4 * 2.0 ** -23)
    f = pinn_amd.fit_breakpoints(t, [0], [512])                         # a table fits on the device as it stands
    assert f.backend == "device" and f.n_used[0] == 512


def test_tracker_equals_fit_breakpoints_on_the_device():
    C.check_tracker("device", dev)


def test_example_segments_on_the_device():
    C.check_example("device", dev)
