"""The weight-gradient launches at row counts where a slice walks SEVERAL row tiles, against a float64 oracle: every route of
plan_workspace (one multi-problem launch, side streams, one launch per layer), both tile walks (interleaved, contiguous with a short and
empty slices), the per-layer packed kernels bench.py times, and the wide nets' workgroup re-numbering over the XCDs.  Cases, reference,
band and mutants: tests/wgrad_routes.py; test_wgrad_routes_host.py proves on the CPU that each case reaches what it names and that the
gate used here tells a skipped row, a skipped tile, a tile counted twice and two exchanged gradient blocks from the reference.

test_gpu_fullsize.py and test_gpu_train_phases.py compare the kernels with themselves at these sizes (repeatable, split calls equal, two
shards add up); here they meet a referee.  One device call per case and precision; every figure is printed as error / gate before
anything asserts (run with -s; recorded in profiles/r06/wgrad_routes.txt)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wgrad_routes as W


@pytest.fixture(scope="module")
def lib():
    from pinn_amd import _lib
    return _lib.load()


_DEV = {}


def device(lib, name, prec, H, nh):
    """(flat gradients, loss sums) of one case and precision on the CPU, computed once."""
    key = (name, prec, H, nh)
    if key not in _DEV:
        import hip_helpers as hh
        ref = W.reference(name, H, nh)
        drop = hh.dropout_struct(1, ref.pl, seed=W.SEED, stream_id=W.STREAM, row_offset=W.ROW0) if ref.mode else None
        g, l = hh.train_grads(lib, H, nh, hh.flat_params(ref.P, H, nh).to(hh.dev()), ref.x.to(hh.dev()), ref.y.to(hh.dev()), drop, precision=prec)
        _DEV[key] = (g.cpu(), l.cpu().numpy())
        del g
        torch.cuda.empty_cache()
    return _DEV[key]


def _param(r):
    # serial_x3: 1.3 GB of workspace and the largest float64 reference
    return pytest.param(r, id=W.run_id(r), marks=[pytest.mark.timeout(600)] if r[0] == "serial_x3" else [])


@pytest.mark.parametrize("run", [_param(r) for r in W.RUNS])
def test_wgrad_route_against_float64(lib, run):
    import hip_helpers as hh
    name, prec, H, nh = run
    ref = W.reference(name, H, nh)
    plan = W.plan(prec, H, nh, ref.n)
    g, l = device(lib, name, prec, H, nh)
    tag = W.run_id(run)
    print("%s: %d rows, t16 %d, route %s, %d slices, %s walk, tiles per slice %s" % (tag, ref.n, plan["t16"], plan["route"], plan["slices"],
                                                                                  plan["walk"], sorted(plan["tiles"].items())))
    assert torch.isfinite(g).all() and np.isfinite(l).all(), tag
    rl, rm = ref.loss_ratios(l)
    print("%s %-24s loss %.3f  mse %.3f   (error / 2e-5 relative)" % (tag, "loss sums", rl, rm))
    grads = [t.double().numpy() for t in hh.unflat(g, H, nh)]
    rows = ref.ratios(grads, W.K_OF[prec], W.excepted(run))
    for tensor, r, x, br, bx in rows:
        print("%s %-24s rms %7s  max %7.3f   (error / gate)    rms %7s  max %7.3f   (error / K band, K = %g)" % (
            tag, tensor, "-" if r is None else "%.3f" % r, x, "-" if br is None else "%.3f" % br, bx, W.K_OF[prec]))
    vs = None
    if prec != W.FP32 and any(r[0] == name and r[1] == W.FP32 and r[2] == H for r in W.RUNS):
        g0, l0 = device(lib, name, W.FP32, H, nh)
        vs = float((g - g0).abs().max()) / (2e-5 * float(g0.abs().max()))
        print("%s %-24s %.3f   (max |g - g_fp32| / (2e-5 max |g_fp32|))" % (tag, "vs exact fp32", vs))
    assert rl <= 1.0 and rm <= 1.0, (tag, "loss", rl, rm)
    bad = [(t, r, x) for t, r, x, _, _ in rows if x > 1.0 or (r is not None and r > 1.0)]
    assert not bad, (tag, bad)
    if vs is not None:
        assert vs <= 1.0, (tag, "vs exact fp32", vs)
        np.testing.assert_allclose(l[:3], l0[:3], rtol=2e-6)
