"""Time the physics residuals under torch autograd (csrc/pinn_residuals.hip).

Per row count (1.1e4, 1e6, 1e7; --quick: fewer repeats):
  fwd_cols        : pinn_residuals(RES_ALL, per-row columns), the forward the backward mirrors
  bwd             : pinn_residuals_backward(RES_ALL, upstream on the four f columns) -> parameter gradients only
  bwd_gx_gu       : the same call also writing d/dx [N, 8] and d/du [N]
  euler_fwd / euler_bwd : pinn_net_f_t / pinn_net_f_t_backward (upstream on f_T, all three outputs' gradients)
  stage_<mode>    : forward + backward of the stage loss mean(f_V^2) + mean(f_T^2) + mean(f_H^2) + mean(f_O^2) through
                    PhysicsInformedNN(physics_autograd=mode), eval mode; "full" also through the DNN ([8, 128 x 3, 1], f32x6)
  stage_eager_<mode> : torch eager fp32 autograd of the same expressions (the oracle's ops) on the device, the DNN output from
                    the same net as torch modules (tools/time_general.py's EagerDNN; "lambdas": under no_grad, "full": differentiable)
Device events around windows of calls after warm-up; the median of the windows; GB/s = the bytes a call must move / time.
One JSON line per row count.

    python tools/time_physics_autograd.py [--quick]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import pinn_amd  # noqa: E402
from time_general import EagerDNN  # noqa: E402
from pinn_amd import _lib, synth  # noqa: E402


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn, inner, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return statistics.median(ts)


def eager_stage_loss(x, u, lam, mn, sc, y_min, y_scale, p_h2o):
    """mean(f_V^2) + mean(f_T^2) + mean(f_H^2) + mean(f_O^2), the oracle's expressions as torch eager fp32 ops."""
    real = (x - mn) / sc
    i = real[:, 0:1] / 270 + 1e-5
    Tk = real[:, 5:6] + 273.15
    P_H2, P_air = real[:, 3:4] / 101 + 1, real[:, 4:5] / 101 + 1
    Tkp = Tk ** 1.334
    pp_H2 = 0.5 * (P_H2 / torch.exp(1.653 * i / Tkp) - p_h2o)
    pp_O2 = P_air / torch.exp(4.192 * i / Tkp) - p_h2o
    b = 8.314 * Tk / 96485
    V = (220170 / 192970 - ((8.314 * Tk) * torch.log(p_h2o / (pp_H2 * pp_O2 ** 0.5))) / 192970 - b * torch.log(i / lam[1]) - i * lam[0]
         + 0.5 * b * torch.log(1 - i / lam[2]))
    fV = V - ((u - y_min) / y_scale) / 5
    i6 = real[:, 0:1] / 270 + 1e-6
    fT = real[:, 5:6] - (lam[4] * (i6 * 270) + lam[6] * (real[:, 1:2] + 1e-6) + 0.5 * real[:, 2:3] + lam[8])
    It = i * 270
    QH = torch.clamp(It / 192970 * 5 * 22.4 * 60, min=1e-8)
    tH = torch.where(It <= lam[11], lam[9] + lam[10] * (It / 100), lam[9] + lam[10] * (lam[11] / 100))
    fH = (real[:, 6:7] + 1e-6) / QH - tH
    QO = torch.clamp(It * 5 / 385940 * 22.4 * 60, min=1e-8)
    thr = torch.abs(lam[15])
    tO = torch.clamp(torch.where(It <= thr, lam[13] + lam[14] * (It / 100), lam[13] + lam[14] * (thr / 100)), 1.05, 15.0)
    aO = (real[:, 7:8] + 1e-6) * 0.21 / QO
    fO = aO - tO + torch.clamp(1 - aO, min=0.0) * 10
    return (fV ** 2).mean() + (fT ** 2).mean() + (fH ** 2).mean() + (fO ** 2).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repeats")
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    reps = 3 if args.quick else 7
    for n in (11000, 1000000, 10000000):
        inner = 20 if n < 100000 else (5 if n < 5000000 else 2)
        ds = synth.make_dataset(min(n, 200000), (), seed=0)
        rep = (n + ds[0].shape[0] - 1) // ds[0].shape[0]
        xs = ds[0].repeat(rep, 1)[:n].contiguous()
        x = xs.to(dev)
        u = (torch.rand(n, generator=torch.Generator().manual_seed(1)) * 1.6 - 0.8).to(dev)
        torch.manual_seed(0)
        m = pinn_amd.PhysicsInformedNN(xs, ds[1].repeat(rep, 1)[:n], [8, 128, 128, 128, 1], ds[4], ds[5], p=0.2, logvar=True,
                                       autograd=True, physics_autograd="lambdas")
        m.verbose = False
        m.dnn.eval()
        aff = m._affine(ds[4])
        lam = m._lambdas()
        work = m._res_work
        cols = torch.empty(_lib.NCOLS, n, device=dev)
        g = torch.randn(_lib.NCOLS, n, device=dev)
        gmask = sum(1 << _lib.C[c] for c in ("FV", "FT", "FH", "FO"))
        gl = torch.empty(17, device=dev)
        gu = torch.empty(n, device=dev)
        gx = torch.empty(n, 8, device=dev)
        res = {"rows": n}

        def fwd():
            _lib.check(lib.pinn_residuals(_p(x), _p(u), None, ctypes.byref(aff), _p(lam), _lib.RES_ALL, n, _p(cols), n, None, None, 0, _s()), "fwd")

        def bwd(with_out):
            _lib.check(lib.pinn_residuals_backward(_p(x), _p(u), ctypes.byref(aff), _p(lam), _lib.RES_ALL, n, _p(g), n, gmask, _p(gl),
                                                   _p(gu) if with_out else None, _p(gx) if with_out else None, _p(work), work.numel(), _s()),
                       "bwd")
        t = res["fwd_cols_ms"] = timed(fwd, inner, reps)
        res["fwd_cols_GBps"] = n * (32 + 4 + 4 * _lib.NCOLS) / t / 1e6
        t = res["bwd_ms"] = timed(lambda: bwd(False), inner, reps)
        res["bwd_GBps"] = n * (32 + 4 + 16) / t / 1e6
        t = res["bwd_gx_gu_ms"] = timed(lambda: bwd(True), inner, reps)
        res["bwd_gx_gu_GBps"] = n * (32 + 4 + 16 + 32 + 4) / t / 1e6
        res["bwd_over_fwd"] = res["bwd_gx_gu_ms"] / res["fwd_cols_ms"]
        out = torch.empty(3, n, device=dev)

        def efwd():
            _lib.check(lib.pinn_net_f_t(_p(x), _p(u), None, None, ctypes.byref(aff), _p(lam), n, _p(out[0]), _p(out[1]), _p(out[2]), _s()), "efwd")

        def ebwd():
            _lib.check(lib.pinn_net_f_t_backward(_p(x), _p(u), None, None, ctypes.byref(aff), _p(lam), n, _p(g[0]), None, None, _p(gl), _p(gu),
                                                 _p(gx), None, None, _p(work), work.numel(), _s()), "ebwd")
        res["euler_fwd_ms"] = timed(efwd, inner, reps)
        res["euler_bwd_ms"] = timed(ebwd, inner, reps)

        def stage():
            loss = sum(torch.mean(fn(m.X, ds[4])[0] ** 2) for fn in (m.net_f_V, m.net_f_T_simple, m.net_f_H, m.net_f_O))
            loss.backward()
        for mode in ("lambdas", "full"):
            m.physics_autograd = mode
            res["stage_%s_ms" % mode] = timed(stage, max(1, inner // 2), reps)
        m.physics_autograd = False
        net = EagerDNN(0.2, [8, 128, 128, 128, 1]).to(dev).eval()
        mn = torch.tensor(ds[4].min_, dtype=torch.float32, device=dev)
        sc = torch.tensor(ds[4].scale_, dtype=torch.float32, device=dev)
        y_min, y_scale = float(ds[5].min_[0]), float(ds[5].scale_[0])
        p_h2o = float(10 ** (-2.1794 + 0.02953 * 55 - 9.1837e-5 * 55 ** 2 + 1.4454e-7 * 55 ** 3))
        lams = [lam[k:k + 1].clone().requires_grad_(True) for k in range(17)]

        def eager(full):
            with torch.set_grad_enabled(full):
                u_e = net(x)[0]
            eager_stage_loss(x, u_e, lams, mn, sc, y_min, y_scale, p_h2o).backward()
        for mode in ("lambdas", "full"):
            res["stage_eager_%s_ms" % mode] = timed(lambda: eager(mode == "full"), max(1, inner // 2), reps)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
        del m, x, g, gx, cols
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
