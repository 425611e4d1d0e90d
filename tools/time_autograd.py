"""Time the DNN under torch autograd: forward + backward of (g_u * u + g_lv * logvar).sum() with DNN(autograd=True).

Per net and row count (1.1e4 and 1e6), train mode, parameters and x requiring grad:
  autograd     : the module call + .backward() (pinn_gnet_forward / pinn_mlp_forward, then pinn_gnet_backward)
  backward     : the pinn_gnet_backward call alone (same rows, masks and upstream gradients)
  train_grads  : pinn_gnet_train_grads at the same shape (forward + aleatoric_loss + backward, the fused-loss entry point)
  eager        : the torch eager fp32 module tree (tools/time_general.py's EagerDNN) with autograd, the same sum
Nets: [8,32,32,32,1], [8,100,100,1], [8,64,200,48,1] (kernels="general") and [8,256,256,256,1] (kernels="auto", f32x6).
Device events around windows of calls after warm-up; the median of the windows.  One JSON line per case.

    python tools/time_autograd.py [--quick]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from time_general import EagerDNN, timed  # noqa: E402

NETS = [([8, 32, 32, 32, 1], "general"), ([8, 100, 100, 1], "general"), ([8, 64, 200, 48, 1], "general"), ([8, 256, 256, 256, 1], "auto")]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repeats")
    args = ap.parse_args()
    import pinn_amd
    from pinn_amd import _lib, synth
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    reps = 3 if args.quick else 7
    for layers, kernels in NETS:
        for n in (11000, 1000000):
            inner = 20 if n < 100000 else 3
            ds = synth.make_dataset(n, (), seed=0)
            x = ds[0].to(dev).contiguous()
            gen = torch.Generator().manual_seed(0)
            gu = torch.randn(n, 1, generator=gen).to(dev)
            glv = torch.randn(n, 1, generator=gen).to(dev)
            res = {"layers": layers, "rows": n, "kernels": kernels}
            torch.manual_seed(0)
            kw = dict(kernels="general") if kernels == "general" else dict(precision="f32x6")
            m = pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=True, autograd=True, **kw)
            m.verbose = False
            dnn = m.dnn
            dnn.train()
            xg = x.clone().requires_grad_(True)

            def fwd_bwd():
                u, lv = dnn(xg)
                (gu * u + glv * lv).sum().backward()
            res["autograd_ms"] = round(timed(fwd_bwd, 3, reps, inner), 4)

            gnet, work = dnn._backward_net(n)
            grads = torch.empty_like(dnn._flat)
            gx = torch.empty(n, 8, device=dev)
            drop = dnn.dropout_struct(0x80000000 + 1, 0)
            gu1, glv1 = gu.reshape(-1).contiguous(), glv.reshape(-1).contiguous()
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

            def bwd():
                _lib.check(lib.pinn_gnet_backward(ctypes.byref(gnet), _p(dnn._flat), _p(x), n, ctypes.byref(drop), _p(gu1), _p(glv1),
                                                  _p(grads), _p(gx), _p(work), work.numel(), st), "pinn_gnet_backward")
            res["backward_ms"] = round(timed(bwd, 3, reps, inner), 4)

            g = _lib.GNet(layers)
            wb = lib.pinn_gnet_workspace_bytes(ctypes.byref(g), n, 0)
            tw = work if kernels == "general" else torch.empty(wb, dtype=torch.uint8, device=dev)
            y = m.u.reshape(-1).contiguous()
            loss = torch.empty(4, dtype=torch.float64, device=dev)

            def tg():
                _lib.check(lib.pinn_gnet_train_grads(ctypes.byref(g), _p(dnn._flat), _p(x), _p(y), n, n, ctypes.byref(drop), _p(grads),
                                                     _p(loss), _p(tw), tw.numel(), st), "pinn_gnet_train_grads")
            res["train_grads_ms"] = round(timed(tg, 3, reps, inner), 4)
            del m, dnn, work, tw
            torch.cuda.empty_cache()

            torch.manual_seed(0)
            e = EagerDNN(0.2, layers).to(dev).train()

            def eager():
                u, lv = e(xg)
                (gu * u + glv * lv).sum().backward()
            res["eager_fp32_ms"] = round(timed(eager, 3, reps, inner), 4)
            res["backward_over_train_grads"] = round(res["backward_ms"] / res["train_grads_ms"], 3)
            del e
            torch.cuda.empty_cache()
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    t0 = time.time()
    main()
    print("# %.0f s" % (time.time() - t0), file=sys.stderr)
