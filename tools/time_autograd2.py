"""Time the DNN's double backward: DNN(autograd="double") under a loss that contains du/dx and dlogvar/dx.

The loss, per net and row count (1.1e4 and 1e6), train mode, parameters and x requiring grad:
    du_dx  = torch.autograd.grad(u.sum(),  x, create_graph=True)[0]
    dlv_dx = torch.autograd.grad(lv.sum(), x, create_graph=True)[0]
    loss   = aleatoric_loss(y, u, lv) + w * mean(du_dx[:, 0] ** 2) + w * mean(dlv_dx ** 2);  loss.backward()
  module     : the forward, both input gradients and loss.backward() through the module (one forward, three
               pinn_gnet_backward calls, two pinn_gnet_backward2 calls)
  backward2  : the pinn_gnet_backward2 call alone, all four outputs (same rows, masks and upstream gradients)
  backward   : the pinn_gnet_backward call alone at the same shape
  eager      : the torch eager fp32 module tree (tools/time_general.py's EagerDNN) doing the same double backward
Nets: [8,32,32,32,1], [8,100,100,1], [8,64,200,48,1] (kernels="general") and [8,256,256,256,1] (kernels="auto", f32x6).
Device events around windows of calls after warm-up; the median of the windows.  One JSON line per case.

    python tools/time_autograd2.py [--quick]
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
from time_general import EagerDNN, _eager_loss, timed  # noqa: E402

NETS = [([8, 32, 32, 32, 1], "general"), ([8, 100, 100, 1], "general"), ([8, 64, 200, 48, 1], "general"), ([8, 256, 256, 256, 1], "auto")]
W = 0.5


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _step(net, loss_fn, xg, y, params):
    for p in params:
        p.grad = None
    xg.grad = None
    u, lv = net(xg)
    du_dx, = torch.autograd.grad(u.sum(), xg, create_graph=True)
    dlv_dx, = torch.autograd.grad(lv.sum(), xg, create_graph=True)
    (loss_fn(y, u, lv) + W * torch.mean(du_dx[:, 0] ** 2) + W * torch.mean(dlv_dx ** 2)).backward()


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
            inner = 10 if n < 100000 else 2
            ds = synth.make_dataset(n, (), seed=0)
            x = ds[0].to(dev).contiguous()
            y = ds[1].to(dev).reshape(-1, 1).contiguous()
            gen = torch.Generator().manual_seed(0)
            gu = torch.randn(n, generator=gen).to(dev)
            glv = torch.randn(n, generator=gen).to(dev)
            vx = torch.randn(n, 8, generator=gen).to(dev)
            res = {"layers": layers, "rows": n, "kernels": kernels}
            torch.manual_seed(0)
            kw = dict(kernels="general") if kernels == "general" else dict(precision="f32x6")
            m = pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=True, autograd="double", **kw)
            m.verbose = False
            dnn = m.dnn
            dnn.train()
            xg = x.clone().requires_grad_(True)
            params = list(dnn.parameters())
            res["module_ms"] = round(timed(lambda: _step(dnn, m.aleatoric_loss, xg, y, params), 3, reps, inner), 4)

            drop = dnn.dropout_struct(0x80000000 + 1, 0)
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            grads = torch.empty_like(dnn._flat)
            gx = torch.empty(n, 8, device=dev)
            ggu = torch.empty(n, device=dev)
            gglv = torch.empty(n, device=dev)
            gnet2, work2 = dnn._backward2_net(n)

            def bwd2():
                _lib.check(lib.pinn_gnet_backward2(ctypes.byref(gnet2), _p(dnn._flat), _p(x), n, ctypes.byref(drop), _p(gu), _p(glv), _p(vx),
                                                   _p(grads), _p(gx), _p(ggu), _p(gglv), _p(work2), work2.numel(), st), "pinn_gnet_backward2")
            res["backward2_ms"] = round(timed(bwd2, 3, reps, inner), 4)

            gnet, work = dnn._backward_net(n)

            def bwd():
                _lib.check(lib.pinn_gnet_backward(ctypes.byref(gnet), _p(dnn._flat), _p(x), n, ctypes.byref(drop), _p(gu), _p(glv),
                                                  _p(grads), _p(gx), _p(work), work.numel(), st), "pinn_gnet_backward")
            res["backward_ms"] = round(timed(bwd, 3, reps, inner), 4)
            del m, dnn, work, work2, params
            torch.cuda.empty_cache()

            torch.manual_seed(0)
            e = EagerDNN(0.2, layers).to(dev).train()
            ep = list(e.parameters())
            res["eager_fp32_ms"] = round(timed(lambda: _step(e, _eager_loss, xg, y, ep), 3, reps, inner), 4)
            res["backward2_over_backward"] = round(res["backward2_ms"] / res["backward_ms"], 3)
            res["eager_over_module"] = round(res["eager_fp32_ms"] / res["module_ms"], 3)
            del e, ep
            torch.cuda.empty_cache()
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    t0 = time.time()
    main()
    print("# %.0f s" % (time.time() - t0), file=sys.stderr)
