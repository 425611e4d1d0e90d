"""Time the general (any layers list) exact-fp32 kernels against torch eager fp32 and, for the reference net, the fused fp32 kernels.

Per layers list: one train_dnn step (forward + aleatoric_loss + backward + Adam, full batch) at 1.1e4 and 1e6 rows, and
get_MC_samples at T = 2000 on 1.1e4 rows.  Three ways each:
  general : PhysicsInformedNN(..., kernels="general")
  eager   : a plain torch.nn restatement of the reference's module tree (Linear / Tanh / Dropout, 01:389-438) with autograd and
            torch.optim.Adam, fp32 on the same GPU, the same rows
  fused   : precision="fp32" on the fused kernels ([8, 256, 256, 256, 1] only)
Device events around the timed window after warm-up; the median of the repeats.  One JSON line per case.

    python tools/time_general.py [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LISTS = [[8, 32, 32, 32, 1], [8, 100, 100, 1], [8, 64, 200, 48, 1], [8, 256, 256, 256, 1]]


class EagerDNN(torch.nn.Module):
    """The reference's DNN (01:389-438) as plain torch modules."""

    def __init__(self, p, layers):
        super().__init__()
        mods = []
        for i in range(len(layers) - 2):
            mods += [torch.nn.Linear(layers[i], layers[i + 1]), torch.nn.Tanh(), torch.nn.Dropout(p)]
        self.layers = torch.nn.Sequential(*mods)
        H = layers[-2]
        self.predict = torch.nn.Linear(H, layers[-1])
        self.var_layers = torch.nn.Sequential(torch.nn.Linear(H, H // 2), torch.nn.Tanh(), torch.nn.Dropout(p),
                                              torch.nn.Linear(H // 2, H // 4), torch.nn.Tanh(), torch.nn.Linear(H // 4, layers[-1]))

    def forward(self, x):
        h = self.layers(x)
        return self.predict(h), torch.log(torch.nn.functional.softplus(self.var_layers(h)) + 1e-6)


def _eager_loss(gt, u, logvar):
    prec = torch.exp(-logvar)
    return torch.mean(0.5 * prec * (gt - u) ** 2 + 0.5 * logvar) + 0.01 * torch.mean(torch.abs(logvar))


def timed(fn, warm, reps, inner=1):
    """median ms per call of fn over `reps` event-bracketed windows of `inner` calls, after `warm` calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repeats")
    args = ap.parse_args()
    import pinn_amd
    from pinn_amd import synth
    dev = torch.device("cuda", 0)
    reps = 3 if args.quick else 7
    for layers in LISTS:
        for n in (11000, 1000000):
            ds = synth.make_dataset(n, (), seed=0)
            x, y = ds[0].to(dev), ds[1].to(dev)
            res = {"layers": layers, "rows": n, "what": "train_step"}
            ways = [("general", dict(kernels="general"))]
            if layers == [8, 256, 256, 256, 1]:
                ways.append(("fused_fp32", dict(precision="fp32")))
            for name, kw in ways:
                torch.manual_seed(0)
                m = pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=True, **kw)
                m.verbose = False
                m.dnn.train()
                step = [0]

                def one():
                    step[0] += 1
                    m.train_step_grads(m.x.detach(), m.u.reshape(-1), 0, n, adam=(0.01, step[0]))
                inner = 20 if n < 100000 else 3
                res[name + "_ms"] = round(timed(one, 3, reps, inner), 4)
                del m
            torch.manual_seed(0)
            e = EagerDNN(0.2, layers).to(dev).train()
            opt = torch.optim.Adam(e.parameters(), lr=0.01)

            def eager():
                opt.zero_grad()
                u, lv = e(x)
                _eager_loss(y, u, lv).backward()
                opt.step()
            res["eager_fp32_ms"] = round(timed(eager, 3, reps, 20 if n < 100000 else 3), 4)
            print(json.dumps(res), flush=True)
        # get_MC_samples: T = 2000 on 1.1e4 rows
        n, T = 11000, 2000
        ds = synth.make_dataset(n, (), seed=0)
        x = ds[0].to(dev)
        res = {"layers": layers, "rows": n, "what": "mc_T2000"}
        ways = [("general", dict(kernels="general"))]
        if layers == [8, 256, 256, 256, 1]:
            ways.append(("fused_fp32", dict(precision="fp32")))
        for name, kw in ways:
            torch.manual_seed(0)
            m = pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.4, logvar=True, **kw)
            m.verbose = False
            res[name + "_ms"] = round(timed(lambda: pinn_amd.get_MC_samples(m, ds[2], ds[4], mc_times=T, dropout=0.4), 1, 3), 3)
            del m
        torch.manual_seed(0)
        e = EagerDNN(0.4, layers).to(dev).train()

        def eager_mc():
            # the reference's loop: T stochastic passes of the whole batch, then the moments (01:1459-1486)
            with torch.no_grad():
                us, lvs = [], []
                for _ in range(T):
                    u, lv = e(x)
                    us.append(u)
                    lvs.append(lv)
                us, lvs = torch.stack(us), torch.stack(lvs)
                return us.var(0, unbiased=False).sqrt(), torch.exp(lvs.mean(0)).sqrt()
        res["eager_fp32_ms"] = round(timed(eager_mc, 1, 3), 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    t0 = time.time()
    main()
    print("# %.0f s" % (time.time() - t0), file=sys.stderr)
