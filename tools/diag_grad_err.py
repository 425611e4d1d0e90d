"""Per-tensor gradient error of every precision family against a float64 autograd, beside torch's own fp32 autograd
(the reference's arithmetic): rms and largest error as multiples of torch's.

usage: diag_grad_err.py H nh N [seed]
       diag_grad_err.py --hidden H [--layers nh] --rows N [--seed S] [--precisions 0,2,3]
       diag_grad_err.py --case ID        one case of tests/wgrad_routes.py (its rows, seed, Philox key and the precisions it runs), with the
                                         route plan_workspace takes and error / K band per tensor, as test_gpu_wgrad_routes.py prints them
Nets wider than 256 run under the split-operand precisions only (--precisions 2)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import pinn_oracle as O
import hip_helpers as hh
from pinn_amd import _lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("pos", nargs="*", type=int, help="H nh N [seed]")
ap.add_argument("--hidden", type=int)
ap.add_argument("--layers", type=int, default=3)
ap.add_argument("--rows", type=int)
ap.add_argument("--seed", type=int, default=17)
ap.add_argument("--precisions", default=None)
ap.add_argument("--case")
ap.add_argument("--dump", help="with --case: write the device's gradient tensors of up to 65 536 elements to this .npz")
a = ap.parse_args()
lib = _lib.load()
rms = lambda e: float(np.sqrt((e ** 2).mean()))

if a.case:
    import wgrad_routes as W
    dump = {}
    for name, prec, H, nh in [r for r in W.RUNS if r[0] == a.case]:
        ref = W.reference(name, H, nh)
        plan = W.plan(prec, H, nh, ref.n)
        drop = hh.dropout_struct(1, ref.pl, seed=W.SEED, stream_id=W.STREAM, row_offset=W.ROW0) if ref.mode else None
        g, l = hh.train_grads(lib, H, nh, hh.flat_params(ref.P, H, nh).to(hh.dev()), ref.x.to(hh.dev()), ref.y.to(hh.dev()), drop, precision=prec)
        print("%s: %d rows, t16 %d, route %s, %d slices, %s walk, tiles per slice %s" % (W.run_id((name, prec, H, nh)), ref.n, plan["t16"], plan["route"],
                                                                                      plan["slices"], plan["walk"], sorted(plan["tiles"].items())))
        print("  loss, mse error / 2e-5 relative: %.3f %.3f" % ref.loss_ratios(l.cpu().numpy()))
        for t, v in zip(ref.names, hh.unflat(g.cpu(), H, nh)):
            if v.numel() <= 65536:
                dump["%s/%s" % (W.run_id((name, prec, H, nh)), t)] = v.numpy()
        for t, r, x, br, bx in ref.ratios([t.double().numpy() for t in hh.unflat(g.cpu(), H, nh)], W.K_OF[prec], W.excepted((name, prec, H, nh))):
            print("  %-24s error / K band (K = %g): rms %7s  max %7.3f      error / gate: rms %7s  max %7.3f" % (
                t, W.K_OF[prec], "-" if br is None else "%.3f" % br, bx, "-" if r is None else "%.3f" % r, x))
    if a.dump:
        np.savez(a.dump, **dump)
    sys.exit(0)

if a.pos:
    H, nh, N = a.pos[:3]
    seed = a.pos[3] if len(a.pos) > 3 else a.seed
else:
    assert a.hidden and a.rows, "give H nh N, or --hidden and --rows, or --case"
    H, nh, N, seed = a.hidden, a.layers, a.rows, a.seed
precs = [int(p) for p in a.precisions.split(",")] if a.precisions else ([0, 2, 3] if H <= 256 else [2])
pl = [0.2] * (nh + 1)
ds = synth.make_dataset(N, (), seed=seed)
x, y = ds[0].contiguous(), ds[1].reshape(-1, 1).contiguous()
P = O.init_params([8] + [H] * nh + [1], seed=seed)
masks = O.philox_masks_for_net(99, 7, 0, N, H, nh, pl)
_, _, g32, _, _ = O.nll_loss_and_grads(P, x, y, pl, masks)
_, _, g64, _, _ = O.nll_loss_and_grads([p.double() for p in P], x.double(), y.double(), pl, masks)
drop = hh.dropout_struct(1, pl, seed=99, stream_id=7, row_offset=0)
res = {}
for prec in precs:
    g, _ = hh.train_grads(lib, H, nh, hh.flat_params(P, H, nh).to(hh.dev()), x.to(hh.dev()), y.reshape(-1).to(hh.dev()), drop, precision=prec)
    res[prec] = hh.unflat(g.cpu(), H, nh)
print("H %d nh %d N %d: error vs float64 as a multiple of torch-fp32's (rms, max), per precision %s; last: torch rms / tensor rms" % (
    H, nh, N, " / ".join(map(str, precs))))
for i, n in enumerate(O.param_names(nh)):
    c = g64[i].numpy().reshape(-1); b = g32[i].double().numpy().reshape(-1)
    line = "%-24s" % n
    for prec in precs:
        v = res[prec][i].double().numpy().reshape(-1)
        line += "  (%5.2f, %5.2f)" % (rms(v - c) / (rms(b - c) + 1e-300), np.abs(v - c).max() / (np.abs(b - c).max() + 1e-300))
    print(line + "   %.1e" % (rms(b - c) / (rms(c) + 1e-300)))
