"""Time the deep-ensemble calls on the GPU: E members in the launches of one against the loop of E single calls.

Per net ([8,256,256,256,1] and [8,64,64,1]), row count (1349, 4200, 1.1e4, 1e5) and E (2, 4, 8, 16), per training step:
  batched   one pinn_gens_train_step over [E, P]
  loop      E pinn_gnet_train_step calls on the members' slices (the parent API: what an ensemble cost before)
  fused     the reference net only: E steps of the default fused path (PhysicsInformedNN.train_step_grads with Adam, "f32x6")
and per predict: pinn_gens_forward + pinn_gens_combine against E pinn_gnet_forward calls and the combine from torch operations.

Method: every variant of a configuration is warmed up (3 calls), then timed `--reps` times in alternation (batched, loop, fused,
batched, ...), each window K consecutive calls between two device events with K chosen from the warm-up so that a window lasts
about `--window-ms`; the median per call goes into one JSON line per configuration, with all windows, and a markdown table of the
ratios closes the run.  The clock and power state (rocm-smi, read only) is printed before and after."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import _common as hh  # noqa: E402
from _common import _lib, lib  # noqa: E402

NETS = [[8, 256, 256, 256, 1], [8, 64, 64, 1]]
ROWS = [1349, 4200, 11000, 100000]
MEMBERS = [2, 4, 8, 16]


def smi():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--showperflevel"], capture_output=True, text=True, timeout=30).stdout
    except Exception as e:      # noqa
        return "rocm-smi failed: %r" % (e,)
    keep = [l.strip() for l in r.splitlines() if any(k in l for k in ("sclk", "mclk", "Power", "Performance Level"))]
    return " | ".join(keep[:8])


def params(layers, e, seed=1):
    from pinn_amd import layout
    offs, total = layout.general_offsets(layers)
    g = torch.Generator().manual_seed(seed)
    f = torch.zeros(e, total)
    for _, shape, off in offs:
        k = int(np.prod(shape))
        f[:, off:off + k] = (torch.rand(e, k, generator=g) * 2 - 1) / (shape[-1] if len(shape) > 1 else max(1, k)) ** 0.5
    return f.to(hh.dev())


def window(fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def measure(variants, reps, window_ms):
    """variants: {name: fn}.  -> {name: (median ms per call, [ms per call of every window], calls per window)}"""
    ks = {}
    for name, fn in variants.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        est = max(window(fn, 1), 1e-3)
        ks[name] = int(max(2, min(400, round(window_ms / est))))
    got = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            got[name].append(window(fn, ks[name]))
    return {name: (float(np.median(v)), [round(t, 4) for t in v], ks[name]) for name, v in got.items()}


def config(layers, n, e, reps, window_ms):
    net = ctypes.byref(_lib.GNet(layers))
    dev = hh.dev()
    g = torch.Generator().manual_seed(n)
    x = (torch.rand(n, 8, generator=g) * 2 - 1).to(dev)
    y = (torch.rand(n, generator=g) * 2 - 1).to(dev)
    fp = params(layers, e)
    state = [torch.zeros_like(fp) for _ in range(3)]      # grads, m, v
    loss = torch.zeros(e, 4, dtype=torch.float64, device=dev)
    wb = lib.pinn_gens_workspace_bytes(net, e, n)
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    w1 = torch.empty(lib.pinn_gnet_workspace_bytes(net, n, 0), dtype=torch.uint8, device=dev)
    u, lv = torch.empty(e, n, device=dev), torch.empty(e, n, device=dev)
    out = torch.empty(3, n, device=dev)
    drop = hh.dropout_struct(_lib.DROP_PHILOX, [0.2] * (len(layers) - 1), seed=5, stream_id=1)
    drops = [hh.dropout_struct(_lib.DROP_PHILOX, [0.2] * (len(layers) - 1), seed=5 + m, stream_id=1) for m in range(e)]
    st, ptr = hh.stream, hh.ptr
    # the timed steps keep lr at 0: the parameters stay where they are, the work is that of any step
    lr = 0.0

    def batched():
        _lib.check(lib.pinn_gens_train_step(net, e, ptr(fp), ptr(x), ptr(y), n, n, ctypes.byref(drop), ptr(state[0]), ptr(loss), ptr(work), wb,
                                            ptr(state[1]), ptr(state[2]), lr, 1, st()), "pinn_gens_train_step")

    def loop():
        for m in range(e):
            _lib.check(lib.pinn_gnet_train_step(net, ptr(fp[m]), ptr(x), ptr(y), n, n, ctypes.byref(drops[m]), ptr(state[0][m]), ptr(loss[m]),
                                                ptr(w1), w1.numel(), ptr(state[1][m]), ptr(state[2][m]), lr, 1, st()), "pinn_gnet_train_step")

    def predict_batched():
        _lib.check(lib.pinn_gens_forward(net, e, ptr(fp), ptr(x), n, None, ptr(u), ptr(lv), ptr(work), wb, st()), "pinn_gens_forward")
        _lib.check(lib.pinn_gens_combine(ptr(u), ptr(lv), e, n, 0, ptr(out[0]), ptr(out[1]), ptr(out[2]), st()), "pinn_gens_combine")

    def predict_loop():
        for m in range(e):
            _lib.check(lib.pinn_gnet_forward(net, ptr(fp[m]), ptr(x), n, None, ptr(u[m]), ptr(lv[m]), ptr(w1), w1.numel(), st()),
                       "pinn_gnet_forward")
        ud = u.double()
        mean = ud.mean(0)
        out[0] = mean.float()
        out[1] = torch.sqrt(torch.exp(lv.double().mean(0))).float()
        out[2] = torch.sqrt(torch.clamp((ud * ud).mean(0) - mean * mean, min=0.0)).float()

    train = {"batched": batched, "loop": loop}
    if layers == NETS[0]:
        import pinn_amd
        from pinn_amd import synth
        ds = synth.make_dataset(n, (), seed=0)
        model = pinn_amd.PhysicsInformedNN(ds[0], ds[1], layers, ds[4], ds[5], p=0.2, logvar=True, seed=5)
        model.verbose = False
        model.dnn.train()
        xm, ym = model.x.detach(), model.u.reshape(-1)

        def fused():
            for _ in range(e):
                model.train_step_grads(xm, ym, 0, n, adam=(lr, 1))
        train["fused"] = fused
    res = {"layers": layers, "rows": n, "members": e}
    for name, (ms, all_ms, k) in measure(train, reps, window_ms).items():
        res["step_%s_ms" % name] = round(ms, 4)
        res["step_%s_all" % name] = all_ms
        res["step_%s_calls_per_window" % name] = k
    for name, (ms, all_ms, k) in measure({"batched": predict_batched, "loop": predict_loop}, reps, window_ms).items():
        res["predict_%s_ms" % name] = round(ms, 4)
        res["predict_%s_all" % name] = all_ms
    res["step_loop_over_batched"] = round(res["step_loop_ms"] / res["step_batched_ms"], 2)
    if "step_fused_ms" in res:
        res["step_fused_over_batched"] = round(res["step_fused_ms"] / res["step_batched_ms"], 2)
    res["predict_loop_over_batched"] = round(res["predict_loop_ms"] / res["predict_batched_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(str(r) for r in ROWS))
    ap.add_argument("--members", default=",".join(str(e) for e in MEMBERS))
    ap.add_argument("--nets", default="0,1", help="indices into NETS")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_ensemble.py measures on the GPU; none is present")
    print("before:", smi(), flush=True)
    rows = []
    for ni in [int(v) for v in args.nets.split(",")]:
        for n in [int(v) for v in args.rows.split(",")]:
            for e in [int(v) for v in args.members.split(",")]:
                r = config(NETS[ni], n, e, args.reps, args.window_ms)
                print(json.dumps(r), flush=True)
                rows.append(r)
                torch.cuda.empty_cache()
    print("after:", smi(), flush=True)
    print("\n| net | rows | E | batched step ms | loop ms | loop / batched | fused x E ms | fused / batched | predict batched ms | predict loop ms | loop / batched |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %d | %.3f | %.3f | %.2f | %s | %s | %.3f | %.3f | %.2f |" % (
            r["layers"], r["rows"], r["members"], r["step_batched_ms"], r["step_loop_ms"], r["step_loop_over_batched"],
            "%.3f" % r["step_fused_ms"] if "step_fused_ms" in r else "-",
            "%.2f" % r["step_fused_over_batched"] if "step_fused_over_batched" in r else "-",
            r["predict_batched_ms"], r["predict_loop_ms"], r["predict_loop_over_batched"]))


if __name__ == "__main__":
    main()
