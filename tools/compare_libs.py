#!/usr/bin/env python
"""Byte identity of the training step's outputs between two builds of the library (same ABI), on seeded inputs:

    python tools/compare_libs.py PARENT.so BRANCH.so [--bench] > profiles/rNN/outputs_parent_vs_branch.txt

Each library runs in a child process of its own (PINN_HIP_LIB) over the same cases; the table has one line per array with its
SHA-256 on either side.  Cases: pinn_mlp_train_grads (gradient vector, loss sums) whole and as split phases (chain, then tail,
then head in calls of their own) over nets x precisions x dropout modes x row counts that between them reach every fused
weight-gradient tiling, the block grid of the wide nets and the three launch routes.  --bench: also
`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs` per precision.  Exit status 1 if any array differs."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PREC = {0: "fp32", 2: "f32x6", 3: "f32x6g6", 1: "bf16"}
NETS = [(128, 3, (0, 2, 3, 1)), (256, 2, (0, 2, 3, 1)), (512, 2, (2, 1))]      # [8,128,128,128,1], [8,256,256,1], [8,512,512,1]
ROWS = (17, 145, 8209, 32913)
SPLIT = (1, 32 | 128, 64 | 256)      # chain; weight gradients + reduction of the tail; of the head


def sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def dump(out):
    sys.path.insert(0, HERE)
    import torch
    import _common as hh
    from _common import _lib, lib
    res = {}
    for H, nh, precs in NETS:
        fp = hh.random_params(H, nh, seed=11)
        for n in ROWS:
            g = torch.Generator().manual_seed(1000 + n)
            x = torch.rand(n, 8, generator=g).to(hh.dev())
            y = torch.rand(n, generator=g).to(hh.dev())
            for prec in precs:
                net = hh.make_net(H, nh, prec)
                wb = lib.pinn_train_workspace_bytes(ctypes.byref(net), n)
                for dname, drop in (("none", None), ("philox", hh.dropout_struct(1, [0.2] * 4, seed=5, stream_id=2))):
                    for how, phases in (("whole", (7,)), ("split", SPLIT)):
                        work = torch.full((wb,), 0xFF, dtype=torch.uint8, device=hh.dev())      # poisoned: NaN patterns
                        grads = torch.full((fp.numel(),), float("nan"), device=hh.dev())
                        loss = torch.full((4,), float("nan"), dtype=torch.float64, device=hh.dev())
                        for ph in phases:
                            _lib.check(lib.pinn_mlp_train_grads_phases(ctypes.byref(net), hh.ptr(fp), hh.ptr(x), hh.ptr(y), n, n,
                                                                       ctypes.byref(drop) if drop is not None else None, hh.ptr(grads), hh.ptr(loss),
                                                                       hh.ptr(work), wb, hh.stream(), ph), "train")
                        torch.cuda.synchronize()
                        key = "H%d nh%d %-7s drop %-6s rows %5d %s" % (H, nh, PREC[prec], dname, n, how)
                        res[key + ": grads"] = (sha(grads), int(torch.isnan(grads).sum()))
                        res[key + ": loss"] = (sha(loss), int(torch.isnan(loss).sum()))
    json.dump(res, open(out, "w"))


def bench_dump(out, tmp):
    import numpy as np
    res = {}
    for prec in ("fp32", "f32x6", "f32x6g6", "bf16"):
        d = os.path.join(tmp, prec)
        subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--precision", prec,
                        "--dump-outputs", d], check=True, stdout=subprocess.DEVNULL)
        for f in sorted(os.listdir(d)):
            a = np.load(os.path.join(d, f))
            res["bench %-7s %s" % (prec, f)] = (hashlib.sha256(a.tobytes()).hexdigest(), int(np.isnan(a).sum()))
    json.dump(res, open(out, "w"))


def main():
    if sys.argv[1] == "--dump":
        return dump(sys.argv[2])
    if sys.argv[1] == "--bench-dump":
        return bench_dump(sys.argv[2], sys.argv[3])
    libs, bench = [os.path.abspath(p) for p in sys.argv[1:3]], "--bench" in sys.argv
    sides = []
    with tempfile.TemporaryDirectory() as tmp:
        for k, so in enumerate(libs):
            env = dict(os.environ, PINN_HIP_LIB=so)
            res = {}
            for mode in ["--dump"] + (["--bench-dump"] if bench else []):
                out = os.path.join(tmp, "%d%s.json" % (k, mode))
                subprocess.run([sys.executable, os.path.abspath(__file__), mode, out, os.path.join(tmp, "bench%d" % k)], env=env, check=True)
                res.update(json.load(open(out)))
            sides.append(res)
    a, b = sides
    print("# %s  vs  %s: array, SHA-256 on either side, NaN elements, verdict" % tuple(sys.argv[1:3]))
    bad = 0
    for key in a:
        same = a[key] == b.get(key)
        bad += not same
        print("%-62s %s %s nan=%d  %s" % (key, a[key][0], b.get(key, ("-",))[0], a[key][1], "same" if same else "DIFFERS"), flush=True)
    print("# %d arrays, %d differ" % (len(a), bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
