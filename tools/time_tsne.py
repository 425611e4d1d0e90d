"""Time exact t-SNE on the GPU (pinn_amd.embedding, csrc/pinn_tsne.hip) at n = 2048 and n = 11000 rows, D = 4:

  * the affinities (perplexity root per row, symmetrised)
  * ms per iteration of the pair pass (pinn_tsne_kl_grad: pair pass with the log terms plus the one-workgroup reduction), and of
    a descent iteration (pinn_tsne_descend: 49 of 50 without the log terms), with the rate at which P (8 n^2 bytes) streams
  * the whole fit_transform (script 03's settings, 1000 iterations)
  * the yardstick: one iteration restated in eager torch float64 on the same GPU (cdist, elementwise, sum).  It is not the
    code under test.

Times are device events around windows of at least 50 iterations after a warm-up of the same shape; the median of 5 windows.
Needs a GPU; prints one line per number and a JSON line at the end.  `--n 2048 11000`, `--skip-fit`.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rows(n, D=4, seed=0):
    rng = np.random.default_rng(seed)
    y = rng.integers(4, size=n)
    centre = -2.0 * np.ones((4, D))
    centre[np.arange(4), np.arange(4) % D] = 2.0
    return 1.0 / (1.0 + np.exp(-(centre[y] + 0.7 * rng.standard_normal((n, D)))))


def windows(torch, fn, reps=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(min(out)), float(max(out))


def eager_iteration(torch, P, Y, upd, gains, alpha, mom, lr):
    d2 = torch.cdist(Y, Y) ** 2
    w = 1.0 / (1.0 + d2)
    w.fill_diagonal_(0.0)
    Z = w.sum()
    pw = (alpha * P - w / Z) * w
    grad = 4.0 * (pw.sum(dim=1, keepdim=True) * Y - pw @ Y)
    inc = upd * grad < 0.0
    gains = torch.where(inc, gains + 0.2, gains * 0.8).clamp_(min=0.01)
    upd = mom * upd - lr * gains * grad
    return Y + upd, upd, gains


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2048, 11000])
    ap.add_argument("--skip-fit", action="store_true")
    args = ap.parse_args()
    import torch
    from pinn_amd import _lib, embedding as E
    from pinn_amd._device import _DevRows, _ptr
    if not torch.cuda.is_available():
        sys.exit("time_tsne.py needs a GPU")
    lib = _lib.load()
    res = {}
    for n in args.n:
        X = torch.from_numpy(rows(n)).cuda()
        r = _DevRows(torch, X)
        stream = torch.cuda.current_stream().cuda_stream
        ws, beta, ent, status = E._dev_affinities(torch, _lib, lib, r, 20.0)
        E._raise_status(status)
        t_aff = windows(torch, lambda: _lib.check(lib.pinn_tsne_affinities(*r.head(), 20.0, _ptr(beta), _ptr(ent), _ptr(status), _ptr(ws.buf),
                                                                             ws.bytes, stream), "affinities"), reps=3)
        Y = (torch.randn(n, 2, dtype=torch.float64, device="cuda") * 3.0).contiguous()
        iters = 50

        def pair():
            for _ in range(iters):
                lib.pinn_tsne_kl_grad(n, _ptr(Y), 1.0, _ptr(ws.buf), ws.bytes, stream)
        t_pair = windows(torch, pair)
        st = torch.zeros(lib.pinn_tsne_state_bytes(n) // 8, dtype=torch.float64, device="cuda")
        st[16:16 + 2 * n] = (1e-4 * torch.randn(2 * n, dtype=torch.float64, device="cuda"))

        def descend():                                          # iterations 0..49 over and over: the header is set anew every call
            lib.pinn_tsne_descend(n, 1, iters, 1000, 12.0, max(n / 48.0, 50.0), 300, 0.0, _ptr(st), _ptr(ws.buf), ws.bytes, stream)
        t_desc = windows(torch, descend)
        P = ws.P.clone()
        Ye, ue, ge = Y.clone(), torch.zeros_like(Y), torch.ones_like(Y)

        def eager():
            nonlocal Ye, ue, ge
            for _ in range(10):
                Ye, ue, ge = eager_iteration(torch, P, Ye, ue, ge, 1.0, 0.8, 50.0)
        t_eager = windows(torch, eager)
        gb = 8.0 * n * n / 1e9
        out = {"affinities_ms": t_aff[0], "pair_pass_ms_per_iter": t_pair[0] / iters, "pair_pass_spread_ms": [t_pair[1] / iters, t_pair[2] / iters],
               "pair_pass_P_GBps": gb / (t_pair[0] / iters / 1e3), "descend_ms_per_iter": t_desc[0] / iters,
               "descend_P_GBps": gb / (t_desc[0] / iters / 1e3), "eager_ms_per_iter": t_eager[0] / 10,
               "eager_over_descend": (t_eager[0] / 10) / (t_desc[0] / iters)}
        del P, Ye, ue, ge
        if not args.skip_fit:
            m = E.DeviceTSNE(backend="device", **E.TSNE_TEST_PARAMS)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            m.fit(X)
            b.record()
            b.synchronize()
            out.update(fit_transform_ms=a.elapsed_time(b), n_iter=m.n_iter_, kl=m.kl_divergence_)
        res[str(n)] = out
        for k, v in out.items():
            print("n = %d  %s = %s" % (n, k, ("%.4g" % v) if isinstance(v, float) else v), flush=True)
        del ws, st
        torch.cuda.empty_cache()
    print(json.dumps({"time_tsne": res}))


if __name__ == "__main__":
    main()
