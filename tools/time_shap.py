"""Time the exact Shapley attributions of pinn_amd.explain on the GPU.

Three workloads, each timed with device events after a warm-up (the median of `--reps` repetitions) and against the same
result composed from the entry points the package had before this module: hybrid rows by torch.where, then
DeviceGMM.diagnose or net_u, then torch reductions, chunked to the same number of hybrid rows.
  diagnosis03  shapley_diagnosis at script 03's size: the mixture fitted to the 1349 training rows of tests/golden/g_gmm.npz
               (K = 20, D = 4, C = 4), those rows as the background, 11 000 rows to explain
  diagnosis8   shapley_diagnosis at D = 8, K = 32, C = 4, B = 256, 10 000 rows
  voltage      shapley_values(voltage_predictor(model)) of the [8, 256, 256, 256, 1] network, 11 000 rows, B = 64, with the
               share of the time spent outside the forward (hybrid + reduce kernels)
The fused path is also compared with the generic path on the same inputs (largest difference), and the float64 host backend
is timed at `--host-rows` rows.  Prints one JSON line per workload.

The share of exp in the fused kernel's time: build a variant whose exponential is one multiply-add,
    tools/build_variant.py shap_noexp "-DPINN_SHAP_NO_EXP" pinn_shap.hip
and run `PINN_HIP_LIB=tools/exp/shap_noexp/libpinn_hip.so tools/time_shap.py --fused-only --only diagnosis03,diagnosis8`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import pinn_amd  # noqa: E402
from pinn_amd import diagnosis, explain, synth  # noqa: E402


FUSED_ONLY = False


def event_ms(fn, reps):
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
    return float(np.median(out))


def composed(predict, X, Bg, dtype, max_hybrid_rows=1 << 22):
    """phi [n, D, C] from torch ops alone."""
    n, D = X.shape
    B, nS = Bg.shape[0], 1 << D
    masks = ((torch.arange(nS, device=X.device)[:, None] >> torch.arange(D, device=X.device)[None, :]) & 1).bool()
    coef = torch.from_numpy(explain.coalition_weights(D)).to(X.device)
    step = max(1, max_hybrid_rows // (nS * B))
    out = []
    for r0 in range(0, n, step):
        x = X[r0:r0 + step]
        H = torch.where(masks[None, :, None, :], x[:, None, None, :], Bg[None, None, :, :]).reshape(-1, D).to(dtype)
        F = predict(H).to(torch.float64)
        v = F.reshape(x.shape[0], nS, B, -1).mean(dim=2)
        out.append(torch.einsum("js,msc->mjc", coef, v))
    return torch.cat(out)


def random_mixture(K, D, C, seed):
    rng = np.random.default_rng(seed)
    means = rng.normal(0.0, 2.0, (K, D))
    cov = np.empty((K, D, D))
    for k in range(K):
        A = rng.normal(0.0, 1.0, (D, D)) * 0.4 + np.eye(D)
        cov[k] = A @ A.T
    g = diagnosis.DeviceGMM(K, backend="device")
    w = rng.uniform(0.5, 1.5, K)
    g.weights_, g.means_, g.covariances_, g.precisions_cholesky_ = w / w.sum(), means, cov, diagnosis._host_factor(cov)
    g.n_iter_, g.converged_, g.lower_bound_, g.lower_bound_changes_ = 1, True, 0.0, []
    cfp = rng.uniform(0.0, 1.0, (K, C)) ** 3
    return g, cfp / cfp.sum(axis=1, keepdims=True), rng


def time_diagnosis(name, gmm, cfp, X, Bg, reps, host_rows):
    K, (n, D), B, C = gmm.n_components, X.shape, Bg.shape[0], cfp.shape[1]
    Xd, Bd, cd = torch.from_numpy(X).cuda(), torch.from_numpy(Bg).cuda(), torch.from_numpy(cfp).cuda()
    pred = lambda Z: gmm.diagnose(Z, cd)[0]
    res = {"workload": name, "rows": n, "B": B, "D": D, "K": K, "C": C}
    res["fused_ms"] = event_ms(lambda: explain.shapley_diagnosis(gmm, cd, Xd, Bd), reps)
    if FUSED_ONLY:
        print(json.dumps(res), flush=True)
        return
    res["generic_ms"] = event_ms(lambda: explain.shapley_values(pred, Xd, Bd), max(2, reps // 2))
    res["composed_torch_ms"] = event_ms(lambda: composed(pred, Xd, Bd, torch.float64), max(2, reps // 2))
    f = explain.shapley_diagnosis(gmm, cd, Xd, Bd).phi
    res["fused_vs_generic_max_diff"] = float((f - explain.shapley_values(pred, Xd, Bd).phi).abs().max())
    res["fused_vs_composed_max_diff"] = float((f - composed(pred, Xd, Bd, torch.float64)).abs().max())
    evals = n * B * ((1 << D) - 2)
    res["fused_model_evaluations_per_s"] = evals / (res["fused_ms"] * 1e-3)
    res["fused_exp_per_s"] = evals * K / (res["fused_ms"] * 1e-3)
    gh = diagnosis.DeviceGMM(K, backend="host")
    gh.weights_, gh.means_, gh.covariances_, gh.precisions_cholesky_ = (diagnosis._as_numpy(a) for a in (gmm.weights_, gmm.means_, gmm.covariances_,
                                                                                                          gmm.precisions_cholesky_))
    gh.n_iter_, gh.converged_, gh.lower_bound_ = 1, True, 0.0
    t0 = time.perf_counter()
    explain.shapley_diagnosis(gh, cfp, X[:host_rows], Bg, backend="host")
    res["host_rows"], res["host_ms"] = host_rows, (time.perf_counter() - t0) * 1e3
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=64)
    ap.add_argument("--only", default="diagnosis03,diagnosis8,voltage")
    ap.add_argument("--fused-only", action="store_true",
                    help="time the fused kernel alone: with PINN_HIP_LIB naming a build with -DPINN_SHAP_NO_EXP, the time without exp")
    args = ap.parse_args()
    only = args.only.split(",")
    global FUSED_ONLY
    FUSED_ONLY = args.fused_only

    if "diagnosis03" in only:
        G = dict(np.load(os.path.join(R, "tests", "golden", "g_gmm.npz"), allow_pickle=False))
        gmm = diagnosis.DeviceGMM(20, labels_init=G["labels_init"], backend="device").fit(G["X_tr"])
        cfp = gmm.label_map(G["X_tr"], G["y_tr"], 4)
        rng = np.random.default_rng(0)
        X = G["X_tr"][rng.integers(G["X_tr"].shape[0], size=11000)] * (1.0 + 0.05 * rng.normal(size=(11000, 4)))
        time_diagnosis("diagnosis03", gmm, cfp, X, G["X_tr"], args.reps, args.host_rows)

    if "diagnosis8" in only:
        gmm, cfp, rng = random_mixture(32, 8, 4, seed=1)
        draw = lambda n: gmm.means_[rng.integers(32, size=n)] + rng.normal(0.0, 1.2, (n, 8))
        time_diagnosis("diagnosis8", gmm, cfp, draw(10000), draw(256), max(2, args.reps // 2), min(args.host_rows, 8))

    if "voltage" in only:
        n, B = 11000, 64
        ds = synth.make_dataset(n + B, (), seed=0)
        torch.manual_seed(0)
        model = pinn_amd.PhysicsInformedNN(ds[0], ds[1], [8, 256, 256, 256, 1], ds[4], ds[5], p=0.2, logvar=True, seed=1)
        model.verbose = False
        X, Bg = ds[0][:n].cuda(), ds[0][n:n + B].cuda()
        pred = explain.voltage_predictor(model)
        spent = []

        def timed(Z):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = pred(Z)
            b.record()
            spent.append((a, b))
            return out
        res = {"workload": "voltage", "rows": n, "B": B, "D": 8, "C": 2, "forwards": n * B * 256}
        res["generic_ms"] = event_ms(lambda: explain.shapley_values(pred, X, Bg, dtype="float32"), args.reps)
        res["composed_torch_ms"] = event_ms(lambda: composed(pred, X.double(), Bg.double(), torch.float32), args.reps)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = explain.shapley_values(timed, X, Bg, dtype="float32")
        b.record()
        b.synchronize()
        inside = sum(s.elapsed_time(e) for s, e in spent)
        res["share_outside_forward"] = 1.0 - inside / a.elapsed_time(b)
        res["generic_vs_composed_max_diff"] = float((r.phi - composed(pred, X.double(), Bg.double(), torch.float32)).abs().max())
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
