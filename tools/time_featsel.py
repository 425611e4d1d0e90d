"""Time the batched feature sweep of pinn_amd.featsel on the GPU against what it replaces ("Feature sweep").

Candidates: the first 25 subsets, all 833 subsets of at most three and all 3213 of at most four of the 17 candidate columns
of the results array.  Train rows: 1.3e3 (script 02's tenth), 1.2e4 and 1e5, with as many validation rows.  Both the
two-class and the five-class spec.  The array is synthetic: every column carries noise and a class-dependent shift of its
own size, so that the fits differ in their iteration counts as real groups do.

Per shape, after one warm-up of each side, alternating, up to `--reps` times (fewer when a repetition would exceed
`--budget-s`): `feature_sweep` end to end (device events around the call, which ends in a device synchronise: it includes
the Python wrapper, the uploads and the header reads) and the loop, per candidate, of `build_classifier().fit` on the rows
in place, `p_fault` of the validation rows and `roc_counts(curve=False)`: the single-model path, which the sweep does not
touch.  The median of each, their ratio, whether both gave the same integers, and the sweep's phases (scaler, Newton passes,
score, sort + AUC: device events between the entry points, from the median run) go into one JSON line per shape."""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_amd import detection as T, featsel as F  # noqa: E402

SPECS = {"two": T.DEFAULT_GROUP_SPEC, "five": T.FIVE_CLASS_GROUP_SPEC}


def synthetic(n, seed=0):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 13, n)
    lab[:13] = lab[13:26] = np.arange(13)
    a = rng.normal(size=(n, 22)) * rng.uniform(0.5, 3.0, 22) + rng.normal(size=22) * 5.0
    a += (0.6 * rng.uniform(0.0, 4.0, 22) * rng.normal(size=(13, 22)))[lab]
    a[:, 17] = lab
    return a


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1300,12000,100000")
    ap.add_argument("--candidates", default="25,833,3213")
    ap.add_argument("--specs", default="two,five")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--budget-s", type=float, default=20.0, help="seconds the repetitions of one shape may take after the warm-up")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_featsel.py measures on the GPU; none is present")
    warnings.simplefilter("ignore")
    all3, all4 = F.feature_subsets(range(17), 1, 3), F.feature_subsets(range(17), 1, 4)
    pools = {25: F.feature_subsets((0, 3, 11, 12, 8), 1, 3), 833: all3, 3213: all4}
    for which in args.specs.split(","):
        spec = SPECS[which]
        for n in [int(s) for s in args.rows.split(",")]:
            arr = synthetic(2 * n)
            res = torch.from_numpy(arr).cuda()
            idx_tr = np.concatenate([np.arange(13), np.arange(26, n + 13)]).astype(np.int64)
            idx_va = np.concatenate([np.arange(13, 26), np.arange(n + 13, 2 * n)]).astype(np.int64)
            lab = arr[:, 17].astype(np.int64)
            y = (lab > 0).astype(np.int64) if which == "two" else (lab + 2) // 3
            y_tr, r_tr, r_va = (torch.from_numpy(v).cuda() for v in (y[idx_tr], idx_tr, idx_va))
            truth = torch.from_numpy(y[idx_va] != 0).cuda()
            for B in [int(s) for s in args.candidates.split(",")]:
                subsets = pools[B] if B in pools else all4[:B]

                def sweep():
                    t = {}
                    return F.feature_sweep(res, subsets, group_spec=spec, split=(idx_tr, idx_va), backend="device", timings=t), t

                def loop():
                    out = []
                    for cols in subsets:
                        clf = T.build_classifier(balanced=True, backend="device").fit(res, y_tr, columns=list(cols), row_index=r_tr)
                        pf = clf.p_fault(res, 0, columns=list(cols), row_index=r_va)
                        out.append((clf.named_steps["logreg"].n_iter_, T.roc_counts(truth, pf, pos_label=True, backend="device", curve=False)["U2"]))
                    return out
                w_sweep, (sw, _) = timed(sweep)
                w_loop, singles = timed(loop)
                reps = int(max(1, min(args.reps, args.budget_s * 1e3 // (w_sweep + w_loop))))
                out = {"spec": which, "train_rows": len(idx_tr), "val_rows": len(idx_va), "candidates": len(subsets), "reps": reps,
                       "same_integers": [(int(a), int(b)) for a, b in zip(sw.n_iter, sw.val_U2)] == [(int(a), int(b)) for a, b in singles],
                       "n_iter_max": int(sw.n_iter.max()), "n_iter_min": int(sw.n_iter.min()), "not_converged": int((~sw.converged).sum())}
                t_sweep, t_loop, phases = [], [], []
                for _ in range(reps):
                    ms, (_, t) = timed(sweep)
                    t_sweep.append(ms)
                    phases.append(t)
                    t_loop.append(timed(loop)[0])
                mid = int(np.argsort(t_sweep)[len(t_sweep) // 2])
                out.update(sweep_ms=float(np.median(t_sweep)), loop_ms=float(np.median(t_loop)), sweep_ms_all=[round(v, 2) for v in t_sweep],
                           loop_ms_all=[round(v, 2) for v in t_loop], phases_ms={k: round(v, 3) for k, v in phases[mid].items()})
                out["loop_over_sweep"] = out["loop_ms"] / out["sweep_ms"]
                print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
