"""Which faults can still be true, and is it none of the four?  A synthetic results array with the four fault classes and a
fifth condition held back (label 13, outside risk.FAULT_RANGE_MAP, its residual columns shifted away from all four).  The
mixture is fitted on a training split and calibrated on a second split; the rest is the test split.  Prints per class, at
90 % and 95 %, for the `lac` and the `density` scores: coverage, mean set size and the share of the held-back rows whose set is
empty (flagged as novel).  Then the recording runs through the online diagnoser chunk by chunk.

    python examples/open_set_diagnosis.py [--rows 1500] [--components 8] [--backend auto|host|device] [--chunk 2048]

Runs with --backend host on a machine without a GPU.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from pinn_amd import diagnosis, faultsets  # noqa: E402
from pinn_amd.detection import stratified_split  # noqa: E402
from pinn_amd.risk import INDEX  # noqa: E402

HELD_BACK = 13
LEVELS = (0.9, 0.95)


def synthetic_results(rows_per_class, seed=0):
    """A results array [n, 22] in time order: runs of the twelve fault labels (three per class) and a run of the held-back
    condition.  Every class moves the residual columns pV, pT, pH, pO its own way; the held-back one moves all of them far
    from the four."""
    rng = np.random.default_rng(seed)
    cols = [INDEX[k] for k in ("pV", "pT", "pH", "pO")]
    shift = {1: (3.0, 0.0, 0.0, 0.5), 4: (0.0, 0.5, 0.0, 3.0), 7: (-3.0, 2.0, 0.0, 0.0), 10: (0.0, 0.0, 3.0, -0.5)}
    parts = []
    for label in list(range(1, 13)) + [HELD_BACK]:
        n = rows_per_class // 3 if label != HELD_BACK else rows_per_class
        A = rng.normal(size=(n, 22))
        centre = np.full(4, 25.0) if label == HELD_BACK else np.asarray(shift[1 + 3 * ((label - 1) // 3)])
        A[:, cols] = centre + rng.normal(size=(n, 4)) * (1.0 + 0.1 * ((label - 1) % 3))
        A[:, INDEX["label"]] = label
        parts.append(A)
    return np.concatenate(parts)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1500, help="rows per fault class")
    ap.add_argument("--components", type=int, default=8)
    ap.add_argument("--backend", default="auto", choices=("auto", "host", "device"))
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    results = synthetic_results(args.rows, args.seed)
    if args.backend == "device":
        import torch
        results = torch.from_numpy(results).cuda()
    features = diagnosis.parse_features(diagnosis.DEFAULT_FEATURES)
    label_map, class_names = diagnosis.build_label_mapper(diagnosis.parse_group_spec(diagnosis.DEFAULT_GROUP_SPEC))
    C = len(class_names)
    _, y, kept = diagnosis.extract_X_y(results, features, label_map, return_index=True, backend=args.backend)
    y_host = y.cpu().numpy() if hasattr(y, "cpu") else np.asarray(y)
    kept_host = kept.cpu().numpy() if hasattr(kept, "cpu") else np.asarray(kept)

    # three splits of the known rows: fit, calibrate, test (stratified_split twice)
    rest, test = stratified_split(y_host, test_size=0.3, random_state=args.seed)
    fit, cal = stratified_split(y_host[rest], test_size=0.4, random_state=args.seed + 1)
    fit, cal = rest[fit], rest[cal]
    lab = results[:, INDEX["label"]]
    lab = lab.cpu().numpy() if hasattr(lab, "cpu") else lab
    held = np.flatnonzero(lab == HELD_BACK)
    rows_of = lambda idx: kept_host[idx]                        # positions among the kept rows -> rows of the array

    gmm = diagnosis.DeviceGMM(args.components, random_state=args.seed, backend=args.backend)
    gmm.fit(results, columns=features, row_index=rows_of(fit))
    cfp = gmm.label_map(results, y_host[fit], C, columns=features, row_index=rows_of(fit))

    # the test rows and the held-back rows together; the held-back ones get a class outside [0, C)
    eval_rows = np.concatenate([rows_of(test), held])
    eval_y = np.concatenate([y_host[test], np.full(held.size, -1, np.int64)])
    print("rows: fit %d, calibration %d, test %d, held back %d; %d components" % (fit.size, cal.size, test.size, held.size, args.components))
    diagnosers = {}
    for kind in ("lac", "density"):
        c = faultsets.calibrate_gmm(gmm, cfp, results, y_host[cal], kind=kind, columns=features, row_index=rows_of(cal), backend=args.backend)
        d = faultsets.GMMSetDiagnoser(gmm, cfp, c, levels=LEVELS, backend=args.backend)
        diagnosers[kind] = d
        rep = d.evaluate(results, eval_y, columns=features, row_index=eval_rows)
        print("\nscore %-8s calibration rows per class %s" % (kind, c.n_cal.tolist()))
        print("  %-22s %s" % ("class", "  ".join("coverage@%.2f" % lv for lv in LEVELS)))
        for ci, name in enumerate(class_names):
            print("  %-22s %s" % (name, "  ".join("%13.4f" % rep.coverage[ci, l] for l in range(len(LEVELS)))))
        print("  %-22s %s" % ("mean set size", "  ".join("%13.4f" % v for v in rep.mean_size)))
        print("  %-22s %s" % ("held back, novel", "  ".join("%13.4f" % v for v in rep.novel_share)))

    # the recording, chunk by chunk, through the density diagnoser
    online = diagnosers["density"]
    print("\n%8s %-22s %-28s %s" % ("rows", "diagnosis (last row)", "90 % set (last row)", "novel rows in the chunk"))
    n_novel = held_novel = 0
    for s in range(0, results.shape[0], args.chunk):
        y_prob, y_pred, sets = online.update(results[s:s + args.chunk])
        novel = int(sets.novel[:, 0].sum())
        n_novel += novel
        is_held = lab[s:s + args.chunk] == HELD_BACK
        flags = sets.novel[:, 0]
        held_novel += int((flags.cpu().numpy() if hasattr(flags, "cpu") else flags)[is_held].sum())
        members = ",".join(class_names[c][:5] for c in sets.members(-1, LEVELS[0])) or "none: unknown fault"
        print("%8d %-22s %-28s %d" % (online.n_seen, class_names[int(y_pred[-1])], members, novel))
    print("novel rows online: %d of %d; of the %d held-back rows: %d" % (n_novel, results.shape[0], held.size, held_novel))
    return held_novel, held.size


if __name__ == "__main__":
    main()
