"""Generate tests/golden/g_iforest.npz: scikit-learn's IsolationForest as reference script 02 runs it (02:571-596), on the
synthetic results array of tools/make_golden_lr.py.

Build machine only: needs a checkout of the reference (`--reference PATH/02_fault_classification_auc.py.py`), scikit-learn,
scipy and matplotlib importable (the script imports them; MPLBACKEND=Agg, nothing is drawn).  Neither the package nor any
test imports this file.  The fixture holds arrays only.

What runs: the reference's parse_features("epi,res"), extract_X_y and label mapping (binary spec), scikit-learn's stratified
split (the script's test size and seed), then
  forest `a`: IsolationForest(n_estimators=200, contamination="auto", random_state=42) on the normal training rows;
  forest `b`: IsolationForest(n_estimators=8, max_samples=1000, random_state=42) on all kept rows (trees of depth 10).
Stored: the three columns of the array that are used (epi, res, label; every value is a float32), the kept rows, the split,
the truth of the test rows; per forest the trees (`feature` int8, `threshold` float64, `left` / `right` int16,
`n_node` int16, concatenated, with `offsets`), `max_samples`, `offset`, and for the test rows `score_samples`,
`decision_function`, `predict`; for forest `a` also roc_curve / auc of -score_samples.

Asserted here: a plain numpy restatement of score_samples (below) equals scikit-learn's output bit for bit; no two test
scores of forest `a` of different truth differ by less than 1e-12 (so its AUC is a function of the ranks alone); 0.5 < AUC < 1.
"""
import argparse
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_lr import BINARY, load_reference, synthetic_results  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g_iforest.npz")
COLS = [11, 12, 17]                                      # epi, res, label


def c_of(n):
    n = np.asarray(n)
    out = np.zeros(n.shape)
    out[n == 2] = 1.0
    big = n > 2
    out[big] = 2.0 * (np.log(n[big] - 1.0) + np.euler_gamma) - 2.0 * (n[big] - 1.0) / n[big]
    return out


def restated_scores(est, X):
    """score_samples in plain numpy: float32 rows, x32 <= threshold, leaf value depth + c(n), float64 sum in tree order."""
    X32 = X.astype(np.float32)
    total = np.zeros(len(X))
    for e in est.estimators_:
        t = e.tree_
        depth = np.zeros(t.node_count, dtype=np.int64)
        for i in range(t.node_count):                    # pre-order: a parent comes before its children
            if t.children_left[i] >= 0:
                depth[t.children_left[i]] = depth[t.children_right[i]] = depth[i] + 1
        value = (depth + 1) + c_of(t.n_node_samples) - 1.0
        node = np.zeros(len(X), dtype=np.int64)
        while True:
            live = np.flatnonzero(t.children_left[node] >= 0)
            if not live.size:
                break
            nd = node[live]
            node[live] = np.where(X32[live, t.feature[nd]] <= t.threshold[nd], t.children_left[nd], t.children_right[nd])
        total += value[node]
    den = len(est.estimators_) * c_of(np.array([est.max_samples_]))
    return -(2 ** (-np.divide(total, den, out=np.ones_like(total), where=den != 0)))


def forest_arrays(est, tag):
    trees = [e.tree_ for e in est.estimators_]
    assert max(t.node_count for t in trees) < 32768 and max(int(t.n_node_samples.max()) for t in trees) < 32768
    return {tag + "_feature": np.concatenate([t.feature for t in trees]).astype(np.int8),
            tag + "_threshold": np.concatenate([t.threshold for t in trees]).astype(np.float64),
            tag + "_left": np.concatenate([t.children_left for t in trees]).astype(np.int16),
            tag + "_right": np.concatenate([t.children_right for t in trees]).astype(np.int16),
            tag + "_n_node": np.concatenate([t.n_node_samples for t in trees]).astype(np.int16),
            tag + "_offsets": np.concatenate([[0], np.cumsum([t.node_count for t in trees])]).astype(np.int32),
            tag + "_max_samples": np.array(est.max_samples_, dtype=np.int64), tag + "_offset": np.array(est.offset_),
            tag + "_max_depth": np.array(max(t.max_depth for t in trees), dtype=np.int64)}


def main():
    from sklearn.ensemble import IsolationForest
    from sklearn.metrics import auc, roc_curve
    from sklearn.model_selection import train_test_split
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="path of the reference's script 02")
    ap.add_argument("--seed", type=int, default=None, help="seed of the synthetic array (default: the one stored in g_lr.npz)")
    args = ap.parse_args()
    warnings.filterwarnings("ignore")
    ref = load_reference(args.reference)
    seed = args.seed if args.seed is not None else int(np.load(os.path.join(ROOT, "tests", "golden", "g_lr.npz"))["seed"])
    a = synthetic_results(seed)
    label_map, names = ref.build_label_mapper(ref.parse_group_spec(BINARY))
    fidx = ref.parse_features(ref.FEAT_GRP1)
    X, y = ref.extract_X_y(a, fidx, label_map)
    det = a[:, 17].astype(np.int32)
    kept = np.flatnonzero(np.array([d in label_map for d in det]) & np.isfinite(a[:, fidx]).all(axis=1))
    assert len(kept) == len(y) and np.array_equal(a[kept][:, fidx], X)
    X_tr, X_te, y_tr, y_te, i_tr, i_te = train_test_split(X, y, np.arange(len(y)), test_size=ref.DEFAULT_TEST_SIZE,
                                                          random_state=ref.DEFAULT_RANDOM_STATE, stratify=y)
    normal = 0
    truth = (y_te != normal).astype(int)
    X_fit = X_tr[y_tr == normal] if np.sum(y_tr == normal) > 10 else X_tr
    out = {"seed": np.array(seed, dtype=np.int64), "col_ids": np.array(COLS, dtype=np.int64), "results_cols": a[:, COLS].astype(np.float32),
           "cols": np.array(fidx, dtype=np.int64), "kept": kept.astype(np.int16), "idx_tr": i_tr.astype(np.int16), "idx_te": i_te.astype(np.int16),
           "y": y.astype(np.int8), "truth": truth.astype(np.int8), "n_fit": np.array(len(X_fit), dtype=np.int64)}
    assert np.array_equal(np.nan_to_num(out["results_cols"].astype(np.float64), nan=-1.0), np.nan_to_num(a[:, COLS], nan=-1.0))
    for tag, est, rows in (("a", IsolationForest(n_estimators=200, contamination="auto", random_state=42), X_fit),
                           ("b", IsolationForest(n_estimators=8, max_samples=1000, random_state=42), X)):
        est.fit(rows)
        s = est.score_samples(X_te)
        assert np.array_equal(restated_scores(est, X_te), s), "the numpy restatement differs from scikit-learn"
        dec = est.decision_function(X_te)
        assert np.array_equal(dec, s - est.offset_)
        gap = np.min(np.abs(s[truth == 1][:, None] - s[truth == 0][None, :]))
        assert tag != "a" or gap >= 1e-12, gap         # forest a's AUC is tested; forest b's 8 trees leave exact ties
        o = forest_arrays(est, tag)
        o.update({tag + "_score": s, tag + "_decision": dec, tag + "_pred": est.predict(X_te).astype(np.int8)})
        if tag == "a":
            fpr, tpr, thr = roc_curve(truth, -s, pos_label=1)
            area = auc(fpr, tpr)
            assert 0.5 < area < 1.0, area
            o.update(a_fpr=fpr, a_tpr=tpr, a_thr=thr, a_auc=np.array(area))
        out.update(o)
        print("forest %s: %d trees, %d nodes, max_samples_ %d, depth %d, min |decision| %.3e, gap between the classes %.3e"
              % (tag, len(est.estimators_), o[tag + "_offsets"][-1], est.max_samples_, o[tag + "_max_depth"], np.abs(dec).min(), gap))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size <= 256 * 1024, size
    print("seed %d, %d bytes, %d rows fitted, %d test rows, AUC %.6f" % (seed, size, len(X_fit), len(y_te), float(out["a_auc"])))


if __name__ == "__main__":
    sys.exit(main())
