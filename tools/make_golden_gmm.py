"""Generate tests/golden/g_gmm.npz by running the reference's script 03 on a synthetic results array.

Build machine only: needs a checkout of the reference (`--reference PATH/03_unsupervised_gmm_fault_diagnosis.py.py`),
scikit-learn, scipy and matplotlib importable (the script imports them; MPLBACKEND=Agg, nothing is drawn).  Neither the
package nor any test imports this file.  The fixture holds arrays only: the split, the labels scikit-learn's k-means
initialisation produced, what the reference fitted and predicted from them, the parsing table, and three measured
quantities: `sens_*` (how far the reference's own fit moves when X_tr is multiplied by 1 + 1e-13 u, u uniform in
[-1, 1], maximum over 5 draws, EM restarted from the same initial labels), and `lb_min / lb_max / acc_min / acc_max` (the
reference over random_state = 0..9 on the same split).  `--time` also prints scikit-learn's wall time for a fit and a
predict_proba at 1e5 rows x 4 features x 20 components (printed, not stored: the fixture regenerates byte for byte).

Conditions on the inputs (asserted here; the next seed is tried when one fails):
  convergence margin  | |change of the lower bound| - tol | >= 1e-8 at every iteration, so 1e-12 cannot change n_iter_;
  decision margin     the two largest entries of every y_prob row differ by at least 1e-6, so y_pred is exact;
  every component keeps n_k >= 1, so the uniform fallback of the label map is not what the fixture tests.
"""
import argparse
import contextlib
import importlib.util
import io
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g_gmm.npz")
N_NORMAL, N_SEG, SEG, K = 800, 12, 150, 20
SCALE = {13: 0.05, 14: 0.5, 15: 0.01, 16: 0.01}                       # sigma of pV, pT, pH, pO on normal rows
DRIFT_COLS = {0: (13, 16), 1: (16, 14), 2: (14, 15), 3: (15, 13)}     # two residual columns per fault class
AMPLITUDE = (6.0, 9.0, 12.0)                                          # ramp height in sigma, by segment of a class
NOISE, DRAWS = 1e-13, 5

FEATURE_SPECS = ["pV,pT,pH,pO", "pV pT；pH|pO", "13.14, 15 ,16", "x0，x1、y_true", "pV,pV,13,res", " epi ; ale ", "pV,bogus", "pV,label", "17",
                 "3,,4", ""]
GROUP_SPECS = ["水淹:1,2,3,|氧饥饿:4,5,6,|膜干:7,8,9,|氢饥饿:10,11,12", "a:1 2 3;b:4.5.6", "a:1,2\nb:-3", "a:1,2|b 3", "a:1,x", "a:1|a:2", " | ",
               "a:|b:7"]


def load_reference(path):
    os.environ.setdefault("MPLBACKEND", "Agg")
    spec = importlib.util.spec_from_file_location("ref03", path)
    ref = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(ref)
    return ref


def synthetic_results(seed):
    rng = np.random.default_rng(seed)
    n = N_NORMAL + N_SEG * SEG
    a = np.zeros((n, 22))
    for c, s in SCALE.items():
        a[:, c] = rng.normal(0.0, s, n)
    ramp = np.linspace(0.0, 1.0, SEG)
    for k in range(1, N_SEG + 1):
        rows = slice(N_NORMAL + (k - 1) * SEG, N_NORMAL + k * SEG)
        a[rows, 17] = k
        for j, c in enumerate(DRIFT_COLS[(k - 1) // 3]):
            a[rows, c] += (1.0 if j == 0 else -1.0) * AMPLITUDE[(k - 1) % 3] * SCALE[c] * (0.35 + 0.65 * ramp)
    a[N_NORMAL + 40, 14] = np.nan                  # one row that extract_X_y must drop
    return a


def capturing_class(GaussianMixture):
    class Capture(GaussianMixture):
        fixed_resp = None
        log = None

        def _initialize_parameters(self, X, random_state):
            if Capture.fixed_resp is not None:
                self._initialize(X, Capture.fixed_resp)
            else:
                super()._initialize_parameters(X, random_state)

        def _initialize(self, X, resp):
            if Capture.log is not None:
                Capture.log["resp_init"] = resp.copy()
            super()._initialize(X, resp)

        def _e_step(self, X):
            if Capture.log is not None:
                if "lpn0" not in Capture.log:
                    lpn, log_resp = self._estimate_log_prob_resp(X)
                    Capture.log["lpn0"], Capture.log["resp0"] = lpn.copy(), np.exp(log_resp)
                    Capture.log["bounds"] = []
                out = super()._e_step(X)
                Capture.log["bounds"].append(float(out[0]))
                return out
            return super()._e_step(X)
    return Capture


def parsing_table(ref):
    def call(fn, spec):
        try:
            return fn(spec), 0
        except KeyError:
            return None, 1
        except ValueError:
            return None, 2
    out = {"feat_specs": np.array(FEATURE_SPECS), "group_specs": np.array(GROUP_SPECS),
           "norm_result": np.array([ref.normalize_feature_spec(s) for s in FEATURE_SPECS])}
    fr, fe = np.full((len(FEATURE_SPECS), 8), -1, dtype=np.int64), []
    for r, s in enumerate(FEATURE_SPECS):
        v, e = call(ref.parse_features, s)
        fe.append(e)
        if v is not None:
            fr[r, :len(v)] = v
    gi, ge = np.full((len(GROUP_SPECS), 4, 6), -99, dtype=np.int64), []
    gn = np.full((len(GROUP_SPECS), 4), "", dtype="U16")
    for r, s in enumerate(GROUP_SPECS):
        v, e = call(ref.parse_group_spec, s)
        ge.append(e)
        if v is not None:
            for g, (name, ids) in enumerate(v.items()):
                gn[r, g] = name
                gi[r, g, :len(ids)] = ids
    out.update(feat_result=fr, feat_error=np.array(fe, dtype=np.int64), group_ids=gi, group_names=gn, group_error=np.array(ge, dtype=np.int64))
    return out


def build(ref, Capture, seed):
    from sklearn.model_selection import train_test_split
    a = synthetic_results(seed)
    feats = ref.parse_features(ref.DEFAULT_FEATURES)
    label_map, names = ref.build_label_mapper(ref.parse_group_spec(ref.DEFAULT_GROUP_SPEC))
    X, y = ref.extract_X_y(a, feats, label_map)
    det = a[:, 17].astype(np.int32)
    kept = np.flatnonzero(np.array([d in label_map for d in det]) & np.isfinite(a[:, feats]).all(axis=1))
    assert len(kept) == len(y)
    idx = np.arange(len(y))
    X_tr, X_te, y_tr, y_te, i_tr, i_te = train_test_split(X, y, idx, test_size=ref.TEST_SIZE, random_state=ref.RANDOM_STATE, stratify=y)
    Capture.fixed_resp, Capture.log = None, {}
    y_prob, y_pred, gmm, cfp = ref.fit_gmm_and_get_probabilities(X_tr, y_tr, X_te, len(names), random_state=ref.RANDOM_STATE, n_components=K)
    log, Capture.log = Capture.log, None
    if not gmm.converged_:
        return None
    bounds = np.array(log["bounds"][:gmm.n_iter_])
    changes = np.diff(np.concatenate([[-np.inf], bounds]))
    if np.min(np.abs(np.abs(changes) - gmm.tol)) < 1e-8:
        return None
    top = np.sort(y_prob, axis=1)
    if np.min(top[:, -1] - top[:, -2]) < 1e-6:
        return None
    resp_tr = gmm.predict_proba(X_tr)
    if resp_tr.sum(axis=0).min() < 1.0:
        return None
    resp_init = log["resp_init"]
    assert np.all((resp_init == 0) | (resp_init == 1))

    # amplification of EM on this data: the reference against itself under 1e-13 relative input noise
    rng = np.random.default_rng(seed + 1)
    sens = np.zeros(5)
    for _ in range(DRAWS):
        Capture.fixed_resp = resp_init
        Xp = X_tr * (1.0 + NOISE * rng.uniform(-1.0, 1.0, X_tr.shape))
        yp2, _, g2, _ = ref.fit_gmm_and_get_probabilities(Xp, y_tr, X_te, len(names), random_state=ref.RANDOM_STATE, n_components=K)
        Capture.fixed_resp = None
        if g2.n_iter_ != gmm.n_iter_:
            return None
        cmax = np.abs(gmm.covariances_).max(axis=(1, 2), keepdims=True)
        sens = np.maximum(sens, [np.abs(g2.weights_ - gmm.weights_).max(), np.abs(g2.means_ - gmm.means_).max() / np.abs(gmm.means_).max(),
                                 (np.abs(g2.covariances_ - gmm.covariances_) / cmax).max(), abs(g2.lower_bound_ - gmm.lower_bound_),
                                 np.abs(yp2 - y_prob).max()])
    lbs, accs = [], []
    for rs in range(10):
        _, yp, g, _ = ref.fit_gmm_and_get_probabilities(X_tr, y_tr, X_te, len(names), random_state=rs, n_components=K)
        lbs.append(g.lower_bound_)
        accs.append(float((yp == y_te).mean()))
    out = {"seed": np.array(seed, dtype=np.int64), "results_cols": a[:, feats + [17]], "kept_rows": kept.astype(np.int64),
           "idx_tr": i_tr.astype(np.int64), "idx_te": i_te.astype(np.int64), "X_tr": X_tr, "y_tr": y_tr.astype(np.int64), "X_te": X_te,
           "y_te": y_te.astype(np.int64), "labels_init": resp_init.argmax(axis=1).astype(np.int64), "weights": gmm.weights_,
           "means": gmm.means_, "covariances": gmm.covariances_, "n_iter": np.array(gmm.n_iter_, dtype=np.int64),
           "lower_bound": np.array(gmm.lower_bound_), "changes": changes, "tol": np.array(gmm.tol), "resp0_head": log["resp0"][:300],
           "log_prob_norm0": log["lpn0"], "comp_fault_prob": cfp, "y_prob": y_prob, "y_pred": y_pred.astype(np.int64),
           "sens": sens, "sens_names": np.array(["weights", "means", "covariances", "lower_bound", "y_prob"]),
           "lb_range": np.array([min(lbs), max(lbs)]), "acc_range": np.array([min(accs), max(accs)])}
    out.update(parsing_table(ref))
    return out


def time_sklearn():
    from sklearn.mixture import GaussianMixture
    rng = np.random.default_rng(3)
    centres = rng.normal(0.0, 4.0, (K, 4))
    X = centres[rng.integers(K, size=100000)] + rng.normal(0.0, 1.0, (100000, 4))
    g = GaussianMixture(n_components=K, covariance_type="full", random_state=0)
    t0 = time.perf_counter()
    g.fit(X)
    t1 = time.perf_counter()
    g.predict_proba(X)
    t2 = time.perf_counter()
    return t1 - t0, g.n_iter_, t2 - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="path of the reference's script 03")
    ap.add_argument("--time", action="store_true", help="also time scikit-learn at 1e5 rows on this CPU")
    args = ap.parse_args()
    warnings.filterwarnings("ignore")
    ref = load_reference(args.reference)
    Capture = capturing_class(ref.GaussianMixture)
    ref.GaussianMixture = Capture
    for seed in range(20300, 20320):
        out = build(ref, Capture, seed)
        if out is not None:
            break
    else:
        raise SystemExit("no seed met the conditions")
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size <= 256 * 1024, size
    print("seed %d, train %d, test %d, n_iter %d, lower bound %.6f, %d bytes" % (seed, len(out["y_tr"]), len(out["y_te"]), out["n_iter"],
                                                                                out["lower_bound"], size))
    print("margins: convergence %.2e, decision %.3f" % (np.min(np.abs(np.abs(out["changes"]) - out["tol"])),
                                                       np.min(np.diff(np.sort(out["y_prob"], axis=1))[:, -1])))
    print("sens (weights, means, covariances, lower bound, y_prob):", out["sens"])
    print("lower bound over 10 seeds %s, accuracy %s, accuracy of the fixture %.4f" % (out["lb_range"], out["acc_range"],
                                                                                    (out["y_pred"] == out["y_te"]).mean()))
    if args.time:
        fit, it, pp = time_sklearn()
        print("scikit-learn on this CPU, 1e5 x 4, %d components: fit %.2f s (%d iterations), predict_proba %.3f s" % (K, fit, it, pp))


if __name__ == "__main__":
    sys.exit(main())
