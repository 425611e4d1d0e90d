"""MC-dropout or a deep ensemble: whose standard deviations are more honest?  On the synthetic recording of
examples/uncertainty_check.py (twelve fault segments): train the MC-dropout model and an ensemble of E networks (all members in
the launches of one), build both results arrays on the device -- the ensemble's through the `ensemble=` keyword, so columns
9-11 come from its members and the residual columns stay the model's -- and print score_uncertainty's coverage, nll, scale and
miscalibration area side by side, for the normal rows and for every fault group.

    python examples/ensemble_uncertainty.py [--rows 6000] [--fault-rows 600] [--epochs 3000] [--members 8] [--rule mc]

The ensemble runs on the any-width kernels (exact fp32) whatever its layers list; `--layers` gives it a smaller net than the
MC-dropout model's [8, 256, 256, 256, 1] if wanted.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pinn_amd  # noqa: E402
from pinn_amd import risk, synth, uncertainty  # noqa: E402


class _Rule:
    """DeepEnsemble with predict()'s rule fixed (the results array calls predict without one)."""

    def __init__(self, ens, rule):
        self.ens, self.rule = ens, rule

    def predict(self, X, device_output=False):
        return self.ens.predict(X, rule=self.rule, device_output=device_output)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--fault-rows", type=int, default=600)
    ap.add_argument("--epochs", type=int, default=3000)
    ap.add_argument("--mc-times", type=int, default=32)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--layers", default="8,256,256,256,1")
    ap.add_argument("--rule", default="mc", choices=("mc", "mixture"))
    args = ap.parse_args()
    layers = [int(v) for v in args.layers.split(",")]

    ds = synth.make_dataset(args.rows, (args.fault_rows,) * 12, seed=0)
    torch.manual_seed(0)
    model = pinn_amd.PhysicsInformedNN(ds[0], ds[1], [8, 256, 256, 256, 1], ds[4], ds[5], p=0.2, logvar=True, seed=1)
    model.verbose = False
    model.train_dnn(args.epochs)
    ens = pinn_amd.DeepEnsemble(layers, args.members, p=0.2, seed=100)
    ens.verbose = False
    ens.fit(ds[0], ds[1], args.epochs)
    print("MC-dropout model: final loss %.3e; ensemble of %d: final loss mean %.3e, worst member %.3e"
          % (model.last_loss, args.members, ens.last_loss.mean(), ens.last_loss.max()))

    arrays = {
        "MC-dropout": pinn_amd.create_comprehensive_results_array_v2(model, ds, mc_times=args.mc_times, dropout=0.2, device_output=True),
        "ensemble": pinn_amd.create_comprehensive_results_array_v2(model, ds, device_output=True, ensemble=_Rule(ens, args.rule)),
    }
    groups = dict(normal=list(risk.NORMAL_LABELS), **{k: list(v) for k, v in risk.FAULT_RANGE_MAP.items()})
    reports = {name: uncertainty.score_uncertainty(a, groups=groups) for name, a in arrays.items()}
    levels = reports["ensemble"]["normal"].levels
    print("\n%-22s %-11s %7s %9s %8s %9s %9s   coverage at %s" % ("group", "source", "rows", "rmse", "scale", "nll", "miscal.", levels))
    for g in groups:
        for name, rep in reports.items():
            r = rep[g]
            print("%-22s %-11s %7d %9.4g %8.3f %9.4g %9.4f   %s" % (g, name, r.n, r.rmse, r.scale, r.nll, r.miscalibration,
                                                                   r.coverage.round(3).tolist()))
    print("\nscale is what s = sqrt(ale^2 + epi^2) should be multiplied by (1 = calibrated); the miscalibration area is 0 for a "
          "calibrated law.  Columns 13-21 of the two arrays are byte-equal: %s"
          % bool(torch.equal(arrays["MC-dropout"][:, 13:], arrays["ensemble"][:, 13:])))


if __name__ == "__main__":
    main()
