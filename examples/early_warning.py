"""Early-warning index end to end on the device: train briefly on a synthetic recording with twelve fault segments, assemble
the results array on the device, estimate mu / sigma on the normal rows, evaluate every (current, fault class) condition in
one call, and replay the recording through the online monitor.

    python examples/early_warning.py [--rows 6000] [--fault-rows 600] [--epochs 3000] [--calibrate]

With --calibrate a small grid of RF parameter sets is swept over all conditions and the normal rows in one device call, and the
set with the longest worst-case lead that stays silent on the normal rows is printed with its table.

The synthetic recording has no current plateaus, so each condition here selects a fault class by its labels and accepts
any current; with a real recording use pinn_amd.risk.RF_CONDITIONS (108 / 270 / 405 A, +-0.5 A).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pinn_amd  # noqa: E402
from pinn_amd import risk, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--fault-rows", type=int, default=600)
    ap.add_argument("--epochs", type=int, default=3000)
    ap.add_argument("--mc-times", type=int, default=32)
    ap.add_argument("--calibrate", action="store_true", help="also sweep a small grid of RF parameter sets and print the chosen one")
    args = ap.parse_args()

    ds = synth.make_dataset(args.rows, (args.fault_rows,) * 12, seed=0)
    x_train, y_train, x_test, y_test, scaler_X, scaler_Y, info = ds
    torch.manual_seed(0)
    model = pinn_amd.PhysicsInformedNN(x_train, y_train, [8, 256, 256, 256, 1], scaler_X, scaler_Y, p=0.2, logvar=True, seed=1)
    model.verbose = False
    model.train_dnn(args.epochs)

    results = pinn_amd.create_comprehensive_results_array_v2(model, ds, mc_times=args.mc_times, dropout=0.2, device_output=True)
    mu, sigma = risk.estimate_mu_sigma_normal(results)
    print("mu   :", dict(zip(risk.RF_RES_KEYS, mu.cpu().numpy().round(6))))
    print("sigma:", dict(zip(risk.RF_RES_KEYS, sigma.cpu().numpy().round(6))))

    conditions = [(0.0, name, None) for name in risk.FAULT_RANGE_MAP]
    table = risk.rf_advance_for_conditions(results, mu, sigma, conditions, current_tol=float("inf"))
    print("\n%-22s %6s %12s %12s %10s" % ("fault class", "rows", "V alarm", "RF warning", "lead"))
    for (_, name, _), r in zip(conditions, table):
        print("%-22s %6d %12s %12s %10s" % (name, r["n"], r["idx_v_alarm"], r["idx_rf_warn"], r["delta_idx"]))
    print("(lead = voltage alarm index - RF warning index, in samples; positive: the RF warning comes first)")

    monitor = risk.RiskMonitor(mu, sigma)
    for s in range(0, x_test.shape[0], 1024):
        monitor.update_rows(model, x_test[s:s + 1024], y_test[s:s + 1024], scaler_X, scaler_Y)
    print("\nonline replay of %d rows in chunks of 1024: first warning at row %s, first danger at row %s, final (C, RF) = %s"
          % (monitor.n_seen, monitor.first_warning, monitor.first_danger, monitor.state))

    if args.calibrate:
        grid = risk.rf_grid(z_safe=[1.5, 2.0, 3.0], lambda_decay=[0.99, 0.9971, 1.0], alpha_smooth=[0.2, 1.0],
                            k_logistic=[5e-4, 2e-3], C0_logistic=[200.0, 500.0], warn_threshold=[0.25, 0.3])
        try:
            cal = risk.calibrate_rf(results, mu, sigma, grid, conditions, current_tol=float("inf"), require_all=False)
        except ValueError as e:
            print("\ncalibration over %d candidates: %s" % (len(grid["z_safe"]), e))
            return
        swept = {k: cal.params[k] for k in grid}
        print("\ncalibration over %d candidates: candidate %d, %s" % (cal.sweep.n_candidates, cal.index, swept))
        print("alarm rows on the %d normal rows: %d, peak RF there %.4f"
              % (sum(b - a for a, b in cal.sweep.quiet_ranges), cal.sweep.quiet_alarm_rows[cal.index], cal.sweep.quiet_peak[cal.index]))
        print("%-22s %6s %12s %12s %10s" % ("fault class", "rows", "V alarm", "RF warning", "lead"))
        for (_, name, _), r in zip(conditions, cal.table):
            print("%-22s %6d %12s %12s %10s" % (name, r["n"], r["idx_v_alarm"], r["idx_rf_warn"], r["delta_idx"]))


if __name__ == "__main__":
    main()
