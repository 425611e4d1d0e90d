"""Per-stage-kind averages of the physics-stage kernels of bench.py's timed steps, from a rocprofv3 kernel trace (csv)."""
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
def pick(sub):
    return [r for r in rows if sub in r["Kernel_Name"]]
kinds = ["V (lambda_PM)", "V (lambda_F)", "T", "H", "O"]
total = 0.0
for name in ("residuals_cached_kernel", "sums_finalize<double>", "lambda_step_kernel"):   # (the finalize was residuals_finalize in traces before profiles/r10)
    k = pick(name)
    assert len(k) % 5 == 0 and len(k) >= 5 * steps, (name, len(k))
    k = k[-5 * steps:]                       # the timed steps: five launches each, in bench.py's stage order
    for i, kind in enumerate(kinds):
        d = [dur(r) for r in k[i::5]]
        total += sum(d) / len(d)
        print("%-26s %-14s n %3d  avg %7.2f us  min %7.2f  max %7.2f   %s" % (name, kind, len(d), sum(d) / len(d), min(d), max(d), k[i]["Kernel_Name"][:70]))
print("sum over the 15 physics-stage launches of a step: %.1f us" % total)
for name in ("train_fwd_x3_kernel", "train_bwd_kernel", "wgrad_p_kernel"):
    k = pick(name)
    per = len(k) // (len(pick("train_bwd_kernel")) or 1)
    k = k[-per * steps:]
    d = [dur(r) for r in k]
    print("%-26s n %3d  avg %8.2f us  min %8.2f  max %8.2f  (per step %.1f us)" % (name, len(d), sum(d) / len(d), min(d), max(d), sum(d) / steps))
