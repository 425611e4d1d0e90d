"""RF(t) on the device against the host backend: time per call (device events, warmed up) and share of the HBM floor.
python tools/time_rf.py [N ...]   (default 100000 1000000 10000000)

Algorithmic bytes per row: the series call reads the 176-B results row once and moves 8 B per stored or re-read
value of S_tot, C, RF_inst, RF_smooth between its three row passes; the statistics call reads the row twice."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import _common as hh
from pinn_amd import risk

HBM = 6.3e12          # achievable bytes/s (MI355X, streaming reads)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


for N in (int(a) for a in (sys.argv[1:] or ["100000", "1000000", "10000000"])):
    dev = hh.dev()
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    arr = torch.zeros(N, 22, dtype=torch.float64, device=dev)
    amp = 1.0 + 2.2 * torch.sin(2 * np.pi * torch.arange(N, device=dev, dtype=torch.float64) / 90000.0) ** 2
    arr[:, 12:17] = torch.randn(N, 5, dtype=torch.float64, device=dev, generator=gen) * amp[:, None]
    arr[:, 8] = 3.4
    mu, sigma = torch.zeros(5, dtype=torch.float64, device=dev), torch.ones(5, dtype=torch.float64, device=dev)
    cfg = risk._Config()
    reps = 200 if N <= 100000 else (50 if N <= 1000000 else 10)
    cases = [
        ("rf_series, all four outputs", lambda: risk._device_series(arr, mu, sigma, cfg, want=("S_tot", "C", "RF_inst", "RF_smooth")), 176 + 6 * 8),
        ("rf_series, RF_smooth only", lambda: risk._device_series(arr, mu, sigma, cfg, want=("RF_smooth",)), 176 + 6 * 8),
        ("rf_stats (mu, sigma)", lambda: risk._device_stats(arr, cfg.cols, 17, (0,)), 2 * 176),
    ]
    rs = risk._device_series(arr, mu, sigma, cfg, want=("RF_smooth",))["RF_smooth"]
    cases.append(("first_alarm on RF_smooth", lambda: risk._device_first(rs, 0.3, "above"), 8))
    for name, fn, bytes_row in cases:
        t = timed(fn, reps)
        floor = bytes_row * N / HBM
        print("N=%d %-30s %9.1f us  %6.0f GB/s (%d B/row algorithmic), HBM floor %.1f us = %.0f %% of the time"
              % (N, name, t * 1e6, bytes_row * N / t / 1e9, bytes_row, floor * 1e6, 100 * floor / t), flush=True)
    if N <= 1000000:
        host = arr.cpu().numpy()
        t0 = time.perf_counter()
        risk.rf_series(host, np.zeros(5), np.ones(5), backend="host")
        th = time.perf_counter() - t0
        t0 = time.perf_counter()
        out = risk.rf_series(host, np.zeros(5), np.ones(5), backend="device")
        tu = time.perf_counter() - t0
        print("N=%d host backend (numpy, sequential loops) %.3f s; device backend from a host array, copies included %.3f s" % (N, th, tu), flush=True)
    # the monitor's usual chunk: one launch
    chunk = arr[:2048]
    mon = risk.RiskMonitor(mu, sigma)
    t = timed(lambda: mon.update(chunk), 200)
    print("N=%d RiskMonitor.update, 2048-row chunk (series + two alarm searches + latch) %.1f us per call" % (N, t * 1e6), flush=True)
    del arr, amp, rs
