#!/usr/bin/env python3
"""Wall time of PeriodSeries.calc() (k_period.hip) on 60 s and 600 s of 44.1 kHz harmonic audio, both methods, host
arrays in / out and a device-resident float64 tensor, defaults otherwise (nwind 2646, maxdelay 882, cand_method 'fft').
Prints one JSON line per case.  Kernel times: run it under

    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/period_time.py --reps 2

and read OUT/*/run_kernel_stats.csv (k_period<...>, k_period_fft, rocFFT).  PERIODICITY.md records the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def harmonic(sr, dur, seed=0):
    t = np.arange(int(sr * dur)) / float(sr)
    ph = 2 * np.pi * np.cumsum(220.0 * (1.0 + 0.03 * np.sin(2 * np.pi * 0.5 * t))) / sr
    return sum(0.5 / h * np.sin(h * ph) for h in range(1, 7)) + 0.001 * np.random.default_rng(seed).standard_normal(len(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--durations", default="60,600")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--methods", default="xcorr,amdf")
    a = ap.parse_args()
    import torch
    from pypevoc_amd import PeriodSeries
    sr = 44100
    for dur in [float(d) for d in a.durations.split(",")]:
        x = harmonic(sr, dur)
        xd = torch.from_numpy(x).cuda()
        for method in a.methods.split(","):
            for where, sig in (("host", x), ("device", xd)):
                ps = PeriodSeries(sig, sr=sr, method=method)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ps.calc()                                            # first call: the rocFFT plan of a new window length, workspace growth
                first = time.perf_counter() - t0
                ts = []
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ps.calc()
                    f0 = ps.get_f0()
                    ts.append(time.perf_counter() - t0)
                print(json.dumps({"dur_s": dur, "method": method, "input": where, "frames": len(f0),
                                  "voiced": float(np.mean(~np.isnan(f0))), "first_ms": 1e3 * first, "best_ms": 1e3 * min(ts),
                                  "median_ms": 1e3 * float(np.median(ts))}), flush=True)


if __name__ == "__main__":
    main()
