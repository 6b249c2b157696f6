#!/usr/bin/env python3
"""Wall time of MelFilterBank(sr=44100).mfcc_and_mel (k_fbank.hip: nwind 1024, hop 441, 26 bands, DCT2) on 60 s and 600 s
of 44.1 kHz harmonic audio: float32 host array in, host arrays out, and a device-resident float32 tensor; with --rows
also the rows route (PVX_FBANK_ROWS=1: k_frames + rocFFT + k_fbank_rows).  After a warm-up call per case, --reps timed
calls, each ending synchronised (the results are host arrays): prints one JSON line per case with the median, the best and
the spread (max - min).  Kernel times and the launch count: run it under

    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/fbank_time.py --reps 2 --durations 60

and read OUT/*/run_kernel_stats.csv.  FILTERBANK.md records the numbers."""
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
    x = sum(0.5 / h * np.sin(h * ph) for h in range(1, 7)) + 0.001 * np.random.default_rng(seed).standard_normal(len(t))
    return x.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--durations", default="60,600")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mode", default="DCT2")
    ap.add_argument("--rows", action="store_true", help="time the rows route as well")
    a = ap.parse_args()
    import torch
    from pypevoc_amd import FFTFilters as ft
    sr = 44100.
    bank = ft.MelFilterBank(sr=sr)
    for dur in [float(d) for d in a.durations.split(",")]:
        x = harmonic(sr, dur)
        xd = torch.from_numpy(x).cuda()
        for route in (("fused", "rows") if a.rows else ("fused",)):
            if route == "rows":
                os.environ["PVX_FBANK_ROWS"] = "1"
            else:
                os.environ.pop("PVX_FBANK_ROWS", None)
            for where, sig in (("host", x), ("device", xd)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c, s, t = bank.mfcc_and_mel(sig, mode=a.mode)        # first call: workspace growth, code objects, a rocFFT plan
                first = time.perf_counter() - t0
                kernels = ft.last_kernels()
                ts = []
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    c, s, t = bank.mfcc_and_mel(sig, mode=a.mode)
                    ts.append(time.perf_counter() - t0)
                print(json.dumps({"dur_s": dur, "input": where, "kernels": kernels, "frames": len(t), "mode": a.mode,
                                  "first_ms": 1e3 * first, "median_ms": 1e3 * float(np.median(ts)), "best_ms": 1e3 * min(ts),
                                  "spread_ms": 1e3 * (max(ts) - min(ts)), "reps": a.reps,
                                  "audio_s_per_s": dur / float(np.median(ts))}), flush=True)
        os.environ.pop("PVX_FBANK_ROWS", None)


if __name__ == "__main__":
    main()
