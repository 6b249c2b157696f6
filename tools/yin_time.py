#!/usr/bin/env python3
"""Wall time of SoundUtils.f0yin (k_yin.hip) on 60 s and 600 s of 44.1 kHz harmonic audio at nwind 1024 / 2048 / 4096, hop
nwind / 2: host arrays in / out and a device-resident float64 tensor, best of --reps after a first call.  Beside each, k_period
with method 'amdf' (PeriodSeries, cand_method 'min', maxdelay nwind / 2) on the same window and the same frames: it runs
the same loop shape, so the two times per lag-sample (one |a - b| or (a - b)^2 accumulated) belong side by side.
Prints one JSON line per case.  Kernel times: run it under

    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/yin_time.py --reps 2

and read OUT/*/run_kernel_stats.csv (k_yin, k_period<...>).  YIN.md records the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.period_time import harmonic  # noqa: E402


def best_of(reps, fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()                                                       # first call: workspace growth, code object load
    first = time.perf_counter() - t0
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, first, min(ts), float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--durations", default="60,600")
    ap.add_argument("--nwinds", default="1024,2048,4096")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from pypevoc_amd import PeriodSeries
    from pypevoc_amd.SoundUtils import f0yin, yin_frames, yin_lags, yin_last_kernels
    sr = 44100
    for dur in [float(d) for d in a.durations.split(",")]:
        x = harmonic(sr, dur)
        xd = torch.from_numpy(x).cuda()
        for nwind in [int(n) for n in a.nwinds.split(",")]:
            hop, L = nwind // 2, nwind // 2
            starts, _ = yin_frames(len(x), sr, nwind, hop)
            lo, hi = yin_lags(nwind, sr)
            lag_samples = len(starts) * (hi + 1) * L                 # lags 1 .. hi + 1, L samples each
            for where, sig in (("host", x), ("device", xd)):
                (freq, _, conf), first, best, med = best_of(a.reps, lambda: f0yin(sig, sr, nwind=nwind, hop=hop))
                print(json.dumps({"what": "f0yin", "kernel": yin_last_kernels(), "dur_s": dur, "nwind": nwind, "input": where,
                                  "frames": len(freq), "median_f0": float(np.median(freq)), "mean_conf": float(np.mean(conf)),
                                  "lag_samples": lag_samples, "first_ms": 1e3 * first, "best_ms": 1e3 * best, "median_ms": 1e3 * med,
                                  "ps_per_lag_sample": 1e12 * best / lag_samples}), flush=True)
            # k_period, amdf: lags mindelay .. maxdelay for the candidates and nwind-1-maxdelay .. nwind-1 for the normaliser,
            # lag l summed over nwind - l samples
            centres = starts + nwind // 2
            md = nwind // 2
            lags = list(range(2, md)) + list(range(nwind - 1 - md, nwind))
            amdf_samples = len(starts) * sum(nwind - l for l in sorted(set(lags)))
            for where, sig in (("host", x), ("device", xd)):
                ps = PeriodSeries(sig, sr=sr, window=nwind, hop=hop, fmin=sr / float(md), fmax=None, method="amdf", cand_method="min")
                assert ps.maxdelay == md, (ps.maxdelay, md)
                res, first, best, med = best_of(a.reps, lambda: ps._run(centres))
                print(json.dumps({"what": "k_period amdf", "dur_s": dur, "nwind": nwind, "input": where, "frames": len(res["count"]),
                                  "lag_samples": amdf_samples, "first_ms": 1e3 * first, "best_ms": 1e3 * best, "median_ms": 1e3 * med,
                                  "ps_per_lag_sample": 1e12 * best / amdf_samples}), flush=True)


if __name__ == "__main__":
    main()
