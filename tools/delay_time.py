#!/usr/bin/env python3
"""Wall time of pypevoc_amd.delay (k_xcorr.hip) on 60 s of a 44.1 kHz source / target pair, float32 (the pair of
tools/transfer_time.py):
  maxdelwind     at its defaults (sample_duration 0.5 s: blocks of 22050 samples, P = 65536, always the FFT route) with
                 delta_time 1 s (60 blocks) and 0.01 s (about 5 950 blocks), from host arrays and from device-resident tensors;
  determineDelay at its default maxdel = 2**16 (two calls of one block, P = 2**17), host and device;
  xcorr_peaks    la = lv = 1024 and 2048 over 5 000 blocks (delta 512), on the direct route and, PVX_XCORR_FFT=1, the FFT
                 route, host and device: the numbers a later change of the route threshold needs.
After a warm-up call per case, --reps timed calls, each ending synchronised (the results are host arrays): prints one JSON line
per case with the median, the best and the spread (max - min); --out appends them to a file (profiles/delay_time.jsonl).
DELAY.md records the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pair(sr, dur, seed=0):
    rng = np.random.default_rng(seed)
    n = int(sr * dur)
    src = rng.standard_normal(n)
    tgt = np.convolve(src, [1.0, 0.5, 0.25, -0.2, 0.1])[:n] + 0.6 * rng.standard_normal(n)
    return src.astype(np.float32), tgt.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--duration", type=float, default=60.)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--deltas", default="1,0.01")
    ap.add_argument("--blocks", type=int, default=5000)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    from pypevoc_amd import delay
    sr = 44100
    src, tgt = pair(sr, a.duration)
    dsrc, dtgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    cases = []
    for delta in [float(d) for d in a.deltas.split(",")]:
        cases.append(("maxdelwind", dict(delta_time=delta), "default", lambda s, t, delta=delta: delay.maxdelwind(s, t, rate=sr, delta_time=delta)[0]))
    cases.append(("determineDelay", dict(maxdel=2**16), "default", lambda s, t: np.atleast_1d(delay.determineDelay(s, t))))
    for L in (1024, 2048):
        for route in ("direct", "fft"):
            cases.append(("xcorr_peaks", dict(la=L, lv=L, delta=512), route,
                          lambda s, t, L=L: delay.xcorr_peaks(t, s, L, L, 0, 512, a.blocks, detrend="linear")[0]))
    lines = []
    for func, params, route, call in cases:
        if route == "fft":
            os.environ["PVX_XCORR_FFT"] = "1"
        else:
            os.environ.pop("PVX_XCORR_FFT", None)
        for where, s, t in (("host", src, tgt), ("device", dsrc, dtgt)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = call(s, t)                                            # first call: workspace growth, code objects, rocFFT plans
            first = time.perf_counter() - t0
            kernels = delay.last_kernels()
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = call(s, t)
                ts.append(time.perf_counter() - t0)
            lines.append(json.dumps(dict(params, func=func, dur_s=a.duration, input=where, kernels=kernels, blocks=int(len(r)) if func != "determineDelay" else 2,
                                         first_ms=1e3 * first, median_ms=1e3 * float(np.median(ts)), best_ms=1e3 * min(ts),
                                         spread_ms=1e3 * (max(ts) - min(ts)), reps=a.reps)))
            print(lines[-1], flush=True)
    os.environ.pop("PVX_XCORR_FFT", None)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
