#!/usr/bin/env python3
"""Wall time of glottal inverse filtering (k_iaif.hip) on 60 s of a 44.1 kHz synthetic vowel, float32: iaif_ola with its
defaults (window 1102, hop 220, 827 taps, orders 48 / 22, one iteration), from a host array and from a device-resident
tensor.  After a warm-up call per case, --reps timed calls, each ending synchronised (the results are host arrays): prints
one JSON line per case with the median, the best and the spread (max - min); --out appends them to a file
(profiles/glottal_time.jsonl).  GLOTTAL.md records the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def vowel(sr, dur, seed=0):
    """A 120 Hz harmonic source with vibrato through three two-pole resonators, over noise of 1e-3 of the peak."""
    n = int(sr * dur)
    t = np.arange(n) / float(sr)
    ph = 2 * np.pi * np.cumsum(120.0 * (1.0 + 0.02 * np.sin(2 * np.pi * 5.0 * t))) / sr
    y = sum(np.sin(h * ph) / h for h in range(1, 40))
    for fc, bw in ((700, 90), (1200, 110), (2600, 140)):
        r = np.exp(-np.pi * bw / sr)
        a1, a2 = -2 * r * np.cos(2 * np.pi * fc / sr), r * r
        out, p1, p2 = np.empty(n), 0.0, 0.0                         # y[i] = x[i] - a1 y[i-1] - a2 y[i-2]: numpy only, ~2 s per resonator
        for i, v in enumerate(y.tolist()):
            p1, p2 = v - a1 * p1 - a2 * p2, p1
            out[i] = p1
        y = out
    y = 0.5 * y / np.abs(y).max()
    return (y + 5e-4 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--durations", default="60")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    from pypevoc_amd.speech import glottal
    sr = 44100.
    lines = []
    for dur in [float(d) for d in a.durations.split(",")]:
        x = vowel(sr, dur)
        xd = torch.from_numpy(x).cuda()
        for where, sig in (("host", x), ("device", xd)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = glottal.iaif_ola(sig, Fs=sr)                          # first call: code objects, workspace
            first = time.perf_counter() - t0
            kernels = glottal.last_kernels()
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = glottal.iaif_ola(sig, Fs=sr)
                ts.append(time.perf_counter() - t0)
            lines.append(json.dumps({"measure": "iaif_ola", "dur_s": dur, "input": where, "kernels": kernels, "frames": len(r[2]),
                                     "first_ms": 1e3 * first, "median_ms": 1e3 * float(np.median(ts)), "best_ms": 1e3 * min(ts),
                                     "spread_ms": 1e3 * (max(ts) - min(ts)), "reps": a.reps,
                                     "audio_s_per_s": dur / float(np.median(ts))}))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
