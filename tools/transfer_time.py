#!/usr/bin/env python3
"""Wall time of pypevoc_amd.TransferFunctions.transferogram (k_xspec.hip) on 60 s of a 44.1 kHz source / target pair, float32:
the reference's default durations (sample_duration 0.5 s, window_duration 0.125 s: NFFT 4096, hop 2048, 9 segments a block;
always the rows route) and two fused geometries (window_duration 0.03 s: NFFT 1024, hop 512, 42 segments a block; 0.06 s: NFFT
2048, hop 1024, 20 segments a block; the fused route and, PVX_XSPEC_ROWS=1, the rows route), each at delta_time 1 s (60 blocks) and 0.01 s (about 5 950 blocks), from host
arrays and from device-resident tensors.  After a warm-up call per case, --reps timed calls, each ending synchronised (the
results are host arrays): prints one JSON line per case with the median, the best and the spread (max - min); --out appends
them to a file (profiles/transfer_time.jsonl).  TRANSFER.md records the numbers."""
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
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    from pypevoc_amd import TransferFunctions as tf
    sr = 44100
    src, tgt = pair(sr, a.duration)
    dsrc, dtgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    lines = []
    for nfft, window_duration, routes in ((4096, .125, ("default",)), (1024, .03, ("fused", "rows")), (2048, .06, ("fused", "rows"))):
        for delta in [float(d) for d in a.deltas.split(",")]:
            for route in routes:
                if route == "rows":
                    os.environ["PVX_XSPEC_ROWS"] = "1"
                else:
                    os.environ.pop("PVX_XSPEC_ROWS", None)
                for where, s, t in (("host", src, tgt), ("device", dsrc, dtgt)):
                    call = lambda: tf.transferogram(s, t, rate=sr, delta_time=delta, window_duration=window_duration)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r = call()                                        # first call: workspace growth, code objects, a rocFFT plan
                    first = time.perf_counter() - t0
                    kernels = tf.last_kernels()
                    assert tf.window_geometry(sr, window_duration)[0] == nfft
                    ts = []
                    for _ in range(a.reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        r = call()
                        ts.append(time.perf_counter() - t0)
                    lines.append(json.dumps({"nfft": nfft, "delta_time": delta, "dur_s": a.duration, "input": where, "kernels": kernels,
                                             "blocks": int(r[0].shape[1]), "first_ms": 1e3 * first, "median_ms": 1e3 * float(np.median(ts)),
                                             "best_ms": 1e3 * min(ts), "spread_ms": 1e3 * (max(ts) - min(ts)), "reps": a.reps}))
                    print(lines[-1], flush=True)
            os.environ.pop("PVX_XSPEC_ROWS", None)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
