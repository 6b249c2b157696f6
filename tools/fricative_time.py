#!/usr/bin/env python3
"""Wall time of pypevoc_amd.speech.fricatives.fricative_rows (k_fric.hip) on a recording's worth of windows: --rows windows (2 000)
of 1024 samples spread over 60 s of a 44.1 kHz float32 signal with nwind 1024 (what FricativeDataFromWav uses: one segment a
window; the fused route and, PVX_FRIC_ROWS=1, the rows route), the same windows at the reference's default nwind 256 (7 segments a
window; always the rows route) and windows of 4096 samples at nwind 2048 (3 segments; both routes), from a host array and from a
device-resident tensor.  After a warm-up call per case, --reps timed batches of --calls calls, each call ending synchronised (the
results are host arrays): prints one JSON line per case with the median, the best and the spread (max - min) of the batches' time
per call; --out appends them to a file.  FRICATIVES.md records the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--duration", type=float, default=60.)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    from pypevoc_amd.speech import fricatives as fr
    sr = 44100
    n = int(sr * a.duration)
    x = (np.random.default_rng(0).standard_normal(n) + 0.1).astype(np.float32)
    dx = torch.from_numpy(x).cuda()
    lines = []
    for length, nwind, routes in ((1024, 1024, ("fused", "rows")), (1024, 256, ("default",)), (4096, 2048, ("fused", "rows"))):
        starts = np.linspace(0, n - length, a.rows).astype(np.int64)
        for route in routes:
            if route == "rows":
                os.environ["PVX_FRIC_ROWS"] = "1"
            else:
                os.environ.pop("PVX_FRIC_ROWS", None)
            for where, s in (("host", x), ("device", dx)):
                call = lambda: fr.fricative_rows(s, starts, length, nwind, sr)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()                                                # first call: workspace growth, code objects, a rocFFT plan
                first = time.perf_counter() - t0
                kernels = fr.last_kernels()
                ts = []
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        call()
                    ts.append((time.perf_counter() - t0) / a.calls)
                lines.append(json.dumps({"length": length, "nwind": nwind, "rows": a.rows, "dur_s": a.duration, "input": where, "kernels": kernels,
                                         "first_ms": 1e3 * first, "median_ms": 1e3 * float(np.median(ts)), "best_ms": 1e3 * min(ts),
                                         "spread_ms": 1e3 * (max(ts) - min(ts)), "reps": a.reps, "calls": a.calls}))
                print(lines[-1], flush=True)
        os.environ.pop("PVX_FRIC_ROWS", None)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
