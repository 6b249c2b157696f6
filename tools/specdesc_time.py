#!/usr/bin/env python3
"""Wall time of the windowed spectral measures (k_specdesc.hip) on 60 s of 44.1 kHz harmonic audio, float32: SpecCentWind and
SpecFlux at nwind 1024, hop 441 (the fused route; with --rows also the rows route, PVX_SPECDESC_ROWS=1) and SpectralMoments
(window 1102, hop 551: always the rows route), each from a host array and from a device-resident tensor.  After a warm-up
call per case, --reps timed calls, each ending synchronised (the results are host arrays): prints one JSON line per case
with the median, the best and the spread (max - min); --out appends them to a file (profiles/specdesc_time.jsonl).
SPECDESC.md records the numbers."""
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
    ap.add_argument("--durations", default="60")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", action="store_true", help="time the rows route of the fused window lengths as well")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    from pypevoc_amd import SoundUtils as su
    from pypevoc_amd.speech import SpeechAnalysis as sa
    sr = 44100.
    measures = [("SpecCentWind", lambda s: su.SpecCentWind(s, sr=sr, nwind=1024, nhop=441)[0], True),
                ("SpecFlux", lambda s: su.SpecFlux(s, sr=sr, nwind=1024, nhop=441)[0], True),
                ("SpectralMoments", lambda s: sa.Periodogram(s, sr)[0], False)]
    lines = []
    for dur in [float(d) for d in a.durations.split(",")]:
        x = harmonic(sr, dur)
        xd = torch.from_numpy(x).cuda()
        for name, call, has_fused in measures:
            for route in (("fused", "rows") if (a.rows and has_fused) else ("default",)):
                if route == "rows":
                    os.environ["PVX_SPECDESC_ROWS"] = "1"
                else:
                    os.environ.pop("PVX_SPECDESC_ROWS", None)
                for where, sig in (("host", x), ("device", xd)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r = call(sig)                                     # first call: workspace growth, code objects, a rocFFT plan
                    first = time.perf_counter() - t0
                    kernels = su.last_kernels()
                    ts = []
                    for _ in range(a.reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        r = call(sig)
                        ts.append(time.perf_counter() - t0)
                    lines.append(json.dumps({"measure": name, "dur_s": dur, "input": where, "kernels": kernels, "values": len(r),
                                             "first_ms": 1e3 * first, "median_ms": 1e3 * float(np.median(ts)), "best_ms": 1e3 * min(ts),
                                             "spread_ms": 1e3 * (max(ts) - min(ts)), "reps": a.reps,
                                             "audio_s_per_s": dur / float(np.median(ts))}))
                    print(lines[-1], flush=True)
            os.environ.pop("PVX_SPECDESC_ROWS", None)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
