#!/usr/bin/env python3
"""Wall time and link traffic of HeterodyneHarmonic on the shape of the reference's examples/phoneme_descriptors.py (44.1 kHz,
3 s, nharm 20, nwind 2048, nhop 512): the decomposition (one pvx_hetharm call) and resynth() (one pvx_hetharm_resynth call)
against what they replace, nharm calls of heterodyne() each fed a complex128 heterodyning signal built in numpy.  After a
warm-up, --reps timed calls each; one JSON line per path with the median, the best, the spread and the bytes that cross the
link per call (counted from the entry points' staging: inputs up, results down).  Kernel times: run it under

    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d OUT -o r --output-format csv -- python tools/hetharm_time.py --reps 2

and read OUT/*kernel_stats.csv.  HETHARM.md and profiles/hetharm_time.jsonl record the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "best_ms": 1e3 * min(ts), "spread_ms": 1e3 * (max(ts) - min(ts)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dur", type=float, default=3.0)
    ap.add_argument("--nharm", type=int, default=20)
    a = ap.parse_args()
    import pypevoc_amd
    sr, nwind, nhop, nharm = 44100, 2048, 512, a.nharm
    n = int(sr * a.dur)
    t = np.arange(n) / float(sr)
    f0 = 140.0 * (1.0 + 0.03 * np.sin(2 * np.pi * 0.7 * t))
    ph = 2 * np.pi * np.cumsum(f0) / sr
    x = sum(0.5 / h * np.cos(h * ph) for h in range(1, nharm)) + 0.001 * np.random.default_rng(0).standard_normal(n)
    kw = dict(sr=sr, f=f0, nharm=nharm, nwind=nwind, nhop=nhop)
    h = pypevoc_amd.HeterodyneHarmonic(x, **kw)
    nfr = h.ah.shape[0]
    shape = {"sr": sr, "nsamp": n, "nharm": nharm, "nwind": nwind, "nhop": nhop, "frames": nfr}

    def old():
        for k in range(nharm):
            pypevoc_amd.heterodyne(x, h.heterodyner_signal(k), h.wind, nhop)

    def old_resynth():
        tvec = np.arange(n) / sr
        y = np.zeros(n)
        for k in range(nharm):
            y += np.real(np.conj(h.heterodyner_signal(k)) * np.interp(tvec, h.th, h.ah[:, k]))
        return y

    rows = [
        ("extract_partials: pvx_hetharm", lambda: h.extract_partials(), 16 * n + 8 * nwind, 16 * nfr * nharm + 8 * nfr),
        ("extract_partials: %d x pvx_heterodyne + numpy hetsig" % nharm, old, nharm * (24 * n + 8 * nwind), nharm * 24 * nfr),
        ("resynth: pvx_hetharm_resynth", lambda: h.resynth(), 8 * n + 16 * nfr * nharm, 8 * n),
        ("resynth: numpy interp per harmonic", old_resynth, 0, 0),
    ]
    for name, fn, up, down in rows:
        r = dict(shape)
        r.update({"path": name, "bytes_to_device": up, "bytes_to_host": down})
        r.update(timed(fn, a.reps))
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
