#!/usr/bin/env python3
"""Wall time of pypevoc_amd.marks (k_marks.hip) on a 16 kHz, 150 Hz synthetic vowel at window_size 256 / 1024: one walk over
60 s, and 256 rows of 1 s in one launch; period_marks_corr and period_marks_peak; host arrays in / out and a device-resident
float64 tensor, best of --reps after a first call.  Prints one JSON line per case.  Kernel-alone times: run it under

    timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- python tools/marks_time.py --reps 2

and read OUT/*/run_kernel_trace.csv (k_marks_corr, k_marks_peak).  --reference PATH times the reference's own functions on
the CPU instead (no GPU needed; PATH is the reference's checkout), on --ref-seconds of the same signal.  MARKS.md records
the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SR = 16000


def vowel(seconds, f0=150.0, seed=0):
    n = int(seconds * SR)
    t = np.arange(n) / float(SR)
    fi = f0 * (1.0 + 0.02 * np.sin(2 * np.pi * 3.0 * t))
    ph = 2 * np.pi * np.cumsum(fi) / SR
    x = sum(0.4 / h * np.sin(h * ph + 0.3 * h) for h in range(1, 6)) + 1e-3 * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32).astype(np.float64)


def track(seconds):
    tf = np.arange(0.0, seconds + 0.01, 0.01)
    return tf, 150.0 * (1.0 + 0.02 * np.sin(2 * np.pi * 3.0 * tf))


def best_of(reps, fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    first = time.perf_counter() - t0
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, first, min(ts), float(np.median(ts))


def reference(path, seconds, windows, reps):
    sys.path.insert(0, path)
    if not hasattr(np, "RankWarning"):
        np.RankWarning = np.exceptions.RankWarning
    from pypevoc import Periodicity as per
    x = vowel(seconds)
    tf, f = track(seconds)
    for W in windows:
        marks, first, best, med = best_of(reps, lambda: per.period_marks_corr(x, sr=SR, tf=tf, f=f, window_size=W), lambda: None)
        print(json.dumps({"what": "reference period_marks_corr", "dur_s": seconds, "window": W, "marks": len(marks), "best_ms": 1e3 * best,
                          "ms_per_step": 1e3 * best / max(len(marks) - 1, 1)}), flush=True)
    (marks, _), first, best, med = best_of(reps, lambda: per.period_marks_peak(x, sr=SR, tf=tf, f=f), lambda: None)
    print(json.dumps({"what": "reference period_marks_peak", "dur_s": seconds, "marks": len(marks), "best_ms": 1e3 * best}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--windows", default="256,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--ref-seconds", type=float, default=1.0)
    a = ap.parse_args()
    windows = [int(w) for w in a.windows.split(",")]
    if a.reference:
        return reference(a.reference, a.ref_seconds, windows, a.reps)
    import torch
    from pypevoc_amd.marks import marks_last_kernels, period_marks_corr, period_marks_peak, period_marks_rows
    sync = torch.cuda.synchronize
    x = vowel(a.seconds)
    tf, f = track(a.seconds)
    xd = torch.from_numpy(x).cuda()
    nrow = a.rows                                                    # rows of 1 s spread over the signal (they may overlap)
    starts = (np.arange(nrow) * ((len(x) - SR) // max(nrow - 1, 1))).astype(np.int64)
    stops = starts + SR
    toff = starts / float(SR)
    for where, sig in (("host", x), ("device", xd)):
        for W in windows:
            marks, first, best, med = best_of(a.reps, lambda: period_marks_corr(sig, sr=SR, tf=tf, f=f, window_size=W), sync)
            print(json.dumps({"what": "period_marks_corr", "kernel": marks_last_kernels(), "dur_s": a.seconds, "window": W, "input": where,
                              "marks": len(marks), "first_ms": 1e3 * first, "best_ms": 1e3 * best, "median_ms": 1e3 * med,
                              "us_per_step": 1e6 * best / max(len(marks) - 1, 1)}), flush=True)
            res, first, best, med = best_of(a.reps, lambda: period_marks_rows(sig, starts, stops, sr=SR, tf=tf, f=f, method="corr", toff=toff,
                                                                              window_size=W), sync)
            n = int(res["count"].sum())
            print(json.dumps({"what": "period_marks_rows corr", "kernel": marks_last_kernels(), "rows": nrow, "row_s": 1.0, "window": W,
                              "input": where, "marks": n, "bad_rows": int((res["status"] != 0).sum()), "first_ms": 1e3 * first,
                              "best_ms": 1e3 * best, "median_ms": 1e3 * med, "us_per_step": 1e6 * best / max(n - nrow, 1)}), flush=True)
        (marks, _), first, best, med = best_of(a.reps, lambda: period_marks_peak(sig, sr=SR, tf=tf, f=f), sync)
        print(json.dumps({"what": "period_marks_peak", "kernel": marks_last_kernels(), "dur_s": a.seconds, "input": where, "marks": len(marks),
                          "first_ms": 1e3 * first, "best_ms": 1e3 * best, "median_ms": 1e3 * med}), flush=True)
        res, first, best, med = best_of(a.reps, lambda: period_marks_rows(sig, starts, stops, sr=SR, tf=tf, f=f, method="peak", toff=toff), sync)
        print(json.dumps({"what": "period_marks_rows peak", "kernel": marks_last_kernels(), "rows": nrow, "row_s": 1.0, "input": where,
                          "marks": int(res["count"].sum()), "bad_rows": int((res["status"] != 0).sum()), "first_ms": 1e3 * first,
                          "best_ms": 1e3 * best, "median_ms": 1e3 * med}), flush=True)


if __name__ == "__main__":
    main()
