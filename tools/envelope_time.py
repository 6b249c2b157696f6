#!/usr/bin/env python3
"""Wall time of Formants(full=True) (k_formant.hip, then k_lpcenv.hip: the LPC spectral envelope on 1024 points per frame, its
peaks and their refinement) against Formants(full=False) on 60 s of a 44.1 kHz synthetic vowel, float32, with the defaults
(decimation by 4, window 276, hop 138, order 10), from a host array and from a device-resident tensor.  After a warm-up call
per case, --reps timed calls, each ending synchronised (the results are host arrays): prints one JSON line per case with the
median, the best and the spread (max - min); --out appends them to a file (profiles/envelope_time.jsonl).  ENVELOPE.md
records the numbers.  Each case runs in a child process of its own under a time limit, and the cases stop at the first that
fails."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.glottal_time import vowel  # noqa: E402


def one_case(where, full, dur, reps):
    import torch
    from pypevoc_amd.speech import envelope, formants
    sr = 44100.
    x = vowel(sr, dur)
    sig = torch.from_numpy(x).cuda() if where == "device" else x
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = envelope.Formants(sig, sr, full=full)                         # first call: code objects, workspace
    first = time.perf_counter() - t0
    kernels = formants.last_kernels() + ("+" + envelope.last_kernels() if full else "")
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = envelope.Formants(sig, sr, full=full)
        ts.append(time.perf_counter() - t0)
    rec = {"measure": "Formants", "full": full, "dur_s": dur, "input": where, "kernels": kernels, "frames": len(r[0]),
           "formants_per_frame": float(np.mean(np.sum(~np.isnan(r[1]), axis=1))),
           "first_ms": 1e3 * first, "median_ms": 1e3 * float(np.median(ts)), "best_ms": 1e3 * min(ts),
           "spread_ms": 1e3 * (max(ts) - min(ts)), "reps": reps, "audio_s_per_s": dur / float(np.median(ts))}
    if full:
        rec["peaks_matched_per_frame"] = float(np.mean(np.sum(~np.isnan(r[3]), axis=1)))
    return json.dumps(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--durations", default="60")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--limit", type=int, default=240, help="seconds a case may take")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)  # child: 'host' or 'device', ':full' appended
    a = ap.parse_args()
    if a.case:
        where, _, full = a.case.partition(":")
        print(one_case(where, full == "full", float(a.durations), a.reps), flush=True)
        return 0
    lines = []
    for dur in a.durations.split(","):
        for case in ("host", "host:full", "device", "device:full"):
            r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--case", case,
                                "--durations", dur, "--reps", str(a.reps)], capture_output=True, text=True)
            if r.returncode != 0:                                     # nothing more is started on the GPU after a failure
                sys.stderr.write(r.stdout + r.stderr)
                return r.returncode
            lines.append(r.stdout.strip().splitlines()[-1])
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
