#!/usr/bin/env python3
"""Wall time of the pitch-jump detector (k_jumps.hip behind PV): JumpDetector.detect_pitch and detect_jumps +
calc_jump_params on a seeded 44.1 kHz glide of 343 frames (the recipe of the J* fixtures: five harmonics, 150 * 2^(1.2 t/T) Hz
with seven steps, 1e-3 noise; nfft 2048, hop 1024), float64 samples on the host, and jumps_rows on 1 / 64 / 1024 device rows of
that track.  A call is short, so a timed window is --calls calls back to back (each ends with host arrays), after a warm-up
window; --reps windows.  One JSON line per measure: per call, the median over the windows, the best and the spread
(max - min); --out appends the lines to a file (profiles/jumps_time.jsonl).  JUMPS.md records the numbers.  Each measure
runs in a child process of its own under a time limit, and the measures stop at the first that fails.

--reference DIR times the reference's detect_pitch and detect_jumps + calc_jump_params on the same signal, once, on this
machine's CPU (no GPU is touched): DIR holds the reference's `pypevoc` package; the shims it needs under today's scipy and
numpy are set first, as tests/golden/make_golden_jumps.py sets them.  --machine words what the line says it ran on."""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR, FRAMES = 44100, 343


def glide(sr, nsamp, seed, nsteps=7, noise=1e-3):
    rng = np.random.default_rng(seed)
    t = np.arange(nsamp) / float(sr)
    dur = nsamp / float(sr)
    f = 150.0 * 2.0**(1.2 * t / dur)
    for k in range(1, nsteps + 1):
        f[t >= dur * k / (nsteps + 1)] *= (1.12 if k % 2 else 0.9)
    ph = 2 * np.pi * np.cumsum(f) / sr
    x = sum(0.3 / h * np.sin(h * ph) for h in range(1, 6)) + noise * rng.standard_normal(nsamp)
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def signal():
    return glide(SR, 2048 + (FRAMES - 1) * 1024 + 1, 1)                # FRAMES frames at nfft 2048, hop 1024


def windows(fn, reps, calls):
    import torch
    t0 = time.perf_counter()
    fn()                                                              # first call: code objects, workspaces
    first = time.perf_counter() - t0

    def window():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        return (time.perf_counter() - t0) / calls

    window()                                                          # warm-up window
    ws = [window() for _ in range(reps)]
    return {"first_ms": 1e3 * first, "calls_per_window": calls, "windows": reps, "median_ms": 1e3 * float(np.median(ws)),
            "best_ms": 1e3 * min(ws), "spread_ms": 1e3 * (max(ws) - min(ws))}


def one_case(case, reps, calls):
    import torch
    from pypevoc_amd.speech.jumps import JumpDetector, jumps_rows
    x = signal()
    jd = JumpDetector()
    jd.detect_pitch(x, SR)
    rec = {"sr": SR, "frames": len(jd.t), "nfft": jd.nfft, "hop": jd.nhop}
    if case == "detect_pitch":
        rec.update(measure="JumpDetector.detect_pitch", input="host float64", **windows(lambda: jd.detect_pitch(x, SR), reps, calls))
    elif case == "detect_jumps":
        def stages():
            jd.detect_jumps()
            jd.calc_jump_params()
        rec.update(measure="JumpDetector.detect_jumps+calc_jump_params", launches=2, **windows(stages, reps, calls))
        rec["jumps"] = int(len(jd.up_jump_indices) + len(jd.down_jump_indices))
    else:
        rows = int(case)
        dev = torch.device("cuda")
        t = torch.from_numpy(np.tile(jd.t, (rows, 1))).to(dev)
        f0 = torch.from_numpy(np.tile(jd.f0, (rows, 1))).to(dev)
        mag = torch.from_numpy(np.tile(jd.mag, (rows, 1))).to(dev)
        out = {}

        def batch():
            out["r"] = jumps_rows(t, f0, mag)
        rec.update(measure="jumps_rows", input="device rows", rows=rows, launches=3, **windows(batch, reps, calls))
        rec["jumps_per_row"] = int(len(out["r"]["jump_times"][0]))
        rec["rows_per_s"] = rows / (rec["median_ms"] * 1e-3)
    return json.dumps(rec)


def reference_case(refdir, machine):
    import importlib
    import warnings
    import scipy.signal
    import scipy.signal.windows
    warnings.simplefilter("ignore")
    np.seterr(all="ignore")
    for name in ("hamming", "hanning", "hann", "blackman"):
        if not hasattr(scipy.signal, name) and hasattr(scipy.signal.windows, name):
            setattr(scipy.signal, name, getattr(scipy.signal.windows, name))
    if not hasattr(np, "float"):
        np.float = float
    sys.path.insert(0, refdir)
    mod = importlib.import_module("pypevoc.speech.PitchJumps")
    x = signal()
    jd = mod.JumpDetector()
    with contextlib.redirect_stdout(io.StringIO()):
        t0 = time.perf_counter()
        jd.detect_pitch(x, SR)
        t1 = time.perf_counter()
        jd.detect_jumps()
        jd.calc_jump_params()
        t2 = time.perf_counter()
    return json.dumps({"measure": "reference JumpDetector", "input": "reference", "machine": machine, "sr": SR, "frames": len(jd.t),
                       "jumps": int(len(jd.up_jump_indices) + len(jd.down_jump_indices)), "detect_pitch_s": t1 - t0,
                       "detect_jumps_calc_jump_params_s": t2 - t1, "runs": 1})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9, help="timed windows per measure")
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--reference", default=None, metavar="DIR", help="time the reference's package under DIR instead, once, on the CPU")
    ap.add_argument("--machine", default="a CPU core of the build container, another machine than the MI355X's host",
                    help="what the reference line says it ran on")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--limit", type=int, default=120, help="seconds a measure may take")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)  # child: 'detect_pitch', 'detect_jumps' or a number of rows
    a = ap.parse_args()
    if a.case:
        print(one_case(a.case, a.reps, a.calls), flush=True)
        return 0
    lines = []
    if a.reference:
        lines.append(reference_case(a.reference, a.machine))
        print(lines[-1], flush=True)
    else:
        for case in ("detect_pitch", "detect_jumps", "1", "64", "1024"):
            r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--case", case,
                                "--reps", str(a.reps), "--calls", str(a.calls)], capture_output=True, text=True)
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
