#!/usr/bin/env python3
"""Wall time of SpeechSegmenter.process + refine_all_all_bands (k_fbank.hip twice, k_seg_detect, k_seg_refine) on 60 s of a
seeded 16 kHz signal of sines, noise and near-silence (240 stretches of 0.25 s; the recipe of the U* fixtures), float32,
rough / fine windows 2048 / 256, from a host array and from a device-resident tensor.  A call takes well under a
millisecond, so a timed window is --calls calls back to back (each ends synchronised: its results are host arrays), after a
warm-up window; --reps windows.  One JSON line per case: per call, the median over the windows, the best and the spread
(max - min), the two stages apart, and the launches counted from last_kernels; --out appends the lines to a file
(profiles/segment_time.jsonl).  SEGMENT.md records the numbers.  Each case runs in a child process of its own under a
time limit, and the cases stop at the first that fails.

--reference DIR times the reference itself, once, on the same signal on this machine's CPU (no GPU is touched): DIR holds
the reference's `pypevoc` package; the shims it needs under today's scipy and numpy (scipy.signal.hamming, np.float) are
set first, as tests/golden/make_golden_segment.py sets them.  --machine words what the line says it ran on."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BANDS = [225., 1000., 2000., 4000.]


def segment_signal(sr, dur, seed, nseg):
    """Sines, noise and near-silence in stretches of dur / nseg seconds, never the same kind twice in a row."""
    rng = np.random.default_rng(seed)
    n = int(sr * dur)
    t = np.arange(n) / float(sr)
    x = np.zeros(n)
    edges = np.linspace(0, n, nseg + 1).astype(int)
    kind = -1
    for a, b in zip(edges[:-1], edges[1:]):
        kind = (kind + 1 + rng.integers(0, 2)) % 3
        if kind == 0:
            x[a:b] = rng.uniform(0.2, 0.6) * np.sin(2 * np.pi * rng.uniform(300., 3500.) * t[a:b] + rng.uniform(0, 6.28))
            x[a:b] += 1e-3 * rng.standard_normal(b - a)
        elif kind == 1:
            x[a:b] = rng.uniform(0.05, 0.3) * rng.standard_normal(b - a)
        else:
            x[a:b] = 1e-4 * rng.standard_normal(b - a)
    return np.asarray(x, dtype=np.float32)


def launches(kernels):
    return sum(len(k.split("+")) for k in kernels if k)


def one_case(where, dur, reps, calls):
    import torch
    from pypevoc_amd.speech import SpeechSegmenter
    sr = 16000.
    x = segment_signal(sr, dur, 1, int(dur * 4))
    sig = torch.from_numpy(x).cuda() if where == "device" else x
    sg = SpeechSegmenter(sr=sr, bands=BANDS)
    sg.set_signal(sig, sr)

    def window(n):
        """n calls back to back: (seconds in process, seconds in refine), and the last call's results."""
        tp = tr = 0.0
        torch.cuda.synchronize()
        for _ in range(n):
            t0 = time.perf_counter()
            seg = sg.process(sig)
            t1 = time.perf_counter()
            new = sg.refine_all_all_bands()
            t2 = time.perf_counter()
            tp += t1 - t0
            tr += t2 - t1
        return tp, tr, len(seg), new

    t0 = time.perf_counter()
    seg = sg.process(sig)                                             # first call: code objects, workspaces
    k1 = sg.last_kernels()
    new = sg.refine_all_all_bands()
    k2 = sg.last_kernels()
    first = time.perf_counter() - t0
    window(calls)                                                     # warm-up window
    ws = [window(calls) for _ in range(reps)]
    tot = [(a + b) / calls for a, b, *_ in ws]
    rec = {"measure": "SpeechSegmenter.process+refine_all_all_bands", "dur_s": dur, "sr": sr, "input": where, "rough_window": 2048,
           "fine_window": 256, "bands": len(sg.rough_fb.fb), "rough_frames": len(sg.detection_func) + 1, "fine_frames": len(sg.fine_time),
           "segments": len(seg), "segments_refined_finite": int(np.isfinite(new).sum()),
           "kernels_process": "+".join(k1), "kernels_refine": "+".join(k2),
           "launches_process": launches(k1), "launches_refine": launches(k2),
           "first_ms": 1e3 * first, "calls_per_window": calls, "windows": reps,
           "median_ms": 1e3 * float(np.median(tot)), "best_ms": 1e3 * min(tot), "spread_ms": 1e3 * (max(tot) - min(tot)),
           "process_median_ms": 1e3 * float(np.median([w[0] for w in ws])) / calls,
           "refine_median_ms": 1e3 * float(np.median([w[1] for w in ws])) / calls, "audio_s_per_s": dur / float(np.median(tot))}
    return json.dumps(rec)


def reference_case(refdir, dur, machine):
    """The reference's own process + refine_all_all_bands on the signal, once, on this machine's CPU."""
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
    mod = importlib.import_module("pypevoc.speech.SpeechSegmenter")
    sr = 16000.
    x = segment_signal(sr, dur, 1, int(dur * 4))
    sg = mod.SpeechSegmenter(sr=sr, bands=list(BANDS))
    sg.set_signal(x, sr)
    t0 = time.perf_counter()
    seg = sg.process(x)
    t1 = time.perf_counter()
    sg.refine_all_all_bands()
    t2 = time.perf_counter()
    return json.dumps({"measure": "reference SpeechSegmenter.process+refine_all_all_bands", "input": "reference",
                       "machine": machine,
                       "dur_s": dur, "sr": sr, "segments": len(seg), "process_s": t1 - t0, "refine_s": t2 - t1, "total_s": t2 - t0, "runs": 1})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--durations", default="60")
    ap.add_argument("--reps", type=int, default=9, help="timed windows per case")
    ap.add_argument("--calls", type=int, default=50, help="calls per timed window")
    ap.add_argument("--reference", default=None, metavar="DIR", help="time the reference's package under DIR instead, once, on the CPU")
    ap.add_argument("--machine", default="a CPU core of the build container, another machine than the MI355X's host",
                    help="what the reference line says it ran on")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--limit", type=int, default=240, help="seconds a case may take")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)  # child: 'host' or 'device'
    a = ap.parse_args()
    if a.case:
        print(one_case(a.case, float(a.durations), a.reps, a.calls), flush=True)
        return 0
    if a.reference:
        line = reference_case(a.reference, float(a.durations.split(",")[0]), a.machine)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        return 0
    lines = []
    for dur in a.durations.split(","):
        for case in ("host", "device"):
            r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--case", case,
                                "--durations", dur, "--reps", str(a.reps), "--calls", str(a.calls)], capture_output=True, text=True)
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
