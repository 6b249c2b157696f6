#!/usr/bin/env python3
"""Generate the P*.npz golden vectors of the time-domain periodicity tracker by IMPORTING the reference
(pypevoc/Periodicity.py: PeriodSeries / PeriodTimeSeries, :251-506).

Run in the build container only (the reference never travels to the GPU box):

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_period.py [P9 ...]

(with names: only the fixtures that start with one of them are written).

The prefix is P: tests/conftest.py's golden_names() picks up every G* / H* file for the phase-vocoder
tests.  Each file holds one signal (float32-exact signals as float32; P6 reads G7's Perlman samples) and
one or more runs; `runs` is a JSON list of {name, ctor: PeriodSeries kwargs, window: null | int | "win_<name>",
mode: "calc" | "at_index" | "pbp", calc / pbp: kwargs, index}.  Per run and frame: the candidates padded with
NaN to ncand (<name>_period, <name>_strength), <name>_count, <name>_preferred (-1 for the reference's []),
<name>_index, and <name>_f0 = get_f0(), <name>_f0_05 = get_f0(0.5), <name>_times, <name>_strength_pref.
Data only.
"""
import json
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import io  # noqa: E402
import contextlib  # noqa: E402
import warnings  # noqa: E402

import numpy as np  # noqa: E402

warnings.simplefilter("ignore")

from pypevoc.Periodicity import PeriodTimeSeries  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
METHODS = ("xcorr", "amdf")
CAND = ("fft", "min", "similar")


def frames_of(pts, ncand):
    n = len(pts.periods)
    per = np.full((n, ncand), np.nan)
    st = np.full((n, ncand), np.nan)
    cnt = np.zeros(n, np.int32)
    pref = np.full(n, -1, np.int32)
    idx = np.zeros(n)
    for i, p in enumerate(pts.periods):
        c = len(p.cand_period)
        cnt[i] = c
        per[i, :c] = p.cand_period
        st[i, :c] = p.cand_strength
        pr = p.preferred
        pref[i] = -1 if (isinstance(pr, list) and len(pr) == 0) else int(pr)
        idx[i] = p.index
    return per, st, cnt, pref, idx


def run(x, name, ctor, window=None, mode="calc", calc=None, pbp=None, index=None, arrays=None):
    kw = dict(ctor)
    if isinstance(window, np.ndarray):
        arrays["win_" + name] = window
        kw["window"] = window
        wdesc = "win_" + name
    else:
        if window is not None:
            kw["window"] = window
        wdesc = window
    pts = PeriodTimeSeries(x, **kw)
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        if mode == "calc":
            pts.calc(**(calc or {}))
        elif mode == "pbp":
            pts.calcPeriodByPeriod(**(pbp or {}))
        else:
            pts.periods = [pts.per_at_index(index)]
    ncand = kw.get("ncand", 8)
    per, st, cnt, pref, idx = frames_of(pts, ncand)
    arrays[name + "_period"] = per
    arrays[name + "_strength"] = st
    arrays[name + "_count"] = cnt
    arrays[name + "_preferred"] = pref
    arrays[name + "_index"] = idx
    arrays[name + "_f0"] = pts.get_f0()
    arrays[name + "_f0_05"] = pts.get_f0(0.5)
    arrays[name + "_times"] = pts.get_times()
    arrays[name + "_strength_pref"] = pts.get_strength().astype(float)
    meta = {"name": name, "ctor": ctor, "window": wdesc, "mode": mode}
    if calc:
        meta["calc"] = calc
    if pbp is not None:
        meta["pbp"] = {k: (v if k != "tf" and k != "f" else k + "_" + name) for k, v in pbp.items()}
        for k in ("tf", "f"):
            if k in pbp:
                arrays[k + "_" + name] = np.asarray(pbp[k], dtype=float)
    if index is not None:
        meta["index"] = index
    return meta


def wanted(fname):
    """Every fixture, or only those whose names start with a command-line argument (`... make_golden_period.py P9`)."""
    return not sys.argv[1:] or fname.startswith(tuple(sys.argv[1:]))


def save(fname, x, sr, runs, arrays, x_store=None):
    if not wanted(fname):
        return
    out = dict(arrays)
    out["x"] = x.astype(np.float32) if x_store is None else x_store
    out["sr"] = np.float64(sr)
    out["runs"] = np.array(json.dumps(runs))
    np.savez_compressed(os.path.join(HERE, fname + ".npz"), **out)
    print(fname, len(runs), "runs", sum(int(v.sum()) for k, v in arrays.items() if k.endswith("_count")), "candidates")


def harmonic_vibrato(sr, dur, f0=220.0, nh=6, seed=0):
    t = np.arange(int(sr * dur)) / float(sr)
    fi = f0 * (1.0 + 0.02 * np.sin(2 * np.pi * 5.0 * t))
    ph = 2 * np.pi * np.cumsum(fi) / sr
    x = sum(0.5 / h * np.sin(h * ph) for h in range(1, nh + 1)) + 0.001 * np.random.default_rng(seed).standard_normal(len(t))
    return x.astype(np.float32).astype(np.float64)       # float32-exact: stored as float32


def main():
    sr = 44100
    # P1 -- harmonic vibrato, both methods x every cand_method, defaults
    x1 = harmonic_vibrato(sr, 1.0)
    arrays, runs = {}, []
    for m in METHODS:
        for c in CAND:
            runs.append(run(x1, "%s_%s" % (m, c), {"sr": sr, "method": m, "cand_method": c}, arrays=arrays))
    save("P1_harm_vibrato", x1, sr, runs, arrays)

    # P2 -- silence gaps and white noise: unvoiced frames, NaN f0, the 0/0 normaliser of an all-zero frame
    rng = np.random.default_rng(1)
    n2 = int(0.8 * sr)
    x2 = np.zeros(n2)
    x2[int(0.25 * sr):int(0.45 * sr)] = 0.3 * rng.standard_normal(int(0.45 * sr) - int(0.25 * sr))
    x2[int(0.6 * sr):] = harmonic_vibrato(sr, 0.2, f0=330.0, seed=2)[:n2 - int(0.6 * sr)]
    x2 = x2.astype(np.float32).astype(np.float64)
    arrays, runs = {}, []
    for m in METHODS:
        for c in CAND:
            runs.append(run(x2, "%s_%s" % (m, c), {"sr": sr, "method": m, "cand_method": c, "fmin": 100}, arrays=arrays))
    save("P2_silence_noise", x2, sr, runs, arrays)

    # P3 -- the reference's unit-test signals (tests/test_periodicity.py): 500 Hz at 48 kHz, per_at_index(2400.0);
    # gen_sin() defaults (440 Hz, 48 kHz, 4800 samples)
    x3 = np.sin(2. * np.pi * 500. / 48000 * np.arange(4800))
    arrays, runs = {}, []
    for m in METHODS:
        runs.append(run(x3, "sin500_" + m, {"sr": 48000, "method": m}, mode="at_index", index=2400.0, arrays=arrays))
    save("P3a_sin500", x3, 48000, runs, arrays, x_store=x3)
    x3b = np.sin(2. * np.pi * 440. / 48000 * np.arange(4800))
    arrays, runs = {}, []
    for m in METHODS:
        runs.append(run(x3b, "sin440_" + m, {"method": m}, mode="at_index", index=2400.0, arrays=arrays))
    save("P3b_gen_sin", x3b, 48000, runs, arrays, x_store=x3b)

    # P4 -- non-default parameters: hanning(2048), explicit hop, fmin / fmax, ncand, thresholds, calc(threshold=...)
    arrays, runs = {}, []
    x4 = x1[:int(0.6 * sr)]
    for m in METHODS:
        for c in CAND:
            ctor = {"sr": sr, "hop": 300, "fmin": 80, "fmax": 1000, "ncand": 3, "threshold": 0.5, "vthresh": 0.3,
                    "fftthresh": 0.2, "method": m, "cand_method": c}
            runs.append(run(x4, "%s_%s" % (m, c), ctor, window=np.hanning(2048), calc={"threshold": 0.6}, arrays=arrays))
    save("P4_nondefault", x4, sr, runs, arrays)

    # P5 -- a window shorter than maxdelay (882 at fmin 50): the clipped slices
    arrays, runs = {}, []
    x5 = x1[:int(0.3 * sr)]
    for m in METHODS:
        for c in CAND:
            runs.append(run(x5, "%s_%s" % (m, c), {"sr": sr, "method": m, "cand_method": c}, window=512, arrays=arrays))
    save("P5_short_window", x5, sr, runs, arrays)

    # P6 -- the Perlman violin excerpt (G7_perlman.npz's samples), fmax=None
    g7 = np.load(os.path.join(HERE, "G7_perlman.npz"))
    x6 = g7["x"] / g7["x_scale"]
    sr6 = float(g7["sr"])
    arrays, runs = {}, []
    for m in METHODS:
        runs.append(run(x6, "perlman_" + m, {"sr": sr6, "method": m, "fmax": None}, arrays=arrays))
    out = dict(arrays)
    out["sr"] = np.float64(sr6)
    out["x_from"] = np.array("G7_perlman")
    out["runs"] = np.array(json.dumps(runs))
    if wanted("P6_perlman"):
        np.savez_compressed(os.path.join(HERE, "P6_perlman.npz"), **out)
        print("P6_perlman", len(runs), "runs")

    # P8a -- a frame beyond the LDS (nwind 8192 > 6144) whose first negative correlation lag lies past maxdelay (960):
    # a 3 Hz swell under a 150 Hz tone, seen through a window whose first half is zero.  Frames where the swell is
    # monotonic have no negative lag at all (the zero half gives 0/0 = NaN beyond nwind/2): the mindelay fallback, voiced;
    # others find it past maxdelay: xcpos empty, unvoiced; the rest find it early.
    sr8 = 96000
    t8 = np.arange(int(0.5 * sr8)) / float(sr8)
    x8 = (np.sin(2 * np.pi * 3 * t8) + 0.15 * sum(np.sin(2 * np.pi * h * 150 * t8) / h for h in range(1, 4))).astype(np.float32).astype(np.float64)
    arrays, runs = {}, []
    for c in CAND:
        runs.append(run(x8, "halfwin_" + c, {"sr": sr8, "fmin": 100, "fmax": 1000, "cand_method": c},
                        window=np.r_[np.zeros(4096), np.ones(4096)], arrays=arrays))
    save("P8a_firstneg_past_maxdelay", x8, sr8, runs, arrays)

    # P8b -- the default window at fmin 40 Hz, 96 kHz: nwind 7200, beyond the LDS, both methods
    x8b = harmonic_vibrato(sr8, 0.5, f0=150.0)
    arrays, runs = {}, []
    for m in METHODS:
        runs.append(run(x8b, "global_" + m, {"sr": sr8, "fmin": 40, "method": m}, arrays=arrays))
    save("P8b_global_window", x8b, sr8, runs, arrays)

    # P7 -- calcPeriodByPeriod on P1's signal, with and without an f0 track
    arrays, runs = {}, []
    x7 = x1[:int(0.5 * sr)]
    runs.append(run(x7, "pbp", {"sr": sr}, mode="pbp", pbp={}, arrays=arrays))
    tf = np.linspace(0, len(x7) / sr, 11)
    f = 220.0 * (1.0 + 0.02 * np.sin(2 * np.pi * 5.0 * tf))
    runs.append(run(x7, "pbp_f", {"sr": sr}, mode="pbp", pbp={"tf": tf, "f": f}, arrays=arrays))
    runs.append(run(x7, "pbp_amdf_thr", {"sr": sr, "method": "amdf"}, mode="pbp", pbp={"threshold": 0.5}, arrays=arrays))
    save("P7_period_by_period", x7, sr, runs, arrays)

    # P9 -- the threshold cases PeakFinder documents and odd windows, 8 kHz, harmonics of a 220 Hz vibrato plus noise at 5 %
    # of the fundamental: threshold 0 (falls back to min(y)); threshold -1 < min(y) (th < 0: non-maxima are admitted with
    # score 0, lowest index first -- the only exact score ties); ncand 1 and 64; hanning(481), under which amdf's peaks stay
    # below 0.5, hence threshold 0.3; a 479-sample window with maxdelay 478 = nwind - 1 (no multiple of 4: the last lags
    # have one or two terms)
    sr9 = 8000
    t9 = np.arange(int(0.5 * sr9)) / float(sr9)
    ph9 = 2 * np.pi * np.cumsum(220.0 * (1.0 + 0.03 * np.sin(2 * np.pi * 3.0 * t9))) / sr9
    x9 = sum(0.5 / h * np.sin(h * ph9) for h in range(1, 7)) + 0.05 * 0.5 * np.random.default_rng(9).standard_normal(len(t9))
    x9 = x9.astype(np.float32).astype(np.float64)
    arrays, runs = {}, []
    base = {"sr": sr9, "fmax": 1000}
    for m in METHODS:
        for c in CAND:
            runs.append(run(x9, "thr0_%s_%s" % (m, c), dict(base, threshold=0, method=m, cand_method=c), arrays=arrays))
            runs.append(run(x9, "thneg_%s_%s" % (m, c), dict(base, threshold=-1.0, method=m, cand_method=c), arrays=arrays))
        # (one candidate, or the same candidates whatever cand_method: 'fft', whose bin count and row stride hold n / 2)
        runs.append(run(x9, "ncand1_" + m, dict(base, ncand=1, method=m), arrays=arrays))
        runs.append(run(x9, "ncand64_" + m, dict(base, ncand=64, method=m), arrays=arrays))
        runs.append(run(x9, "odd481_" + m, dict(base, threshold=0.3, method=m), window=np.hanning(481), arrays=arrays))
        runs.append(run(x9, "w479_" + m, dict(base, fmin=16.72, method=m), window=479, arrays=arrays))
    save("P9_thresholds_odd", x9, sr9, runs, arrays)


if __name__ == "__main__":
    main()
