#!/usr/bin/env python3
"""Generate the Y*.npz golden vectors of pypevoc_amd.delay by IMPORTING the reference (pypevoc/TransferFunctions.py:
maxdelwind :199-244, block_delay :188-196, determineDelay :80-109) and running its three functions unchanged.

Run in the build container only (the reference never travels to the GPU box; scipy and matplotlib are needed here and nowhere
else):

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_delay.py

(PYPEVOC_REFERENCE names the reference's checkout.)

Each file holds float32-exact signals (stored as float32, int16 ones as int16) and `cases`, a JSON list:
  Y1_maxdelwind      {name, source, target: keys of the signals, dtype, slice: null | [start, stop], kw: the call's keywords}
                     -> <name>_delay, <name>_strength, <name>_times
  Y2_block_delay     {name, source, target, dtype, slice, window: null | name of a numpy window} -> <name>_lag, <name>_max
  Y3_determine_delay {name, source, target, dtype, slice, tslice: the target's own slice (null: `slice`), maxdel} -> <name>_delay
Signals: a seeded noise source, and that source delayed, through a short FIR, plus independent noise; an int16 pair; a 200 Hz
sine pair, so that the peaks repeat; stretches of exact silence; a slow ramp on a target.  The reference is given the
float32 signals widened to float64 (scipy's detrend works in the type it is given), the device the stored type.

The guard (a condition, not a measurement): a case is refused when a non-silent block's winning value -- |value| for
determineDelay -- exceeds any other lag's by less than 1e-6 norm(a') norm(v'), 500 times the bound on the device's values, so
that a correct device result cannot pick another lag and no block ever has to be left out of a test.  A case is also refused
when the reference's own correlation (scipy's detrend, np.correlate) is further than 1e-12 norm norm from the restatement of
tests/delay_refs.py, or when the reference's outputs are not what that restatement gives.  Data only.
"""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ.get("PYPEVOC_REFERENCE", "/root/reference"))

import numpy as np  # noqa: E402

warnings.simplefilter("ignore")

import scipy.signal as sig  # noqa: E402
from pypevoc import TransferFunctions as tf  # noqa: E402

import delay_refs as dr  # noqa: E402

CAP = 300000
FIR = np.array([1.0, 0.5, 0.25, -0.2, 0.1])


def f32exact(x):
    return np.asarray(x, dtype=np.float32)


def pair(n, seed, delay, g=0.3, gain=1.0):
    """(source, target): target = gain * (source delayed by `delay` samples, through FIR) + g * independent noise."""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(n)
    src /= np.abs(src).max()
    src = f32exact(src)
    d = np.concatenate([np.zeros(delay), src.astype(np.float64)])[:n]
    tgt = gain * np.convolve(d, FIR)[:n] + g * np.std(src) * rng.standard_normal(n)
    return src, f32exact(tgt)


def signal(key, case, arrays, which="slice"):
    x = arrays[key]
    if case["dtype"] == "float64":
        x = x.astype(np.float64)
    sl = case.get(which) or case.get("slice")
    if sl:
        x = x[sl[0]:sl[1]]
    assert str(x.dtype) == case["dtype"], (case["name"], x.dtype)
    return x


def wide(x):
    """What the reference is given: float32 samples as float64 (scipy's detrend would otherwise work in float32)."""
    return x.astype(np.float64) if x.dtype == np.float32 else x


def guard(name, r):
    live = r["scale"] > 0
    assert dr.guard_holds(r), (name, "guard", (r["margin"][live] / r["scale"][live]).min())
    return float((r["margin"][live] / r["scale"][live]).min()) if live.any() else np.inf


def self_check(name, ref_corr, r, b=0):
    scale = r["scale"][b]
    if scale == 0:
        assert not np.any(ref_corr), (name, b, "the reference's silent block is not exactly zero")
        return 0.0
    w = float(np.max(np.abs(ref_corr - r["corr"][b])) / scale)
    assert w <= dr.SELF_BOUND, (name, b, w)
    return w


def save(fname, arrays, out, cases):
    out = dict(arrays, **out)
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, fname + ".npz")
    np.savez(path, **out)
    size = os.path.getsize(path)
    assert size <= CAP, (fname, size)
    print("%s: %d bytes" % (fname, size))


def run_maxdelwind(fname, arrays, cases):
    out = {}
    for case in cases:
        name, kw = case["name"], case["kw"]
        src, tgt = signal(case["source"], case, arrays), signal(case["target"], case, arrays)
        delay, strength, times = tf.maxdelwind(wide(src), wide(tgt), **kw)
        d, s, t, r = dr.maxdelwind(src, tgt, **kw)
        assert np.array_equal(times, t) and delay.shape == d.shape == strength.shape, name
        m, w = np.inf, 0.0
        if r is not None:
            m = guard(name, r)
            rate = kw["rate"]
            sl, first = int(kw["sample_duration"] * rate), int(kw.get("start_time", 0.) * rate)
            i0 = np.arange(first, min(len(src), len(tgt)) - first - sl, int(kw.get("delta_time", 1.) * rate))
            assert len(i0) == len(times)
            for b, s0 in enumerate(i0):
                ref = np.correlate(sig.detrend(wide(tgt[s0:s0 + sl])), sig.detrend(wide(src[s0:s0 + sl])), "full")
                w = max(w, self_check(name, ref, r, b))
            assert np.array_equal(delay, d), (name, delay, d)
            assert np.all(np.abs(strength - s) <= dr.SELF_BOUND * r["scale"]), name
        out[name + "_delay"], out[name + "_strength"], out[name + "_times"] = delay, np.asarray(strength, dtype=np.float64), times
        print("%-22s %3d blocks  margin %.2e  reference against the restatement %.1e" % (name, len(times), m, w))
    save(fname, arrays, out, cases)


def run_block_delay(fname, arrays, cases):
    out = {}
    for case in cases:
        name = case["name"]
        src, tgt = signal(case["source"], case, arrays), signal(case["target"], case, arrays)
        window = None if case["window"] is None else getattr(np, case["window"])(len(src))
        lag, mx = tf.block_delay(wide(src), wide(tgt), window=window)
        l2, m2, r = dr.block_delay(src, tgt, window)
        m = guard(name, r)
        w = np.ones(len(src)) if window is None else window
        ws = self_check(name, np.correlate(w * src, w * tgt, "full"), r)
        assert int(lag) == l2 and abs(float(mx) - m2) <= dr.SELF_BOUND * max(r["scale"][0], 1e-300), (name, lag, l2)
        out[name + "_lag"], out[name + "_max"] = np.int64(lag), np.float64(mx)
        print("%-22s lag %6d  margin %.2e  reference against the restatement %.1e" % (name, lag, m, ws))
    save(fname, arrays, out, cases)


def run_determine_delay(fname, arrays, cases):
    out = {}
    for case in cases:
        name = case["name"]
        src, tgt = signal(case["source"], case, arrays), signal(case["target"], case, arrays, "tslice")
        delay = tf.determineDelay(wide(src), wide(tgt), maxdel=case["maxdel"])
        d2, rx, ry = dr.determine_delay(src, tgt, case["maxdel"])
        m = min(guard(name, rx), guard(name, ry))
        xd, yd = wide(src)[:case["maxdel"]], wide(tgt)[:case["maxdel"]]
        w = max(self_check(name, np.correlate(xd, xd, "full"), rx), self_check(name, np.correlate(yd, xd, "full"), ry))
        assert int(delay) == d2, (name, delay, d2)
        out[name + "_delay"] = np.int64(delay)
        print("%-22s delay %6d  margin %.2e  reference against the restatement %.1e" % (name, delay, m, w))
    save(fname, arrays, out, cases)


def mcase(name, source, target, dtype="float32", sl=None, **kw):
    return dict(name=name, source=source, target=target, dtype=dtype, slice=sl, kw=kw)


def main():
    # Y1: maxdelwind at rate 8000.  Blocks of 800 samples take the direct route, of 2400 the FFT route.
    src, tgt = pair(12000, 31, 37)
    ss, st = src[:8000].copy(), tgt[:8000].copy()
    ss[1600:2400] = 0                                                 # block 2 of blocks of 0.1 s every 0.1 s: a silent source ...
    st[3200:4000] = 0                                                 # ... block 4: a silent target ...
    ss[4800:5600] = 0
    st[4800:5600] = 0                                                 # ... block 6: both
    ramp = f32exact(tgt[:6000].astype(np.float64) + np.linspace(-3.0, 5.0, 6000))
    s16, t16 = pair(6000, 32, 11)
    t16 = t16 / np.abs(t16).max()
    t = np.arange(4000) / 8000.0
    rng = np.random.default_rng(33)
    sine_src = f32exact(np.sin(2 * np.pi * 200.0 * t) + 1e-3 * rng.standard_normal(4000))
    sine_tgt = f32exact(0.8 * np.sin(2 * np.pi * 200.0 * (t - 9 / 8000.0)) + 1e-3 * rng.standard_normal(4000))
    arrays = dict(src=src, tgt=tgt, sil_src=ss, sil_tgt=st, ramp_tgt=ramp, src16=np.round(s16 * 32000).astype(np.int16),
                  tgt16=np.round(t16 * 32000).astype(np.int16), sine_src=sine_src, sine_tgt=sine_tgt)
    run_maxdelwind("Y1_maxdelwind", arrays, [
        mcase("positive", "src", "tgt", sl=[0, 8000], rate=8000, delta_time=0.1, sample_duration=0.1),
        mcase("negative", "tgt", "src", sl=[0, 8000], rate=8000, delta_time=0.1, sample_duration=0.1),
        mcase("overlapping_start", "src", "tgt", rate=8000, start_time=0.25, delta_time=0.03, sample_duration=0.1),
        mcase("gaps_f64", "src", "tgt", dtype="float64", rate=8000, delta_time=0.35, sample_duration=0.064),
        mcase("silences", "sil_src", "sil_tgt", rate=8000, delta_time=0.1, sample_duration=0.1),
        mcase("ramp", "src", "ramp_tgt", sl=[0, 6000], rate=8000, delta_time=0.15, sample_duration=0.1),
        mcase("int16", "src16", "tgt16", dtype="int16", rate=8000, delta_time=0.1, sample_duration=0.12),
        mcase("sine", "sine_src", "sine_tgt", rate=8000, delta_time=0.05, sample_duration=0.1),
        mcase("long_blocks", "src", "tgt", rate=8000, delta_time=0.4, sample_duration=0.3),
        mcase("no_block", "src", "tgt", sl=[0, 700], rate=8000, delta_time=0.1, sample_duration=0.1),
    ])
    # Y2: block_delay.  Lengths 300 (direct) and 2049 (the first length of the FFT route), with and without a window
    src, tgt = pair(2049, 34, 5)
    s16, t16 = pair(300, 35, 3)
    t16 = t16 / np.abs(t16).max()
    arrays = dict(src=src, tgt=tgt, zeros=np.zeros(10, dtype=np.float32), src16=np.round(s16 * 32000).astype(np.int16),
                  tgt16=np.round(t16 * 32000).astype(np.int16))

    def bcase(name, source, target, dtype="float32", sl=None, window=None):
        return dict(name=name, source=source, target=target, dtype=dtype, slice=sl, window=window)
    run_block_delay("Y2_block_delay", arrays, [
        bcase("b300", "src", "tgt", sl=[0, 300]),
        bcase("b300_hanning", "src", "tgt", sl=[100, 400], window="hanning"),
        bcase("b300_identical", "src", "src", sl=[0, 300]),
        bcase("b300_swapped_f64", "tgt", "src", dtype="float64", sl=[0, 300]),
        bcase("b2049", "src", "tgt"),
        bcase("b2049_hanning", "src", "tgt", window="hanning"),
        bcase("b2049_identical", "tgt", "tgt"),
        bcase("b300_int16", "src16", "tgt16", dtype="int16"),
        bcase("zeros10", "zeros", "zeros"),
    ])
    # Y3: determineDelay.  A negated, delayed target (the abs); a target shorter than maxdel; maxdel larger than both; 2**14
    src, tgt = pair(20000, 36, 211, gain=-1.0)
    s2, t2 = pair(5000, 37, 64)
    arrays = dict(src=src, neg_tgt=tgt, src2=s2, tgt2=t2)

    def dcase(name, source, target, maxdel, dtype="float32", sl=None, tslice=None):
        return dict(name=name, source=source, target=target, dtype=dtype, slice=sl, tslice=tslice, maxdel=maxdel)
    run_determine_delay("Y3_determine_delay", arrays, [
        dcase("negated_3000", "src", "neg_tgt", 3000, sl=[0, 4000]),
        dcase("short_target", "src2", "tgt2", 4096, tslice=[0, 2000]),
        dcase("maxdel_beyond_both", "src2", "tgt2", 2**16),
        dcase("swapped_f64", "tgt2", "src2", 1500, dtype="float64"),
        dcase("maxdel_16384", "src", "neg_tgt", 2**14),
    ])


if __name__ == "__main__":
    main()
