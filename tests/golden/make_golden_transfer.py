#!/usr/bin/env python3
"""Generate the X*.npz golden vectors of pypevoc_amd.TransferFunctions by IMPORTING the reference
(pypevoc/TransferFunctions.py: transferogram :112-185, tfe :21-26, and the psd / csd / cohere it takes from matplotlib.mlab)
and running its functions unchanged.

Run in the build container only (the reference never travels to the GPU box; matplotlib and scipy are needed here and
nowhere else):

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_transfer.py

(PYPEVOC_REFERENCE names the reference's checkout.)  transferogram's default window_hop=None makes noverlap a float, and mlab
raises TypeError for every input: every case passes window_hop.

Each file holds float32-exact signals (stored as float32, int16 ones as int16) and `cases`, a JSON list of
  {name, func: transferogram | tfe | csd | psd | cohere, x, y: keys of the signals in the function's own argument order
   (transferogram: source, target; y null: no second signal), dtype: float32 | float64 | int16, slice: null | [start, stop],
   kw: keyword arguments of the call (window: {"array": key} or {"callable": name of a numpy window}), raises: null | name of
   the exception the reference raises}.
Per case: transferogram <name>_resp, <name>_freq, <name>_times, <name>_coh; the others <name>_out, <name>_freq.
Signals: a noise or chirp source over a noise floor of 1e-3 of the peak, and that source through a short FIR plus independent
noise, so that the coherence spans roughly 0.5 .. 1; deliberate stretches of exact silence in X2.
Before a case is written the reference's result is compared with a plain float64 numpy restatement of mlab's formula: it must
be within 1e-11 in the scaled units of the tests (TRANSFER.md), so that no fixture is committed on which the reference itself
is marginal against the tests' bounds.  Data only.
"""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, os.environ.get("PYPEVOC_REFERENCE", "/root/reference"))

import numpy as np  # noqa: E402

warnings.simplefilter("ignore")

from pypevoc import TransferFunctions as tf  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SELF_BOUND = 1e-11
CAP = 385067
FIR = np.array([1.0, 0.5, 0.25, -0.2, 0.1])


def f32exact(x):
    return np.asarray(x, dtype=np.float32)


def pair(n, seed, kind="noise", sr=8000, g=0.6):
    """(source, target): target = source through FIR + g * independent noise; both float32-exact."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        src = rng.standard_normal(n)
        src /= np.abs(src).max()
    else:
        t = np.arange(n) / float(sr)
        src = np.sin(2 * np.pi * (100.0 * t + (0.45 * sr - 100.0) * t * t / (2 * t[-1])))
        src = src + 1e-3 * rng.standard_normal(n)                    # the noise floor
    src = f32exact(src)
    tgt = np.convolve(src.astype(np.float64), FIR)[:n] + g * np.std(src) * rng.standard_normal(n)
    return src, f32exact(tgt)


def window_of(spec, arrays):
    if spec is None:
        return None
    if "array" in spec:
        return arrays[spec["array"]].astype(np.float64)
    f = getattr(np, spec["callable"])
    return lambda x: f(len(x)) * x


def signal(key, case, arrays):
    if key is None:
        return None
    x = arrays[key]
    if case["dtype"] == "float64":
        x = x.astype(np.float64)
    if case.get("slice"):
        x = x[case["slice"][0]:case["slice"][1]]
    assert str(x.dtype) == case["dtype"]
    return x


# ---- float64 numpy restatement of mlab ---------------------------------------------------------------------------------
def np_spectra(x, y, nfft, step, wind):
    """Unscaled means over the segments of conj(Y) X, |X|^2, |Y|^2 of one block."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    nseg = (len(x) - nfft) // step + 1
    X = np.array([np.fft.rfft(x[s * step: s * step + nfft] * wind) for s in range(nseg)])
    Y = np.array([np.fft.rfft(y[s * step: s * step + nfft] * wind) for s in range(nseg)])
    return (np.conj(Y) * X).mean(axis=0), (np.abs(X)**2).mean(axis=0), (np.abs(Y)**2).mean(axis=0)


def density(s, nfft, fs, wind):
    c = np.full(nfft // 2 + 1, 2.0)
    c[0] = 1.0
    if not nfft % 2:
        c[-1] = 1.0
    return s * c / fs / (wind**2).sum()


def padded(x, nfft):
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([x, np.zeros(nfft - len(x))]) if len(x) < nfft else x


def worst(got, want, scale):
    """Largest |got - want| / scale over the entries with a positive scale; the others must agree as nan or as exact zeros."""
    got, want, scale = np.asarray(got), np.asarray(want), np.asarray(scale)
    assert got.shape == want.shape == scale.shape, (got.shape, want.shape, scale.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok] == 0, want[ok] == 0)
    with np.errstate(all="ignore"):
        live = ok & (scale > 0) & np.isfinite(scale)
    assert np.all(want[ok & ~live] == 0)
    return float(np.max(np.abs(got[live] - want[live]) / scale[live], initial=0.0))


def check_transferogram(case, arrays, resp, freq, times, coh):
    kw = case["kw"]
    rate = kw["rate"]
    src, tgt = signal(case["x"], case, arrays), signal(case["y"], case, arrays)
    nfft, step = tf.nextpow2(kw["window_duration"] * rate), tf.nextpow2(kw["window_hop"] * rate)
    wind = np.hanning(nfft)
    slen = int(kw["sample_duration"] * rate)
    n = len(src) if tgt is None else min(len(src), len(tgt))
    s0 = int(kw.get("start_time", 0.) * rate)
    i0 = np.arange(s0, n - s0 - slen, int(kw.get("delta_time", 1.) * rate))
    assert np.array_equal(times, (i0 + slen / 2) / float(rate)) and len(i0) > 0
    assert np.max(np.abs(freq - np.arange(nfft // 2 + 1) * rate / nfft)) <= 1e-12 * rate and freq[-1] > 0
    w = 0.0
    for j, i in enumerate(i0):
        a = src[i:i + slen]
        b = a if tgt is None else tgt[i:i + slen]
        sxy, sxx, syy = np_spectra(padded(a, nfft), padded(b, nfft), nfft, step, wind)
        pxy, pxx, pyy = (density(s, nfft, rate, wind) for s in (sxy, sxx, syy))
        with np.errstate(all="ignore"):
            if tgt is None:
                w = max(w, worst(resp[:, j], pxx, pxx))
            else:
                w = max(w, worst(resp[:, j], pxy / pxx, np.sqrt(pyy / pxx)), worst(coh[:, j], np.abs(pxy)**2 / (pxx * pyy), np.ones(len(pxx)) * (pxx * pyy > 0)))
    return w


def check_mlab(case, arrays, out):
    kw = case["kw"]
    nfft, fs, nov = kw["NFFT"], kw["Fs"], kw.get("noverlap", 0)
    x, y = signal(case["x"], case, arrays), signal(case["y"], case, arrays)
    win = window_of(kw.get("window"), arrays)
    wind = np.hanning(nfft) if win is None else (win if isinstance(win, np.ndarray) else win(np.ones(nfft)))
    a = padded(x, nfft)
    b = a if y is None else padded(y, nfft)
    # csd(a, b) = mean conj(A) B: np_spectra's first argument is the unconjugated one
    sba, sbb, saa = np_spectra(b, a, nfft, nfft - nov, wind)
    pab, paa, pbb = (density(s, nfft, fs, wind) for s in (sba, saa, sbb))
    with np.errstate(all="ignore"):
        if case["func"] == "psd":
            return worst(out, paa, paa)
        if case["func"] == "csd":
            return worst(out, pab, np.sqrt(paa * pbb))
        if case["func"] == "cohere":
            return worst(out, np.abs(pab)**2 / (paa * pbb), np.ones(len(paa)))
        # tfe(y = a, x = b) = csd(a, b) / psd(b)
        return worst(out, pab / pbb, np.sqrt(paa / pbb))


def run_cases(fname, arrays, cases):
    out = dict(arrays)
    for case in cases:
        kw = dict(case["kw"])
        if "window" in kw:
            kw["window"] = window_of(kw["window"], arrays)
        x, y = signal(case["x"], case, arrays), signal(case["y"], case, arrays)
        name = case["name"]
        if case.get("raises"):
            try:
                getattr(tf, case["func"])(x, y, **kw)
            except Exception as e:                                    # noqa: BLE001
                assert type(e).__name__ == case["raises"], (name, e)
            else:
                raise AssertionError("%s: the reference did not raise" % name)
            print("%-28s raises %s" % (name, case["raises"]))
            continue
        if case["func"] == "transferogram":
            resp, freq, times, coh = tf.transferogram(x, y, **kw)
            w = check_transferogram(case, arrays, resp, freq, times, coh)
            out[name + "_resp"], out[name + "_freq"], out[name + "_times"], out[name + "_coh"] = resp, freq, times, coh
            shape = resp.shape
        else:
            args = (x,) if case["func"] == "psd" else (x, y)
            res, freq = getattr(tf, case["func"])(*args, **kw)
            w = check_mlab(case, arrays, res)
            out[name + "_out"], out[name + "_freq"] = res, freq
            shape = res.shape
        assert w <= SELF_BOUND, (name, w)
        print("%-28s %-14s %-12s reference against float64 numpy %.1e" % (name, case["func"], shape, w))
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, fname + ".npz")
    np.savez(path, **out)
    size = os.path.getsize(path)
    assert size <= CAP, (fname, size)
    print("%s: %d bytes" % (fname, size))


def tcase(name, x, y, dtype="float32", sl=None, **kw):
    return dict(name=name, func="transferogram", x=x, y=y, dtype=dtype, slice=sl, kw=kw, raises=None)


def mcase(name, func, x, y, dtype="float32", sl=None, raises=None, **kw):
    return dict(name=name, func=func, x=x, y=y, dtype=dtype, slice=sl, kw=kw, raises=raises)


def main():
    # X1: the fused windows 512 and 1024.  t512: 15 overlapping blocks (more than the waves of a workgroup) of 7 segments at
    # step NFFT/4; t1024: nseg = 2 (L = 2 NFFT, noverlap 0), blocks with gaps, start_time > 0; t512_f64: float64 samples
    src, tgt = pair(16000, 11)
    run_cases("X1_fused", dict(src=src, tgt=tgt), [
        tcase("t512", "src", "tgt", sl=[0, 7000], rate=8000, delta_time=0.05, sample_duration=0.16, window_duration=0.064, window_hop=0.016),
        tcase("t1024_nseg2", "src", "tgt", rate=8000, start_time=0.1, delta_time=0.4, sample_duration=0.256, window_duration=0.128,
              window_hop=0.128),
        tcase("t512_f64_half", "src", "tgt", dtype="float64", sl=[3000, 9000], rate=8000, start_time=0.05, delta_time=0.3,
              sample_duration=0.2, window_duration=0.064, window_hop=0.032),
    ])
    # X2: 2048 (5 segments at step NFFT/2, overlapping blocks); silences: source, target, both silent for a block each;
    # target=None (psd; 1024 and blocks shorter than NFFT)
    src, tgt = pair(12000, 12)
    ss, st = pair(8192, 13)
    ss[1024:2048] = 0
    st[3072:4096] = 0
    ss[5120:6144] = 0
    st[5120:6144] = 0
    run_cases("X2_fused_edges", dict(src=src, tgt=tgt, sil_src=ss, sil_tgt=st), [
        tcase("t2048", "src", "tgt", rate=8000, delta_time=0.5, sample_duration=0.8, window_duration=0.256, window_hop=0.128),
        tcase("t512_silences", "sil_src", "sil_tgt", rate=8192, delta_time=0.125, sample_duration=0.125, window_duration=0.0625,
              window_hop=0.03125),
        tcase("t1024_psd", "src", None, sl=[0, 9000], rate=8000, start_time=0.1, delta_time=0.3, sample_duration=0.3,
              window_duration=0.128, window_hop=0.064),
        tcase("t512_psd_silences", "sil_src", None, rate=8192, delta_time=0.125, sample_duration=0.125, window_duration=0.0625,
              window_hop=0.015625),
        tcase("t1024_psd_short_blocks", "src", None, sl=[0, 4000], rate=8000, delta_time=0.1, sample_duration=0.1, window_duration=0.128,
              window_hop=0.064),
    ])
    # X3: the rows route.  4096 on an int16 pair; 256 on a chirp (step NFFT/4, 17 overlapping blocks; step NFFT/2 with gaps)
    s16, t16 = pair(22000, 14, sr=16000)
    t16 = t16 / np.abs(t16).max()
    i16 = dict(src16=np.round(s16 * 32000).astype(np.int16), tgt16=np.round(t16 * 32000).astype(np.int16))
    cs, ct = pair(6000, 15, kind="chirp")
    run_cases("X3_rows", dict(chirp_src=cs, chirp_tgt=ct, **i16), [
        tcase("t4096_int16", "src16", "tgt16", dtype="int16", rate=16000, delta_time=0.5, sample_duration=0.8, window_duration=0.3,
              window_hop=0.15),
        tcase("t512_int16", "src16", "tgt16", dtype="int16", sl=[1000, 9000], rate=16000, delta_time=0.1, sample_duration=0.1,
              window_duration=0.032, window_hop=0.016),
        tcase("t256", "chirp_src", "chirp_tgt", rate=8000, delta_time=0.04, sample_duration=0.072, window_duration=0.032, window_hop=0.008),
        tcase("t256_gaps", "chirp_src", "chirp_tgt", rate=8000, start_time=0.02, delta_time=0.2, sample_duration=0.1, window_duration=0.032,
              window_hop=0.016),
    ])
    # X4: mlab's functions themselves at NFFT 333, noverlap 100; an array and a callable window; a signal shorter than NFFT;
    # the ValueError of a signal shorter than 2 NFFT
    src, tgt = pair(4000, 16)
    rng = np.random.default_rng(17)
    warr = f32exact(0.2 + np.blackman(333) + 0.05 * rng.random(333))
    run_cases("X4_mlab", dict(src=src, tgt=tgt, warr=warr), [
        mcase("tfe333", "tfe", "tgt", "src", NFFT=333, Fs=8000, noverlap=100),
        mcase("csd333", "csd", "src", "tgt", NFFT=333, Fs=8000, noverlap=100),
        mcase("psd333", "psd", "src", None, NFFT=333, Fs=8000, noverlap=100),
        mcase("cohere333", "cohere", "src", "tgt", NFFT=333, Fs=8000, noverlap=100),
        mcase("tfe333_window_array", "tfe", "tgt", "src", NFFT=333, Fs=8000, noverlap=100, window={"array": "warr"}),
        mcase("csd512_window_callable", "csd", "src", "tgt", NFFT=512, Fs=2, noverlap=256, window={"callable": "hamming"}),
        mcase("cohere1024_f64", "cohere", "src", "tgt", dtype="float64", NFFT=1024, Fs=8000, noverlap=768),
        mcase("psd256_defaults", "psd", "src", None, sl=[0, 1000], NFFT=256, Fs=2),
        mcase("tfe512_short", "tfe", "tgt", "src", sl=[0, 300], NFFT=512, Fs=8000),
        mcase("psd333_short", "psd", "src", None, sl=[100, 200], NFFT=333, Fs=8000),
        mcase("cohere512_too_short", "cohere", "src", "tgt", sl=[0, 1000], raises="ValueError", NFFT=512, Fs=8000),
    ])


if __name__ == "__main__":
    main()
