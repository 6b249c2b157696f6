#!/usr/bin/env python3
"""Generate the V*.npz golden vectors of glottal inverse filtering by IMPORTING the reference (pypevoc/speech/glottal.py:
iaif_ola :36-84, InverseFilter :143-246).

Run in the build container only (the reference never travels to the GPU box; scipy is needed here and nowhere else):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_glottal.py

What it takes to run the reference under scipy 1.15 (GLOTTAL.md); the functions themselves run unchanged:
  * pypevoc.speech imports only with scipy.signal.hamming = scipy.signal.windows.hamming set first;
  * InverseFilter hands firls its weights as the fourth positional argument, which scipy now takes by keyword only:
    scipy.signal.firls is wrapped to pass it on as `weight`.

Signals are float32-exact synthetic vowels (stored as float32, the int16 one as int16): a 120 Hz harmonic source with
vibrato through three or four two-pole resonators, over noise of 1e-3 of the peak.  Each file holds `cases`, a JSON list of
  {name, x: key of the signal, dtype: float32 | float64 | int16, slice: null | [start, stop], Fs,
   kw: keyword arguments of iaif_ola beyond Fs (wind_func by numpy name), nwind, nhop, tract_order, glottal_order: the
   values the call used}
and per case <name>_glot, _dglot, _vt, _gc (the four returns), _hpfilt_b, _winspos (wins > 0), _frames (up to three frame
numbers: first, middle, last) with InverseFilter.apply's _fg, _fdg, _fvt, _fgc of those frames, and _sens_glot,
_sens_dglot, _sens_vt, _sens_gc: the largest change of each return over 8 seeded reruns in which every lag of every lpc
call is perturbed by a uniform value within +-nwind * 2^-53 * r[0], the worst-case rounding of an nwind-term float64 dot
product (sum |v_i v_i+k| <= r[0]).  Data only.
"""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import scipy.linalg  # noqa: E402
import scipy.signal  # noqa: E402
import scipy.signal.windows  # noqa: E402

warnings.simplefilter("ignore")
scipy.signal.hamming = scipy.signal.windows.hamming
_firls = scipy.signal.firls


def firls_positional_weight(numtaps, bands, desired, weight=None, **kw):
    return _firls(numtaps, bands, desired, weight=weight, **kw)


scipy.signal.firls = firls_positional_weight

from pypevoc.speech import glottal as gl  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
RERUNS = 8
_lpc_red = gl.lpc_red


def perturbed_lpc(rng):
    def lpc(w, order, axis=-1):
        nsamp = w.shape[axis]
        r = np.correlate(w, w, 'full')[nsamp - 1:nsamp + order]
        r = r + rng.uniform(-1.0, 1.0, len(r)) * nsamp * 2.0**-53 * r[0]
        return scipy.linalg.solve_toeplitz(r[:-1], -r[1:])
    return lpc


def vowel(Fs, dur, seed, formants=((700, 90), (1200, 110), (2600, 140), (3500, 180))):
    n = int(round(Fs * dur))
    t = np.arange(n) / float(Fs)
    f0 = 120.0 * (1.0 + 0.02 * np.sin(2 * np.pi * 5.0 * t))
    ph = 2 * np.pi * np.cumsum(f0) / Fs
    src = np.zeros(n)
    h = 1
    while h * 125.0 < 0.45 * Fs:
        src += np.sin(h * ph) / h
        h += 1
    y = src
    for fc, bw in formants:
        if fc < 0.4 * Fs:
            r = np.exp(-np.pi * bw / Fs)
            y = scipy.signal.lfilter([1.0], [1.0, -2 * r * np.cos(2 * np.pi * fc / Fs), r * r], y)
    y = 0.5 * y / np.abs(y).max()
    y = y + 1e-3 * 0.5 * np.random.default_rng(seed).standard_normal(n)
    return y.astype(np.float32)


def case_signal(store, case):
    x = store[case["x"]]
    if case["dtype"] == "float64":
        x = x.astype(np.float64)
    if case["slice"]:
        x = x[case["slice"][0]:case["slice"][1]]
    assert str(x.dtype) == case["dtype"]
    return x


def run_case(store, name, xkey, dtype, Fs, kw, slc=None):
    case = dict(name=name, x=xkey, dtype=dtype, slice=slc, Fs=Fs, kw=dict(kw))
    x = case_signal(store, case)
    call = dict(kw)
    if "wind_func" in call:
        call["wind_func"] = getattr(np, call["wind_func"])
    gl.lpc_red = _lpc_red
    glot, dglot, vt, gc = gl.iaif_ola(x, Fs=Fs, **call)
    nwind = call.get("nwind") or int(np.round(25 / 1000 * Fs))
    nhop = call.get("nhop") or int(nwind / 5)
    pt = call.get("tract_order") if call.get("tract_order") is not None else 2 * int(np.round(Fs / 2000)) + 4
    pg = call.get("glottal_order") if call.get("glottal_order") is not None else 2 * int(np.round(Fs / 4000))
    n_it = call.get("n_it", 1)
    case.update(nwind=nwind, nhop=nhop, tract_order=pt, glottal_order=pg)
    inv = gl.InverseFilter(Fs=Fs, nwind=nwind, tract_order=pt, glottal_order=pg, leaky_integration=call.get("leaky_integration", 0.99))
    wind = call.get("wind_func", np.hanning)(nwind)
    wins = np.zeros(len(x))
    starts = list(range(0, max(len(x) - nwind, 0), nhop))
    for ist in starts:
        wins[ist:ist + nwind] += wind
    assert len(starts) == len(vt)
    frames = sorted(set([0, len(starts) // 2, len(starts) - 1])) if starts else []
    fr = [inv.apply(x[starts[q]:starts[q] + nwind], n_it=n_it) for q in frames]
    sens = dict(glot=0.0, dglot=0.0, vt=0.0, gc=0.0)
    for k in range(RERUNS if starts else 0):
        gl.lpc_red = perturbed_lpc(np.random.default_rng(1000 + k))
        out = gl.iaif_ola(x, Fs=Fs, **call)
        for key, a, b in zip(("glot", "dglot", "vt", "gc"), out, (glot, dglot, vt, gc)):
            sens[key] = max(sens[key], float(np.max(np.abs(a - b))))
    gl.lpc_red = _lpc_red
    store[name + "_glot"], store[name + "_dglot"], store[name + "_vt"], store[name + "_gc"] = glot, dglot, vt, gc
    store[name + "_hpfilt_b"] = inv.hpfilt_b
    store[name + "_winspos"] = wins > 0
    store[name + "_frames"] = np.array(frames, dtype=np.int64)
    store[name + "_fg"] = np.array([f[0] for f in fr]).reshape(len(frames), nwind)
    store[name + "_fdg"] = np.array([f[1] for f in fr]).reshape(len(frames), nwind)
    store[name + "_fvt"] = np.array([f[2] for f in fr]).reshape(len(frames), pt + 1)
    store[name + "_fgc"] = np.array([f[3] for f in fr]).reshape(len(frames), (pg if n_it else 1) + 1)
    for key, v in sens.items():
        store[name + "_sens_" + key] = np.float64(v)
    print("%-18s n %5d frames %3d nwind %4d taps %3d orders %2d/%2d n_it %d  sens glot %.2e dglot %.2e vt %.2e gc %.2e  peak |glot| %.2e"
          % (name, len(x), len(starts), nwind, len(inv.hpfilt_b), pt, pg, n_it, sens["glot"], sens["dglot"], sens["vt"], sens["gc"],
             np.abs(glot).max()))
    return case


def write(fname, store, cases):
    store["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, fname)
    np.savez(path, **store)
    print("%s: %d bytes" % (fname, os.path.getsize(path)))
    assert os.path.getsize(path) < 400000


def main():
    s = {"x11k": vowel(11025, 0.15, 1)}
    write("V1_11k.npz", s, [run_case(s, "v11k", "x11k", "float32", 11025, {}),
                            run_case(s, "v11k_w256_h100", "x11k", "float32", 11025, dict(nwind=256, nhop=100))])
    s = {"x22k": vowel(22050, 0.12, 2)}
    write("V2_22k.npz", s, [run_case(s, "v22k_it%d" % k, "x22k", "float32", 22050, dict(n_it=k)) for k in (0, 1, 2)])
    s = {"x44k": vowel(44100, 0.1, 3)}
    write("V3_44k.npz", s, [run_case(s, "v44k", "x44k", "float32", 44100, {})])
    x = vowel(11025, 0.1, 4)
    s = {"xe": x, "xe_i16": np.round(x.astype(np.float64) * 30000).astype(np.int16)}
    nw = int(np.round(25 / 1000 * 11025))
    write("V4_edges.npz", s, [run_case(s, "e_i16", "xe_i16", "int16", 11025, {}),
                              run_case(s, "e_f64", "xe", "float64", 11025, {}),
                              run_case(s, "e_noframe", "xe", "float32", 11025, {}, [0, nw]),
                              run_case(s, "e_oneframe", "xe", "float32", 11025, {}, [100, 100 + nw + 1]),
                              run_case(s, "e_hamming", "xe", "float32", 11025, dict(wind_func="hamming"))])


if __name__ == "__main__":
    main()
