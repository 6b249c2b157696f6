#!/usr/bin/env python3
"""Generate the L*.npz golden vectors of the formant tracker by IMPORTING the reference (pypevoc/speech/SpeechAnalysis.py:
Formants :220-319, lpc :9-24, lpc2form :186-209).

Run in the build container only (the reference never travels to the GPU box; scipy is needed here and nowhere else):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_formants.py

pypevoc.speech imports only with scipy.signal.hamming = scipy.signal.windows.hamming set first (make_golden_glottal.py,
whose `vowel` generator and lag perturbation are reused); Formants itself runs unchanged.  It pre-emphasises its argument in
place, so every call gets a fresh float64 copy of the signal.

Each file holds `cases`, a JSON list of {name, x: key of the signal, dtype: float32 | float64 | int16 (what the device is
given; the reference is called on the float64 copy), slice, Fs, kw: keyword arguments of Formants beyond Fs, down, FsN,
nwind, hop, nframes, order}, and per case
  <name>_Time, _Form, _BandWidths   the three returns
  _taps      the filter of resample_poly (scipy.signal.firwin as resample_poly calls it; absent at down 1)
  _lpc       [frames][order]  what the reference's lpc returned per frame
  _roots     [frames][order]  np.roots([1, a]) per frame, in np.roots' order
  _sens_form, _sens_bw, _sens_roots   the largest change of Form, BandWidths and of the roots (in the order of
             tests/formants_refs.py: canon) over 8 seeded reruns in which every lag of every lpc call moves by a uniform
             value within +-nwind * 2^-53 * r[0] (make_golden_glottal.py: perturbed_lpc), over the stable frames
  _stable    [frames] bool: false where a rerun changes the frame's NaN pattern or its count of exactly-real roots, or where
             the frame has two or more roots at angle 0 (np.argsort's order among equal angles is eig's own)
Data only."""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402
import scipy.signal  # noqa: E402

import make_golden_glottal as mgg  # noqa: E402  (sets the scipy shims and the reference's path)
from pypevoc.speech import SpeechAnalysis as sa  # noqa: E402
from tests.formants_refs import canon  # noqa: E402

warnings.simplefilter("ignore")
RERUNS = 8
_lpc = sa.lpc


def recording_lpc(inner, rows):
    def lpc(w, order, axis=-1):
        a = inner(w, order)
        rows.append(a)
        return a
    return lpc


def run_once(x, Fs, kw, inner):
    rows = []
    sa.lpc = recording_lpc(inner, rows)
    try:
        out = sa.Formants(np.array(x, dtype=np.float64), Fs, **kw)
    finally:
        sa.lpc = _lpc
    order = kw.get("modelOrd", 10)
    a = np.array(rows).reshape(len(rows), order)
    roots = np.array([np.roots(np.concatenate(([1], r))) for r in a]).reshape(len(rows), order)
    return out, a, roots


def nreal(r):
    return int(np.sum(r.imag == 0))


def run_case(store, name, xkey, dtype, Fs, kw, slc=None):
    case = dict(name=name, x=xkey, dtype=dtype, slice=slc, Fs=Fs, kw=dict(kw))
    x = mgg.case_signal(store, case)
    (Time, Form, BW), a, roots = run_once(x, Fs, kw, _lpc)
    nfr, order = len(Time), kw.get("modelOrd", 10)
    down = int(Fs / kw.get("fMax", 5500) / 2)
    wLen = -(-len(x) // down)
    FsN = int(Fs * wLen / float(len(x)))
    case.update(down=down, FsN=FsN, nwind=int(round(FsN * kw.get("tWind", 0.025))), hop=int(round(FsN * kw.get("tHop", 0.0125))),
                nframes=nfr, order=order)
    assert len(a) == nfr and Form.shape == (nfr, int(order / 2))
    stable = np.array([np.sum((r.imag == 0) & (r.real >= 0)) < 2 for r in roots], dtype=bool).reshape(nfr)
    twoneg = sum(int(np.sum((r.imag == 0) & (r.real < 0)) >= 2) for r in roots)
    reruns = []
    for k in range(RERUNS if nfr else 0):
        (_, F2, B2), _, r2 = run_once(x, Fs, kw, mgg.perturbed_lpc(np.random.default_rng(2000 + k)))
        reruns.append((F2, B2, r2))
        for f in range(nfr):
            if not (np.array_equal(np.isnan(F2[f]), np.isnan(Form[f])) and np.array_equal(np.isnan(B2[f]), np.isnan(BW[f]))
                    and nreal(r2[f]) == nreal(roots[f])):
                stable[f] = False
    sens = dict(form=0.0, bw=0.0, roots=0.0)
    for F2, B2, r2 in reruns:
        for f in np.nonzero(stable)[0]:
            ok = ~np.isnan(Form[f])
            if ok.any():
                sens["form"] = max(sens["form"], float(np.max(np.abs(F2[f][ok] - Form[f][ok]))))
                sens["bw"] = max(sens["bw"], float(np.max(np.abs(B2[f][ok] - BW[f][ok]))))
            sens["roots"] = max(sens["roots"], float(np.max(np.abs(canon(r2[f]) - canon(roots[f])))))
    assert nfr == 0 or stable.mean() >= 0.95, (name, stable.mean())
    store[name + "_Time"], store[name + "_Form"], store[name + "_BandWidths"] = Time, Form, BW
    if down > 1:
        store[name + "_taps"] = scipy.signal.firwin(2 * 10 * down + 1, 1.0 / down, window=("kaiser", 5.0))
    store[name + "_lpc"], store[name + "_roots"], store[name + "_stable"] = a, roots, stable
    for key, v in sens.items():
        store[name + "_sens_" + key] = np.float64(v)
    print("%-12s n %6d Fs %5d down %d FsN %5d frames %3d order %2d  stable %.2f  real roots/frame %s  frames with two negative real roots %d  "
          "sens form %.2e bw %.2e roots %.2e" % (name, len(x), Fs, down, FsN, nfr, order, stable.mean() if nfr else 1.0,
                                                 sorted(set(nreal(r) for r in roots)), twoneg, sens["form"], sens["bw"], sens["roots"]))
    return case


def write(fname, store, cases):
    store["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, fname)
    np.savez(path, **store)
    print("%s: %d bytes" % (fname, os.path.getsize(path)))
    assert os.path.getsize(path) < 400000


def main():
    s = {"x44k": mgg.vowel(44100, 0.3, 11), "x22k": mgg.vowel(22050, 0.3, 12), "x11k": mgg.vowel(11025, 0.3, 13),
         "x16k": mgg.vowel(16000, 0.3, 14)}
    write("L1_rates.npz", s, [run_case(s, "a_44k", "x44k", "float64", 44100, {}),
                              run_case(s, "b_22k", "x22k", "float64", 22050, {}),
                              run_case(s, "c_11k", "x11k", "float64", 11025, {}),
                              run_case(s, "d_16k", "x16k", "float64", 16000, {})])
    x = mgg.vowel(22050, 0.3, 15)
    # five resonances: with the generator's four, an order-11 model without pre-emphasis has two roots on the positive real
    # axis in 12 of 21 frames, which the stability rule above excludes
    five = ((700, 90), (1200, 110), (2600, 140), (3500, 180), (4300, 200))
    s = {"x11k5": mgg.vowel(11025, 0.3, 13, formants=five), "xg": x, "xg_i16": np.round(x.astype(np.float64) * 30000).astype(np.int16)}
    write("L2_options.npz", s, [run_case(s, "e_nopre_o11", "x11k5", "float64", 11025, dict(hpFreq=0, modelOrd=11)),
                                run_case(s, "f_o16", "x11k5", "float64", 11025, dict(modelOrd=16, bwMax=1000)),
                                run_case(s, "g_f32", "xg", "float32", 22050, {}),
                                run_case(s, "g_i16", "xg_i16", "int16", 22050, {})])
    s = {"x11k": mgg.vowel(11025, 0.3, 13)}
    write("L3_edges.npz", s, [run_case(s, "h_oneframe", "x11k", "float64", 11025, {}, [200, 200 + 277 + 138]),
                              run_case(s, "i_noframe", "x11k", "float64", 11025, {}, [200, 200 + 300])])


if __name__ == "__main__":
    main()
