#!/usr/bin/env python3
"""Generate the E*.npz golden vectors of the spectral-envelope half of the formant tracker by IMPORTING the reference
(pypevoc/speech/SpeechAnalysis.py: Formants(full=True) :298-311, lpc2form_full :211-218; pypevoc/PeakFinder.py: refine_all).

Run in the build container only, after make_golden_formants.py (the reference never travels to the GPU box; scipy is needed
here and nowhere else):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_envelope.py

The cases are those of L1_rates, L2_options and L3_edges (make_golden_formants.py, whose machinery is reused): an E case
names its L file and case, which hold the signal, the geometry, Form, BandWidths and the `_lpc` rows -- nothing is stored
twice.  This run must reproduce the L file's Form, BandWidths and `_lpc` bit for bit, or it stops.

Each file holds `cases`, a JSON list of {name, file: the L file, order, npts, FsN, nframes}, and per case
  <name>_Peaks, _Amplitudes   the fourth and fifth return of Formants(full=True)
  _npk  [frames]              the envelope's peaks per frame (PeakFinder on abs(freqz), 1024 points)
  _idx  [frames][order]       their integer indices, -1 beyond npk
  _pkF, _pkA [frames][order]  their refined frequencies and amplitudes (pks.pos, pks.val), NaN beyond npk
  _sens_peaks, _sens_amp, _sens_pkF, _sens_pkA   the largest absolute change of Peaks, Amplitudes, pkF and pkA over the 8
             seeded reruns of make_golden_formants.py (every lag of every lpc call perturbed), over the stable frames
  _stable    [frames] bool: false where the L file's `_stable` is, or where a rerun changes the frame's npk, its peak
             indices, the NaN pattern of Peaks / Amplitudes, or which peak a formant picks
At least 95 % of a case's frames must be stable.  Data only."""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_golden_formants as mgf  # noqa: E402  (sets the scipy shims and the reference's path)
from make_golden_formants import mgg, sa  # noqa: E402

warnings.simplefilter("ignore")
NPTS = 1024
_PeakFinder = sa.PeakFinder


def recording_peakfinder(rec):
    class Recording(_PeakFinder):
        def refine_all(self, *args, **kw):
            _PeakFinder.refine_all(self, *args, **kw)
            rec.append((np.array(self._idx, dtype=np.int64), np.array(self.pos, dtype=np.float64), np.array(self.val, dtype=np.float64)))
    return Recording


def run_full(x, Fs, kw, inner):
    """Formants(full=True) with every frame's lpc row and envelope peaks recorded."""
    rows, rec = [], []
    sa.lpc = mgf.recording_lpc(inner, rows)
    sa.PeakFinder = recording_peakfinder(rec)
    try:
        out = sa.Formants(np.array(x, dtype=np.float64), Fs, full=True, **kw)
    finally:
        sa.lpc = mgf._lpc
        sa.PeakFinder = _PeakFinder
    assert len(rec) == len(rows) == len(out[0])
    return out, rows, rec


def picks(Form, rec):
    """[frames][cols]: which of the frame's peaks each formant takes (-1: no formant, or no peak)."""
    p = -np.ones(Form.shape, dtype=np.int64)
    for f in range(Form.shape[0]):
        for c in range(Form.shape[1]):
            if not np.isnan(Form[f, c]) and len(rec[f][1]):
                p[f, c] = int(np.argmin(np.abs(rec[f][1] - Form[f, c])))
    return p


def padded(rec, order):
    n = len(rec)
    npk = np.array([len(r[0]) for r in rec], dtype=np.int32).reshape(n)
    assert n == 0 or npk.max() <= order, npk.max()
    idx = -np.ones((n, order), dtype=np.int32)
    pkF, pkA = np.nan * np.ones((n, order)), np.nan * np.ones((n, order))
    for f, (i, p, v) in enumerate(rec):
        idx[f, :len(i)], pkF[f, :len(i)], pkA[f, :len(i)] = i, p, v
    return npk, idx, pkF, pkA


def run_case(store, L, lfile, case):
    name, Fs, kw = case["name"], case["Fs"], case["kw"]
    x = mgg.case_signal(L, case)
    (Time, Form, BW, Peaks, Amp), rows, rec = run_full(x, Fs, kw, mgf._lpc)
    nfr, order = case["nframes"], case["order"]
    same = lambda a, b: a.shape == b.shape and np.array_equal(a, b, equal_nan=True)  # noqa: E731
    assert same(Time, L[name + "_Time"]) and same(Form, L[name + "_Form"]) and same(BW, L[name + "_BandWidths"]), name
    assert same(np.array(rows).reshape(nfr, order), L[name + "_lpc"]), name
    stable = np.array(L[name + "_stable"], dtype=bool).copy()
    pk0 = picks(Form, rec)
    reruns = []
    for k in range(mgf.RERUNS if nfr else 0):
        (_, F2, _, P2, A2), _, rec2 = run_full(x, Fs, kw, mgg.perturbed_lpc(np.random.default_rng(2000 + k)))
        pk2 = picks(F2, rec2)
        reruns.append((P2, A2, rec2))
        for f in range(nfr):
            if not (len(rec2[f][0]) == len(rec[f][0]) and np.array_equal(rec2[f][0], rec[f][0])
                    and np.array_equal(np.isnan(P2[f]), np.isnan(Peaks[f])) and np.array_equal(np.isnan(A2[f]), np.isnan(Amp[f]))
                    and np.array_equal(pk2[f], pk0[f])):
                stable[f] = False
    sens = dict(peaks=0.0, amp=0.0, pkF=0.0, pkA=0.0)
    for P2, A2, rec2 in reruns:
        for f in np.nonzero(stable)[0]:
            ok = ~np.isnan(Peaks[f])
            if ok.any():
                sens["peaks"] = max(sens["peaks"], float(np.max(np.abs(P2[f][ok] - Peaks[f][ok]))))
                sens["amp"] = max(sens["amp"], float(np.max(np.abs(A2[f][ok] - Amp[f][ok]))))
            if len(rec[f][0]):
                sens["pkF"] = max(sens["pkF"], float(np.max(np.abs(rec2[f][1] - rec[f][1]))))
                sens["pkA"] = max(sens["pkA"], float(np.max(np.abs(rec2[f][2] - rec[f][2]))))
    assert nfr == 0 or stable.mean() >= 0.95, (name, stable.mean())
    npk, idx, pkF, pkA = padded(rec, order)
    store[name + "_Peaks"], store[name + "_Amplitudes"] = Peaks, Amp
    store[name + "_npk"], store[name + "_idx"], store[name + "_pkF"], store[name + "_pkA"] = npk, idx, pkF, pkA
    store[name + "_stable"] = stable
    for key, v in sens.items():
        store[name + "_sens_" + key] = np.float64(v)
    print("%-12s frames %3d order %2d  stable %.2f (L's %.2f)  peaks/frame %s  amplitudes up to %.3g  sens peaks %.2e amp %.2e pkF %.2e pkA %.2e"
          % (name, nfr, order, stable.mean() if nfr else 1.0, np.mean(L[name + "_stable"]) if nfr else 1.0, sorted(set(npk.tolist())),
             np.nanmax(pkA) if nfr else 0.0, sens["peaks"], sens["amp"], sens["pkF"], sens["pkA"]))
    return dict(name=name, file=lfile, order=order, npts=NPTS, FsN=case["FsN"], nframes=nfr)


def main():
    for fname, lfiles in (("E1_full.npz", ("L1_rates.npz", "L2_options.npz")), ("E2_edges.npz", ("L3_edges.npz",))):
        store, cases = {}, []
        for lfile in lfiles:
            L = np.load(os.path.join(HERE, lfile))
            for case in json.loads(str(L["cases"])):
                cases.append(run_case(store, L, lfile, case))
        mgf.write(fname, store, cases)


if __name__ == "__main__":
    main()
