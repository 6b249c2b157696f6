#!/usr/bin/env python3
"""Generate the U*.npz golden vectors of the speech segmenter by IMPORTING the reference
(pypevoc/speech/SpeechSegmenter.py: SpeechSegmenter.process :203-222, refine_segments_parabolic :252-260,
refine_all_all_bands :304-314, refine_interval :316-389).

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_segment.py

The reference needs three shims under today's scipy and numpy: scipy.signal.hamming / hanning (moved to
scipy.signal.windows) and np.float (removed in numpy 1.24; mode 'pctYY' calls it).  The module is loaded by name through
importlib.  The prefix is U.  Each file holds signals (float32-exact; U3 reads G7's int16 Perlman samples: `x_from`) and
`cases`, a JSON list of {name, x, slice, sr, bands, rough_window, fine_window, detect_thresh, thrs, intervals, modes}.  Per
case, with <n> the case's name:
  <n>_rough_spec, <n>_tfb      the rough bank's energies and frame times as the reference computed them
  <n>_refine_tsegs             the times the refinement ran on: process()'s segments, then the case's extra_tsegs
  <n>_det, <n>_idx, <n>_seg    detection function, kept peak indices, process()'s segments; <n>_raises = 1 where process raises
  <n>_fpos, <n>_par_seg        refine_segments_parabolic's positions and segments; <n>_par_raises = 1 where it raises
  <n>_fine_spec, <n>_tfine     the fine bank's energies and times
  <n>_<thr>_valb / _vala / _cross / _bandpk / _weight [nseg][nband], <n>_<thr>_refined [nseg]
                               refine_all_all_bands(thr) on process()'s segments, thr tags 'tNone', 't3.0'; the per-band
                               values are read off the reference's own np.median / np.argmin calls through a recording proxy
  <n>_iv<k>_<mode>_trans / _bandtrans / _tfine / _finespec, or <n>_iv<k>_<mode>_raises = the exception's name
  <n>_sens_det, _sens_par_seg, _sens_<thr>_valb / _vala / _refined, _sens_iv<k>_<mode>_trans / _bandtrans
                               the largest |change| of that quantity over NPERT reruns with every band energy multiplied by
                               1 + 1e-9 g, g seeded standard normal (1e-9 relative is k_fbank.hip's contract)
  <n>_stable_det (one flag), <n>_<thr>_stable [nseg]
                               false where a rerun changed a discrete choice: the peak set, a crossing index, a NaN pattern
The generator stops unless at least 90 % of a case's segments are stable.  Data only.
"""
import importlib
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import scipy.signal  # noqa: E402
import scipy.signal.windows  # noqa: E402

warnings.simplefilter("ignore")
np.seterr(all="ignore")
for _n in ("hamming", "hanning", "hann", "blackman"):
    if not hasattr(scipy.signal, _n) and hasattr(scipy.signal.windows, _n):
        setattr(scipy.signal, _n, getattr(scipy.signal.windows, _n))
if not hasattr(np, "float"):
    np.float = float

seg_mod = importlib.import_module("pypevoc.speech.SpeechSegmenter")

HERE = os.path.dirname(os.path.abspath(__file__))
NPERT = 8
REL = 1e-9
MODES = ("minmax", "median", "mean", "pct10")


class Recorder(object):
    """Stands in for the module's `np` while refine_segment_all_bands runs: passes everything through, and keeps what
    np.median returned and which element np.argmin chose among which crossings."""

    def __init__(self):
        self.events = []
        self._rr = None

    def __getattr__(self, name):
        return getattr(np, name)

    def median(self, a):
        v = np.median(a)
        self.events.append(("median", v))
        return v

    def flatnonzero(self, a):
        r = np.flatnonzero(a)
        self._rr = r
        return r

    def argmin(self, a):
        i = np.argmin(a)
        self.events.append(("cross", int(self._rr[i])))
        return i


def segment_signal(sr, dur, seed, nseg=24):
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


def cached_bank(fb, w):
    """The bank's specout on w, computed once; returns a setter that makes fb.specout give it back times 1 + REL g."""
    spec, t = fb.specout(w)
    spec = np.array(spec)
    state = {"factor": 1.0}

    def specout(_w):
        return spec * state["factor"], np.array(t)

    fb.specout = specout

    def perturb(rng):
        state["factor"] = 1.0 if rng is None else 1.0 + REL * rng.standard_normal(spec.shape)

    return spec, np.array(t), perturb


def run_refine(sg, segs, thr):
    """refine_all_all_bands(thr) on segs with the per-band choices recorded."""
    rec = Recorder()
    seg_mod.np = rec
    try:
        sg.segments = np.array(segs)
        refined = np.array(sg.refine_all_all_bands(thr=thr), dtype=np.float64)
    finally:
        seg_mod.np = np
    nseg, nband = len(segs), sg.fine_fb.fb.shape[0]
    valb, vala = np.full((nseg, nband), np.nan), np.full((nseg, nband), np.nan)
    cross = np.full((nseg, nband), -1, dtype=np.int32)
    cell = -1
    half = 0
    for ev, v in rec.events:
        if ev == "median":
            if half == 0:
                cell += 1
                valb[cell // nband, cell % nband] = v
            else:
                vala[cell // nband, cell % nband] = v
            half ^= 1
        else:
            cross[cell // nband, cell % nband] = v
    assert cell == nseg * nband - 1, (cell, nseg, nband)
    return valb, vala, cross, refined


def nan_eq(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def absdiff(a, b):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return np.where(np.isnan(d), 0.0, d)


def one_case(c, x, out):
    n = c["name"]
    sr = c["sr"]
    w = x if not c.get("slice") else x[c["slice"][0]:c["slice"][1]]
    sg = seg_mod.SpeechSegmenter(sr=sr, bands=list(c["bands"]), detect_thresh=c["detect_thresh"], rough_window=c["rough_window"],
                                 fine_window=c["fine_window"])
    sg.set_signal(w, sr)
    out[n + "_bands"] = np.array(sg.bands, dtype=np.float64)
    out[n + "_pkthresh"] = np.float64(sg.pkthresh)
    try:
        rough, tfb, pert_rough = cached_bank(sg.rough_fb, w)
        seg = np.array(sg.process(w))
    except Exception as e:                                           # no rough frame: numpy's AxisError
        assert isinstance(e, ValueError), repr(e)
        out[n + "_raises"] = np.int64(1)
        return
    out[n + "_rough_spec"], out[n + "_tfb"] = rough, tfb
    det, idx = np.array(sg.detection_func), np.array(sg.detection_func_indexes_int)
    out[n + "_det"], out[n + "_idx"], out[n + "_seg"] = det, idx.astype(np.int32), seg
    try:
        sg.refine_segments_parabolic()
    except ValueError:                                               # one rough frame: np.interp on an empty axis
        assert len(det) == 0
        out[n + "_par_raises"] = np.int64(1)
        sg.segments = seg
    fpos, par = np.array(sg.detection_function_indexes_ref, dtype=np.float64), np.array(sg.segments, dtype=np.float64)
    out[n + "_fpos"], out[n + "_par_seg"] = fpos, par
    fine, tfine, pert_fine = cached_bank(sg.fine_fb, w) if len(w) > sg.fine_fb.nwind else (None, None, None)
    base = {}
    seg = np.concatenate([seg, np.array(c.get("extra_tsegs") or [], dtype=np.float64)])   # times given by hand (an empty iaft)
    out[n + "_refine_tsegs"] = seg
    if fine is not None:
        out[n + "_fine_spec"], out[n + "_tfine"] = fine, tfine
        for thr in c["thrs"]:
            tag = "t%s" % thr
            valb, vala, cross, refined = run_refine(sg, seg, thr)
            base[tag] = (valb, vala, cross, refined)
            pk = np.where(cross >= 0, 0.0, seg[:, None] if len(seg) else 0.0) if len(seg) else np.zeros((0, valb.shape[1]))
            ranges = [np.flatnonzero(np.logical_and(tfine > t - (c["rough_window"] * 2) / float(sr), tfine < t)) for t in seg]
            for s in range(len(seg)):
                for b in range(valb.shape[1]):
                    if cross[s, b] >= 0:
                        pk[s, b] = tfine[cross[s, b] + min(ranges[s])] * sr
            out["%s_%s_valb" % (n, tag)], out["%s_%s_vala" % (n, tag)], out["%s_%s_cross" % (n, tag)] = valb, vala, cross
            out["%s_%s_bandpk" % (n, tag)], out["%s_%s_weight" % (n, tag)] = pk, np.abs(valb - vala)
            out["%s_%s_refined" % (n, tag)] = refined
    # refine_interval: the interval's fine bank is computed on a slice, so it is not cached; perturbed through a wrapper
    ivals = {}
    for k, (t0, t1) in enumerate(c.get("intervals") or []):
        for mode in c["modes"]:
            key = "%s_iv%d_%s" % (n, k, mode)
            sgi = seg_mod.SpeechSegmenter(sr=sr, bands=list(c["bands"]), rough_window=c["rough_window"], fine_window=c["fine_window"])
            sgi.set_signal(w, sr)
            try:
                tr = np.array(sgi.refine_interval(t0, t1, mode=mode))
                out[key + "_trans"], out[key + "_bandtrans"] = tr, np.array(sgi.bandtrans)
                out[key + "_tfine"], out[key + "_finespec"] = np.array(sgi.tfine), np.array(sgi.finespec)
                ivals[key] = (sgi, t0, t1, mode, tr)
            except Exception as e:
                out[key + "_raises"] = np.array(type(e).__name__)
    # sensitivities
    rng = np.random.default_rng(c.get("pert_seed", 99))
    sens = {"det": np.zeros_like(det), "par_seg": np.zeros_like(par)}
    stable_det = True
    stab = {tag: np.ones(len(seg), dtype=bool) for tag in base}
    for tag, (valb, vala, cross, refined) in base.items():
        sens[tag + "_valb"], sens[tag + "_vala"], sens[tag + "_refined"] = np.zeros_like(valb), np.zeros_like(vala), np.zeros_like(refined)
    for key in ivals:
        sens[key[len(n) + 1:] + "_trans"] = np.zeros(2)
        sens[key[len(n) + 1:] + "_bandtrans"] = np.zeros_like(out[key + "_bandtrans"])
    for _ in range(NPERT):
        pert_rough(rng)
        sg.process(w)
        det2, idx2 = np.array(sg.detection_func), np.array(sg.detection_func_indexes_int)
        same = np.array_equal(idx2, idx) and nan_eq(det2, det)
        stable_det &= same
        sens["det"] = np.maximum(sens["det"], absdiff(det2, det))
        if same and len(det):
            sg.refine_segments_parabolic()
            sens["par_seg"] = np.maximum(sens["par_seg"], absdiff(sg.segments, par))
        if fine is not None:
            pert_fine(rng)
            for tag, (valb, vala, cross, refined) in base.items():
                thr = None if tag == "tNone" else float(tag[1:])
                vb2, va2, cr2, rf2 = run_refine(sg, seg, thr)         # (the unperturbed segments: the stages are tested apart)
                ok = np.all(cr2 == cross, axis=1) & np.all(np.isnan(vb2) == np.isnan(valb), axis=1) & \
                    np.all(np.isnan(va2) == np.isnan(vala), axis=1) & (np.isnan(rf2) == np.isnan(refined))
                stab[tag] &= ok
                sens[tag + "_valb"] = np.maximum(sens[tag + "_valb"], absdiff(vb2, valb))
                sens[tag + "_vala"] = np.maximum(sens[tag + "_vala"], absdiff(va2, vala))
                sens[tag + "_refined"] = np.maximum(sens[tag + "_refined"], np.where(ok, absdiff(rf2, refined), 0.0))
        for key, (sgi, t0, t1, mode, tr) in ivals.items():
            plain = type(sgi.fine_fb).specout

            def noisy(wv, _fb=sgi.fine_fb, _plain=plain):
                s, t = _plain(_fb, wv)
                return s * (1.0 + REL * rng.standard_normal(np.shape(s))), t

            sgi.fine_fb.specout = noisy
            try:
                tr2 = np.array(sgi.refine_interval(t0, t1, mode=mode))
                k2 = key[len(n) + 1:] + "_trans"
                sens[k2] = np.maximum(sens[k2], absdiff(tr2, tr))
                k3 = key[len(n) + 1:] + "_bandtrans"
                sens[k3] = np.maximum(sens[k3], absdiff(sgi.bandtrans, out[key + "_bandtrans"]))
            finally:
                del sgi.fine_fb.specout
    pert_rough(None)
    for k, v in sens.items():
        out["%s_sens_%s" % (n, k)] = v
    out[n + "_stable_det"] = np.bool_(stable_det)
    for tag, v in stab.items():
        out["%s_%s_stable" % (n, tag)] = v
        if len(v):
            assert v.mean() >= 0.9, (n, tag, v)
    assert stable_det, n
    print("%-22s nfr %4d  peaks %2d  stable_det %s  %s  sens det %.2e par %.2e ref %s" % (
        n, len(tfb), len(idx), stable_det, {t: int(v.sum()) for t, v in stab.items()}, sens["det"].max() if len(det) else 0,
        sens["par_seg"].max() if len(par) else 0, {t: "%.2e" % sens[t + "_refined"].max() for t in base if len(seg)}))


def save(fname, arrays, cases, extra=None):
    out = dict(arrays)
    for c in cases:
        one_case(c, arrays[c["x"]], out)
    out["cases"] = np.array(json.dumps(cases))
    if extra:
        for k in extra.pop("drop", []):
            del out[k]
        out.update(extra)
    path = os.path.join(HERE, fname + ".npz")
    np.savez_compressed(path, **out)
    print(fname, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


def case(name, x="x", sr=16000.0, bands=(225., 1000., 2000., 4000.), rough_window=2048, fine_window=256, detect_thresh=0.7,
         thrs=(None, 3.0), **kw):
    c = {"name": name, "x": x, "sr": sr, "bands": list(bands), "rough_window": rough_window, "fine_window": fine_window,
         "detect_thresh": detect_thresh, "thrs": list(thrs), "modes": list(MODES)}
    c.update(kw)
    return c


def main():
    geoms = ((2048, 256), (1024, 128), (512, 64), (2048, 64))
    for k, seed in enumerate((1, 2)):
        x = segment_signal(16000.0, 6.0, seed)
        cases = [case("g%d_%d" % g, rough_window=g[0], fine_window=g[1],
                      intervals=[[1.0, 1.25], [3.5, 3.75]] if g == (2048, 256) and k == 0 else None) for g in geoms]
        save("U%d_segments_seed%d" % (k + 1, seed), {"x": x}, cases)
    g7 = np.load(os.path.join(HERE, "G7_perlman.npz"))
    x7 = g7["x"][:60000]
    assert x7.dtype == np.int16
    sr7 = float(g7["sr"])
    save("U3_perlman", {"x": x7}, [case("perlman", sr=sr7, bands=(225., 2000., 4000., 8000., 15000.))],
         extra={"drop": ["x"], "x_from": np.array("G7_perlman"), "x_len": np.int64(len(x7))})
    # edges: a gap of digital silence (-inf dB, NaN in the detection function), 1 / 2 / 3 rough frames, no rough frame, and
    # times at and beyond the signal's end, where no fine frame lies after (or on either side of) the segment
    x4 = segment_signal(16000.0, 3.0, 5, nseg=12)
    x4[20000:26000] = 0.0
    e = {"rough_window": 1024, "fine_window": 128}
    save("U4_edges", {"x": x4},
         [case("silence_gap", **e), case("nfr0", slice=[0, 1024], **e), case("nfr1", slice=[0, 1025], **e),
          case("nfr2", slice=[0, 1537], **e), case("nfr3", slice=[0, 2049], **e),
          case("tseg_at_end", slice=[0, 16000 + 1024 + 40], extra_tsegs=[(16000 + 1024 + 40) / 16000.0, 2.5], **e)])


if __name__ == "__main__":
    main()
