#!/usr/bin/env python3
"""Generate the Q*.npz golden vectors of HeterodyneHarmonic by IMPORTING the reference (pypevoc/Heterodyne.py:261-542).

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hetharm.py

The prefix is Q (existing tests glob G* and H*).  Each file holds `cases`, a JSON list of
  {name, ctor: kwargs of HeterodyneHarmonic without x / f / tf, f: "scalar" | "array" | "pairs", partials: [[n, filter], ..],
   filtered: [n, ..], adjust: null | {nwind, nhop}, self_dist: {output: float}}
and per case <name>_x, <name>_f (and <name>_tf), then what the reference computed: _ah, _th, _idxh, _fmin, _fvec, _resynth,
_rp_<n>_<0|1> (resynth_partial), _fh_<n> (filter_harmonic), _fcols (the property f), _angle_ratios, _partial_frequencies, _adj_f0c, _adj_th.
A case with no frame stores only _ah, _th, _idxh, _fmin, _fvec (the reference's resynthesis raises on it).

self_dist[output] is the reference's own distance from the truth: max |reference - long double| / max |reference|, where
the long double value evaluates the same formulas (running phase, window sums, interpolation, product) on np.longdouble
with pi to that precision, from the same float64 inputs.  The tests' tolerances are multiples of it.  Data only.
"""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

warnings.simplefilter("ignore")

from pypevoc import Heterodyne as het  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
PI_LD = LD(4) * np.arctan(LD(1))
assert np.finfo(LD).eps < 2e-19, "np.longdouble is no wider than float64 here"


# ---- the long double evaluation ---------------------------------------------------------------------------------------
def ld_hetsig(fvec, n):
    ph = LD(2) * PI_LD * LD(n) * np.cumsum(np.asarray(fvec).astype(LD))
    return np.cos(ph), np.sin(ph)


def ld_heterodyne(x, fvec, n, wind, hop):
    """2 * sum(x * exp(i n phi) * wind) / sum(wind) per frame, as two long double arrays"""
    c, s = ld_hetsig(fvec, n)
    xl, wl = np.asarray(x).astype(LD), np.asarray(wind).astype(LD)
    wn = np.sum(wl)
    re, im = [], []
    for ii in range(0, len(xl) - len(wl), hop):
        xw = xl[ii:ii + len(wl)] * wl
        re.append(LD(2) * np.sum(xw * c[ii:ii + len(wl)]) / wn)
        im.append(LD(2) * np.sum(xw * s[ii:ii + len(wl)]) / wn)
    return np.array(re, dtype=LD), np.array(im, dtype=LD)


def ld_ah(h):
    cols = [ld_heterodyne(h.x, h.fvec, n, h.wind, h.nhop) for n in range(h.nharm)]
    re = np.stack([c[0] for c in cols], axis=1)
    im = np.stack([c[1] for c in cols], axis=1)
    re[:, 0] /= 2
    im[:, 0] /= 2
    return re, im


def ld_interp(nsamp, nwind, nhop, v):
    """np.interp(t/sr, th, v) for th on the samples nwind//2 + i*nhop, clamped, in long double"""
    t = np.arange(nsamp)
    nfr = len(v)
    if nfr == 1:
        return np.full(nsamp, v[0], dtype=LD)
    r = t - nwind // 2
    i0 = np.clip(r // nhop, 0, nfr - 2)
    fr = np.clip((r - i0 * nhop).astype(LD) / LD(nhop), LD(0), LD(1))
    return v[i0] + (v[i0 + 1] - v[i0]) * fr


def ld_partial(h, are, aim, n, mask=None):
    hr, hi = ld_interp(h.nsamp, h.nwind, h.nhop, are[:, n]), ld_interp(h.nsamp, h.nwind, h.nhop, aim[:, n])
    if mask is not None:
        hr[mask] = 0
        hi[mask] = 0
    c, s = ld_hetsig(h.fvec, n)
    return c * hr + s * hi, hr, hi


def dist(ref, ld_re, ld_im=None):
    ref = np.asarray(ref)
    if ref.size == 0:
        return 0.0
    d = np.abs(ref.real.astype(LD) - ld_re) if ld_im is None else np.hypot(ref.real.astype(LD) - ld_re, ref.imag.astype(LD) - ld_im)
    return float(np.max(d) / LD(np.max(np.abs(ref))))


# ---- signals ----------------------------------------------------------------------------------------------------------
def tone(f0, sr, amps, seed, noise=1e-3, dc=0.05, env=None):
    """sum of harmonics of the per-sample track f0 (Hz) with amplitudes amps[h-1], a DC offset and a noise floor"""
    ph = 2 * np.pi * np.cumsum(f0 / sr)
    x = sum(a * np.cos(k * ph + 0.3 * k) for k, a in enumerate(amps, 1))
    if env is not None:
        x = x * env
    return x + dc + noise * np.random.default_rng(seed).standard_normal(len(f0))


def run_case(case, x, f, tf, out):
    name = case["name"]
    kw = dict(case["ctor"])
    h = het.HeterodyneHarmonic(x, tf=tf, f=f, **kw)
    out[name + "_x"] = x
    out[name + "_f"] = np.asarray(f, dtype=np.float64)
    if tf is not None:
        out[name + "_tf"] = np.asarray(tf, dtype=np.float64)
    out[name + "_ah"] = h.ah
    out[name + "_th"] = h.th
    out[name + "_idxh"] = h.idxh
    out[name + "_fmin"] = np.float64(h.fmin)
    out[name + "_fvec"] = h.fvec
    sd = {}
    case["self_dist"] = sd
    nfr = h.ah.shape[0]
    assert nfr == len(range(0, h.nsamp - h.nwind, h.nhop)) == len(h.th)
    if nfr == 0:
        return h
    are, aim = ld_ah(h)
    sd["ah"] = dist(h.ah, are, aim)
    y = h.resynth()
    out[name + "_resynth"] = y
    yl = sum(ld_partial(h, are, aim, n)[0] for n in range(h.nharm))
    sd["resynth"] = dist(y, yl)
    for n in case["filtered"]:
        fh = h.filter_harmonic(n)
        out[name + "_fh_%d" % n] = fh
        _, hr, hi = ld_partial(h, are, aim, n, mask=(fh == 0))
        sd["fh_%d" % n] = dist(fh, hr, hi)
    for n, flt in case["partials"]:
        yp = h.resynth_partial(n, filter=bool(flt))
        out[name + "_rp_%d_%d" % (n, flt)] = yp
        mask = (h.filter_harmonic(n) == 0) if flt else None
        sd["rp_%d_%d" % (n, flt)] = dist(yp, ld_partial(h, are, aim, n, mask=mask)[0])
    out[name + "_fcols"] = h.f
    out[name + "_angle_ratios"] = h.angle_ratios
    if nfr > 1:
        out[name + "_partial_frequencies"] = h.partial_frequencies
    if case.get("adjust"):
        a = case["adjust"]
        f0c, tha = h.calc_adjusted_freq(h.fvec, nwind=a["nwind"], nhop=a["nhop"])
        out[name + "_adj_f0c"] = f0c
        out[name + "_adj_th"] = tha
        wind = h.wfun(a["nwind"])
        hr, hi = ld_heterodyne(h.x, h.fvec, 1, wind, a["nhop"])
        ang = np.arctan2(hi, hr)
        d = np.diff(ang)
        d = d - LD(2) * PI_LD * np.round(d / (LD(2) * PI_LD))          # np.unwrap: jumps folded into (-pi, pi]
        dph = np.concatenate(([LD(0)], d))
        ic = np.arange(0, h.nsamp - a["nwind"], a["nhop"]) + a["nwind"] // 2
        f0l = h.fvec[ic].astype(LD) - dph / LD(a["nhop"]) / LD(2) / PI_LD
        sd["adj_f0c"] = dist(f0c, f0l)
    print("  %-18s nsamp %5d frames %3d nharm %2d  self_dist %s" % (name, h.nsamp, nfr, h.nharm, {k: "%.1e" % v for k, v in sd.items()}))
    return h


def save(fname, items):
    out, cases = {}, []
    hs = []
    for case, x, f, tf in items:
        hs.append(run_case(case, x, f, tf, out))
        cases.append(case)
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, fname + ".npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (fname, len(cases), os.path.getsize(path)))
    assert os.path.getsize(path) < 900 * 1024
    return hs


def case(name, ctor, fkind, partials=(), filtered=(), adjust=None):
    return {"name": name, "ctor": ctor, "f": fkind, "partials": [list(p) for p in partials], "filtered": list(filtered), "adjust": adjust}


def check_q5(h, nharm):
    """every term of filter_harmonic's mask decides between 10 % and 90 % of the samples of some harmonic, and no sample
    sits within 1e-9 (relative) of a threshold"""
    tvec = np.arange(h.nsamp) / h.sr
    f0 = h.f0
    share = {"fmin": [], "fmax": [], "nyquist": [], "amp": []}
    for n in range(nharm):
        hf = np.interp(tvec, h.th, h.ah[:, n])
        rmsmin = np.max(np.abs(hf)) * h.ampthr
        assert np.min(np.abs(np.abs(hf) - rmsmin)) > 1e-9 * rmsmin, n
        share["fmin"].append(np.mean(f0 < h.fmin))
        share["fmax"].append(np.mean(f0 > h.fmax))
        share["nyquist"].append(np.mean(f0 * n > h.sr / 2.2))
        share["amp"].append(np.mean(np.abs(hf) < rmsmin))
        if n:
            assert np.min(np.abs(f0 * n - h.sr / 2.2)) > 1e-9 * h.sr, n
    assert np.min(np.abs(f0 - h.fmin)) > 1e-9 * h.fmin and np.min(np.abs(f0 - h.fmax)) > 1e-9 * h.fmax
    for k, v in share.items():
        assert any(0.1 < s < 0.9 for s in v), (k, v)
    print("  Q5 mask shares:", {k: ["%.2f" % s for s in v] for k, v in share.items()})


def main():
    sr = 8000
    # Q1 -- a number for f: 200 Hz, the defaults' shape (nharm 5, nwind 1024, nhop 512)
    n1 = 6000
    x1 = tone(np.full(n1, 200.0), sr, [0.5, 0.25, 0.125, 0.06], seed=1)
    save("Q1_scalar_f", [(case("scalar", {"sr": sr, "nharm": 5, "nwind": 1024, "nhop": 512}, "scalar",
                               partials=[(0, 0), (1, 0), (4, 0), (2, 1)], filtered=[1]), x1, 200.0, None)])

    # Q2 -- per-sample vibrato track, 20 harmonics (three groups of the extraction kernel, the last one partial), an odd
    # window and a hop that divides nothing
    n2 = 5000
    t2 = np.arange(n2) / sr
    f2 = 150.0 * (1.0 + 0.02 * np.sin(2 * np.pi * 4.0 * t2))
    x2 = tone(f2, sr, [0.5 / k for k in range(1, 21)], seed=2)
    save("Q2_vibrato_nharm20", [(case("vibrato", {"sr": sr, "nharm": 20, "nwind": 511, "nhop": 100, "fmax": 2000}, "array",
                                      partials=[(1, 0), (7, 0), (8, 0), (19, 0), (15, 1)], filtered=[3, 19]), x2, f2, None)])

    # Q3 -- tf / f pairs, nine harmonics (one past a group), include_dc
    n3 = 4000
    tf3 = np.linspace(0.0, n3 / sr, 9)
    fp3 = np.array([180., 185., 195., 210., 220., 215., 200., 190., 185.])
    f3 = np.interp(np.arange(n3) / sr, tf3, fp3)
    x3 = tone(f3, sr, [0.4 / k for k in range(1, 9)], seed=3, dc=0.2)
    save("Q3_pairs_dc", [(case("pairs", {"sr": sr, "nharm": 9, "nwind": 512, "nhop": 128, "include_dc": True}, "pairs",
                               partials=[(0, 0), (8, 0), (8, 1)], filtered=[0, 8]), x3, fp3, tf3)])

    # Q4 -- one frame (nsamp = nwind + 1) and none (nsamp = nwind)
    x4 = tone(np.full(1025, 250.0), sr, [0.5, 0.2], seed=4)
    save("Q4_one_and_no_frame",
         [(case("one_frame", {"sr": sr, "nharm": 3, "nwind": 1024, "nhop": 512}, "scalar", partials=[(1, 0), (1, 1)], filtered=[1]), x4, 250.0, None),
          (case("no_frame", {"sr": sr, "nharm": 3, "nwind": 1024, "nhop": 512}, "scalar"), x4[:1024], 250.0, None)])

    # Q5 -- the filter: an f0 sweep that starts below fmin, ends above fmax and takes harmonics past sr/2.2 on its way; the
    # amplitude decays and has a gap
    n5 = 6000
    t5 = np.arange(n5) / sr
    f5 = 60.0 + 440.0 * t5 / t5[-1] + 0.0137
    env = np.exp(-2.0 * t5)
    env[2300:3200] = 0.0
    x5 = tone(f5, sr, [0.5 / k for k in range(1, 12)], seed=5, env=env, noise=1e-5, dc=0.0)
    ctor5 = {"sr": sr, "nharm": 12, "nwind": 512, "nhop": 128, "fmin": 120.0, "fmax": 400.0}
    h5, = save("Q5_filter", [(case("filter", ctor5, "array", partials=[(5, 1), (10, 1), (3, 0)],
                                   filtered=[1, 3, 5, 8, 10, 11]), x5, f5, None)])
    assert h5.fmin == 120.0
    check_q5(h5, 12)

    # Q6 -- calc_adjusted_freq on the normalised track, with a window and a hop of its own; the tone sits 3 Hz off the track
    n6 = 6000
    x6 = tone(np.full(n6, 203.0), sr, [0.5, 0.25, 0.1], seed=6)
    save("Q6_adjusted_freq", [(case("adjust", {"sr": sr, "nharm": 4, "nwind": 1024, "nhop": 512}, "scalar", partials=[(1, 0)],
                                    adjust={"nwind": 300, "nhop": 77}), x6, 200.0, None)])


if __name__ == "__main__":
    main()
