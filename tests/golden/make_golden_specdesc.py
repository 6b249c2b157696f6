#!/usr/bin/env python3
"""Generate the M*.npz golden vectors of the windowed spectral measures by IMPORTING the reference
(pypevoc/SoundUtils.py: SpecCentWind :142-160, SpecFlux :196-231, AvgWind :163-193; pypevoc/speech/SpeechAnalysis.py:
SpectralMoments :82-139, DistribMoments :54-80, rmsWind :321-346).

Run in the build container only (the reference never travels to the GPU box; scipy is needed here and nowhere else):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_specdesc.py

What it takes to run the reference under Python 3, numpy 2 and scipy 1.15 (SPECDESC.md):
  * pypevoc.speech imports only with scipy.signal.hamming = scipy.signal.windows.hamming set first (a default argument,
    SpeechAnalysis.py:83);
  * SpecCentWind slices with nwind/2 (SoundUtils.py:154): nwind is passed as FloorInt, an int whose true division by an
    int floor-divides; the function itself runs unchanged.
SpectralMoments hands (freqS[idx], SxxS[idx]) to DistribMoments: the generator wraps that function to record them, so the
periodogram in a fixture is the reference's own; a second run with fCut = -1 records every bin.

Each file holds float32-exact signals (stored as float32, int16 ones as int16) and `cases`, a JSON list of
  {name, func: SpecCentWind | SpecFlux | AvgWind | rmsWind | SpectralMoments, x: key of the signal,
   dtype: float32 | float64 | int16, slice: null | [start, stop], kw: keyword arguments of the call}.
Per case <name>_out and <name>_t (SpectralMoments: <name>_<cog|std|skew|kurt|level>, <name>_freq, <name>_sxx -- what
DistribMoments was given -- and <name>_sxx_full, and sens_<..>: the largest change of each of the five outputs over 16 seeded
perturbations of sxx_full by up to 1e-9 relative per bin; <name>_geom: window, hop and nFrames).  M3 also holds
hamming_<n>: scipy.signal.windows.hamming(n) for the window lengths of its cases.
Before a case is written the reference's float64 result is compared with a long-double evaluation of the same formula
(scipy.fft on np.longdouble): it must be within 1e-11 relative -- the centroid relative to itself, the flux relative to
||X_i|| + ||X_i+1|| over the band, the periodogram per bin -- so that no fixture is committed on which the reference itself
is marginal against the tests' 1e-9.  Data only.
"""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import scipy.fft  # noqa: E402
import scipy.signal  # noqa: E402
import scipy.signal.windows  # noqa: E402

warnings.simplefilter("ignore")
scipy.signal.hamming = scipy.signal.windows.hamming

from pypevoc import SoundUtils as su  # noqa: E402
from pypevoc.speech import SpeechAnalysis as sa  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SELF_BOUND = 1e-11
MOMENTS = ("cog", "std", "skew", "kurt", "level")
LD = np.longdouble


class FloorInt(int):
    """nwind for SpecCentWind: nwind/2 is nwind//2, as the Python 2 the reference was written for had it."""

    def __truediv__(self, other):
        return FloorInt(int(self) // other) if isinstance(other, int) else int(self) / other


def f32exact(x):
    return np.asarray(x, dtype=np.float32)


# ---- signals: chirps and onsets over a noise floor of 1e-3 of the peak -------------------------------------------------
def chirp_onsets(sr, n, f0, f1, seed, period):
    """A chirp from f0 to f1 whose amplitude restarts every `period` samples (decaying bursts: onsets), two octave partials."""
    t = np.arange(n) / float(sr)
    ph = 2 * np.pi * (f0 * t + (f1 - f0) * t * t / (2 * t[-1]))
    env = np.exp(-4.0 * (np.arange(n) % period) / float(period)) * (0.3 + 0.7 * ((np.arange(n) // period) % 2))
    x = env * (0.6 * np.sin(ph) + 0.3 * np.sin(2 * ph + 0.5))
    x = x / np.abs(x).max()
    return x + 1e-3 * np.random.default_rng(seed).standard_normal(n)


def vowel_fricative(sr, n, seed):
    """A harmonic 'vowel' that gives way to a high-passed noise 'fricative' and back, over the noise floor."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(sr)
    f0 = 140.0 * (1 + 0.02 * np.sin(2 * np.pi * 4 * t))
    ph = 2 * np.pi * np.cumsum(f0) / sr
    vow = sum(np.sin(h * ph) / h**1.2 for h in range(1, int(sr / 2.2 / 150)))
    fric = np.diff(rng.standard_normal(n + 1))
    mix = 0.5 * (1 + np.tanh(8 * np.sin(2 * np.pi * 2.5 * t)))
    x = mix * vow / np.abs(vow).max() + (1 - mix) * 0.4 * fric / np.abs(fric).max()
    return x + 1e-3 * rng.standard_normal(n)


def signal(case, arrays):
    x = arrays[case["x"]]
    if case["dtype"] == "float64":
        x = x.astype(np.float64)
    if case.get("slice"):
        x = x[case["slice"][0]:case["slice"][1]]
    return x


# ---- long-double restatements -------------------------------------------------------------------------------------------
def ld_mags(x, wind, starts):
    xl = np.asarray(x).astype(LD)
    wl = np.asarray(wind).astype(LD)
    out = []
    for s in starts:
        S = scipy.fft.fft(xl[s:s + len(wl)] * wl)
        assert S.dtype == np.clongdouble
        out.append(np.sqrt(S.real**2 + S.imag**2))
    return np.array(out, dtype=LD).reshape(len(starts), len(wl))


def check_centroid(name, x, out, nwind, nhop, sr):
    m = ld_mags(x, np.blackman(nwind), np.arange(len(out)) * nhop)[:, :nwind // 2]
    ff = np.arange(nwind // 2).astype(LD) / LD(nwind) * LD(sr)
    den = m.sum(axis=1)
    live = den != 0
    assert np.array_equal(np.isnan(out), ~live), name
    ld = (m[live] * ff).sum(axis=1) / den[live]
    err = float(np.max(np.abs(out[live] - ld) / np.abs(ld), initial=0.0))
    print("  %-26s values %3d (nan %d)  reference vs long double %.2e" % (name, len(out), int((~live).sum()), err))
    assert err <= SELF_BOUND, (name, err)


def check_flux(name, x, out, nwind, nhop, sr, kw):
    wind = kw.get("windfunc", np.blackman)(nwind)
    m = ld_mags(x, wind, np.arange(len(out) + 1) * nhop)
    minf, maxf = kw.get("minf", 0), kw.get("maxf", np.inf)
    minbin = int(minf / sr * nwind)
    maxbinf = float(maxf) / sr * nwind
    maxbin = nwind if maxbinf > nwind else int(maxbinf)
    band = m[:, minbin:maxbin]
    ld = np.sqrt(((band[:-1] - band[1:])**2).sum(axis=1))
    scale = np.sqrt((band[:-1]**2).sum(axis=1)) + np.sqrt((band[1:]**2).sum(axis=1))
    assert np.array_equal(out == 0, scale == 0), name                 # exact zeros: empty band, silence
    nz = scale != 0
    err = float(np.max(np.abs(out[nz] - ld[nz]) / scale[nz], initial=0.0))
    rel = float(np.max(ld[nz] / scale[nz], initial=0.0))
    print("  %-26s values %3d (zero %d, band %d bins)  reference vs long double %.2e  largest flux / scale %.2f" %
          (name, len(out), int((~nz).sum()), band.shape[1], err, rel))
    assert err <= SELF_BOUND, (name, err)
    return rel


def check_psd(name, x, sxx_full, nwind, nhop, nfr):
    wl = scipy.signal.windows.hamming(nwind)
    m = ld_mags(x, wl, np.arange(nfr) * nhop)[:, :nwind // 2]
    ld = np.sqrt((m**2).sum(axis=0) / LD(nfr))
    err = float(np.max(np.abs(sxx_full - ld) / ld))
    print("  %-26s frames %3d bins %3d  reference sqrt(P) vs long double %.2e  (span %.1e)" % (name, nfr, len(ld), err, float(ld.max() / ld.min())))
    assert err <= SELF_BOUND / 2, (name, err)                         # (the square root halves a relative error)


# ---- the reference calls ------------------------------------------------------------------------------------------------
def kwargs_of(case):
    kw = dict(case["kw"])
    if "windfunc" in kw:
        kw["windfunc"] = getattr(np, kw["windfunc"])
    if kw.get("maxf") == "inf":
        kw["maxf"] = np.inf
    return kw


def spectral_moments(x, kw):
    """The reference's dict, and what it handed to DistribMoments."""
    seen = []
    orig = sa.DistribMoments

    def spy(xx, ff, mm=4):
        seen.append((np.array(xx), np.array(ff)))
        return orig(xx, ff, mm)
    sa.DistribMoments = spy
    try:
        d = sa.SpectralMoments(x, **kw)
    finally:
        sa.DistribMoments = orig
    assert len(seen) == 1
    return d, seen[0][0], seen[0][1]


def moments_from(freq_full, sxx_full, fcut):
    idx = freq_full > fcut
    cog, std, skew, kurt, _ = sa.DistribMoments(freq_full[idx], sxx_full[idx], 4)
    return dict(cog=cog, std=std, skew=skew, kurt=kurt, level=np.sqrt(np.mean(sxx_full**2)))


def run_case(case, arrays, out, stats):
    name, func = case["name"], case["func"]
    x = signal(case, arrays)
    kw = kwargs_of(case)
    if func == "SpecCentWind":
        kk = dict(kw)
        kk["nwind"] = FloorInt(kk["nwind"])
        v, t = su.SpecCentWind(x, **kk)
        if len(v):
            check_centroid(name, x, v, kw["nwind"], kw["nhop"], kw["sr"])
    elif func == "SpecFlux":
        v, t = su.SpecFlux(x, **kw)
        if len(v):
            stats.append((name, check_flux(name, x, v, kw["nwind"], kw["nhop"], kw["sr"], kw)))
    elif func == "AvgWind":
        v, t = su.AvgWind(x, **kw)
    elif func == "rmsWind":
        t, v = sa.rmsWind(x, **kw)
    elif func == "SpectralMoments":
        d, freq, sxx = spectral_moments(x, kw)
        for k in MOMENTS:
            out[name + "_" + k] = np.float64(d[k])
        out[name + "_freq"] = freq
        out[name + "_sxx"] = sxx
        kfull = dict(kw)
        kfull["fCut"] = -1
        dfull, freq_full, sxx_full = spectral_moments(x, kfull)
        out[name + "_freq_full"] = freq_full
        out[name + "_sxx_full"] = sxx_full
        nwind, hop = int(np.round(kw["Fs"] * kw.get("tWind", 0.025))), int(np.round(kw["Fs"] * kw.get("tHop", 0.0125)))
        nfr = int((len(x) - nwind - 1) / hop)
        out[name + "_geom"] = np.array([nwind, hop, nfr], dtype=np.int64)
        if nfr > 0:
            fcut = kw.get("fCut", 300)
            assert np.array_equal(sxx_full[freq_full > fcut], sxx)
            base = moments_from(freq_full, sxx_full, fcut)
            for k in MOMENTS:                                         # the restatement the perturbations go through is the reference's
                assert base[k] == d[k] or abs(base[k] - d[k]) <= 4e-16 * abs(d[k]), (name, k, base[k], d[k])
            check_psd(name, x, sxx_full, nwind, hop, nfr)
            rng = np.random.default_rng(777)
            sens = dict((k, 0.0) for k in MOMENTS)
            for _ in range(16):
                pert = moments_from(freq_full, sxx_full * (1 + 1e-9 * rng.uniform(-1, 1, len(sxx_full))), fcut)
                for k in MOMENTS:
                    sens[k] = max(sens[k], abs(pert[k] - base[k]))
            for k in MOMENTS:
                assert sens[k] > 0, (name, k)
                out[name + "_sens_" + k] = np.float64(sens[k])
            print("  %-26s %s" % ("", "  ".join("%s %.6g (sens %.1e)" % (k, d[k], sens[k]) for k in MOMENTS)))
        else:
            print("  %-26s nFrames %d: %s" % (name, nfr, "  ".join("%s %r" % (k, float(d[k])) for k in MOMENTS)))
        return
    else:
        raise ValueError(func)
    out[name + "_out"] = np.asarray(v, dtype=np.float64)
    out[name + "_t"] = np.asarray(t, dtype=np.float64)
    if func in ("AvgWind", "rmsWind") or len(v) == 0:
        print("  %-26s values %3d" % (name, len(v)))


def write(fname, arrays, cases, need_flux=False, extra=None):
    print(fname)
    out = dict(arrays)
    out.update(extra or {})
    stats = []
    for c in cases:
        run_case(c, arrays, out, stats)
    if need_flux:                                                     # zeros cannot pass the flux test
        assert max(r for _, r in stats) >= 0.1, stats
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, fname + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("  -> %s %d bytes" % (os.path.basename(path), size))
    assert size <= 385067, size                                       # the largest F* fixture


def case(name, func, x, dtype="float32", sl=None, **kw):
    return {"name": name, "func": func, "x": x, "dtype": dtype, "slice": sl, "kw": kw}


def main():
    sr = 44100
    x44 = f32exact(chirp_onsets(sr, 20000, 200.0, 6000.0, 11, 3700))
    gap44 = x44.copy()
    gap44[7000:10100] = 0.0
    # ---- M1: the fused window lengths, hops that do not divide them, 26 .. 39 frames
    cases = []
    for nwind, hop in ((512, 500), (1024, 600), (2048, 700)):
        cases.append(case("cent%d" % nwind, "SpecCentWind", "x44", sr=sr, nwind=nwind, nhop=hop))
        cases.append(case("flux%d" % nwind, "SpecFlux", "x44", sr=sr, nwind=nwind, nhop=hop))
    cases += [case("flux512_inner", "SpecFlux", "x44", sr=sr, nwind=512, nhop=500, minf=500, maxf=5000),
              case("flux512_mirror", "SpecFlux", "x44", sr=sr, nwind=512, nhop=500, minf=1000, maxf=0.75 * sr),
              case("flux512_above_sr", "SpecFlux", "x44", sr=sr, nwind=512, nhop=500, minf=0, maxf=2.0 * sr),
              case("flux512_neg_minf", "SpecFlux", "x44", sr=sr, nwind=512, nhop=500, minf=-2000, maxf="inf"),
              case("flux512_empty", "SpecFlux", "x44", sr=sr, nwind=512, nhop=500, minf=5000, maxf=1000),
              case("flux1024_hann_f64", "SpecFlux", "x44", "float64", sr=sr, nwind=1024, nhop=600, windfunc="hanning"),
              case("cent512_gap", "SpecCentWind", "gap44", sr=sr, nwind=512, nhop=500),
              case("flux512_gap", "SpecFlux", "gap44", sr=sr, nwind=512, nhop=500),
              case("flux2048_gap", "SpecFlux", "gap44", sr=sr, nwind=2048, nhop=700, minf=300, maxf=9000)]
    write("M1_fused", {"x44": x44, "gap44": gap44}, cases, need_flux=True)

    # ---- M2: the rows route (256, odd 333, 1000), int16 samples, AvgWind and rmsWind
    sr2 = 16000
    x16 = f32exact(chirp_onsets(sr2, 9000, 150.0, 3000.0, 12, 1900))
    i16 = np.round(x16.astype(np.float64) / np.abs(x16).max() * 20000).astype(np.int16)
    gap16 = x16.copy()
    gap16[3000:4200] = 0.0
    # AvgWind runs on the rectified signal: an average of terms of one sign is as well conditioned as its terms, so its
    # 1e-12 relative bound is about the kernel; on the chirp itself a frame's terms cancel to 1e-6 of their size, and any
    # other order of the same float64 sum is 1e-11 away
    rect16 = np.abs(x16)
    cases = []
    for nwind, hop in ((256, 200), (333, 150), (1000, 450)):
        cases.append(case("cent%d" % nwind, "SpecCentWind", "x16", sr=sr2, nwind=nwind, nhop=hop))
        cases.append(case("flux%d" % nwind, "SpecFlux", "x16", sr=sr2, nwind=nwind, nhop=hop))
    cases += [case("flux333_inner", "SpecFlux", "x16", sr=sr2, nwind=333, nhop=150, minf=400, maxf=3000),
              case("flux333_mirror", "SpecFlux", "x16", sr=sr2, nwind=333, nhop=150, minf=100, maxf=0.8 * sr2),
              case("flux333_above_sr", "SpecFlux", "x16", sr=sr2, nwind=333, nhop=150, minf=0, maxf=3.0 * sr2),
              case("flux333_neg_minf", "SpecFlux", "x16", sr=sr2, nwind=333, nhop=150, minf=-1500, maxf="inf"),
              case("flux333_empty", "SpecFlux", "x16", sr=sr2, nwind=333, nhop=150, minf=3000, maxf=400),
              case("cent256_i16", "SpecCentWind", "i16", "int16", sr=sr2, nwind=256, nhop=200),
              case("flux1000_i16", "SpecFlux", "i16", "int16", sr=sr2, nwind=1000, nhop=450),
              case("cent333_gap", "SpecCentWind", "gap16", sr=sr2, nwind=333, nhop=150),
              case("flux256_gap", "SpecFlux", "gap16", sr=sr2, nwind=256, nhop=200),
              case("avg256", "AvgWind", "rect16", sr=sr2, nwind=256, nhop=100),
              case("rms300_hann", "rmsWind", "x16", sr=sr2, nwind=300, nhop=130, windfunc="hanning")]
    write("M2_rows", {"x16": x16, "i16": i16, "gap16": gap16, "rect16": rect16}, cases, need_flux=True)

    # ---- M3: SpectralMoments at 8, 16 and 44.1 kHz (windows 200, 400, 1102); 8 kHz: 57 frames = four blocks of 16
    v8 = f32exact(vowel_fricative(8000, 6000, 21))
    v16 = f32exact(vowel_fricative(16000, 8000, 22))
    v44 = f32exact(vowel_fricative(44100, 20000, 23))
    gap8 = v8.copy()
    gap8[1500:3100] = 0.0
    cases = [case("mom8k", "SpectralMoments", "v8", Fs=8000),
             case("mom8k_f64_fcut1k", "SpectralMoments", "v8", "float64", Fs=8000, fCut=1000),
             case("mom8k_gap", "SpectralMoments", "gap8", Fs=8000),
             case("mom16k", "SpectralMoments", "v16", Fs=16000),
             case("mom22k_w551", "SpectralMoments", "v44", sl=[0, 12000], Fs=22040, fCut=500),
             case("mom44k", "SpectralMoments", "v44", Fs=44100)]
    # (and the windows themselves: scipy.signal.windows.hamming and np.hamming differ in the last bit)
    wins = dict(("hamming_%d" % n, scipy.signal.windows.hamming(n)) for n in (200, 400, 551, 1102))
    assert any(not np.array_equal(w, np.hamming(len(w))) for w in wins.values())
    write("M3_moments", {"v8": v8, "v16": v16, "v44": v44, "gap8": gap8}, cases, extra=wins)

    # ---- M4: no frame.  SpecCentWind / SpecFlux: two arrays of shape (0,); SpectralMoments: nFrames = 0 (200 .. 300 samples
    # at 8 kHz: 0/0) and nFrames < 0 (shorter than the window: zeros / -1)
    cases = [case("cent_none", "SpecCentWind", "v8", sl=[0, 512], sr=8000, nwind=512, nhop=128),
             case("cent_short", "SpecCentWind", "v8", sl=[0, 100], sr=8000, nwind=512, nhop=128),
             case("flux_none", "SpecFlux", "v8", sl=[0, 512 + 128], sr=8000, nwind=512, nhop=128),
             case("flux_none_rows", "SpecFlux", "v8", sl=[0, 300], sr=8000, nwind=333, nhop=100),
             case("flux_one", "SpecFlux", "v8", sl=[0, 512 + 129], sr=8000, nwind=512, nhop=128),
             case("cent_one", "SpecCentWind", "v8", sl=[0, 513], sr=8000, nwind=512, nhop=128)]
    for n in (200, 250, 300, 100, 0):
        cases.append(case("mom8k_n%d" % n, "SpectralMoments", "v8", sl=[0, n], Fs=8000))
    write("M4_edges", {"v8": v8[:700]}, cases)


if __name__ == "__main__":
    main()
