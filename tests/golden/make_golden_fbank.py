#!/usr/bin/env python3
"""Generate the F*.npz golden vectors of the FFT filter banks by IMPORTING the reference
(pypevoc/FFTFilters.py: FilterBank.specout :274-292, MelFilterBank.mfcc / mfcc_and_mel :352-374).

Run in the build container only (the reference never travels to the GPU box; scipy is needed here and nowhere else):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fbank.py

The prefix is F (tests/conftest.py's golden_names() globs G* only).  Each file holds one or more signals (float32-exact,
stored as float32; F7 reads G7's int16 Perlman samples: `x_from`) and `cases`, a JSON list of
  {name, cls: FilterBank | TriangularFilterBank | MelFilterBank, ctor: kwargs, fspecs: null | [PiecewiseFilterSpec kwargs],
   x: key of the signal, dtype: float32 | int16 | float64, slice: null | [start, stop], preemph: null | {hpFreq, Fs},
   zero_rows: rows of fb set to 0 after construction, modes: cepstral modes computed,
   raises: {specout: null | exception name, mfcc: null | exception name}}.
Per case: <name>_fb, <name>_fvec, <name>_wind, <name>_label (JSON), <name>_hop, <name>_spec, <name>_t and <name>_cep_<mode>.
Before a case is written its band energies are compared with a long-double evaluation (scipy.fft on np.longdouble): the
float64 reference must be within 1e-11 relative of it, so that no fixture is committed on which the reference itself is
marginal against the tests' 1e-9.  Data only.
"""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import scipy.fft  # noqa: E402

warnings.simplefilter("ignore")

from pypevoc import FFTFilters as ft  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ("DCT1", "DCT2", "DCT3", "DCT4", "IFFT")
SELF_BOUND = 1e-11


def f32exact(x):
    return np.asarray(x, dtype=np.float32)


def harmonic_vibrato(sr, dur, f0=220.0, nharm=8, seed=1234, noise=0.001):
    """8-harmonic tone, 1 % / 5 Hz vibrato, amplitudes 0.5 / h, white noise floor (the G4 signal's recipe)."""
    t = np.arange(int(sr * dur)) / float(sr)
    fi = f0 * (1.0 + 0.01 * np.sin(2 * np.pi * 5.0 * t))
    ph = 2 * np.pi * np.cumsum(fi) / sr
    x = sum(0.5 / h * np.sin(h * ph) for h in range(1, nharm + 1))
    return x + noise * np.random.default_rng(seed).standard_normal(len(t))


def build(case):
    cls = getattr(ft, case["cls"])
    kw = dict(case["ctor"])
    if case.get("fspecs") is not None:
        kw["fspec_list"] = [ft.PiecewiseFilterSpec(**{k: (np.array(v) if isinstance(v, list) else v) for k, v in s.items()})
                            for s in case["fspecs"]]
    bank = cls(**kw)
    for r in case.get("zero_rows") or []:
        bank.fb[r, :] = 0.0
    return bank


def signal(case, arrays):
    x = arrays[case["x"]]
    if case["dtype"] == "float64":
        x = x.astype(np.float64)
    if case.get("slice"):
        x = x[case["slice"][0]:case["slice"][1]]
    if case.get("preemph"):
        x = ft.preemph(x, **case["preemph"])
    return x


def longdouble_spec(bank, w):
    out = []
    n = 0
    wl = np.asarray(w).astype(np.longdouble)
    while n < len(w) - bank.nwind:
        S = scipy.fft.fft(wl[n:n + bank.nwind] * bank.wind.astype(np.longdouble))
        assert S.dtype == np.clongdouble
        p = S.real**2 + S.imag**2
        out.append([np.sum(p * bank.fb[i].astype(np.longdouble)) for i in range(bank.fb.shape[0])])
        n += bank.hop
    return np.array(out, dtype=np.longdouble)


def run_case(case, arrays, out):
    name = case["name"]
    bank = build(case)
    w = signal(case, arrays)
    out[name + "_fb"] = bank.fb
    out[name + "_fvec"] = bank.fvec
    out[name + "_wind"] = bank.wind
    out[name + "_hop"] = np.int64(bank.hop)
    out[name + "_label"] = np.array(json.dumps(list(bank.label)))
    raises = {"specout": None, "mfcc": None}
    try:
        spec, t = bank.specout(w)
    except Exception as e:                                            # noqa: BLE001
        raises["specout"] = type(e).__name__
        spec = t = None
    if spec is not None:
        out[name + "_spec"] = spec
        out[name + "_t"] = t
        if spec.size:
            ld = longdouble_spec(bank, w)
            assert ld.shape == spec.shape
            nz = ld != 0
            assert ((spec == 0) == ~nz).all(), name
            err = float(np.max(np.abs(spec[nz] - ld[nz]) / np.abs(ld[nz]))) if nz.any() else 0.0
            span = float(spec[nz].max() / spec[nz].min()) if nz.any() else 1.0
            print("  %-28s frames %4d bands %3d  reference vs long double %.2e  (span %.1e)" % (name, spec.shape[0], spec.shape[1], err, span))
            assert err <= SELF_BOUND, (name, err)
    for mode in case.get("modes") or []:
        try:
            c, s2, t2 = bank.mfcc_and_mel(w, mode=mode)
            assert np.array_equal(s2, spec) and np.array_equal(t2, t)
            out[name + "_cep_" + mode] = c
        except Exception as e:                                        # noqa: BLE001
            raises["mfcc"] = type(e).__name__
    case["raises"] = raises


def save(fname, arrays, cases, extra=None):
    out = dict(arrays)
    for c in cases:
        run_case(c, arrays, out)
    if extra:
        for k in extra.pop("drop", []):
            out.pop(k)
        out.update(extra)
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, fname + ".npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (fname, len(cases), os.path.getsize(path)))
    assert os.path.getsize(path) < 900 * 1024


def case(name, cls, ctor, x="x", dtype="float32", fspecs=None, modes=(), **kw):
    c = {"name": name, "cls": cls, "ctor": ctor, "fspecs": fspecs, "x": x, "dtype": dtype, "slice": None, "preemph": None,
         "zero_rows": None, "modes": list(modes)}
    c.update(kw)
    return c


def main():
    # F1 -- the flagship bank: MelFilterBank(sr=44100), nwind 1024, hop 441, 26 bands, all five cepstral modes
    sr = 44100.0
    x1 = f32exact(harmonic_vibrato(sr, 0.6))
    save("F1_mel44k", {"x": x1}, [case("mel44k", "MelFilterBank", {"sr": sr}, modes=MODES),
                                  case("mel44k_f64", "MelFilterBank", {"sr": sr}, dtype="float64", modes=("DCT2",))])

    # F2 -- the other two fused sizes: 512 at 16 kHz, 2048 at 96 kHz with twind = .02
    x2a = f32exact(harmonic_vibrato(16000.0, 0.8, f0=180.0, seed=7))
    x2b = f32exact(harmonic_vibrato(96000.0, 0.25, f0=440.0, seed=8))
    save("F2_mel16k_96k", {"x16": x2a, "x96": x2b},
         [case("mel16k", "MelFilterBank", {"sr": 16000.0}, x="x16", modes=MODES),
          case("mel96k", "MelFilterBank", {"sr": 96000.0, "twind": .02}, x="x96", modes=MODES),
          case("mel16k_n40", "MelFilterBank", {"sr": 16000.0, "n": 40, "fmin": 100.}, x="x16", modes=("DCT2", "IFFT"))])

    # F3 -- MelFilterBank(sr=8000): nwind 256 (rows route); fmax = 8000 > sr/2, so the top bands live in the upper
    # half of the spectrum (bins beyond nwind/2)
    x3 = f32exact(harmonic_vibrato(8000.0, 1.0, f0=150.0, seed=9))
    save("F3_mel8k", {"x": x3}, [case("mel8k", "MelFilterBank", {"sr": 8000.0}, modes=MODES)])
    fb = np.load(os.path.join(HERE, "F3_mel8k.npz"))["mel8k_fb"]
    assert (fb[-1, 129:] != 0).any() and (fb[-1, :128] == 0).all()

    # F4 -- silence gaps: exact zeros for whole frames, frames straddling the onsets; the -inf / nan pattern of mfcc
    n4 = 12000
    x4 = harmonic_vibrato(16000.0, n4 / 16000.0, f0=200.0, seed=10)
    x4[:2500] = 0.0
    x4[5000:7300] = 0.0
    x4[10500:] = 0.0
    x4 = f32exact(x4)
    save("F4_silence_gaps", {"x": x4}, [case("gaps16k", "MelFilterBank", {"sr": 16000.0}, modes=MODES),
                                        case("gaps8k", "MelFilterBank", {"sr": 8000.0}, modes=MODES)])

    # F5 -- the default FilterBank() (two flat bands, sr 1, nwind 256) and SpeechChunker's lp / hp / bp banks
    # (SpeechChunker.py:84-97) at nwind 4096, hop 2048
    x5 = f32exact(harmonic_vibrato(44100.0, 0.5, f0=110.0, seed=11))
    chunk = {"sr": 44100.0, "nwind": 4096, "nhop": 2048}
    save("F5_flat_banks", {"x": x5},
         [case("default", "FilterBank", {}, slice=[0, 6000]),
          case("chunk_lp", "FilterBank", chunk, fspecs=[{"freq": 5000, "mode": "lp", "sr": 44100.0}]),
          case("chunk_hp", "FilterBank", chunk, fspecs=[{"freq": 50, "mode": "hp", "sr": 44100.0}]),
          case("chunk_bp", "FilterBank", chunk, fspecs=[{"freq": [50, 5000], "mode": "bp", "sr": 44100.0}]),
          case("chunk_bs", "FilterBank", chunk, fspecs=[{"freq": [1000, 3000], "mode": "bs", "sr": 44100.0}])])

    # F6 -- a window that is no power of two (1000), align_edges on and off, and an odd one (999)
    x6 = f32exact(harmonic_vibrato(16000.0, 0.5, f0=250.0, seed=12))
    bp = [{"freq": [300, 3400], "mode": "bp", "sr": 16000.0}, {"freq": 1000, "mode": "lp", "sr": 16000.0},
          {"freq": [0., 500., 1500., 4000.], "gain": [0., 1., .25, 0.], "sr": 16000.0, "label": "vertices"}]
    save("F6_nonpow2", {"x": x6},
         [case("n1000_aligned", "FilterBank", {"nwind": 1000, "nhop": 160, "sr": 16000.0, "align_edges": True}, fspecs=bp),
          case("n1000_exact", "FilterBank", {"nwind": 1000, "nhop": 160, "sr": 16000.0, "align_edges": False}, fspecs=bp),
          case("n999_odd", "FilterBank", {"nwind": 999, "nhop": 200, "sr": 16000.0}, fspecs=bp)])

    # F7 -- TriangularFilterBank as SpeechSegmenter builds it (SpeechSegmenter.py:132-135, 186-199: octave-like flim,
    # nwind 2048 and 256) on G7's int16 Perlman samples, raw and after preemph
    g7 = np.load(os.path.join(HERE, "G7_perlman.npz"))
    x7 = g7["x"][:60000]
    assert x7.dtype == np.int16
    sr7 = float(g7["sr"])
    bands = [225., 2000., 4000., 8000., 15000.]
    save("F7_perlman_triangular", {"x": x7},
         [case("rough_int16", "TriangularFilterBank", {"flim": bands, "sr": sr7, "nwind": 2048}, dtype="int16"),
          case("rough_preemph", "TriangularFilterBank", {"flim": bands, "sr": sr7, "nwind": 2048}, dtype="int16",
               preemph={"hpFreq": 50., "Fs": sr7}),
          case("fine_preemph", "TriangularFilterBank", {"flim": bands, "sr": sr7, "nwind": 256}, dtype="int16",
               preemph={"hpFreq": 50., "Fs": sr7}, slice=[20000, 30000])],
         extra={"drop": ["x"], "x_from": np.array("G7_perlman"), "x_len": np.int64(len(x7))})

    # F8 -- edge cases: no frame at all, exactly one, a hop beyond the window, an fb row zeroed by hand
    x8 = f32exact(harmonic_vibrato(16000.0, 0.25, f0=300.0, seed=13))
    save("F8_edges", {"x": x8},
         [case("len_eq_nwind", "MelFilterBank", {"sr": 16000.0}, slice=[0, 512], modes=("DCT2", "IFFT")),
          case("len_nwind_plus1", "MelFilterBank", {"sr": 16000.0}, slice=[0, 513], modes=MODES),
          case("shorter_than_nwind", "MelFilterBank", {"sr": 16000.0}, slice=[0, 100], modes=("DCT2",)),
          case("hop_gt_nwind", "FilterBank", {"nwind": 512, "nhop": 700, "sr": 16000.0},
               fspecs=[{"freq": [300, 3400], "mode": "bp", "sr": 16000.0}]),
          case("hop_gt_nwind_rows", "FilterBank", {"nwind": 256, "nhop": 300, "sr": 16000.0},
               fspecs=[{"freq": [300, 3400], "mode": "bp", "sr": 16000.0}]),
          case("zero_row", "MelFilterBank", {"sr": 16000.0}, zero_rows=[3], modes=MODES),
          case("zero_row_rows", "MelFilterBank", {"sr": 8000.0}, zero_rows=[0, 25], modes=MODES)])


if __name__ == "__main__":
    main()
