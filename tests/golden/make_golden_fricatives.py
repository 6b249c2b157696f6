#!/usr/bin/env python3
"""Generate the Z*.npz golden vectors of the fricative descriptors by IMPORTING the reference (pypevoc/speech/SpeechAnalysis.py:
FricativeDataFromSnip :349-384) and scipy.signal.welch, which it calls.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_fricatives.py /path/to/the/reference/checkout

(or PYPEVOC_REFERENCE in the environment; scipy is needed here and nowhere else).  pypevoc.speech imports only with
scipy.signal.hamming = scipy.signal.windows.hamming set first (a default argument, SpeechAnalysis.py:83).

Signals are float32-exact: seeded noise through a two-pole resonance plus a white floor of 5 % of it, so that no bin is empty;
one int16 signal has an offset of about 3000 counts under noise of about 300, so that the mean removal matters.

Each file holds its signals and `cases`, a JSON list of {name, x: key of the signal, dtypes: the sample types the tests run the
case in, starts, L, nwind, sr}.  Per case: <name>_ref [rows][8], the reference's values in the order f_max, rms, slope_left,
slope_right, cent, stdev, skew, kurt; <name>_psd [rows][nb], scipy.signal.welch's rows; <name>_freq [nb]; <name>_imax [rows].

A case is REFUSED unless, for every row,
  1. the second-largest bin is <= (1 - 1e-6) x the largest: imax, and with it both strict comparisons of the refinement, cannot
     flip under the tests' 1e-9 per bin;
  2. min S >= 1e-8 max S;
  3. the reference is within 1e-11 relative of an np.longdouble evaluation of the formulas (tests/fricative_refs.py with
     scipy.fft on np.longdouble), for the psd per bin and for the eight values.
Data only."""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PYPEVOC_REFERENCE")
if not REFERENCE:
    sys.exit(__doc__)
sys.path.insert(0, REFERENCE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import scipy.fft  # noqa: E402
import scipy.signal  # noqa: E402
import scipy.signal.windows  # noqa: E402

warnings.simplefilter("ignore")
scipy.signal.hamming = scipy.signal.windows.hamming

from pypevoc.speech import SpeechAnalysis as sa  # noqa: E402

import fricative_refs as R  # noqa: E402

LD = np.longdouble
SELF_BOUND = 1e-11


def resonant_noise(n, sr, fres, r, seed):
    """Seeded noise through a two-pole resonance at fres, plus a white floor of 5 % of it."""
    rng = np.random.default_rng(seed)
    th = 2 * np.pi * fres / sr
    y = scipy.signal.lfilter([1.0], [1.0, -2 * r * np.cos(th), r * r], rng.standard_normal(n))
    y = y / y.std()
    return y + 0.05 * rng.standard_normal(n)


def run_case(c, arrays, out):
    x = arrays[c["x"]]
    L, nwind, sr = c["L"], c["nwind"], c["sr"]
    ref, psd, imaxs = [], [], []
    worst = dict(top=0.0, floor=np.inf, psd=0.0, val=0.0)
    for s in c["starts"]:
        w = x[s:s + L].astype(np.float64)                             # (scipy computes a float32 signal's spectrum in float32)
        assert len(w) == L, (c["name"], s)
        d = sa.FricativeDataFromSnip(w, nwind=nwind, sr=sr)
        freq, S = scipy.signal.welch(w, nperseg=nwind, fs=sr)
        srt = np.sort(S)
        worst["top"] = max(worst["top"], srt[-2] / srt[-1])
        worst["floor"] = min(worst["floor"], srt[0] / srt[-1])
        ld, lfreq, lS = R.fricative_snip(w, nwind, sr, LD, scipy.fft.rfft)
        assert lS.dtype == LD and np.array_equal(lfreq, freq)
        worst["psd"] = max(worst["psd"], float(np.max(np.abs(S - lS) / lS)))
        assert ld["imax"] == int(np.argmax(S))
        for k in R.REFERENCE_KEYS:
            worst["val"] = max(worst["val"], float(abs(d[k] - ld[k]) / abs(ld[k])))
        ref.append([float(d[k]) for k in R.REFERENCE_KEYS])
        psd.append(S)
        imaxs.append(int(np.argmax(S)))
    print("  %-18s rows %2d nb %4d  second/top %.3f  min/max %.1e  reference vs long double: psd %.1e values %.1e"
          % (c["name"], len(ref), len(freq), worst["top"], worst["floor"], worst["psd"], worst["val"]))
    assert worst["top"] <= 1 - 1e-6, (c["name"], "condition 1", worst["top"])
    assert worst["floor"] >= 1e-8, (c["name"], "condition 2", worst["floor"])
    assert worst["psd"] <= SELF_BOUND and worst["val"] <= SELF_BOUND, (c["name"], "condition 3", worst)
    out[c["name"] + "_ref"] = np.array(ref)
    out[c["name"] + "_psd"] = np.array(psd)
    out[c["name"] + "_freq"] = freq
    out[c["name"] + "_imax"] = np.array(imaxs, dtype=np.int32)


def write(fname, arrays, cases):
    print(fname)
    out = dict(arrays)
    for c in cases:
        run_case(c, arrays, out)
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, fname + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("  -> %s %d bytes" % (os.path.basename(path), size))
    assert size <= 150000, size
    return size


def case(name, x, starts, L, nwind, sr, dtypes=("float32",)):
    return {"name": name, "x": x, "dtypes": list(dtypes), "starts": [int(s) for s in starts], "L": int(L), "nwind": int(nwind), "sr": sr}


def main():
    sr = 16000
    n = 6000
    x16 = np.asarray(resonant_noise(n, sr, 3100.0, 0.93, 41), dtype=np.float32)
    lo16 = np.asarray(resonant_noise(n, sr, 900.0, 0.9, 42), dtype=np.float32)
    i16 = np.round(3000 + 300 * resonant_noise(n, sr, 4500.0, 0.95, 43)).astype(np.int16)
    total = 0
    # ---- Z1: the rows route.  The reference's default nwind (7 segments); nper = 300 of nwind 333; odd nper; L = nwind + 1
    total += write("Z1_rows", {"x16": x16, "lo16": lo16},
                   [case("w256", "x16", (0, 1700, n - 1024), 1024, 256, sr),
                    case("w333_l300", "lo16", (5, 2001), 300, 333, sr),
                    case("w256_l255", "x16", (100, 3000), 255, 256, sr),
                    case("w256_l257", "lo16", (0, n - 257), 257, 256, sr)])
    # ---- Z2: the fused route at 512.  13 snippets of two segments (more than a workgroup has waves), unsorted and overlapping,
    # one at sample 0 and one ending on the last sample; one segment exactly, and one sample more
    starts = (2100, 0, 700, 701, 5232 - 768, n - 768, 64, 3000, 1500, 2999, 4000, 333, 2500)
    total += write("Z2_fused512", {"x16": x16, "lo16": lo16},
                   [case("w512_l768", "x16", starts, 768, 512, sr),
                    case("w512_l512", "lo16", (1000, n - 512), 512, 512, sr),
                    case("w512_l513", "lo16", (999, 0), 513, 512, sr)])
    # ---- Z3: 1024 on the int16 signal with its offset, the same samples as float32 and float64; 2048 with three segments
    long16 = np.asarray(resonant_noise(9000, sr, 2000.0, 0.97, 44), dtype=np.float32)
    total += write("Z3_fused", {"i16": i16, "long16": long16},
                   [case("w1024_i16", "i16", (0, 1111, 2048, n - 1024), 1024, 1024, sr, ("int16", "float32", "float64")),
                    case("w2048_l4096", "long16", (300, 9000 - 4096), 4096, 2048, sr)])
    print("total %d bytes" % total)
    assert total <= 300000, total


if __name__ == "__main__":
    main()
