#!/usr/bin/env python3
"""Generate the J*.npz golden vectors of the pitch-jump detector by IMPORTING the reference
(pypevoc/speech/PitchJumps.py: zscore_wind :50-64, linreg_err :67-84, linreg2_err :87-121, JumpDetector :140-270;
pypevoc/speech/SpeechChunker.py: SilenceDetector :40-164).

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_jumps.py DIR      (DIR holds the reference's `pypevoc` package)

The reference is loaded by name through importlib with the shims make_golden_segment.py uses (scipy.signal.hamming /
hanning, np.float), and with stdout silenced (PV prints its progress).  The prefix is J.  Signals are float32-exact:
seeded five-harmonic glides 150 * 2^(1.2 t/T) Hz with steps of x1.12 and x0.9 at T k/(n+1), plus 1e-3 noise.

J0  PV itself at hop == nfft: x_<sr>, and f, mag, ph, t of PV(x, sr, nfft, hop=nfft, npks=20) at 16 kHz (512 / 512) and 8 kHz
    (256 / 256).
J1-J4  `cases`, a JSON list of {name, x, sr, args (the constructor's), slope_t}.  Per case, with <n> its name: <n>_mag, _t,
    _f0, _nfft, _nhop (detect_pitch); _isel, _le (the linreg2_err series detect_jumps computed), _up_idx, _dn_idx, _up_t,
    _dn_t; _intcpts, _sumres; _times (process's return); _tc_<column> (get_jump_table's columns) or _table_raises = the
    exception's name.
J5  three glides between 1.5 s stretches of 1e-4 noise at 16 kHz: band_ / plain_ + ax, at, ath, amin, amax, clusters, tst, tend
    of SilenceDetector(fmin=50, fmax=1000) and the plain detector, and per region <k> of the band detector r<k>_* as above, made
    by calling process on the reference's own slices with the detector arguments `args`.
J6  zscore_wind (both kinds), linreg_err and linreg2_err (the three flag settings) on seeded tracks, hop 1 and 3: `calls`, a
    JSON list of {name, fn, t, x, kwargs}; <name> is the output.
_sens_*: the largest |change| of each continuous output over NPERT reruns of the reference's stages with f0 + 1e-9 g Hz (the
    float64 path's contract), mag (1 + 1e-12 g) and, for the silence detector, the frame amplitudes times 1 + 1e-9 g, g seeded
    standard normal; for J6 the track plus 1e-9 g.  The generator stops unless EVERY case is stable under these: the same
    isel, the same jump indices, the same clusters and regions.  Data only.
"""
import contextlib
import importlib
import io
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "pypevoc")):
    sys.exit("usage: make_golden_jumps.py DIR   (the directory that holds the reference's pypevoc package)")
sys.path.insert(0, sys.argv[1])

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

pj = importlib.import_module("pypevoc.speech.PitchJumps")
chunker = importlib.import_module("pypevoc.speech.SpeechChunker")
pvmod = importlib.import_module("pypevoc.PVAnalysis")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jumps_refs  # noqa: E402  (tests/jumps_refs.py: window_spreads)
NPERT = 8
J5_ARGS = {"regressor_t": 0.3, "t_threshold": 6}                     # (a 2.2 s region leaves the default 0.5 s sides little room)
COLUMNS = ("segment_time", "f_before", "f_after", "f_cent", "df", "residue_before", "residue_after", "residue_total")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def glide(sr, dur, seed, nsteps=3, noise=1e-3):
    rng = np.random.default_rng(seed)
    n = int(sr * dur)
    t = np.arange(n) / float(sr)
    f = 150.0 * 2.0**(1.2 * t / dur)
    for k in range(1, nsteps + 1):
        f[t >= dur * k / (nsteps + 1)] *= (1.12 if k % 2 else 0.9)
    ph = 2 * np.pi * np.cumsum(f) / sr
    x = sum(0.3 / h * np.sin(h * ph) for h in range(1, 6)) + noise * rng.standard_normal(n)
    return np.asarray(x, dtype=np.float32)


class LeRecorder(object):
    """Keeps what linreg2_err returned to detect_jumps."""

    def __init__(self):
        self.plain = pj.linreg2_err
        self.le = None

    def __call__(self, *a, **k):
        self.le = self.plain(*a, **k)
        return self.le

    def __enter__(self):
        pj.linreg2_err = self
        return self

    def __exit__(self, *exc):
        pj.linreg2_err = self.plain


def stages(jd):
    """detect_jumps and calc_jump_params on jd's current mag, t, f0: a dict of what they set."""
    with LeRecorder() as rec:
        jd.detect_jumps()
    jd.calc_jump_params()
    return {"isel": np.array(jd.isel), "le": np.array(rec.le), "up_idx": np.array(jd.up_jump_indices, dtype=np.int32),
            "dn_idx": np.array(jd.down_jump_indices, dtype=np.int32), "up_t": np.array(jd.up_jump_times), "dn_t": np.array(jd.down_jump_times),
            "intcpts": np.array(jd.intcpts, dtype=np.float64), "sumres": np.array(jd.sumres, dtype=np.float64)}


def absdiff(a, b):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return np.where(np.isnan(d), 0.0, d)


def detector_case(prefix, x, sr, args, slope_t, out, pert_seed=99):
    jd = pj.JumpDetector(**args)
    if slope_t is not None:
        jd.slope_t = slope_t
    quiet(jd.detect_pitch, x.astype(np.float64), sr)
    mag, t, f0 = np.array(jd.mag), np.array(jd.t), np.array(jd.f0)
    base = stages(jd)
    wle = int(jd.regressor_t / jd.pitch_t_hop)
    if base["isel"].sum() > 2 * wle:                                  # no degenerate window: neither side is specified there (JUMPS.md)
        spreads = jumps_refs.window_spreads(t[base["isel"]], f0[base["isel"]], jumps_refs.LINREG2, wle, wle)
        assert spreads.min() >= 1e-6, (prefix, "has a window whose residuals spread less than 1e-6 of |x|", spreads.min())
    out[prefix + "_mag"], out[prefix + "_t"], out[prefix + "_f0"] = mag, t, f0
    out[prefix + "_nfft"], out[prefix + "_nhop"] = np.int64(jd.nfft), np.int64(jd.nhop)
    for k, v in base.items():
        out["%s_%s" % (prefix, k)] = v
    out[prefix + "_times"] = np.sort(np.concatenate([jd.up_jump_times, jd.down_jump_times]))
    try:
        tab = jd.get_jump_table()
        for c in COLUMNS:
            out["%s_tc_%s" % (prefix, c)] = np.array(tab[c], dtype=np.float64)
    except Exception as e:
        out[prefix + "_table_raises"] = np.array(type(e).__name__)
    rng = np.random.default_rng(pert_seed)
    sens = {k: np.zeros_like(base[k]) for k in ("le", "intcpts", "sumres")}
    for _ in range(NPERT):
        jd.f0 = f0 + 1e-9 * rng.standard_normal(f0.shape)
        jd.mag = mag * (1.0 + 1e-12 * rng.standard_normal(mag.shape))
        again = stages(jd)
        for k in ("isel", "up_idx", "dn_idx"):
            assert np.array_equal(again[k], base[k]), (prefix, k, "is not stable: choose another seed")
        for k in sens:
            assert np.array_equal(np.isnan(again[k]), np.isnan(base[k])), (prefix, k)
            sens[k] = np.maximum(sens[k], absdiff(again[k], base[k]))
    for k, v in sens.items():
        out["%s_sens_%s" % (prefix, k)] = v
    out[prefix + "_stable"] = np.bool_(True)
    print("%-14s sr %6d nfft %4d hop %4d frames %3d selected %3d up %s down %s max|le| %.1f sens le %.1e intcpts %.1e sumres %.1e" % (
        prefix, sr, jd.nfft, jd.nhop, len(t), int(base["isel"].sum()), base["up_idx"], base["dn_idx"],
        np.abs(base["le"]).max() if len(base["le"]) else 0.0, sens["le"].max() if sens["le"].size else 0.0,
        sens["intcpts"].max() if sens["intcpts"].size else 0.0, sens["sumres"].max() if sens["sumres"].size else 0.0))
    return base


def save(fname, out):
    path = os.path.join(HERE, fname + ".npz")
    np.savez_compressed(path, **out)
    print(fname, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


def detector_file(fname, signals, cases):
    out = dict(signals)
    for c in cases:
        detector_case(c["name"], signals[c["x"]], c["sr"], c["args"], c.get("slope_t"), out)
    out["cases"] = np.array(json.dumps(cases))
    save(fname, out)


def silence_record(tag, x, sr, out, **kw):
    sd = chunker.SilenceDetector(x.astype(np.float64), sr, **kw)
    ax = np.array(sd.ax)
    for k in ("ax", "at", "clusters", "tst", "tend"):
        out["%s_%s" % (tag, k)] = np.array(getattr(sd, k))
    for k in ("ath", "amin", "amax"):
        out["%s_%s" % (tag, k)] = np.float64(getattr(sd, k))
    # the walk and the percentiles under amplitudes times 1 + 1e-9 g: 20 log10 of that is ax + 20 log10(1 + 1e-9 g)
    rng = np.random.default_rng(7)
    sens, sens_ax = 0.0, np.zeros_like(ax)
    for _ in range(NPERT):
        sd.ax = ax + 20 * np.log10(1.0 + 1e-9 * rng.standard_normal(ax.shape))
        sens_ax = np.maximum(sens_ax, absdiff(sd.ax, ax))
        sd._percentile_discriminator(pct=5)
        tst, tend = sd._clusters_to_time_int(min_int=0.1, max_int=5)
        assert np.array_equal(sd.clusters, out[tag + "_clusters"]) and np.array_equal(tst, out[tag + "_tst"]) and \
            np.array_equal(tend, out[tag + "_tend"]), (tag, "is not stable")
        sens = max(sens, abs(sd.ath - out[tag + "_ath"]))
    out[tag + "_sens_ath"] = np.float64(sens)
    out[tag + "_sens_ax"] = sens_ax                                   # per frame, as every continuous output
    print("%-6s frames %d regions %s .. %s ath %.3f sens %.1e sens ax %.1e .. %.1e" % (
        tag, len(ax), out[tag + "_tst"], out[tag + "_tend"], out[tag + "_ath"], sens, sens_ax.min(), sens_ax.max()))
    return out[tag + "_tst"], out[tag + "_tend"]


def main():
    # J0: PV at hop == nfft
    out = {}
    for sr, nfft in ((16000, 512), (8000, 256)):
        x = glide(sr, 1.0, 40 + nfft, nsteps=1)
        pv = pvmod.PV(x.astype(np.float64), sr, nfft=nfft, hop=nfft)
        quiet(pv.run_pv)
        out["x_%d" % sr] = x
        for k in ("f", "mag", "ph", "t"):
            out["%s_%d" % (k, sr)] = np.array(getattr(pv, k))
        out["f0_%d" % sr] = np.array(pv.calc_f0())
        print("J0 sr %d nfft %d frames %d" % (sr, nfft, len(pv.t)))
    save("J0_pv_hop_nfft", out)

    # J1-J3: process at the three rates
    for k, (sr, dur, seed) in enumerate(((16000, 6.0, 1), (22050, 6.0, 2), (44100, 4.0, 3))):
        detector_file("J%d_process_%d" % (k + 1, sr), {"x": glide(sr, dur, seed)}, [{"name": "p", "x": "x", "sr": sr, "args": {}}])

    # J4: options and edges, 16 kHz
    sig = {"x": glide(16000, 4.0, 4, nsteps=2), "x_smooth": glide(16000, 3.0, 5, nsteps=0), "x_short": glide(16000, 1.2, 6, nsteps=1),
           "x_zero": np.zeros(24000, dtype=np.float32)}
    detector_file("J4_options_edges", sig, [
        {"name": "reg03", "x": "x", "sr": 16000, "args": {"regressor_t": 0.3}},
        {"name": "thr20", "x": "x", "sr": 16000, "args": {"t_threshold": 20}},
        {"name": "mag05", "x": "x", "sr": 16000, "args": {"mag_threshold": 0.05}},
        {"name": "slope02", "x": "x", "sr": 16000, "args": {}, "slope_t": 0.2},
        {"name": "nojump", "x": "x_smooth", "sr": 16000, "args": {}},
        {"name": "short", "x": "x_short", "sr": 16000, "args": {}},
        {"name": "silence", "x": "x_zero", "sr": 16000, "args": {}}])

    # J5: three glides between stretches of faint noise
    sr = 16000
    rng = np.random.default_rng(50)
    parts = []
    for k in range(3):
        parts.append(np.asarray(1e-4 * rng.standard_normal(int(1.5 * sr)), dtype=np.float32))
        parts.append(glide(sr, 2.2, 51 + k, nsteps=1))
    parts.append(np.asarray(1e-4 * rng.standard_normal(int(1.5 * sr)), dtype=np.float32))
    x = np.concatenate(parts)
    out = {"x": x, "sr": np.int64(sr)}
    tst, tend = silence_record("band", x, sr, out, fmin=50, fmax=1000)
    silence_record("plain", x, sr, out)
    assert len(tst) == 3 and len(out["plain_tst"]) == 3
    for k, (a, b) in enumerate(zip(tst, tend)):
        detector_case("r%d" % k, x[int(a * sr):int(b * sr)], sr, J5_ARGS, None, out)
    out["args"] = np.array(json.dumps(J5_ARGS))
    save("J5_regions", out)

    # J6: the windowed statistics on seeded tracks
    rng = np.random.default_rng(60)
    n = 90
    t = np.cumsum(0.02 + 0.002 * rng.random(n))
    xa = 200.0 + 30.0 * t + 0.5 * rng.standard_normal(n)
    xa[n // 2:] += 12.0
    xb = 180.0 * 2.0**(0.4 * t) + 0.3 * rng.standard_normal(n)
    xb[30:] *= 0.93
    out = {"t": t, "xa": xa, "xb": xb}
    calls = []
    for xn in ("xa", "xb"):
        for hop in (1, 3):
            for wl, wr in ((5, 5), (12, 7)):
                tag = "%s_h%d_w%d_%d" % (xn, hop, wl, wr)
                calls.append({"name": "zmean_" + tag, "fn": "zscore_wind", "x": xn, "kwargs": {"wleft": wl, "wright": wr, "hop": hop, "kind": "mean"}})
                calls.append({"name": "zmedian_" + tag, "fn": "zscore_wind", "x": xn, "kwargs": {"wleft": wl, "wright": wr, "hop": hop, "kind": "median"}})
                calls.append({"name": "linreg_" + tag, "fn": "linreg_err", "x": xn, "t": "t", "kwargs": {"wleft": wl, "wright": wr, "hop": hop}})
                for ul, ur in ((True, True), (True, False), (False, True)):
                    calls.append({"name": "linreg2_%s_l%d_r%d" % (tag, ul, ur), "fn": "linreg2_err", "x": xn, "t": "t",
                                  "kwargs": {"wleft": wl, "wright": wr, "hop": hop, "use_l": ul, "use_r": ur}})
    for c in calls:
        fn = getattr(pj, c["fn"])
        xs = out[c["x"]]
        args = (out["t"], xs) if "t" in c else (xs,)
        base = fn(*args, **c["kwargs"])
        out[c["name"]] = base
        prng = np.random.default_rng(61)
        sens = np.zeros_like(base)
        for _ in range(NPERT):
            xp = xs + 1e-9 * prng.standard_normal(xs.shape)
            sens = np.maximum(sens, absdiff(fn(*((out["t"], xp) if "t" in c else (xp,)), **c["kwargs"]), base))
        out["sens_" + c["name"]] = sens
    out["calls"] = np.array(json.dumps(calls))
    print("J6 %d calls, largest sens %.1e" % (len(calls), max(out["sens_" + c["name"]].max() for c in calls)))
    save("J6_winstat", out)


if __name__ == "__main__":
    main()
