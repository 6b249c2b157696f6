"""k_yin.hip (SoundUtils.f0yin) against tests/yin_refs.py on every frame of every case: the integer pick and the flag
identical, tau / freq / conf inside the derived rounding bounds, the ties of the S == 0 rule ordered as the statements order
them.  The reference's own margins over these frames are checked in test_yin_refs_cpu.py.  `-s` prints the worst error
per case (YIN.md, "Measured errors")."""
import ctypes
import functools
import math

import numpy as np
import pytest

from . import yin_refs as R
from .test_yin_refs_cpu import impulse_pairs

pytestmark = pytest.mark.gpu

KEYS = ("freq", "conf", "tau", "pick", "flag")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def run_case(name):
    from pypevoc_amd.SoundUtils import f0yin
    case = R.CASE[name]
    return f0yin(R.signal(case.sig), R.SR, nwind=case.nwind, hop=case.hop, full=True, **dict(case.kw))


def compare(name, res, refs):
    """Every frame of res against refs; returns (worst |error| / bound, worst |dtau|, frames with an unbounded tau)."""
    assert len(res["freq"]) == len(refs) > 0
    worst, wtau, unbounded = 0.0, 0.0, 0
    for i, ref in enumerate(refs):
        got = (res["pick"][i], res["tau"][i], res["freq"][i], res["conf"][i], res["flag"][i])
        assert R.frame_errors(ref, *got) == [], (name, i)
        w, dt = R.worst_ratio(ref, got[1], got[2], got[3])
        worst, wtau = max(worst, w), max(wtau, dt)
        unbounded += ref.b_tau == math.inf
    return worst, wtau, unbounded


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_case_matches_reference(name):
    case = R.CASE[name]
    res = run_case(name)
    starts, lo, hi, tol = R.case_params(case)
    assert np.array_equal(res["starts"], starts)
    assert np.array_equal(res["time"], (starts + case.nwind / 2.0) / R.SR)
    worst, wtau, unbounded = compare(name, res, R.case_refs(name))
    print("%s: %d frames, worst |error| / bound %.3g, worst |dtau| %.3g, %d frames with den ~ 0" % (name, len(starts), worst, wtau, unbounded))


def test_picks_at_both_ends_of_the_lag_range():
    for name, end in (("a_pick_lo", 1), ("a_pick_hi", 2)):
        bound = R.case_params(R.CASE[name])[end]
        picks = run_case(name)["pick"]
        assert (picks == bound).any(), (name, bound, picks)
        assert ((picks >= R.case_params(R.CASE[name])[1]) & (picks <= R.case_params(R.CASE[name])[2])).all()


def test_every_split_of_the_work_runs():
    from pypevoc_amd.SoundUtils import f0yin_rows, yin_last_kernels
    for name, kernel in (("a256", "k_yin/seg4"), ("b1024", "k_yin/seg2"), ("b8192", "k_yin")):
        case = R.CASE[name]
        row = f0yin_rows(R.signal(case.sig), [0], case.nwind, R.SR)
        assert yin_last_kernels() == kernel
        assert same_bits(row["tau"], run_case(name)["tau"][:1])


def test_window_beyond_the_maximum_is_unsupported():
    import pypevoc_amd
    from pypevoc_amd import _lib
    from pypevoc_amd.SoundUtils import f0yin
    x = R.signal("b8192")
    with pytest.raises(pypevoc_amd.PvxError) as e:
        f0yin(x, R.SR, nwind=8193, hop=1024)
    assert "status -5" in str(e.value) and "8193" in str(e.value)
    lib = _lib.load()
    starts = np.zeros(1, dtype=np.int64)
    out = np.zeros(2)
    rc = lib.pvx_yin(_lib.dptr(x), len(x), starts.ctypes.data_as(_lib.c_int64_p), 1, 8193, 2, 100, 0.15, float(R.SR),
                     _lib.dptr(out[:1]), _lib.dptr(out[1:]), None, None, None)
    assert rc == -5                                                  # PVX_ERR_UNSUPPORTED
    for nwind, lo, hi in ((7, 2, 2), (256, 1, 100), (256, 50, 49), (256, 2, 127)):
        assert lib.pvx_yin(_lib.dptr(x), len(x), starts.ctypes.data_as(_lib.c_int64_p), 1, nwind, lo, hi, 0.15, float(R.SR),
                           _lib.dptr(out[:1]), _lib.dptr(out[1:]), None, None, None) == -2      # PVX_ERR_INVALID
    # tau, flag and pick are optional
    assert lib.pvx_yin(_lib.dptr(x), len(x), starts.ctypes.data_as(_lib.c_int64_p), 1, 256, 2, 126, 0.15, float(R.SR),
                       _lib.dptr(out[:1]), _lib.dptr(out[1:]), None, None, None) == 1
    ref = R.yin_frame_ref(x[:256], 0.15, 2, 126, R.SR)
    assert R.frame_errors(ref, ref.pick, ref.tau, out[0], out[1], ref.flag) == []


def test_silent_and_constant_frames():
    res, refs = run_case("d_silence"), R.case_refs("d_silence")
    silent = res["flag"] == R.SILENT
    assert silent.sum() == sum(r.flag == R.SILENT for r in refs) >= 8
    for k in ("freq", "conf", "tau"):
        assert same_bits(res[k][silent], np.zeros(silent.sum()))     # +0.0
    assert not res["pick"][silent].any()
    x = R.signal("szero")
    starts = R.case_params(R.CASE["d_silence"])[0]
    kinds = set()
    for s, f in zip(starts, res["flag"]):
        fr = x[s:s + 256]
        if not fr.any():
            kinds.add("zero")
            assert f == R.SILENT
        elif (fr == fr[0]).all():
            kinds.add("dc")
            assert f == R.SILENT
        elif not fr[:128].any():
            kinds.add("half")
            assert f != R.SILENT
    assert kinds == {"zero", "dc", "half"}


def test_noise_takes_the_fallback():
    for name in ("e_noise256", "e_noise1024"):
        assert (run_case(name)["flag"] == R.FALLBACK).all()


def test_out_of_bounds_tolerance_is_the_default(capsys):
    from pypevoc_amd.SoundUtils import f0yin
    x = R.signal("harm256")
    base = run_case("a256")
    for tolerance in (1.5, 0.0, -1.0):
        res = f0yin(x, R.SR, nwind=256, hop=64, tolerance=tolerance, full=True)
        assert "Tolerance not set" in capsys.readouterr().err
        for k in KEYS:
            assert same_bits(res[k], base[k]), (tolerance, k)
    other = f0yin(R.signal("noise256"), R.SR, nwind=256, hop=128, tolerance=0.5, full=True)
    assert same_bits(other["pick"], run_case("e_noise_tol05")["pick"])


def test_exact_integer_period():
    from pypevoc_amd.SoundUtils import f0yin
    res = f0yin(impulse_pairs(512 + 80 * 4), R.SR, nwind=512, hop=80, full=True)
    assert len(res["pick"]) == 4
    assert (res["pick"] == 80).all() and (res["flag"] == 0).all()
    assert same_bits(res["conf"], np.ones(4))
    assert (np.abs(res["tau"] - 80.0) <= 0.5).all()


def test_the_references_call():
    from pypevoc_amd.SoundUtils import aubio_f0yin, f0yin
    x = R.signal("b1024")
    freq, time, conf = aubio_f0yin(x, R.SR, 1024, 512)
    assert len(freq) == len(time) == len(conf) == 6
    res = run_case("b1024")
    assert same_bits(freq, res["freq"]) and same_bits(conf, res["conf"]) and same_bits(time, res["time"])
    f2, t2, c2 = f0yin(x, R.SR, 1024, 512)
    assert same_bits(f2, freq) and same_bits(c2, conf)
    assert (np.abs(freq - 220.0) < 15.0).all() and (conf > 0.9).all()
