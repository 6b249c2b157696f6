"""Pitch jumps without a GPU: tests/jumps_refs.py -- the closed forms the kernels use -- against the reference's recorded
outputs (J1 .. J6, tests/golden/make_golden_jumps.py), the host half of SilenceDetector on the recorded amplitudes, the
entry points' argument checks and limits, the stubs and the package's exports.  JUMPS.md has the bounds: discrete outputs
equal, continuous ones within 2 * sens element by element."""
import json
import os

import numpy as np
import pytest

from . import jumps_refs as R
from .conftest import GOLDEN


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def detector_cases():
    """(id, fixture, prefix, constructor arguments, slope_t) of every recorded JumpDetector case."""
    out = []
    for fname in ("J1_process_16000", "J2_process_22050", "J3_process_44100", "J4_options_edges"):
        g = load(fname)
        for c in json.loads(str(g["cases"])):
            out.append(("%s-%s" % (fname[:2], c["name"]), g, c["name"], c["args"], c.get("slope_t"), c))
    g = load("J5_regions")
    for k in range(3):
        out.append(("J5-r%d" % k, g, "r%d" % k, json.loads(str(g["args"])), None, None))
    return out


CASES = detector_cases()


def within(a, b, sens, what):
    a, b, sens = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(sens, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    d = np.where(np.isnan(a), 0.0, np.abs(a - b))
    bad = d > 2 * sens
    assert not bad.any(), (what, int(bad.sum()), float(d[bad].max()), float(sens[bad].min()))
    return float(d.max()) if d.size else 0.0


def check_against_fixture(got, g, p, what):
    """got: a dict with isel, le, up_idx, dn_idx, intcpts, sumres; g[p + '_...']: the reference's."""
    assert np.array_equal(got["isel"], g[p + "_isel"]), what
    assert np.array_equal(got["up_idx"], g[p + "_up_idx"]) and np.array_equal(got["dn_idx"], g[p + "_dn_idx"]), what
    worst = {"le": within(got["le"], g[p + "_le"], g[p + "_sens_le"], what + " le")}
    if g[p + "_intcpts"].size:
        worst["intcpts"] = within(got["intcpts"], g[p + "_intcpts"], g[p + "_sens_intcpts"], what + " intcpts")
        worst["sumres"] = within(got["sumres"], g[p + "_sumres"], g[p + "_sens_sumres"], what + " sumres")
    else:
        assert np.asarray(got["intcpts"]).size == 0 and np.asarray(got["sumres"]).size == 0, what
    return worst


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_reproduces_the_recorded_detector(case):
    cid, g, p, args, slope_t, _ = case
    kw = {k: args[k] for k in ("pitch_t_hop", "regressor_t", "t_threshold", "mag_threshold") if k in args}
    got = R.detect(g[p + "_mag"], g[p + "_t"], g[p + "_f0"], slope_t=slope_t, **kw)
    worst = check_against_fixture(got, g, p, cid)
    assert not got["jump_status"].any()
    print(cid, worst)


def test_restatement_reproduces_the_recorded_window_statistics():
    g = load("J6_winstat")
    kinds = {"zscore_wind": None, "linreg_err": R.LINREG, "linreg2_err": R.LINREG2}
    for c in json.loads(str(g["calls"])):
        kw = c["kwargs"]
        kind = kinds[c["fn"]]
        if kind is None:
            kind = R.ZMEAN if kw["kind"] == "mean" else R.ZMEDIAN
        flags = (R.USE_L if kw.get("use_l", True) else 0) | (R.USE_R if kw.get("use_r", True) else 0)
        x = g[c["x"]]
        got = R.winstat(g["t"] if "t" in c else x, x, kind, kw["wleft"], kw["wright"], kw["hop"], flags)
        within(got, g[c["name"]], g["sens_" + c["name"]], c["name"])
        assert R.window_spreads(g["t"], x, kind, kw["wleft"], kw["wright"], kw["hop"]).min() >= 1e-6, c["name"]


def test_the_three_arithmetics_agree_to_rounding():
    g = load("J1_process_16000")
    t, f0 = g["p_t"], g["p_f0"]
    ld = R.winstat(t, f0, R.LINREG2, 25, 25, ar=R.LONG)
    for ar in (R.PLAIN, R.BFLY):
        d = R.rel_distance(R.winstat(t, f0, R.LINREG2, 25, 25, ar=ar), ld)
        assert 0 < d < 1e-9, (ar.name, d)


def test_silence_detector_host_half_on_the_recorded_amplitudes():
    """The percentiles and the walk over the clusters are host numpy in the mirror as in the reference: from the recorded
    frame amplitudes they give the recorded clusters and regions."""
    from pypevoc_amd.speech.chunker import SilenceDetector
    g = load("J5_regions")
    sr = int(g["sr"])
    for tag in ("band", "plain"):
        sd = SilenceDetector.__new__(SilenceDetector)
        sd.sr, sd.nwind = sr, int(0.92 * sr)
        sd.nfr = int(sd.nwind / 2)
        sd.ax, sd.at = g[tag + "_ax"], g[tag + "_at"]
        sd._percentile_discriminator(pct=5)
        assert sd.ath == g[tag + "_ath"] and sd.amin == g[tag + "_amin"] and sd.amax == g[tag + "_amax"]
        assert np.array_equal(sd.clusters, g[tag + "_clusters"])
        tst, tend = sd._clusters_to_time_int(min_int=0.1, max_int=5)
        assert np.array_equal(tst, g[tag + "_tst"]) and np.array_equal(tend, g[tag + "_tend"]) and len(tst) == 3


# ---- the entry points' argument checks: answered before a device is needed ------------------------------------------------
def _lib():
    from pypevoc_amd import _lib as L
    return L, L.load()


def test_winstat_refuses_window_sides_beyond_the_limits_without_a_launch():
    L, lib = _lib()
    n = 600
    t, x, out = np.arange(n, dtype=np.float64), np.zeros(n), np.empty(n)

    def call(kind=3, wl=5, wr=5, hop=1, flags=3, rows=1, nmax=n, ln=None):
        return lib.pvx_winstat(L.dptr(t), L.dptr(x), ln, rows, nmax, kind, wl, wr, hop, flags, L.dptr(out))

    for kind in range(4):
        assert call(kind=kind, wl=2) == L.PVX_ERR_UNSUPPORTED and call(kind=kind, wl=257) == L.PVX_ERR_UNSUPPORTED
        assert call(kind=kind, wr=2) == L.PVX_ERR_UNSUPPORTED and call(kind=kind, wr=257) == L.PVX_ERR_UNSUPPORTED
        assert call(kind=kind, wr=-1) == L.PVX_ERR_UNSUPPORTED                  # the reference's negative-wright branch
        assert lib.pvx_jumps_last_kernels() == b""
    assert call(kind=3, wr=0) == L.PVX_ERR_UNSUPPORTED                          # LINREG2 needs a right side
    assert call(kind=4) == L.PVX_ERR_INVALID and call(kind=-1) == L.PVX_ERR_INVALID
    assert call(hop=0) == L.PVX_ERR_INVALID and call(flags=4) == L.PVX_ERR_INVALID
    assert call(rows=-1) == L.PVX_ERR_INVALID and call(nmax=-1) == L.PVX_ERR_INVALID
    assert call(rows=1 << 20, nmax=1 << 12) == L.PVX_ERR_INVALID                # rows * nmax >= 2^31
    bad = np.array([n + 1], dtype=np.int32)
    assert call(ln=bad.ctypes.data_as(L.c_int32_p)) == L.PVX_ERR_INVALID
    assert call(rows=0) == 0 and call(nmax=0) == 1                              # nothing to do: no device needed
    assert lib.pvx_winstat(None, None, None, 1, n, 0, 5, 5, 1, 0, None) == L.PVX_ERR_INVALID
    assert lib.pvx_winstat_dev(None, None, None, 1, n, 3, 2, 5, 1, 3, None, None) == L.PVX_ERR_UNSUPPORTED


def test_select_and_pick_refuse_bad_arguments():
    L, lib = _lib()
    n = 16
    a = np.zeros(n)
    i32 = np.zeros(n, dtype=np.int32)
    ip = i32.ctypes.data_as(L.c_int32_p)

    def sel(rows=1, nmax=n, K=1):
        return lib.pvx_jump_select(L.dptr(a), L.dptr(a), L.dptr(a), None, rows, nmax, K, 0.01, L.dptr(a), ip, L.dptr(a), L.dptr(a), ip, ip)

    assert sel(K=4097) == L.PVX_ERR_UNSUPPORTED and sel(K=0) == L.PVX_ERR_INVALID
    assert sel(rows=-1) == L.PVX_ERR_INVALID and sel(nmax=-1) == L.PVX_ERR_INVALID and sel(rows=0) == 0
    assert lib.pvx_jump_select(None, None, None, None, 1, n, 1, 0.01, None, None, None, None, None, None) == L.PVX_ERR_INVALID
    assert lib.pvx_jump_select_resident(None, L.dptr(a), 0.01, L.dptr(a), ip, L.dptr(a), L.dptr(a), ip, ip) == L.PVX_ERR_INVALID

    def pick(rows=1, nmax=n, nsl=5, maxjump=4):
        return lib.pvx_jump_pick(L.dptr(a), L.dptr(a), L.dptr(a), None, rows, nmax, 10.0, nsl, maxjump, ip, ip, ip, L.dptr(a), L.dptr(a), ip, None)

    assert pick(nsl=0) == L.PVX_ERR_INVALID and pick(maxjump=-1) == L.PVX_ERR_INVALID and pick(rows=-1) == L.PVX_ERR_INVALID
    assert pick(rows=0) == 0
    assert lib.pvx_jump_pick(L.dptr(a), L.dptr(a), L.dptr(a), None, 1, n, 10.0, 5, 4, None, None, ip, None, None, None, None) == L.PVX_ERR_INVALID
    assert lib.pvx_jumps_last_kernels() == b""


def test_python_layer_validates_before_it_launches():
    from pypevoc_amd.speech import jumps as J
    x = np.linspace(0., 1., 40)
    for fn in (J.zscore_wind, lambda v, **kw: J.linreg_err(v, v, **kw), lambda v, **kw: J.linreg2_err(v, v, **kw)):
        for kw in ({"wleft": 2}, {"wleft": 257}, {"wright": 257}, {"wright": -1}, {"wright": 2}):
            with pytest.raises(NotImplementedError):
                fn(x, **kw)
    with pytest.raises(NotImplementedError):
        J.linreg2_err(x, x, wright=0)
    with pytest.raises(ValueError):
        J.zscore_wind(x, kind="mode")
    with pytest.raises(ValueError):
        J.linreg_err(x[:-1], x)
    with pytest.raises(ValueError):
        J.linreg_err(x, x, hop=0)
    assert J.zscore_wind(np.zeros(0)).shape == (0,)                   # nothing to launch
    assert J.nextpow2(2 * 16000 / 70) == 512 and J.nextpow2(0.02 * 16000) == 512 and J.nextpow2(0.02 * 44100) == 1024
    with pytest.raises(NotImplementedError):
        J.jumps_rows(np.zeros((1, 8)), np.zeros((1, 8)), np.zeros((1, 8)), regressor_t=0.02)      # wle = 1


def test_detector_constructor_and_host_methods():
    from pypevoc_amd.speech import JumpDetector
    jd = JumpDetector()
    assert (jd.min_freq, jd.pitch_t_hop, jd.regressor_t, jd.t_threshold, jd.mag_threshold, jd.slope_t) == (70, 0.02, 0.5, 10, 0.01, 0.5)
    jd = JumpDetector(regressor_t=0.3)
    assert jd.slope_t == 0.3
    # the table's columns from attributes set by hand (host arithmetic only)
    g = load("J1_process_16000")
    jd.up_jump_times, jd.down_jump_times = g["p_up_t"], g["p_dn_t"]
    jd.intcpts, jd.sumres = g["p_intcpts"], g["p_sumres"]
    cols = jd.jump_table_columns()
    assert list(cols) == ["segment_time", "f_before", "f_after", "f_cent", "df", "residue_before", "residue_after", "residue_total"]
    for k, v in cols.items():
        assert np.array_equal(v, g["p_tc_" + k]), k
    tab = jd.get_jump_table()
    assert list(tab.columns) == list(cols) and np.array_equal(tab["df"].to_numpy(), g["p_tc_df"])
    jd.up_jump_times = jd.down_jump_times = np.zeros(0)
    jd.intcpts = jd.sumres = np.array([])
    with pytest.raises(IndexError):                                   # the reference's outcome without a jump (J4: nojump, short, silence)
        jd.jump_table_columns()
    for name in ("nojump", "short", "silence"):
        assert str(load("J4_options_edges")[name + "_table_raises"]) == "IndexError"


def test_stubs_raise_with_the_reference_lines():
    from pypevoc_amd.speech import chunker, jumps
    for fn, where in ((jumps.avg_interpolator, "PitchJumps.py:124"), (jumps.file_reader, "PitchJumps.py:292"),
                      (jumps.pitch_jump_file, "PitchJumps.py:305"), (chunker.MultiChannelSegmenter, "SpeechChunker.py:216"),
                      (chunker.analyse_rec, "SpeechChunker.py:411"), (chunker.process_file_list, "SpeechChunker.py:444"),
                      (chunker.main, "SpeechChunker.py:497")):
        with pytest.raises(NotImplementedError) as e:
            fn()
        assert where in str(e.value), (where, str(e.value))
    sd = chunker.SilenceDetector.__new__(chunker.SilenceDetector)
    for name, where in (("to_textgrid", ":166"), ("recognise", ":181"), ("_k_means_discriminator", ":100")):
        with pytest.raises(NotImplementedError) as e:
            getattr(sd, name)()
        assert "SpeechChunker.py" + where in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        chunker.SilenceDetector(np.zeros(10), 1, method="kmeans")
    assert "SpeechChunker.py:100" in str(e.value)


def test_speech_package_exports_the_jump_modules():
    import pypevoc_amd.speech as sp
    for name in ("jumps", "chunker", "JumpDetector"):
        assert hasattr(sp, name)
    assert not hasattr(sp, "SilenceDetector")                         # (tests/test_segment_cpu.py: imported from speech.chunker)
    assert sp.chunker.SilenceDetector is not None and sp.jumps.JumpDetector is sp.JumpDetector
    for name in ("nextpow2", "zscore_wind", "linreg_err", "linreg2_err", "jumps_rows", "segment_and_detect_jumps", "avg_interpolator",
                 "file_reader", "pitch_jump_file"):
        assert hasattr(sp.jumps, name)
