"""Pitch jumps end to end on the GPU against the reference's recorded outputs (J0 .. J5, tests/golden/make_golden_jumps.py),
from host and device-resident signals.  JUMPS.md has the bounds: choices equal; continuous outputs within 2 * sens element
by element; empty results and IndexError where the reference has them.  J0 pins PV itself at hop == nfft, which
detect_pitch picks at 8 and 16 kHz, to the float64 path's contract (tests/test_hip_parity.py)."""
import json

import numpy as np
import pytest

from .test_jumps_cpu import CASES, check_against_fixture, load, within

pytestmark = pytest.mark.gpu


def on_gpu(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda")


@pytest.mark.parametrize("sr", [16000, 8000])
def test_pv_at_hop_equal_to_nfft(sr):
    """J0.  float64 samples at nfft 512 take k_pv_rev's form without a sliding window, nfft 256 the rocFFT path (JUMPS.md)."""
    import pypevoc_amd
    from pypevoc_amd import _lib
    g = load("J0_pv_hop_nfft")
    nfft = {16000: 512, 8000: 256}[sr]
    x = g["x_%d" % sr].astype(np.float64)
    for sig in (x, on_gpu(x)):
        p = pypevoc_amd.PV(sig, sr, nfft=nfft, hop=nfft, npks=20, progress=False)
        p.run_pv()
        f, mag, ph, t = g["f_%d" % sr], g["mag_%d" % sr], g["ph_%d" % sr], g["t_%d" % sr]
        assert p.nframes == len(t) and np.array_equal(np.asarray(p.f) > 0, f > 0)
        v = f > 0
        print("J0", sr, "kernels", _lib.load().pvx_plan_last_kernels(p._plan.handle).decode(), "df", np.abs(p.f - f).max(),
              "dmag", (np.abs(p.mag - mag)[v] / mag[v]).max(), "dph", np.abs(p.ph - ph)[v].max())
        assert np.abs(p.f - f).max() <= 1e-9
        assert (np.abs(p.mag - mag)[v] / mag[v]).max() <= 1e-12
        assert np.abs(p.ph - ph)[v].max() <= 1e-10
        assert np.abs(np.asarray(p.t) - t).max() <= 1e-12
        assert np.abs(p.calc_f0() - g["f0_%d" % sr]).max() <= 1e-9


def detector_for(args, slope_t):
    from pypevoc_amd.speech.jumps import JumpDetector
    jd = JumpDetector(**args)
    if slope_t is not None:
        jd.slope_t = slope_t
    return jd


def attributes(jd):
    return {"isel": jd.isel, "le": jd.le, "up_idx": jd.up_jump_indices, "dn_idx": jd.down_jump_indices, "intcpts": jd.intcpts,
            "sumres": jd.sumres}


DETECTOR = [c for c in CASES if c[5] is not None]                     # J1 .. J4 (J5's regions: the last test)


@pytest.mark.parametrize("case", DETECTOR, ids=[c[0] for c in DETECTOR])
def test_process_against_the_reference(case):
    cid, g, p, args, slope_t, c = case
    x = g[c["x"]].astype(np.float64)
    sr = c["sr"]
    results = []
    for where, sig in (("host", x), ("device", on_gpu(x))):
        jd = detector_for(args, slope_t)
        times = jd.process(sig, sr)
        what = "%s from a %s signal" % (cid, where)
        assert (jd.nfft, jd.nhop) == (int(g[p + "_nfft"]), int(g[p + "_nhop"])), what
        mag, t, f0 = g[p + "_mag"], g[p + "_t"], g[p + "_f0"]
        assert np.abs(jd.t - t).max() <= 1e-12 and np.abs(jd.f0 - f0).max() <= 1e-9, what
        assert np.all(np.abs(jd.mag - mag) <= 1e-12 * mag), what
        worst = check_against_fixture(attributes(jd), g, p, what)
        assert jd.status == 0 and not np.asarray(jd.jump_status).any(), what
        assert np.abs(times - g[p + "_times"]).max() <= 1e-12 if len(times) else len(g[p + "_times"]) == 0, what
        assert np.array_equal(jd.up_jump_times, jd.t[jd.isel][jd.up_jump_indices]), what
        assert np.array_equal(jd.down_jump_times, jd.t[jd.isel][jd.down_jump_indices]), what
        if p + "_table_raises" in g:
            assert jd.intcpts.shape == (0,) and jd.sumres.shape == (0,), what
            with pytest.raises(IndexError):
                jd.jump_table_columns()
        else:
            cols = jd.jump_table_columns()
            assert np.array_equal(cols["segment_time"], times) and np.array_equal(cols["f_before"], jd.intcpts[:, 0]), what
            assert np.array_equal(cols["residue_total"], np.sum(jd.sumres, axis=1)), what
        print(what, worst)
        results.append(attributes(jd))
    for k in ("isel", "up_idx", "dn_idx"):
        assert np.array_equal(results[0][k], results[1][k]), k


def test_detect_jumps_follows_attributes_set_by_hand():
    """mag, t and f0 replaced after detect_pitch (the recorded ones): the stages run on them, and calc_jump_params follows
    index lists and a slope_t set by hand."""
    g = load("J4_options_edges")
    p = "slope02"
    jd = detector_for({}, None)
    jd.mag, jd.t, jd.f0 = g[p + "_mag"], g[p + "_t"], g[p + "_f0"]
    jd.detect_jumps()
    jd.slope_t = 0.2
    jd.calc_jump_params()
    check_against_fixture(attributes(jd), g, p, "by hand")
    jd.up_jump_indices, jd.down_jump_indices = np.array([1]), np.array([], dtype=int)     # one point on the left
    jd.calc_jump_params()
    assert np.isnan(jd.intcpts[0, 0]) and np.isnan(jd.sumres[0, 0]) and np.isfinite(jd.intcpts[0, 1]) and jd.jump_status[0] == 1


def test_a_nan_in_the_track_gives_nan_and_a_status_bit():
    g = load("J1_process_16000")
    jd = detector_for({}, None)
    f0 = g["p_f0"].copy()
    f0[60] = np.nan
    jd.mag, jd.t, jd.f0 = g["p_mag"], g["p_t"], f0
    jd.detect_jumps()
    assert jd.status == 2 and np.isnan(jd.le[36:85]).all() and not np.isnan(jd.le[86:]).any()
    assert np.array_equal(jd.down_jump_indices, [141])                # the jump at 47 is inside the NaN's reach; 94's right side is clean
    jd.calc_jump_params()
    assert len(jd.intcpts) == len(jd.up_jump_indices) + 1


def test_window_statistics_wrappers_against_the_reference():
    """J6 through zscore_wind, linreg_err and linreg2_err themselves: the kind constants, t = None -> x and the use_l / use_r
    flags of the Python layer, hop 1 and 3."""
    from pypevoc_amd.speech import jumps
    g = load("J6_winstat")
    calls = json.loads(str(g["calls"]))
    assert {c["fn"] for c in calls} == {"zscore_wind", "linreg_err", "linreg2_err"}
    worst = {}
    for c in calls:
        x = g[c["x"]]
        got = getattr(jumps, c["fn"])(*((g["t"], x) if "t" in c else (x,)), **c["kwargs"])
        assert jumps.last_kernels() == "k_winstat", c["name"]
        worst[c["fn"]] = max(worst.get(c["fn"], 0.0), within(got, g[c["name"]], g["sens_" + c["name"]], c["name"]))
    print("J6 wrappers", worst)
    x = g["xa"]
    assert np.isnan(jumps.linreg2_err(g["t"], x, use_l=False, use_r=False)[5:-5]).all()        # np.mean([])
    assert np.array_equal(jumps.zscore_wind(x, hop=None), jumps.zscore_wind(x, hop=1))


@pytest.mark.parametrize("where", ["host", "device"])
def test_segment_and_detect_jumps_against_the_recorded_regions(where):
    from pypevoc_amd.speech.chunker import SilenceDetector
    from pypevoc_amd.speech.jumps import segment_and_detect_jumps
    g = load("J5_regions")
    sr = int(g["sr"])
    x = g["x"].astype(np.float64)
    sig = x if where == "host" else on_gpu(x)
    for tag, kw in (("band", {"fmin": 50, "fmax": 1000}), ("plain", {})):
        sd = SilenceDetector(sig, sr, **kw)
        assert np.abs(sd.at - g[tag + "_at"]).max() <= 1e-12, tag
        within(sd.ax, g[tag + "_ax"], g[tag + "_sens_ax"], tag + " ax")   # frame by frame
        assert abs(sd.ath - float(g[tag + "_ath"])) <= 2 * float(g[tag + "_sens_ath"]), tag
        assert np.array_equal(sd.clusters, g[tag + "_clusters"]), tag
        assert np.array_equal(sd.tst, g[tag + "_tst"]) and np.array_equal(sd.tend, g[tag + "_tend"]), tag
        print(tag, "ax", np.abs(sd.ax - g[tag + "_ax"]).max(), "ath", abs(sd.ath - float(g[tag + "_ath"])))
    args = json.loads(str(g["args"]))
    df, segments = segment_and_detect_jumps(sig, sr, **args)
    assert np.array_equal(segments["start"], g["band_tst"]) and np.array_equal(segments["end"], g["band_tend"])
    assert list(segments["nbr"]) == [0, 1, 2]
    assert list(df.columns) == ["segment_time", "f_before", "f_after", "f_cent", "df", "residue_before", "residue_after", "residue_total",
                                "rec_time", "region_nbr"]
    for k in range(3):
        part = df[df["region_nbr"] == k]
        p = "r%d" % k
        assert np.abs(part["segment_time"].to_numpy() - g[p + "_times"]).max() <= 1e-12
        assert np.array_equal(part["rec_time"].to_numpy(), part["segment_time"].to_numpy() + g["band_tst"][k])
        ic = np.stack([part["f_before"].to_numpy(), part["f_after"].to_numpy()], axis=1)
        sr_ = np.stack([part["residue_before"].to_numpy(), part["residue_after"].to_numpy()], axis=1)
        within(ic, g[p + "_intcpts"], g[p + "_sens_intcpts"], p + " intcpts")
        within(sr_, g[p + "_sumres"], g[p + "_sens_sumres"], p + " sumres")
        assert np.array_equal(part["df"].to_numpy(), ic[:, 1] - ic[:, 0])
