"""HeterodyneHarmonic without a device: the plain numpy restatement (tests/hetharm_refs.py) against the reference's recorded
outputs (tests/golden/Q*.npz, make_golden_hetharm.py) within 4 * self_dist, the framing / th / fmin rules, the entries that
raise because the reference cannot run them, and the margins the generator promised for the filter case."""
import glob
import json
import os

import numpy as np
import pytest

from . import hetharm_refs as hr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR = 1e-13          # rounding of the comparison itself, relative to the array's maximum


def hetharm_cases():
    """[(file, case name)] of every recorded case"""
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "Q*.npz"))):
        for c in json.loads(str(np.load(p)["cases"])):
            out.append((os.path.basename(p)[:-4], c["name"]))
    return out


_CACHE = {}


def load_case(fname, name):
    """(case dict, {key without the case's prefix: array}); loaded once per file and never modified"""
    if fname not in _CACHE:
        z = np.load(os.path.join(GOLDEN, fname + ".npz"))
        _CACHE[fname] = ({c["name"]: c for c in json.loads(str(z["cases"]))}, {k: z[k] for k in z.files})
    cases, arrays = _CACHE[fname]
    pre = name + "_"
    g = {k[len(pre):]: v for k, v in arrays.items() if k.startswith(pre)}
    for v in g.values():
        v.setflags(write=False)
    return cases[name], g


def ctor_f(case, g):
    """the f / tf arguments of the constructor as the generator passed them"""
    if case["f"] == "scalar":
        return float(g["f"]), None
    return g["f"], (g["tf"] if case["f"] == "pairs" else None)


def rel_dist(got, want):
    want = np.asarray(want)
    assert np.shape(got) == want.shape, (np.shape(got), want.shape)
    if want.size == 0:
        return 0.0
    return float(np.max(np.abs(np.asarray(got) - want)) / np.max(np.abs(want)))


def check(got, want, self_dist, factor, what):
    d, tol = rel_dist(got, want), factor * self_dist + FLOOR
    print("%-28s distance %.2e  tolerance %.2e (self_dist %.2e)" % (what, d, tol, self_dist))
    assert d <= tol, (what, d, tol)


ALL = hetharm_cases()


def test_every_case_is_recorded():
    assert [f for f, _ in ALL] == ["Q1_scalar_f", "Q2_vibrato_nharm20", "Q3_pairs_dc", "Q4_one_and_no_frame", "Q4_one_and_no_frame",
                                   "Q5_filter", "Q6_adjusted_freq"]


@pytest.mark.parametrize("fname,name", ALL)
def test_restatement_matches_reference(fname, name):
    case, g = load_case(fname, name)
    kw, sd = case["ctor"], case["self_dist"]
    sr, nwind, nhop, nharm = kw["sr"], kw["nwind"], kw["nhop"], kw["nharm"]
    x = g["x"]
    f, tf = ctor_f(case, g)
    fvec, fmin = hr.track(len(x), sr, f, tf, kw.get("fmin", 0.1))
    assert np.array_equal(fvec, g["fvec"]) and fmin == float(g["fmin"])
    th, idxh = hr.frame_times(len(x), sr, nwind, nhop)
    assert np.array_equal(th, g["th"]) and np.array_equal(idxh, g["idxh"])
    ah = hr.extract_all(x, fvec, nharm, np.hanning(nwind), nhop)
    assert ah.shape == g["ah"].shape == (hr.nframes(len(x), nwind, nhop), nharm)
    if ah.shape[0] == 0:
        assert sd == {}
        return
    check(ah, g["ah"], sd["ah"], 4, "ah")
    ref_ah = g["ah"]
    fmax, ampthr = kw.get("fmax", 1000), kw.get("ampthr", 0.1)
    check(hr.resynth(ref_ah, fvec, sr, nwind, nhop), g["resynth"], sd["resynth"], 4, "resynth")
    for n in case["filtered"]:
        fh = hr.filter_harmonic(ref_ah, fvec, n, sr, nwind, nhop, fmin, fmax, ampthr)
        assert np.array_equal(fh == 0, g["fh_%d" % n] == 0), n
        check(fh, g["fh_%d" % n], sd["fh_%d" % n], 4, "filter_harmonic(%d)" % n)
    for n, flt in case["partials"]:
        y = hr.resynth_partial(ref_ah, fvec, n, sr, nwind, nhop, bool(flt), fmin, fmax, ampthr)
        check(y, g["rp_%d_%d" % (n, flt)], sd["rp_%d_%d" % (n, flt)], 4, "resynth_partial(%d, %s)" % (n, bool(flt)))
    dc = kw.get("include_dc", False)
    fcols = hr.f_cols(fvec, sr, th, nharm, dc)
    assert np.allclose(fcols, g["fcols"], rtol=1e-14, atol=0)
    assert np.allclose(hr.angle_ratios(ref_ah, dc), g["angle_ratios"], rtol=0, atol=1e-12)
    if "partial_frequencies" in g:
        assert np.allclose(hr.partial_frequencies(ref_ah, fcols, sr, nhop, dc), g["partial_frequencies"], rtol=1e-12, atol=1e-9)
    if case["adjust"]:
        a = case["adjust"]
        f0c, tha = hr.calc_adjusted_freq(x, fvec, sr, np.hanning(a["nwind"]), a["nhop"])
        assert np.array_equal(tha, g["adj_th"])
        check(f0c, g["adj_f0c"], sd["adj_f0c"], 4, "calc_adjusted_freq")


@pytest.mark.parametrize("nsamp,nwind,nhop", [(6000, 1024, 512), (5000, 511, 100), (1025, 1024, 512), (1024, 1024, 512), (100, 1024, 512),
                                              (1535, 511, 512), (1536, 511, 512), (4000, 512, 128)])
def test_framing_matches_the_analysis_framing(nsamp, nwind, nhop):
    from pypevoc_amd import _lib
    nfr = hr.nframes(nsamp, nwind, nhop)
    assert nfr == _lib.nframes_host(nsamp, nwind, nhop) == max(0, -(-(nsamp - nwind) // nhop))
    th, idxh = hr.frame_times(nsamp, 8000, nwind, nhop)
    assert len(th) == nfr
    assert np.array_equal(th, (nwind // 2 + np.arange(nfr) * nhop) / 8000)
    assert len(idxh) - nfr in (0, 1) and np.array_equal(idxh[:nfr], nwind // 2 + np.arange(nfr) * nhop)


def test_fmin_is_raised_to_the_tracks_minimum():
    assert hr.track(100, 8000, 200.0, None, 0.1)[1] == 200.0
    assert hr.track(100, 8000, 200.0, None, 250.0)[1] == 250.0
    fv, fmin = hr.track(100, 8000, np.linspace(90.0, 300.0, 100), None, 120.0)
    assert fmin == 120.0 and fv[0] == 90.0 / 8000
    assert hr.track(100, 8000, [100.0, 300.0], [0.0, 0.01], 50.0)[1] == 100.0


def _bare():
    """an instance that went through no constructor (the constructor launches the extraction)"""
    from pypevoc_amd.Heterodyne import HeterodyneHarmonic
    return object.__new__(HeterodyneHarmonic)


@pytest.mark.parametrize("call", [
    lambda m: m.HeterodyneHarmonic(np.zeros(4000), sr=8000, f=200.0, nper=3),
    lambda m: _bare().set_fvec(200.0, adjust=True),
    lambda m: _bare().get_voice_component(np.zeros(10), 8000, np.zeros(10), 3),
    lambda m: _bare().harmonic_frequencies(1),
    lambda m: m.Heterodyne(np.zeros(100)),
    lambda m: m.heterodyne_corr(np.zeros(100), 8000, [100.0, 200.0]),
], ids=["nper", "set_fvec_adjust", "get_voice_component", "harmonic_frequencies", "Heterodyne", "heterodyne_corr"])
def test_unsupported_entries_raise(call):
    from pypevoc_amd import Heterodyne as m
    with pytest.raises(NotImplementedError, match="not mirrored"):
        call(m)


def test_class_is_exported():
    import pypevoc_amd
    assert pypevoc_amd.HeterodyneHarmonic is pypevoc_amd.Heterodyne.HeterodyneHarmonic
    assert "HeterodyneHarmonic" in pypevoc_amd.__all__


def test_q5_mask_shares_and_threshold_margins():
    """from the stored arrays: every term of the mask zeroes between 10 % and 90 % of the samples of some harmonic, and no
    sample's |hf| is within 1e-9 (relative) of the amplitude threshold"""
    case, g = load_case("Q5_filter", "filter")
    kw = case["ctor"]
    sr, nwind, nhop, nharm = kw["sr"], kw["nwind"], kw["nhop"], kw["nharm"]
    fvec, fmin = g["fvec"], float(g["fmin"])
    assert fmin == kw["fmin"]
    shares = {"fmin": [], "fmax": [], "nyquist": [], "amp": []}
    for n in range(nharm):
        hf = hr.interp_amp(len(fvec), nwind, nhop, g["ah"][:, n])
        rmsmin = np.max(np.abs(hf)) * kw.get("ampthr", 0.1)
        assert np.min(np.abs(np.abs(hf) - rmsmin)) > 1e-9 * rmsmin, n
        m = hr.filter_mask(hf, fvec * sr, n, sr, fmin, kw["fmax"], kw.get("ampthr", 0.1))
        for k in shares:
            shares[k].append(float(np.mean(m[k])))
        if n in case["filtered"]:
            assert np.array_equal(m["fmin"] | m["fmax"] | m["nyquist"] | m["amp"], g["fh_%d" % n] == 0), n
    for k, v in shares.items():
        assert any(0.1 < s < 0.9 for s in v), (k, v)
