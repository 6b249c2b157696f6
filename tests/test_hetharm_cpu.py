"""HeterodyneHarmonic without a device: the plain numpy restatement (tests/hetharm_refs.py) against the reference's recorded
outputs (tests/golden/Q*.npz, make_golden_hetharm.py) within 4 * self_dist, the framing / th / fmin rules, the entries that
raise because the reference cannot run them, and the margins the generator promised for the filter case.  Then the exact-phase
reference of tests/test_hetharm_diff_gpu.py: against a long double evaluation and the restatement, the exactness of dyadic sums,
and a numpy model of the device's three-launch scan whose deliberate slips must land far outside the GPU test's bounds."""
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


# ---- the exact-phase reference of tests/test_hetharm_diff_gpu.py, pinned without a device ---------------------------------
ULP = 2.0 ** -52
LD = np.longdouble


def ld_carrier(k, h, q=30):
    """exp(2j * pi * h * cumsum(k) / 2**q) on long double: the sum and its product with h are exact there (under 2**64), the
    cycles are reduced mod 1 exactly, and pi enters once"""
    p = LD(h) * np.cumsum(np.asarray(k).astype(LD)) * LD(2) ** -q
    a = LD(2) * (LD(4) * np.arctan(LD(1))) * (p - np.rint(p))
    return np.cos(a), np.sin(a)


def test_exact_reference_agrees_with_the_restatement():
    """20 000 samples of a dyadic track: the exact functions are within 4 ulp (of S, or of the bound's amplitude sum) of a long
    double evaluation, and they are as far from the float64 restatement as the restatement is from long double"""
    if not np.finfo(LD).eps < 2.0 ** -60:
        pytest.skip("np.longdouble is no wider than float64 here: nothing to measure the restatement's own error with")
    n, wlen, hop, nharm = 20000, 511, 100, 9
    rng = np.random.default_rng(20000)
    k, fvec = hr.dyadic_track(rng, n, 0.01, 0.06)
    x, wind = rng.standard_normal(n), np.hanning(wlen)
    nfr = hr.nframes(n, wlen, hop)
    frames = np.arange(nfr)
    rest = hr.extract_all(x, fvec, nharm, wind, hop)
    exact, S = hr.extract_all_exact(x, k, range(nharm), wind, hop, frames)
    idx = frames[:, None] * hop + np.arange(wlen)
    xw = (x[idx] * wind).astype(LD)
    ld = np.zeros((nfr, nharm), dtype=complex)
    ldre, ldim = [], []
    for h in range(nharm):
        c, s = ld_carrier(k, h)
        sc = LD(1 if h == 0 else 2) / np.sum(wind.astype(LD))
        ldre.append(np.sum(xw * c[idx], axis=1) * sc)
        ldim.append(np.sum(xw * s[idx], axis=1) * sc)
    ldre, ldim = np.stack(ldre, axis=1), np.stack(ldim, axis=1)

    def dist(a):
        return np.hypot((a.real.astype(LD) - ldre).astype(float), (a.imag.astype(LD) - ldim).astype(float))

    own, rerr = float(np.max(dist(exact) / S)), float(np.max(dist(rest)))
    print("extraction: exact - long double %.2f ulp of S; restatement - long double %.2e; exact - restatement %.2e"
          % (own / ULP, rerr, np.max(np.abs(exact - rest))))
    assert own <= 4 * ULP
    assert rerr > 100 * ULP                                              # the restatement is the looser one, by far
    assert np.max(np.abs(exact - rest)) <= rerr + 4 * ULP * S.max()
    # resynthesis of a random ah
    ah = hr.random_ah(rng, nfr, nharm)
    yr = hr.resynth(ah, fvec, hr.SR, wlen, hop)
    ye, B = hr.resynth_exact(ah, k, range(nharm), hr.SR, wlen, hop)
    i0, i1 = hr.knots(n, wlen, hop, nfr)
    t = (np.arange(n) - wlen // 2 - i0 * hop).clip(0, hop).astype(LD) / LD(hop)
    yl = np.zeros(n, dtype=LD)
    for h in range(nharm):
        c, s = ld_carrier(k, h)
        u, v = ah[i0, h], ah[i1, h]
        yl += c * (u.real.astype(LD) + (v.real.astype(LD) - u.real.astype(LD)) * t) + s * (u.imag.astype(LD) + (v.imag.astype(LD) - u.imag.astype(LD)) * t)
    amp = B / (2 * 16 * ULP)                                             # sum_h |ah[i0, h]| + |ah[i1, h]|
    own, rerr = float(np.max(np.abs((ye - yl).astype(float)) / amp)), float(np.max(np.abs((yr - yl).astype(float))))
    print("resynthesis: exact - long double %.2f ulp of the amplitude sum; restatement - long double %.2e; exact - restatement %.2e"
          % (own / ULP, rerr, np.max(np.abs(ye - yr))))
    assert own <= 4 * ULP
    assert rerr > 100 * ULP
    assert np.max(np.abs(ye - yr)) <= rerr + 4 * ULP * amp.max()


def test_dyadic_sums_are_exact():
    """past two rounds of the tile scan: np.cumsum(fvec), the tiles' sums and the model of the device's scan are the integers"""
    n = 2 * 256 * 2048 + 5
    k, fvec = hr.dyadic_track(np.random.default_rng(3), n, 0.01, 0.06)
    K = np.cumsum(k)
    assert int(K[-1]).bit_length() <= 47
    assert np.array_equal(np.cumsum(fvec) * 2.0 ** 30, K.astype(float)) and np.array_equal((np.cumsum(fvec) * 2.0 ** 30).astype(np.int64), K)
    ends = np.append(np.arange(2048, n, 2048), n) - 1
    assert np.array_equal(np.add.reduceat(fvec, np.arange(0, n, 2048)) * 2.0 ** 30, np.diff(K[ends], prepend=0).astype(float))
    assert np.array_equal(hr.scan_model(fvec) * 2.0 ** 30, K.astype(float))
    assert np.array_equal(fvec * hr.SR, k * 2.0 ** -17)                  # the track in Hz is exact as well


def test_scan_frames_hold_every_seam():
    for n in hr.SCAN_NS:
        fr, nfr = hr.scan_frames(n, hr.SCAN_WLEN, hr.SCAN_HOP), hr.nframes(n, hr.SCAN_WLEN, hr.SCAN_HOP)
        assert len(fr) <= 64 and fr[0] == 0 and fr[-1] == nfr - 1
        for b in (2048, 4096, 6144, (n - 1) // 2048 * 2048, ((n - 1) // 2048 - 1) * 2048, 524288, 1048576):
            want = [i for i in range(max(0, b // hr.SCAN_HOP - 6), min(nfr, b // hr.SCAN_HOP + 1)) if i * hr.SCAN_HOP <= b < i * hr.SCAN_HOP + hr.SCAN_WLEN]
            assert b <= 0 or set(want) <= set(fr.tolist()), (n, b)


@pytest.mark.parametrize("n", hr.SCAN_NS)
def test_a_slipped_scan_is_far_outside_the_bounds(n):
    """the model of the three-launch scan is bit-equal to the integers; with each deliberate slip, wherever the slip changes
    the phase of a sample at all, the resynthesis (every sample) is at least 1000 times over its bound, and wherever it changes
    a sample that some frame reads, the extraction at the frames of scan_frames is too.  (Where the last tile starts behind the
    last frame's window, as at 2049, 4097, 524 289 and 1 048 581 samples, 'last_tile' and a carry that only that tile takes change
    samples no frame reads: those the resynthesis alone can see.)"""
    c = hr.scan_case(n)
    k, fvec, x, ah, frames = c["k"], c["fvec"], c["x"], c["ah"], c["frames"]
    wlen, hop, harm, wind = hr.SCAN_WLEN, hr.SCAN_HOP, range(hr.SCAN_NHARM), np.hanning(hr.SCAN_WLEN)
    K = np.cumsum(k)
    assert np.array_equal(hr.scan_model(fvec) * 2.0 ** 30, K.astype(float))
    a0, S = hr.extract_all_exact(x, k, harm, wind, hop, frames)
    y0, B = hr.resynth_exact(ah, k, harm, hr.SR, wlen, hop)
    covered = (hr.nframes(n, wlen, hop) - 1) * hop + wlen                # samples below this are read by some frame
    seen = {}
    for slip in hr.SCAN_SLIPS:
        Ks = hr.scan_model(fvec, slip=slip) * 2.0 ** 30
        assert np.array_equal(Ks, np.rint(Ks))
        Ks = Ks.astype(np.int64)
        wrong = np.nonzero(Ks != K)[0]
        if len(wrong) == 0:
            continue
        Km = Ks % (1 << 30)
        ry = float(np.max(np.abs(hr.resynth_exact(ah, k, harm, hr.SR, wlen, hop, K=Km)[0] - y0) / B))
        seen[slip] = [ry, None]
        assert ry >= 1000, (slip, ry)
        if wrong[0] < covered:
            ra = float(np.max(np.abs(hr.extract_all_exact(x, k, harm, wind, hop, frames, K=Km)[0] - a0) / hr.extract_bound(S, wlen)))
            seen[slip][1] = ra
            assert ra >= 1000, (slip, ra)
    print("n %d: slip -> distance / bound of (resynthesis, extraction): %s"
          % (n, {s: tuple("-" if r is None else "%.1e" % r for r in v) for s, v in seen.items()}))
    assert {"inclusive", "index"} <= set(seen) and all(v[1] is not None for s, v in seen.items() if s in ("inclusive", "index"))
    assert ("last_tile" in seen) == (n % 2048 != 0 and n > 2048) and ("carry" in seen) == (n > 524288)
    if n == 1048581:
        assert seen["carry"][1] is not None
