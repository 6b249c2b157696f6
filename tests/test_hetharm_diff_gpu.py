"""k_hetharm.hip on the MI355X against the exact-phase reference of tests/hetharm_refs.py (HETHARM.md, "Exact-phase tests").

Every track is dyadic, fvec[t] = k[t] * 2**-30 with seeded integers k, at sr = 8192: the running phase is an integer over 2**30
whatever order it is added in, on the device as in numpy, so the reference's carrier is correct to an ulp at a million samples
and a scan that loses a term is a slip, not rounding.  Two bounds, derived from the kernels' arithmetic and not tuned:
  extraction, per frame and harmonic   |ah - exact| <= 2 * (G + 10 + wlen / 64) * 2**-52 * S,   S = 2 / sum(wind) * sum_j |x_j wind_j|
  resynthesis, per sample              |y - exact|  <= 2 * (G + 8) * 2**-52 * sum_h (|ah[i0, h]| + |ah[i0 + 1, h]|)
with G = 8 (PVX_HH_GROUP).  Every test prints its largest distance / bound.  Measured on an MI355X, the largest of each group:
  (a) ah 0.008 (n 524 288), resynth() 0.036 (n 524 288), extract_partial(7 / 8 / 9) 0.006      (b) ah 0.074 (wlen 2), resynth() 0.024
  (c) pvx_hetharm 0.011 (first 15, count 18), pvx_hetharm_resynth 0.046 (first 7, count 2 and first 2**20 - 3, count 3)
  (d) between knots 0.200 of 3 * 2**-53 * (|u| + |v|); on the knots and outside them bit for bit      (e) kept values 0.142, same bound
The device is 14 to 100 times inside its bounds: no slip, and nothing was changed in the kernels.
Groups: (a) tile and carry seams of the phase scan, n up to 1 048 581; (b) window shapes, wlen 1 .. 1000 and hop 1 .. wlen + 3;
(c) harmonic windows first / count through the C ABI, up to harmonic 2**20 - 1; (d) the knots of the interpolation, bit for
bit; (e) the strict comparisons of the filter mask; (f) a device-resident signal."""
import numpy as np
import pytest

from . import hetharm_refs as hr

pytestmark = pytest.mark.gpu

SR = hr.SR
PVX_ERR_INVALID = -2                                                    # include/pvx.h


def bits(a):
    """the words of a float64 array, or the (re, im) pairs of words of a complex one as rows"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64).reshape(-1, 2) if a.dtype == np.complex128 else a.view(np.uint64)


def ratio(dist, bound):
    """largest distance / bound; a zero bound admits a zero distance only"""
    dist, bound = np.broadcast_arrays(np.asarray(dist, dtype=float), np.asarray(bound, dtype=float))
    if dist.size == 0:
        return 0.0
    assert not np.isnan(dist).any() and not np.isnan(bound).any()
    r = np.where(bound > 0, dist / np.where(bound > 0, bound, 1.0), np.where(dist == 0, 0.0, np.inf))
    return float(np.max(r))


def within(what, dist, bound):
    r = ratio(dist, bound)
    print("%-64s largest distance / bound %.3f" % (what, r))
    assert r <= 1.0, (what, r)
    return r


def harmonic(x, hz, wlen, hop, nharm, **kw):
    from pypevoc_amd import HeterodyneHarmonic
    return HeterodyneHarmonic(x, sr=SR, f=hz, nwind=wlen, nhop=hop, nharm=nharm, **kw)


def with_ah(h, ah, **attrs):
    """a copy of h that resynthesises from ah (all columns, the DC one included)"""
    c = h.clone()
    c.camp = np.array(ah)
    for k, v in attrs.items():
        setattr(c, k, v)
    return c


# ---- (a) tile and carry seams of the phase scan, (f) device-resident input ---------------------------------------------
_CASES, _BUILT = {}, {}


def scan_case(n):
    if n not in _CASES:
        c = hr.scan_case(n)
        for v in c.values():
            v.setflags(write=False)
        _CASES[n] = c
    return _CASES[n]


def scan_built(n, device=False, nharm=hr.SCAN_NHARM):
    key = (n, device, nharm)
    if key not in _BUILT:
        c = scan_case(n)
        x = c["x"]
        if device:
            import torch
            x = torch.from_numpy(np.array(x)).cuda()
        h = harmonic(x, c["fvec"] * SR, hr.SCAN_WLEN, hr.SCAN_HOP, nharm)
        assert np.array_equal(h.fvec, c["fvec"])                         # the class hands the device the dyadic values
        _BUILT[key] = h
    return _BUILT[key]


@pytest.mark.parametrize("n", hr.SCAN_NS)
def test_scan_seams_extraction(n):
    c, h = scan_case(n), scan_built(n)
    frames = c["frames"]
    nfr = hr.nframes(n, hr.SCAN_WLEN, hr.SCAN_HOP)
    assert h.ah.shape == (nfr, hr.SCAN_NHARM) and len(frames) <= 64 and frames[0] == 0 and frames[-1] == nfr - 1
    exact, S = hr.extract_all_exact(c["x"], c["k"], range(hr.SCAN_NHARM), np.hanning(hr.SCAN_WLEN), hr.SCAN_HOP, frames)
    within("(a) n %d: ah at %d frames" % (n, len(frames)), np.abs(h.ah[frames] - exact), hr.extract_bound(S, hr.SCAN_WLEN))


@pytest.mark.parametrize("n", hr.SCAN_NS)
def test_scan_seams_resynthesis(n):
    """every sample, from a random ah: the resynthesis is tested apart from the extraction"""
    c = scan_case(n)
    y = with_ah(scan_built(n), c["ah"]).resynth()
    exact, B = hr.resynth_exact(c["ah"], c["k"], range(hr.SCAN_NHARM), SR, hr.SCAN_WLEN, hr.SCAN_HOP)
    assert y.shape == (n,)
    within("(a) n %d: resynth() at every sample" % n, np.abs(y - exact), B)


def test_partials_either_side_of_a_group_past_the_carry():
    """extract_partial(7), (8), (9) at 524 289 samples: the exact value at the seam frames, and the full call's columns bit for bit"""
    n = 524289
    c, h9, h10 = scan_case(n), scan_built(n), scan_built(n, nharm=10)
    assert np.array_equal(bits(h10.ah[:, :9]), bits(h9.ah))
    wind = np.hanning(hr.SCAN_WLEN)
    for p in (7, 8, 9):
        col, ic = h9.extract_partial(p)
        assert np.array_equal(bits(col), bits(h10.ah[:, p])), p
        assert np.array_equal(ic, hr.SCAN_WLEN // 2 + np.arange(len(col)) * hr.SCAN_HOP)
        exact, S = hr.extract_exact(c["x"], c["k"], p, wind, hr.SCAN_HOP, c["frames"])
        within("(a) n %d: extract_partial(%d)" % (n, p), np.abs(col[c["frames"]] - exact), hr.extract_bound(S, hr.SCAN_WLEN))


def test_device_resident_signal_past_the_carry():
    n = 524289
    c, h, d = scan_case(n), scan_built(n), scan_built(n, device=True)
    assert d._xdev is not None and isinstance(d.ah, np.ndarray)
    assert np.array_equal(bits(d.ah), bits(h.ah))
    assert np.array_equal(bits(with_ah(d, c["ah"]).resynth()), bits(with_ah(h, c["ah"]).resynth()))


# ---- (b) window shapes --------------------------------------------------------------------------------------------------
WLENS = (1, 2, 63, 64, 65, 127, 1000)


@pytest.mark.parametrize("wlen,wname", [(w, f) for w in WLENS for f in ("rect", "hanning") if f == "rect" or w > 2])
def test_window_shapes(wlen, wname):
    """hop 1, 7, wlen, wlen + 3 and n one past the window, on and one past the second frame's strict limit, and four or five frames
    (np.hanning sums to 0 at wlen 2 and is np.ones at wlen 1: rectangular only there)"""
    wfun = np.ones if wname == "rect" else np.hanning
    nharm, ra, ry, count = 9, 0.0, 0.0, 0
    for hop in sorted({1, 7, wlen, wlen + 3}):
        for n in sorted({wlen + 1, wlen + hop, wlen + hop + 1, wlen + 3 * hop + 2}):
            rng = np.random.default_rng([wlen, hop, n])
            k, fvec = hr.dyadic_track(rng, n, 0.01, 0.06)
            x = rng.standard_normal(n)
            h = harmonic(x, fvec * SR, wlen, hop, nharm, wfun=wfun)
            nfr = hr.nframes(n, wlen, hop)
            assert 1 <= nfr <= 200 and h.ah.shape == (nfr, nharm), (hop, n)
            th, idxh = hr.frame_times(n, SR, wlen, hop)
            assert np.array_equal(h.th, th) and np.array_equal(h.idxh, idxh)
            assert np.array_equal(h.extract_partial(1)[1], wlen // 2 + np.arange(nfr) * hop), (hop, n)
            exact, S = hr.extract_all_exact(x, k, range(nharm), wfun(wlen), hop, np.arange(nfr))
            ra = max(ra, ratio(np.abs(h.ah - exact), hr.extract_bound(S, wlen)))
            ah = hr.random_ah(rng, nfr, nharm)
            ye, B = hr.resynth_exact(ah, k, range(nharm), SR, wlen, hop)
            ry = max(ry, ratio(np.abs(with_ah(h, ah).resynth() - ye), B))
            count += 1
    print("(b) wlen %4d %-7s %2d shapes: largest distance / bound  ah %.3f  resynth() %.3f" % (wlen, wname, count, ra, ry))
    assert ra <= 1.0 and ry <= 1.0, (ra, ry)


# ---- (c) harmonic windows through the C ABI -----------------------------------------------------------------------------
C_N, C_WLEN, C_HOP = 6000, 256, 64
C_WINDOWS = ((0, 1), (0, 8), (0, 9), (5, 6), (7, 2), (8, 8), (15, 18), (1000, 3), (2 ** 20 - 3, 3))
_C = {}


def c_case():
    if not _C:
        from pypevoc_amd import _lib
        rng = np.random.default_rng(6000)
        k, fvec = hr.dyadic_track(rng, C_N, 0.01, 0.06)
        _C.update(lib=_lib.load(), k=k, fvec=fvec, x=rng.standard_normal(C_N), wind=np.hanning(C_WLEN), nfr=hr.nframes(C_N, C_WLEN, C_HOP))
        _lib.init()
    return _C


def cplx_ptr(a):
    from pypevoc_amd import _lib
    return a.view(np.float64).ctypes.data_as(_lib.c_double_p)


def c_extract(first, count, fill=0.0):
    """pvx_hetharm, not halving: (status, ah [nfr, count], icent)"""
    from pypevoc_amd import _lib
    c = c_case()
    ah = np.full((c["nfr"], count), fill, dtype=np.complex128)
    ic = np.zeros(c["nfr"], dtype=np.int64)
    r = c["lib"].pvx_hetharm(_lib.dptr(c["x"]), C_N, _lib.dptr(c["fvec"]), _lib.dptr(c["wind"]), C_WLEN, C_HOP, first, count, 0, cplx_ptr(ah),
                             ic.ctypes.data_as(_lib.c_int64_p))
    return r, ah, ic


def c_resynth(ah, first, count):
    """pvx_hetharm_resynth, unfiltered, harmonics first .. first + count - 1 of ah's columns"""
    from pypevoc_amd import _lib
    c = c_case()
    y = np.full(C_N, np.nan)
    r = c["lib"].pvx_hetharm_resynth(_lib.dptr(c["fvec"]), C_N, cplx_ptr(ah), ah.shape[0], ah.shape[1], C_WLEN, C_HOP, first, count, 0, float(SR), 0.0,
                                     np.inf, 0.0, _lib.dptr(y), None)
    assert r == C_N, _lib.load().pvx_last_error()
    return y


@pytest.mark.parametrize("first,count", C_WINDOWS)
def test_group_windows_extraction(first, count):
    c = c_case()
    r, ah, ic = c_extract(first, count)
    assert r == c["nfr"] == 90 and np.array_equal(ic, C_WLEN // 2 + np.arange(90) * C_HOP)
    exact, S = hr.extract_all_exact(c["x"], c["k"], range(first, first + count), c["wind"], C_HOP, np.arange(90), halve_dc=False)
    within("(c) pvx_hetharm first %d count %d" % (first, count), np.abs(ah - exact), hr.extract_bound(S, C_WLEN))
    for j in range(count):
        r1, one, _ = c_extract(first + j, 1)
        assert r1 == 90 and np.array_equal(bits(one[:, 0]), bits(ah[:, j])), (first, count, j)


def test_harmonics_past_the_limit_are_refused():
    from pypevoc_amd import _lib
    r, ah, _ = c_extract(2 ** 20 - 2, 3, fill=7.0)                       # first + count = 2**20 + 1
    assert r == PVX_ERR_INVALID and b"harmonics" in _lib.load().pvx_last_error()
    assert np.all(ah == 7.0)                                             # nothing ran: the output is untouched
    assert c_extract(2 ** 20 - 3, 3)[0] == 90 and c_extract(2 ** 20 - 1, 1)[0] == 90


@pytest.mark.parametrize("first,count", C_WINDOWS)
def test_group_windows_resynthesis(first, count):
    """nharm_total = first + count, random ah in the columns asked for (the other columns are never read)"""
    c = c_case()
    rng = np.random.default_rng([first, count])
    ah = np.zeros((c["nfr"], first + count), dtype=np.complex128)
    ah[:, first:] = hr.random_ah(rng, c["nfr"], count)
    y = c_resynth(ah, first, count)
    exact, B = hr.resynth_exact(ah[:, first:], c["k"], range(first, first + count), SR, C_WLEN, C_HOP)
    within("(c) pvx_hetharm_resynth first %d count %d" % (first, count), np.abs(y - exact), B)
    ysum = np.zeros(C_N)
    for j in range(count):
        ysum += c_resynth(ah, first + j, 1)
    assert np.array_equal(bits(ysum), bits(y))


# ---- (d) the knots of the interpolation, (e) the filter mask ---------------------------------------------------------------
KNOT_SHAPES = ((64, 16, 1), (64, 16, 2), (65, 1, 40), (511, 100, 7))


def knot_case(wlen, hop, nfr, nharm=6):
    """a signal of exactly nfr frames, a dyadic track (82 .. 491 Hz) and a random ah"""
    n = wlen + (nfr - 1) * hop + 1 + (hop - 1) // 2
    assert hr.nframes(n, wlen, hop) == nfr
    rng = np.random.default_rng([wlen, hop, nfr])
    k, fvec = hr.dyadic_track(rng, n, 0.01, 0.06)
    return n, fvec * SR, rng.standard_normal(n), hr.random_ah(rng, nfr, nharm)


def interp_bound(ah_col, n, wlen, hop):
    i0, i1 = hr.knots(n, wlen, hop, len(ah_col))
    return 3 * 2.0 ** -53 * (np.abs(ah_col[i0]) + np.abs(ah_col[i1]))


@pytest.mark.parametrize("wlen,hop,nfr", KNOT_SHAPES)
def test_interpolation_knots(wlen, hop, nfr):
    n, hz, x, ah = knot_case(wlen, hop, nfr)
    h = with_ah(harmonic(x, hz, wlen, hop, 6, fmin=0, fmax=np.inf, ampthr=0), ah)
    assert h.fmin == hz.min() and 5 * hz.max() < SR / 2.2                # limits that cut nothing
    t = np.arange(n)
    kn = wlen // 2 + np.arange(nfr) * hop
    r = 0.0
    for m in (0, 1, 5):
        hf = h.filter_harmonic(m)
        assert hf.shape == (n,) and hf.dtype == np.complex128
        head, tail = t <= wlen // 2, t >= kn[-1]
        assert np.all(bits(hf[head]) == bits(ah[:1, m])), m
        assert np.array_equal(bits(hf[kn]), bits(ah[:, m])), m
        assert np.all(bits(hf[tail]) == bits(ah[-1:, m])), m
        r = max(r, ratio(np.abs(hf - hr.interp_amp(n, wlen, hop, ah[:, m])), interp_bound(ah[:, m], n, wlen, hop)))
        # and the signal of that amplitude is the unfiltered one: nothing was cut
        assert np.array_equal(bits(h.resynth_partial(m, filter=True)), bits(h.resynth_partial(m)))
    print("(d) wlen %d hop %d frames %d: between knots, largest distance / bound %.3f" % (wlen, hop, nfr, r))
    assert r <= 1.0


_E = {}


def mask_case():
    if not _E:
        n, hz, x, ah = knot_case(511, 100, 7, nharm=9)
        hz.setflags(write=False)
        _E.update(n=n, hz=hz, x=x, ah=ah)
    return _E


def check_filtered(what, h, m, hz, ah, fmin, fmax, ampthr):
    """filter_harmonic(m) of h against hetharm_refs: the same zero pattern, kept values within the interpolation's bound"""
    n, wlen, hop = len(hz), 511, 100
    hf = h.filter_harmonic(m)
    ref = hr.interp_amp(n, wlen, hop, ah[:, m])
    mk = hr.filter_mask(ref, hz, m, SR, fmin, fmax, ampthr)
    cut = mk["fmin"] | mk["fmax"] | mk["nyquist"] | mk["amp"]
    assert np.array_equal(hf == 0, cut), what
    r = ratio(np.abs(hf - ref)[~cut], interp_bound(ah[:, m], n, wlen, hop)[~cut])
    print("(e) %-52s %4d of %d samples cut; kept values, largest distance / bound %.3f" % (what, int(cut.sum()), n, r))
    assert r <= 1.0
    return hf, mk


def test_filter_band_limits_are_strict():
    e = mask_case()
    hz = np.array(e["hz"])
    fmin, fmax = 200.0, 300.0
    hz[100:104] = fmin, np.nextafter(fmin, 0), fmax, np.nextafter(fmax, np.inf)
    hz[104:108] = np.nextafter(fmin, np.inf), np.nextafter(fmax, 0), fmin, fmax
    h = with_ah(harmonic(e["x"], hz, 511, 100, 9, fmin=fmin, fmax=fmax, ampthr=0), e["ah"])
    assert h.fmin == fmin and np.array_equal(h.fvec * SR, hz)
    hf, mk = check_filtered("f0 on and one ulp outside fmin 200 / fmax 300", h, 1, hz, e["ah"], fmin, fmax, 0)
    assert np.array_equal(hf[100:108] == 0, [False, True, False, True, False, False, False, False])
    assert mk["fmin"].sum() > 100 and mk["fmax"].sum() > 100 and not mk["amp"].any() and not mk["nyquist"].any()


def test_filter_nyquist_limit_is_strict():
    e = mask_case()
    hz, nyq = np.array(e["hz"]), SR / 2.2
    hz[50:53] = nyq / 8, np.nextafter(nyq / 8, np.inf), np.nextafter(nyq / 8, 0)    # times 8 is exact
    h = with_ah(harmonic(e["x"], hz, 511, 100, 9, fmin=0, fmax=np.inf, ampthr=0), e["ah"])
    hf, mk = check_filtered("harmonic 8 on and one ulp either side of sr / 2.2", h, 8, hz, e["ah"], h.fmin, np.inf, 0)
    assert np.array_equal(hf[50:53] == 0, [False, True, False])
    assert 20 < mk["nyquist"].sum() < e["n"] - 100 and not (mk["fmin"] | mk["fmax"] | mk["amp"]).any()
    check_filtered("harmonic 7 under sr / 2.2 everywhere", h, 7, hz, e["ah"], h.fmin, np.inf, 0)
    assert 7 * hz.max() < nyq


def test_filter_amplitude_threshold():
    """ampthr 1.0 keeps the samples that sit on the column's largest knot and nothing else; ampthr 0 cuts nothing"""
    e = mask_case()
    n, ah = e["n"], np.array(e["ah"])
    ah[0, 1], ah[3, 2], ah[6, 3] = 6 - 8j, -8 + 6j, 10j                  # the largest of their columns: first, interior, last knot
    kn = 511 // 2 + np.arange(7) * 100
    t = np.arange(n)
    h = with_ah(harmonic(e["x"], e["hz"], 511, 100, 9, fmin=0, fmax=np.inf), ah, ampthr=1.0)
    hf, _ = check_filtered("ampthr 1.0, largest knot first", h, 1, e["hz"], ah, h.fmin, np.inf, 1.0)
    assert np.array_equal(hf != 0, t <= kn[0]) and np.all(hf[t <= kn[0]] == ah[0, 1])
    hf, _ = check_filtered("ampthr 1.0, largest knot interior", h, 2, e["hz"], ah, h.fmin, np.inf, 1.0)
    assert np.array_equal(hf != 0, t == kn[3]) and hf[kn[3]] == ah[3, 2]
    # behind the last knot np.interp returns the end value itself (interp_amp rounds u + (v - u) * 1 there): the pattern by hand
    hf = h.filter_harmonic(3)
    assert np.array_equal(hf != 0, t >= kn[6]) and np.all(hf[t >= kn[6]] == ah[6, 3])
    for m in (1, 2, 3):
        hf, mk = check_filtered("ampthr 0, harmonic %d" % m, with_ah(h, ah, ampthr=0), m, e["hz"], ah, h.fmin, np.inf, 0)
        assert hf.all()


def test_filter_nan_knot():
    """a NaN knot: np.max propagates it, the amplitude term compares against NaN and cuts nothing; the amplitude and the signal
    are NaN in the two segments that touch the knot (their far ends excluded) and nowhere else"""
    e = mask_case()
    n, ah = e["n"], np.array(e["ah"])
    ah[3, 2] = complex(np.nan, np.nan)
    kn = 511 // 2 + np.arange(7) * 100
    t = np.arange(n)
    h = with_ah(harmonic(e["x"], e["hz"], 511, 100, 9, fmin=0, fmax=np.inf), ah, ampthr=0.5)
    hf, y = h.filter_harmonic(2), h.resynth_partial(2, filter=True)
    nan = (t > kn[2]) & (t < kn[4])
    assert np.array_equal(np.isnan(hf.real), nan) and np.array_equal(np.isnan(hf.imag), nan) and np.array_equal(np.isnan(y), nan)
    assert np.array_equal(np.isnan(np.interp(t, kn, ah[:, 2].real)), nan)                 # numpy's own pattern
    ref = hr.interp_amp(n, 511, 100, ah[:, 2])
    mk = hr.filter_mask(ref, e["hz"], 2, SR, h.fmin, np.inf, 0.5)
    assert not (mk["fmin"] | mk["fmax"] | mk["nyquist"] | mk["amp"]).any() and hf[~nan].all()
    ok = ~nan & ~np.isnan(ref)
    within("(e) NaN knot: kept values outside its segments", np.abs(hf - ref)[ok], interp_bound(np.nan_to_num(ah[:, 2]), n, 511, 100)[ok])
    assert np.array_equal(bits(hf[kn[[2, 4]]]), bits(ah[[2, 4], 2]))
    # with the knot finite the same threshold does cut
    fin = with_ah(h, e["ah"], ampthr=0.5)
    hf2, mk2 = check_filtered("ampthr 0.5 without the NaN", fin, 2, e["hz"], e["ah"], h.fmin, np.inf, 0.5)
    assert 0 < mk2["amp"].sum() < n
