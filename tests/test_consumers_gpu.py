"""Differential tests of the kernels beside the analysis path, at the shapes and arguments where they branch:

  k_desc.hip      k_f0, k_hpower_rows, k_hpower behind PV.calc_f0 / PV.calc_harmonic_power on resident results, against
                  the plain per-frame references of tests/plain_refs.py applied to the arrays the same object hands out;
  k_harmonic.hip  k_harmonic_rows<float|double> against oracle.harmonic through test_hip_parity._harm_compare, on inputs
                  built to reach named branches (tests/test_plain_refs_cpu.py confirms on the CPU that they do);
  k_reduce.hip    k_heterodyne, k_rms_frames, k_funcwind<CPX> against plain per-frame loops.

Descriptor signals (22.05 kHz, nfft 1024, hop 256, float64 samples and analysis):
  (a) a 6-harmonic tone with 3 % vibrato over noise at 1e-3, two stretches of exact zeros longer than nfft (all-silent
      frames) and pkthresh 0.05, which leaves the slots after the sixth empty in voiced frames;
  (b) white noise.  At nfft 1024 the peak picker's salience radius of 5 bins leaves at most about 50 peaks in a frame, so
      with K = 64 .. 100 the upper slots of (b) are empty: it fills every slot only up to K = 20;
  (c) two steady sines;
  (d) 71 steady sines 7 bins apart, added here because (b) cannot do it: 71 valid slots per frame, so with K = 100 the
      second trip of k_hpower's slot loop and of k_hpower_rows' column loop work on values, not on zeros.
The peak picker writes a frame's peaks into its first slots, so no resident result has an empty slot between valid ones;
arrays with such holes reach the references and the host path in tests/test_plain_refs_cpu.py.

NaN.  k_f0's running maximum skips NaN magnitudes where np.max propagates them.  A NaN sample makes every bin of the
frames that contain it NaN; no bin then compares greater than its neighbour, the peak picker finds nothing and those frames
come out all-empty (f = mag = 0), on the oracle and on the device alike (test_f0_of_a_signal_with_a_nan_sample).  No row of
a resident `mag` holds a NaN beside finite entries, so no caller of the device path can tell the two maxima apart; the
kernel's comment says which one it computes.  Arrays edited on the host take the numpy path, which propagates."""
import functools

import numpy as np
import pytest

from .plain_refs import calc_f0_ref, funcwind_ref, harmonic_power_ref, heterodyne_ref, rms_ref
from .test_hip_parity import _harm_compare, amd, run_pv  # noqa: F401  (amd: the module-scoped fixture)
from .test_plain_refs_cpu import REDUCERS, SR, harmonic_case, hpower_bound, reduction_cases, reduction_signal

pytestmark = pytest.mark.gpu

NFFT, HOP = 1024, 256
PKTHRESH = {"a": 0.05, "b": 0.005, "c": 0.05, "d": 0.05}


def _nsamp(F):
    return NFFT + HOP * (F - 1) + 1                                  # ceil((n - nfft) / hop) = F frames


@functools.lru_cache(maxsize=None)
def _full_signal(kind):
    n = _nsamp(1030)
    t = np.arange(n) / SR
    if kind == "a":
        rng = np.random.default_rng(101)
        ph = 2 * np.pi * np.cumsum(330.0 * (1 + 0.03 * np.sin(2 * np.pi * 5.0 * t))) / SR
        x = sum(0.3 / h * np.sin(h * ph) for h in range(1, 7)) + 1e-3 * rng.standard_normal(n)
        x[5000:6500] = 0.0
        x[40000:42000] = 0.0
    elif kind == "b":
        x = 0.1 * np.random.default_rng(102).standard_normal(n)
    elif kind == "c":
        x = 0.4 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t)
    else:
        rng = np.random.default_rng(104)
        x = np.zeros(n)
        for k in range(71):
            x += (0.012 + 0.001 * (k % 5)) * np.sin(2 * np.pi * (7 * k + 9.3) * SR / NFFT * t + rng.uniform(0, 2 * np.pi))
    x.setflags(write=False)
    return x


def signal(kind, F):
    return _full_signal(kind)[: _nsamp(F)]


def analysed(amd, kind, F, K, x=None):
    p = run_pv(amd, signal(kind, F) if x is None else x, SR, NFFT, HOP, K, pkthresh=PKTHRESH[kind], precision=64)
    assert p._on_device() and p.nframes == F
    return p


def check_f0(p, args=()):
    """Device calc_f0 first, then the arrays come to the host and the plain reference runs on them."""
    fm = p.calc_f0(*args)
    idx = np.array(p.fundamental_idx)
    assert p._on_device()
    rfm, ridx = calc_f0_ref(p.f, p.mag, *args)
    assert fm.dtype == np.float64 and np.array_equal(fm.view(np.int64), rfm.view(np.int64)), args   # a selected copy: bit-equal
    assert np.array_equal(idx, ridx), args
    return rfm, ridx


def check_hpower(p, thr=None, raises=False):
    """Device calc_harmonic_power against the plain reference; returns the measured worst relative hpower error."""
    args = () if thr is None else (thr,)
    K = p.npeaks
    if raises:
        with pytest.raises(IndexError):
            p.calc_harmonic_power(*args)
        assert p._on_device()
        with pytest.raises(IndexError):
            harmonic_power_ref(p.f, p.mag, *args)
        return 0.0
    p.calc_harmonic_power(*args)
    hp, nh = np.array(p.hpower), np.array(p.nharmonics)
    assert p._on_device()
    rhp, rnh = harmonic_power_ref(p.f, p.mag, *args)
    assert np.array_equal(nh, rnh), thr
    assert np.array_equal(hp == 0, rhp == 0), thr                    # exact zeros stay exact zeros
    rel = np.abs(hp - rhp) / np.where(rhp == 0, 1.0, rhp)
    print("hpower F=%d K=%d thr=%r: worst relative error %.3g (bound %.3g)" % (p.nframes, K, thr, rel.max(), hpower_bound(K)))
    assert rel.max() <= hpower_bound(K), (thr, rel.max())
    return rel.max()


# every F of {1, 3, 255, 257, 1030} and every K of {1, 3, 20, 64, 65, 100} on (a) and on (b); K = 65 and 100 with F = 257.
# `raises`: a valid slot >= F, which the reference's row indexing turns into an IndexError
DESCRIPTOR_CASES = [
    ("a", 1, 1, False), ("a", 3, 3, False), ("a", 255, 20, False), ("a", 257, 64, False), ("a", 257, 65, False),
    ("a", 257, 100, False), ("a", 1030, 3, False), ("a", 3, 20, True),
    ("b", 1, 1, False), ("b", 3, 3, False), ("b", 255, 64, False), ("b", 257, 20, False), ("b", 257, 65, False),
    ("b", 257, 100, False), ("b", 1030, 20, False), ("b", 1, 3, True),
    ("d", 257, 100, False), ("d", 255, 65, False),
]


@pytest.mark.parametrize("kind,F,K,raises", DESCRIPTOR_CASES, ids=["%s-F%d-K%d" % c[:3] for c in DESCRIPTOR_CASES])
def test_descriptors_on_resident_results(amd, kind, F, K, raises):
    """Frame counts around k_f0's block of 256 and k_hpower's block of 4 waves, slot counts around the wave width, F < K."""
    p = analysed(amd, kind, F, K)
    rfm, _ = check_f0(p)
    check_hpower(p, raises=raises)
    valid = p.f > 0
    if kind == "a" and F >= 255:
        assert (~valid).all(axis=1).sum() >= 4                       # all-silent frames: (0.0, 0), zero rows
        assert not rfm[(~valid).all(axis=1)].any()
        if K >= 20:
            assert not valid[:, 12:].any() and valid[:, 5].any()     # later slots stay empty in voiced frames
    if kind == "b" and K <= 20 and F >= 255:
        assert valid.all(axis=0).any() and valid[:, K - 1].any()     # every slot in use
    if kind == "d":
        assert (valid.sum(axis=1) > 64).all()                        # valid slots past a wave's width


@pytest.mark.parametrize("kind,F,K", [("a", 255, 20), ("b", 257, 20)])
def test_descriptor_arguments(amd, kind, F, K):
    """The non-default arguments reach the kernels: (fmin, fmax, thr) incl. thr = 1 (nothing exceeds the maximum) and
    fmin > fmax (both all zeros), f_threshold incl. 0 (|x| < 0 never holds: every count is 0, the peak's own included)."""
    p = analysed(amd, kind, F, K)
    for args in ((50, 10000, 0.1), (300, 2000, 0.3), (0, 1e9, 0.0), (50, 10000, 1.0), (2000, 300, 0.1)):
        rfm, ridx = check_f0(p, args)
        if args[2] == 1.0 or args[0] > args[1]:
            assert not rfm.any() and not ridx.any()
        else:
            assert rfm.any()
    seen = set()
    for thr in (0.01, 0.05, 0.5, 0.0):
        check_hpower(p, thr)
        seen.add(float(p.nharmonics.sum()))
        if thr == 0.0:
            assert not p.nharmonics.any() and not p.hpower.any()
    assert len(seen) == 4                                            # each threshold gives another answer


def test_harmonic_power_with_fewer_frames_than_slots(amd):
    """F = 3 < K = 20.  Noise fills slots >= 3: IndexError on the device path as from the reference's row indexing.  Two
    sines over a high threshold use slots 0 and 1 only: rows 0 and 1 exist, k_hpower_rows writes zeros for the rows that
    do not, and the values equal the reference's."""
    p = analysed(amd, "b", 3, 20)
    check_f0(p)
    assert (p.f[:, 3:] > 0).any()
    check_hpower(p, raises=True)
    p = analysed(amd, "c", 3, 20)
    check_f0(p)
    assert (p.f[:, :2] > 0).all() and not (p.f[:, 2:] > 0).any()
    check_hpower(p)
    assert p.hpower[:, :2].all() and not p.hpower[:, 2:].any()


def test_f0_of_a_signal_with_a_nan_sample(amd, oracle):
    """One NaN sample in signal (a): the frames that contain it come out all-empty, no row of `mag` holds a NaN beside
    finite entries (device and oracle), and the device calc_f0 equals the NaN-propagating reference on every row."""
    x = signal("a", 255).copy()
    x[20000] = np.nan
    o = oracle.analyze(x, SR, NFFT, HOP, 20, PKTHRESH["a"])
    p = analysed(amd, "a", 255, 20, x=x)
    rfm, ridx = check_f0(p)
    check_hpower(p)
    hit = (np.arange(255) * HOP <= 20000) & (20000 < np.arange(255) * HOP + NFFT)
    assert hit.sum() == 4
    for mag, f in ((o["mag"], o["f"]), (p.mag, p.f)):
        assert not np.isnan(mag).any() and not np.isnan(f).any()
        assert not mag[hit].any() and not f[hit].any()
    assert not rfm[hit].any() and not ridx[hit].any() and rfm[~hit].any()
    # the other analysis routes (float32, the nfft-2048 kernels): no row with a NaN beside finite entries either, and
    # calc_f0 equal to the propagating reference
    for nfft, hop, precision in ((1024, 256, 32), (2048, 512, 64), (2048, 512, 32)):
        q = run_pv(amd, x, SR, nfft, hop, 20, pkthresh=PKTHRESH["a"], precision=precision)
        assert q._on_device()
        check_f0(q)
        assert not (np.isnan(q.mag).any(axis=1) & np.isfinite(q.mag).any(axis=1)).any(), (nfft, precision)


# ------------------------------------------------------------------ k_harmonic.hip
def _run_harmonic(amd, c, precision):
    p = amd.PVHarmonic(c["x"], c["sr"], nfft=c["nfft"], hop=c["hop"], npks=c["K"], progress=False, precision=precision)
    assert p.fmin == c["fmin"]
    p.set_f0(c["f0"])
    p.run_pv()
    return p


@pytest.mark.parametrize("name,precision", [("deep", 64), ("few", 64), ("bin1", 64), ("nyq", 64), ("deep", 32), ("few", 32), ("bin1", 32)])
def test_harmonic_branches_against_oracle(amd, oracle, name, precision):
    """Seeded f0 tracks with 0 and NaN entries on about 40 frames (test_plain_refs_cpu.harmonic_case says which branch
    each reaches and test_harmonic_cases_reach_their_branches confirms it):
      deep  7 trips of the harmonic loop, K = 100 > 64, residual over ~400 partial sums
      few   nh = 3 < K: trailing slots stay 0; frame 0 has nh = 0
      bin1  first harmonic on bin 1: left clamp of the 3-bin sum; re-centred harmonics, K = 80
      nyq   last harmonic on bin N2 - 1: right clamp, odd nfft
    What the fixtures reach, computed with the oracle from their f0 tracks: H1 / H2 have nh = 98 .. 101 (two trips of the
    harmonic loop, K = 8 / 24), H3 nh = 42 (one trip, K = 3), H4 nh = 7 < K = 12 in its first half and nh = 880 (14 trips,
    first harmonic on bin 1, measured below fmin so nothing is re-centred) in its second.  A last harmonic on bin N2 - 1
    occurs in 9 / 10 / 21 frames of H1 / H2 / H4, always past the K stored ones: the right clamp only enters their
    residuals.  No fixture has K > 64, re-centred harmonics beyond the first trip that are stored, or a stored harmonic
    on N2 - 1; the seeded case of test_hip_parity (nh = 35, K = 10) takes one trip."""
    c = harmonic_case(name)
    p = _run_harmonic(amd, c, precision)
    o = oracle.harmonic(c["x"], c["sr"], c["f0"], c["nfft"], c["hop"], c["K"], c["fmin"])
    g = dict(o, nframes=c["frames"], hop=c["hop"], sr=c["sr"])
    fin = np.isfinite(o["residuals"])
    tot = (o["mag"] ** 2).sum(axis=1) + np.where(fin, o["residuals"], 0.0) ** 2
    print("harmonic %s/%d: |df| %.3g Hz, |dmag| %.3g, |dph| %.3g, residual**2 %.3g of the frame energy" % (
        name, precision, np.nanmax(np.abs(p.f - o["f"])), np.abs(p.mag - o["mag"]).max(), np.abs(p.ph - o["ph"]).max(),
        (np.abs(p.residuals[fin] ** 2 - o["residuals"][fin] ** 2) / tot[fin]).max()))
    _harm_compare(p, g, precision)
    if name == "few":
        assert not p.f[:, 3:].any() and not p.mag[:, 3:].any() and not p.ph[:, 3:].any()
        assert not p.f[0].any() and p.residuals[0] > 0


@pytest.mark.parametrize("precision", [64, 32])
def test_harmonic_deep_case_in_chunks_of_16_rows(amd, monkeypatch, precision):
    """The deep case over 90 frames with a NaN gap of 40 under PVX_MAX_ROWS=16: the previous valid spectrum of the frame
    after the gap sits three launches back (the carried row), at float32 as at float64, bitwise the single launch."""
    c = harmonic_case("deep", frames=90)
    c["f0"][20:60] = np.nan
    a = _run_harmonic(amd, c, precision)
    monkeypatch.setenv("PVX_MAX_ROWS", "16")
    b = _run_harmonic(amd, c, precision)
    assert np.isfinite(a.residuals[60:]).any() and np.isnan(a.residuals[20:60]).all()
    for k in ("f", "mag", "ph", "residuals", "t"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), k
    assert np.array_equal(a.oldfft, b.oldfft)


# ------------------------------------------------------------------ k_reduce.hip
def _tol(ref):
    return 1e-13 * max(1.0, float(np.abs(ref).max()))                # the project's bound for these kernels


@pytest.mark.parametrize("wlen,hop,n,exact", reduction_cases())
def test_reductions_against_plain_loops(amd, wlen, hop, n, exact):
    """heterodyne, RMSWind and FuncWind (six reducers; power 1 and 2 on reals; sum / mean / std / var on a complex signal)
    with np.hanning: windows shorter than a wave (most lanes add nothing), 64 and 65, hop > wlen, hop = 1, 1 / 2 / 3 / 5
    frames (a ragged last block), and n - wlen an exact multiple of hop (`exact`: the frame at n - wlen does not exist)."""
    from pypevoc_amd import SoundUtils as su
    from pypevoc_amd.Heterodyne import heterodyne
    x = reduction_signal(n)
    xc = reduction_signal(n, cpx=True)
    w = np.hanning(wlen)
    nfr = len(range(0, n - wlen, hop))
    if exact:
        assert (n - wlen) % hop == 0 and nfr == (n - wlen) // hop
    hs = np.exp(-2j * np.pi * 0.0123 * np.arange(n))
    worst = 0.0
    h, ic = heterodyne(x, hs, wind=w, hop=hop)
    rh, ric = heterodyne_ref(x, hs, w, hop)
    assert len(h) == nfr and np.array_equal(ic, ric)
    worst = max(worst, np.abs(h - rh).max() / _tol(rh))
    assert np.abs(h - rh).max() <= _tol(rh)
    r, t = su.RMSWind(x, sr=SR, nwind=wlen, nhop=hop, windfunc=np.hanning)
    rr = rms_ref(x, w, hop)
    assert len(r) == nfr == len(t) and np.array_equal(t, (2 * np.arange(nfr) * hop + wlen) / 2.0 / SR)
    worst = max(worst, np.abs(r - rr).max() / _tol(rr))
    assert np.abs(r - rr).max() <= _tol(rr)
    for name in REDUCERS:
        for power in (1, 2):
            got, _ = su.FuncWind(name, x, sr=SR, nwind=wlen, nhop=hop, power=power, windfunc=np.hanning)
            ref = funcwind_ref(name, x, w, hop, power)
            assert got.shape == (nfr,) and got.dtype == np.float64
            if name in ("max", "min"):
                assert np.array_equal(got, ref), (name, power)
            else:
                worst = max(worst, np.abs(got - ref).max() / _tol(ref))
                assert np.abs(got - ref).max() <= _tol(ref), (name, power)
        if name not in ("max", "min"):
            got, _ = su.FuncWind(name, xc, sr=SR, nwind=wlen, nhop=hop, power=1, windfunc=np.hanning)
            ref = funcwind_ref(name, xc, w, hop, 1)
            assert got.shape == (nfr,) and got.dtype == ref.dtype
            worst = max(worst, np.abs(got - ref).max() / _tol(ref))
            assert np.abs(got - ref).max() <= _tol(ref), name
    print("reductions wlen=%d hop=%d n=%d: %d frames, worst error %.3g of the bound" % (wlen, hop, n, nfr, worst))


def test_reductions_min_max_with_nan_and_inf(amd):
    """np.min / np.max propagate a NaN into exactly the frames that contain it; -inf comes through min and +inf through
    max with the neighbouring frames finite (the sample never sits under one of np.hanning's zero end samples, where
    inf * 0 would be NaN); max of complex frames still raises."""
    from pypevoc_amd import SoundUtils as su
    wlen, hop, at = 63, 20, 150
    x = reduction_signal(400)
    starts = np.arange(0, len(x) - wlen, hop)
    holds = (starts <= at) & (at < starts + wlen)
    assert holds.sum() >= 3 and not ((starts == at) | (starts + wlen - 1 == at)).any()
    for name, fn, inf in (("min", np.min, -np.inf), ("max", np.max, np.inf)):
        xn = x.copy()
        xn[at] = np.nan
        got, _ = su.FuncWind(fn, xn, nwind=wlen, nhop=hop, windfunc=np.hanning)
        assert np.array_equal(np.isnan(got), holds), name
        assert np.array_equal(got, funcwind_ref(name, xn, np.hanning(wlen), hop), equal_nan=True), name
        xi = x.copy()
        xi[at] = inf
        got, _ = su.FuncWind(fn, xi, nwind=wlen, nhop=hop, windfunc=np.hanning)
        assert np.array_equal(got == inf, holds) and np.isfinite(got[~holds]).all(), name
        assert np.array_equal(got, funcwind_ref(name, xi, np.hanning(wlen), hop)), name
    # a window shorter than a wave: the lanes that add nothing must not bring their +-inf start values in
    got, _ = su.FuncWind(np.min, x, nwind=7, nhop=3, windfunc=np.hanning)
    assert np.isfinite(got).all()
    with pytest.raises(RuntimeError):
        su.FuncWind(np.max, reduction_signal(400, cpx=True), nwind=wlen, nhop=hop)
