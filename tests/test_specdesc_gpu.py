"""Windowed spectral measures on the MI355X (k_specdesc.hip through pypevoc_amd.SoundUtils and pypevoc_amd.speech) against
the reference's outputs (tests/golden/M*.npz, make_golden_specdesc.py).

Bounds (SPECDESC.md).  The project holds the magnitudes of a spectrum to 1e-9 relative per bin; from that follow
  centroid     1e-9 relative (a ratio of two sums of non-negative terms), the reference's nan (a silent frame) a nan;
  flux         1e-9 * (||X_i|| + ||X_i+1||) absolute over the band (triangle inequality; the scale is computed with numpy
               from the fixture's signal), an exact zero of the reference (empty band, silence) exactly zero;
  periodogram  1e-9 relative per bin;
  AvgWind, rmsWind  1e-12 relative: they run the existing reduction kernel;
  cog, std, skew, kurt, level  four times the change the fixture recorded for perturbations of 1e-9 of the periodogram.
No frame, bin or case is left out.  Host and device-resident input, chunked and unchunked: identical bits.  The fused and
the rows route are different transforms: each within the bounds of the reference, and of each other."""
import ctypes

import numpy as np
import pytest

from .test_specdesc_cpu import MOMENTS, all_cases, case_kwargs, case_signal, flux_scale, get_case, np_mean_power

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ROWS = "k_frames+rocfft+k_specdesc_rows"
FUSED = (512, 1024, 2048)


def expected_kernels(nwind, psd=False):
    if nwind in FUSED:
        return "k_specdesc_fused<%d>" % nwind + ("+k_specdesc_mean" if psd else "")
    return ROWS + ("+k_specdesc_mean" if psd else "")


def assert_centroid(got, ref, what):
    assert got.shape == ref.shape and got.dtype == np.float64, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    err = float(np.max(np.abs(got[ok] - ref[ok]) / np.abs(ref[ok]), initial=0.0))
    print("%s: centroid max rel err %.3e (%d nan)" % (what, err, int((~ok).sum())))
    assert err <= RTOL, (what, err)


def assert_flux(got, ref, scale, what):
    assert got.shape == ref.shape and got.dtype == np.float64, what
    assert np.array_equal(got == 0, ref == 0), what                   # exact zeros stay exact zeros
    assert np.array_equal(ref == 0, scale == 0), what
    nz = scale != 0
    err = float(np.max(np.abs(got[nz] - ref[nz]) / scale[nz], initial=0.0))
    print("%s: flux max err / (|X_i| + |X_i+1|) %.3e (%d exact zeros)" % (what, err, int((~nz).sum())))
    assert err <= RTOL, (what, err)


def assert_power(got, ref, what):
    assert got.shape == ref.shape and got.dtype == np.float64 and (ref > 0).all(), what
    err = float(np.max(np.abs(got - ref) / ref))
    print("%s: periodogram max rel err %.3e over %d bins" % (what, err, len(ref)))
    assert err <= RTOL, (what, err)


def run(case, x):
    from pypevoc_amd import SoundUtils as su
    return getattr(su, case["func"])(x, **case_kwargs(case))


# ---- accuracy against the fixtures ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cname", all_cases("SpecCentWind", "SpecFlux"))
def test_centroid_and_flux_match_the_reference(name, cname):
    from pypevoc_amd import SoundUtils as su
    g, case = get_case(name, cname)
    ref, tref = g[cname + "_out"], g[cname + "_t"]
    got, t = run(case, case_signal(g, case))
    assert t.dtype == np.float64 and t.shape == tref.shape and np.array_equal(t, tref)
    if ref.size == 0:
        assert got.shape == (0,) and got.dtype == np.float64 and su.last_kernels() == ""
        return
    assert su.last_kernels() == expected_kernels(case["kw"]["nwind"])
    if case["func"] == "SpecCentWind":
        assert_centroid(got, ref, cname)
    else:
        assert_flux(got, ref, flux_scale(name, cname, len(ref))[0], cname)


@pytest.mark.parametrize("name,cname", all_cases("AvgWind", "rmsWind"))
def test_windowed_reductions_match_the_reference(name, cname):
    from pypevoc_amd import SoundUtils as su
    from pypevoc_amd.speech import SpeechAnalysis as sa
    g, case = get_case(name, cname)
    x = case_signal(g, case)
    if case["func"] == "AvgWind":
        got, t = su.AvgWind(x, **case_kwargs(case))
    else:
        t, got = sa.rmsWind(x, **case_kwargs(case))
    ref = g[cname + "_out"]
    assert got.shape == ref.shape and got.dtype == np.float64 and np.array_equal(t, g[cname + "_t"])
    err = float(np.max(np.abs(got - ref) / np.abs(ref)))
    print("%s: max rel err %.3e" % (cname, err))
    assert err <= 1e-12, (cname, err)


@pytest.mark.parametrize("name,cname", all_cases("SpectralMoments"))
def test_spectral_moments_match_the_reference(name, cname):
    from pypevoc_amd import SoundUtils as su
    from pypevoc_amd.speech import SpeechAnalysis as sa
    g, case = get_case(name, cname)
    kw = case_kwargs(case)
    x = case_signal(g, case)
    nwind, hop, nfr = (int(v) for v in g[cname + "_geom"])
    got = sa.SpectralMoments(x, **kw)
    P, freq = sa.Periodogram(x, kw["Fs"])
    assert sorted(got) == sorted(MOMENTS) and np.array_equal(freq, g[cname + "_freq_full"])
    assert P.shape == (nwind // 2,) and P.dtype == np.float64
    if nfr <= 0:                                                      # the reference's zeros / nFrames: nothing was launched
        assert su.last_kernels() == ""
        for k in MOMENTS:
            want = float(g[cname + "_" + k])
            assert (np.isnan(got[k]) and np.isnan(want)) or (got[k] == want == 0), (cname, k, got[k], want)
        assert np.array_equal(np.sqrt(P), g[cname + "_sxx_full"], equal_nan=True)
        return
    assert su.last_kernels() == expected_kernels(nwind, psd=True)
    assert_power(P, g[cname + "_sxx_full"]**2, cname)
    for k in MOMENTS:
        want, sens = float(g[cname + "_" + k]), float(g[cname + "_sens_" + k])
        print("%s: %s %.12g, off the reference by %.3e (bound %.3e)" % (cname, k, got[k], abs(got[k] - want), 4 * sens))
        assert abs(got[k] - want) <= 4 * sens, (cname, k, got[k], want, sens)
    # windFunc is accepted and ignored, as the reference ignores it
    assert sa.SpectralMoments(x, windFunc=np.ones, **kw) == got


# ---- routes ----------------------------------------------------------------------------------------------------------------
def periodogram_case(nwind, mult=12, seed=4):
    """A signal and a rate whose SpectralMoments window is nwind samples and whose hop does not divide it."""
    rng = np.random.default_rng(seed + nwind)
    n = mult * nwind
    Fs = 40.0 * nwind
    x = (np.sin(2 * np.pi * 0.013 * np.arange(n)**1.1) * np.exp(-3.0 * (np.arange(n) % 2500) / 2500.0) + 1e-3 * rng.standard_normal(n)).astype(np.float32)
    return x, Fs, dict(tWind=0.025, tHop=0.0125 * 0.9)


@pytest.mark.parametrize("nwind", [512, 1024, 2048, 256, 1000])
def test_periodogram_routes_against_numpy(nwind, monkeypatch):
    from pypevoc_amd import SoundUtils as su
    from pypevoc_amd.speech import SpeechAnalysis as sa
    x, Fs, kw = periodogram_case(nwind)
    nw, hop, nfr = sa.frame_geometry(len(x), Fs, kw["tWind"], kw["tHop"])
    assert nw == nwind and nwind % hop != 0 and nfr > 16
    want = np_mean_power(x, nwind, hop, nfr, sa.hamming(nwind))
    P, _ = sa.Periodogram(x, Fs, **kw)
    assert su.last_kernels() == expected_kernels(nwind, psd=True)
    assert_power(P, want, "nwind %d against numpy" % nwind)
    if nwind in FUSED:
        monkeypatch.setenv("PVX_SPECDESC_ROWS", "1")
        Pr, _ = sa.Periodogram(x, Fs, **kw)
        assert su.last_kernels() == ROWS + "+k_specdesc_mean"
        monkeypatch.delenv("PVX_SPECDESC_ROWS")
        assert_power(Pr, want, "nwind %d rows against numpy" % nwind)
        assert_power(Pr, P, "nwind %d rows against fused" % nwind)


@pytest.mark.parametrize("name,cname", [(n, c) for n, c in all_cases("SpecCentWind", "SpecFlux") if n == "M1_fused"])
def test_fused_and_rows_routes_agree(name, cname, monkeypatch):
    from pypevoc_amd import SoundUtils as su
    g, case = get_case(name, cname)
    x = case_signal(g, case)
    ref = g[cname + "_out"]
    vf, tf = run(case, x)
    assert su.last_kernels().startswith("k_specdesc_fused")
    monkeypatch.setenv("PVX_SPECDESC_ROWS", "1")
    vr, tr = run(case, x)
    assert su.last_kernels() == ROWS
    monkeypatch.delenv("PVX_SPECDESC_ROWS")
    assert np.array_equal(tf, tr)
    if case["func"] == "SpecCentWind":
        assert_centroid(vr, ref, cname + " rows against the reference")
        assert_centroid(vr, vf, cname + " rows against fused")
    else:
        scale = flux_scale(name, cname, len(ref))[0]
        assert_flux(vr, ref, scale, cname + " rows against the reference")
        assert_flux(vr, vf, scale, cname + " rows against fused")


# ---- the same bits wherever the samples come from and however the call is cut ------------------------------------------------
BITS = [("M1_fused", "cent512"), ("M1_fused", "flux1024_hann_f64"), ("M1_fused", "flux2048_gap"), ("M1_fused", "cent2048"),
        ("M2_rows", "cent256_i16"), ("M2_rows", "flux1000_i16"), ("M2_rows", "flux333_mirror"), ("M2_rows", "cent333_gap")]
BITS_PSD = [("M3_moments", "mom8k"), ("M3_moments", "mom8k_f64_fcut1k"), ("M3_moments", "mom44k")]


@pytest.mark.parametrize("name,cname", BITS)
def test_device_resident_and_chunked_input_are_bit_identical(name, cname, monkeypatch):
    import torch
    g, case = get_case(name, cname)
    x = case_signal(g, case)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    assert str(xd.dtype) == "torch." + case["dtype"]
    v, t = run(case, x)
    vd, td = run(case, xd)
    assert v.tobytes() == vd.tobytes() and np.array_equal(t, td)
    nwind = case["kw"]["nwind"]
    for limit in (20000, 4 * nwind + 4, 100000):                      # a few values, ONE value, many values per chunk
        monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(limit))
        v2, t2 = run(case, x)
        assert v2.tobytes() == v.tobytes() and np.array_equal(t2, t), limit
    monkeypatch.delenv("PVX_MAX_DEVICE_BYTES")


@pytest.mark.parametrize("name,cname", BITS_PSD)
def test_periodogram_of_device_resident_and_chunked_input_is_bit_identical(name, cname, monkeypatch):
    import torch
    from pypevoc_amd.speech import SpeechAnalysis as sa
    g, case = get_case(name, cname)
    kw = case_kwargs(case)
    x = case_signal(g, case)
    nwind, hop, nfr = (int(v) for v in g[cname + "_geom"])
    assert nfr > 2 * 16                                               # several blocks
    P, _ = sa.Periodogram(x, kw["Fs"])
    Pd, _ = sa.Periodogram(torch.from_numpy(np.ascontiguousarray(x)).cuda(), kw["Fs"])
    assert P.tobytes() == Pd.tobytes()
    want = sa.SpectralMoments(x, **kw)
    for limit in (x.itemsize * (nwind + 20 * hop), 4 * nwind + 4, 1 << 20):   # blocks of 16 frames: one per chunk, one again, all
        monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(limit))
        P2, _ = sa.Periodogram(x, kw["Fs"])
        assert P2.tobytes() == P.tobytes(), limit
        assert sa.SpectralMoments(x, **kw) == want
    monkeypatch.delenv("PVX_MAX_DEVICE_BYTES")


@pytest.mark.parametrize("nwind", [512, 2048])
def test_fused_periodogram_chunked_and_device_resident(nwind, monkeypatch):
    import torch
    from pypevoc_amd.speech import SpeechAnalysis as sa
    x, Fs, kw = periodogram_case(nwind, mult=20)
    _, hop, nfr = sa.frame_geometry(len(x), Fs, kw["tWind"], kw["tHop"])
    assert nfr > 2 * 16
    P, _ = sa.Periodogram(x, Fs, **kw)
    Pd, _ = sa.Periodogram(torch.from_numpy(x).cuda(), Fs, **kw)
    assert P.tobytes() == Pd.tobytes()
    monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(4 * (nwind + 20 * hop)))
    P2, _ = sa.Periodogram(x, Fs, **kw)
    monkeypatch.delenv("PVX_MAX_DEVICE_BYTES")
    assert P2.tobytes() == P.tobytes()


def test_long_signal_equals_its_pieces():
    """Another grid, another run, another position in the call: value i of a long call has the bits of value 0 of a call that
    starts at its frame."""
    from pypevoc_amd import SoundUtils as su
    x = np.random.default_rng(6).standard_normal(200000).astype(np.float32)
    for nwind, hop in ((1024, 441), (333, 100)):
        c, t = su.SpecCentWind(x, sr=44100, nwind=nwind, nhop=hop)
        f, tf = su.SpecFlux(x, sr=44100, nwind=nwind, nhop=hop, minf=100, maxf=30000)
        assert len(c) == (len(x) - nwind + hop - 1) // hop and len(f) == (len(x) - hop - nwind + hop - 1) // hop
        for i in (0, 1, 2, 3, 4, 5, 200, len(f) - 1):
            ci, _ = su.SpecCentWind(x[i * hop: i * hop + nwind + 1], sr=44100, nwind=nwind, nhop=hop)
            fi, _ = su.SpecFlux(x[i * hop: i * hop + nwind + hop + 1], sr=44100, nwind=nwind, nhop=hop, minf=100, maxf=30000)
            assert ci.shape == fi.shape == (1,) and ci.tobytes() == c[i: i + 1].tobytes() and fi.tobytes() == f[i: i + 1].tobytes(), (nwind, i)


# ---- edges -----------------------------------------------------------------------------------------------------------------
def test_no_frame_shapes_and_kinds():
    import torch
    from pypevoc_amd import SoundUtils as su
    from pypevoc_amd.speech import SpeechAnalysis as sa
    for w in (np.zeros(1024), np.zeros(100, dtype=np.float32), np.zeros(0), torch.zeros(1024, dtype=torch.float64, device="cuda")):
        for fn in (su.SpecCentWind, su.SpecFlux):
            v, t = fn(w, sr=8000)
            assert v.shape == (0,) and t.shape == (0,) and v.dtype == np.float64 and t.dtype == np.float64 and su.last_kernels() == ""
    d = sa.SpectralMoments(np.ones(250, dtype=np.float32), 8000)
    assert all(np.isnan(d[k]) for k in MOMENTS)
    d = sa.SpectralMoments(np.ones(100, dtype=np.float32), 8000)
    assert d["level"] == 0 and all(np.isnan(d[k]) for k in MOMENTS[:4])
    with pytest.raises(ValueError):
        su.SpecFlux(np.zeros((2, 4000)))


def test_silent_signal():
    from pypevoc_amd import SoundUtils as su
    for nwind in (512, 333):
        x = np.zeros(5000, dtype=np.float32)
        f, _ = su.SpecFlux(x, nwind=nwind, nhop=200)
        c, _ = su.SpecCentWind(x, nwind=nwind, nhop=200)
        assert len(f) and (f == 0).all() and not np.signbit(f).any() and np.isnan(c).all()


def test_frame_count_beyond_the_signal_is_refused():
    from pypevoc_amd import _lib
    lib = _lib.load()
    _lib.init()
    x = np.zeros(2000)
    wind = np.hanning(512)
    a = np.ones(257)
    out = np.zeros(64)
    args = lambda nfr, meas: (ctypes.c_void_p(x.ctypes.data), _lib.PVX_F64, len(x), _lib.dptr(wind), 512, 100, nfr, meas, _lib.dptr(a),
                              _lib.dptr(a), _lib.dptr(out))
    assert lib.pvx_specdesc(*args(15, 0)) == 15                       # 14 * 100 + 512 = 1912 <= 2000
    assert lib.pvx_specdesc(*args(16, 0)) == _lib.PVX_ERR_SIZE
    assert lib.pvx_specdesc(*args(14, 1)) == 14                       # the flux reads frame 14 too
    assert lib.pvx_specdesc(*args(15, 1)) == _lib.PVX_ERR_SIZE
    assert lib.pvx_specdesc(*args(0, 1)) == 0 and lib.pvx_specdesc_last_kernels() == b""
    assert lib.pvx_specdesc(*args(3, 7)) < 0


@pytest.mark.parametrize("nwind", [512, 200])
def test_long_calls_cross_groups_batches_and_run_lengths(nwind, monkeypatch):
    """70 000 frames in one call: the fused periodogram's workspace holds 4096 blocks at a time and the rows route transforms
    about 21 000 frames of 200 samples per batch, a flux batch overlapping the next by a row; flux runs are 16 frames long
    here and 4 in the chunks of the host call.  The bits are those of the chunked call, the values numpy's."""
    import torch
    from pypevoc_amd import SoundUtils as su
    from pypevoc_amd.speech import SpeechAnalysis as sa
    hop, nfr = 8, 70000
    Fs = 40.0 * nwind
    x = np.random.default_rng(nwind).standard_normal(nfr * hop + nwind + 1).astype(np.float32)
    kw = dict(tWind=0.025, tHop=hop / Fs)
    assert sa.frame_geometry(len(x), Fs, **kw) == (nwind, hop, nfr)
    xd = torch.from_numpy(x).cuda()
    P, _ = sa.Periodogram(xd, Fs, **kw)
    f, _ = su.SpecFlux(xd, sr=Fs, nwind=nwind, nhop=hop, minf=0.1 * Fs, maxf=0.7 * Fs)
    c, _ = su.SpecCentWind(xd, sr=Fs, nwind=nwind, nhop=hop)
    assert len(f) == nfr and len(c) == nfr + 1
    monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(1 << 17))          # 32 768 samples: about 4000 frames per chunk
    P2, _ = sa.Periodogram(x, Fs, **kw)
    f2, _ = su.SpecFlux(x, sr=Fs, nwind=nwind, nhop=hop, minf=0.1 * Fs, maxf=0.7 * Fs)
    c2, _ = su.SpecCentWind(x, sr=Fs, nwind=nwind, nhop=hop)
    monkeypatch.delenv("PVX_MAX_DEVICE_BYTES")
    assert P2.tobytes() == P.tobytes() and f2.tobytes() == f.tobytes() and c2.tobytes() == c.tobytes()
    frames = np.lib.stride_tricks.sliding_window_view(x.astype(np.float64), nwind)[::hop]
    acc = np.zeros(nwind // 2)
    for i in range(0, nfr, 5000):
        acc += (np.abs(np.fft.rfft(frames[i: min(i + 5000, nfr)] * sa.hamming(nwind), axis=1))[:, : nwind // 2]**2).sum(axis=0)
    assert_power(P, acc / nfr, "nwind %d, %d frames against numpy" % (nwind, nfr))
    # a flux value at every position of a run and on both sides of a batch boundary (20 971 rows of 200 samples)
    band = su.fold_bins(su.flux_band(Fs, nwind, 0.1 * Fs, 0.7 * Fs), nwind)
    for i in (0, 15, 16, 17, 20968, 20969, 20970, 20971, 65535, 65536, nfr - 1):
        m = np.abs(np.fft.rfft(frames[i: i + 2] * np.blackman(nwind), axis=1))
        want = np.sqrt(np.sum(band * (m[0] - m[1])**2))
        scale = np.sqrt(np.sum(band * m[0]**2)) + np.sqrt(np.sum(band * m[1]**2))
        assert abs(f[i] - want) <= RTOL * scale, (nwind, i)
        wc = np.sum(m[0][: nwind // 2] * np.arange(nwind // 2) / float(nwind) * Fs) / np.sum(m[0][: nwind // 2])
        assert abs(c[i] - wc) <= RTOL * wc, (nwind, i)
