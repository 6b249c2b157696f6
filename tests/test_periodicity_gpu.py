"""Time-domain periodicity on the MI355X (k_period.hip through pypevoc_amd.PeriodSeries) against the reference's outputs
(tests/golden/P*.npz, make_golden_period.py): counts, preferred and the voiced / NaN pattern identical, periods and
strengths within 1e-9 relative; plus the reference's own unit tests, device-resident input, calc == per_at_index, chunked
long signals and the edge cases."""
import numpy as np
import pytest

from .test_periodicity_cpu import ctor_kwargs, load_period_golden, period_golden_names

pytestmark = pytest.mark.gpu

RTOL = 1e-9


def run_like(g, r, x=None):
    from pypevoc_amd import PeriodTimeSeries
    ps = PeriodTimeSeries(g["x"] if x is None else x, **ctor_kwargs(g, r))
    if r["mode"] == "calc":
        ps.calc(**r.get("calc", {}))
    elif r["mode"] == "pbp":
        kw = {k: (g[v] if k in ("tf", "f") else v) for k, v in r["pbp"].items()}
        ps.calcPeriodByPeriod(**kw)
    else:
        ps.periods = [ps.per_at_index(r["index"])]
    return ps


def frames(ps, ncand):
    n = len(ps.periods)
    per = np.full((n, ncand), np.nan)
    st = np.full((n, ncand), np.nan)
    cnt = np.zeros(n, np.int32)
    pref = np.full(n, -1, np.int32)
    for i, p in enumerate(ps.periods):
        c = len(p.cand_period)
        cnt[i] = c
        per[i, :c] = p.cand_period
        st[i, :c] = p.cand_strength
        pref[i] = -1 if isinstance(p.preferred, list) else int(p.preferred)
    return per, st, cnt, pref


def assert_close(a, b, what):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, what
    assert (np.isnan(a) == np.isnan(b)).all(), what
    m = ~np.isnan(a)
    err = np.abs(a[m] - b[m]) / np.maximum(np.abs(b[m]), 1e-300)
    assert err.size == 0 or err.max() <= RTOL, (what, float(err.max()))


def xcorr_scores(g, r, centre):
    """The integer-lag similarity the reference picks xcorr peaks from (Periodicity.py:131-146, numpy) for one frame:
    {lag: value} at the interior maxima."""
    from pypevoc_amd import PeriodSeries
    ps = PeriodSeries(g["x"], **ctor_kwargs(g, r))
    n, w = ps.nwind, np.asarray(ps.wind, float)
    xs = ps.x[centre - n // 2:centre - n // 2 + n]
    xw = (xs - np.mean(xs)) * w
    xc = np.correlate(xw, xw, "full") / np.correlate(w, w, "full")
    neg = np.flatnonzero(xc[n - 1:] < 0)
    imin = max(neg.min() if len(neg) else ps.mindelay, ps.mindelay)
    y = (xc / max(xc[n - 1 - ps.maxdelay:n - 1 + ps.maxdelay]))[n - 1 + imin:n - 1 + ps.maxdelay]
    return {k + imin: y[k] for k in range(1, len(y) - 1) if y[k - 1] < y[k] >= y[k + 1]}


def check_against(g, r, ps):
    """Counts, preferred and the NaN pattern identical, values within RTOL.  One exception: a frame whose ncand-th and
    (ncand+1)-th correlation peaks tie to 4 ulp (a pure sine: every peak is 1.0 or 1.0 - 2**-52) keeps one or the
    other by the last bit of a sum, in the reference as here; there the candidates both keep and the preferred period
    must agree."""
    n = r["name"]
    ncand = r["ctor"].get("ncand", 8)
    per, st, cnt, pref = frames(ps, ncand)
    gper, gst, gpref = g[n + "_period"].copy(), g[n + "_strength"].copy(), g[n + "_preferred"].copy()
    assert np.array_equal(cnt, g[n + "_count"]), n
    for i in range(len(cnt)):
        if cnt[i] == 0 or np.allclose(np.sort(per[i, :cnt[i]]), np.sort(gper[i, :cnt[i]]), rtol=RTOL, atol=0):
            continue
        assert r["ctor"].get("method", "xcorr") == "xcorr" and r["mode"] != "pbp", (n, i, per[i], gper[i])
        sc = sorted(xcorr_scores(g, r, int(np.round(g[n + "_index"][i]))).values(), reverse=True)
        assert len(sc) > ncand and sc[ncand - 1] - sc[ncand] <= 4 * np.spacing(sc[ncand - 1]), (n, i, per[i], gper[i])
        both = [p for p in per[i, :cnt[i]] if np.isclose(gper[i, :cnt[i]], p, rtol=RTOL, atol=0).any()]
        assert len(both) == cnt[i] - 1, (n, i)
        assert abs(per[i, pref[i]] - gper[i, gpref[i]]) <= RTOL * gper[i, gpref[i]], (n, i)
        per[i], gper[i], st[i], gst[i] = np.nan, np.nan, np.nan, np.nan
        pref[i] = gpref[i]
    assert np.array_equal(pref, gpref), n
    assert_close(per, gper, n + " period")
    assert_close(st, gst, n + " strength")
    for k, v in (("_f0", ps.get_f0()), ("_f0_05", ps.get_f0(0.5)), ("_times", ps.get_times()), ("_strength_pref", ps.get_strength())):
        assert_close(v, g[n + k], n + k)


def golden_runs():
    out = []
    for name in period_golden_names():
        _, runs = load_period_golden(name)
        out += [(name, r["name"]) for r in runs]
    return out


@pytest.mark.parametrize("name,run", golden_runs())
def test_matches_reference(name, run):
    g, runs = load_period_golden(name)
    r = [q for q in runs if q["name"] == run][0]
    check_against(g, r, run_like(g, r))


def gen_sin(f=440, sr=48000, nsamp=4800):
    return np.sin(2. * np.pi * float(f) / sr * np.arange(nsamp))


def test_reference_unit_tests():
    """tests/test_periodicity.py::testPeriodicity of the reference, restated."""
    from pypevoc_amd import PeriodTimeSeries
    f0, sr, nsam = 500., 48000, 4800
    pts = PeriodTimeSeries(gen_sin(f=f0, sr=sr, nsamp=nsam), sr=sr, method='xcorr')
    p0 = pts.per_at_index(nsam / 2).get_preferred_period()
    assert abs(sr / p0 - f0) <= 1.0
    x = gen_sin()
    p0 = PeriodTimeSeries(x, method='xcorr').per_at_index(len(x) / 2).get_preferred_period()
    assert isinstance(p0, float)


@pytest.mark.parametrize("method", ["xcorr", "amdf"])
def test_device_tensor_is_bit_identical(method):
    import torch
    from pypevoc_amd import PeriodSeries
    g, runs = load_period_golden("P1_harm_vibrato")
    host = PeriodSeries(g["x"], sr=44100, method=method)
    host.calc()
    dev = PeriodSeries(torch.from_numpy(g["x"]).cuda(), sr=44100, method=method)
    dev.calc()
    a, b = frames(host, 8), frames(dev, 8)
    for u, v in zip(a, b):
        assert np.array_equal(u, v, equal_nan=True)


@pytest.mark.parametrize("method,cand", [("xcorr", "fft"), ("amdf", "similar")])
def test_calc_equals_per_at_index(method, cand):
    from pypevoc_amd import PeriodSeries
    g, _ = load_period_golden("P2_silence_noise")
    ps = PeriodSeries(g["x"], sr=44100, method=method, cand_method=cand, fmin=100)
    ps.calc()
    a = frames(ps, 8)
    one = [ps.per_at_index(p.index) for p in ps.periods]
    ps.periods = one
    b = frames(ps, 8)
    for u, v in zip(a, b):
        assert np.array_equal(u, v, equal_nan=True)


def harmonic(sr, dur, seed=0):
    t = np.arange(int(sr * dur)) / float(sr)
    ph = 2 * np.pi * np.cumsum(220.0 * (1.0 + 0.03 * np.sin(2 * np.pi * 0.5 * t))) / sr
    return sum(0.5 / h * np.sin(h * ph) for h in range(1, 7)) + 0.001 * np.random.default_rng(seed).standard_normal(len(t))


@pytest.mark.parametrize("method", ["xcorr", "amdf"])
def test_long_signal_in_one_calc_equals_chunks(method):
    from pypevoc_amd import PeriodSeries
    x = harmonic(44100, 61.0)
    ps = PeriodSeries(x, sr=44100, method=method)
    ps.calc()
    whole = ps._run(np.arange(ps.nwind, ps.nx - ps.nwind, ps.hop))
    idx = np.arange(ps.nwind, ps.nx - ps.nwind, ps.hop)
    parts = [ps._run(c) for c in np.array_split(idx, 7)]
    for k in ("period", "strength", "count", "preferred"):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts]), equal_nan=True), k
    per, st, cnt, pref = frames(ps, 8)
    assert np.array_equal(cnt, whole["count"]) and np.array_equal(per, whole["period"], equal_nan=True)
    assert (cnt > 0).mean() > 0.9


def test_zero_frames():
    from pypevoc_amd import PeriodSeries
    ps = PeriodSeries(np.ones(2 * 2646), sr=44100)
    ps.calc()
    assert ps.periods == [] and len(ps.get_f0()) == 0 and len(ps.get_times()) == 0


@pytest.mark.parametrize("method", ["xcorr", "amdf"])
def test_all_zero_signal_is_unvoiced(method):
    from pypevoc_amd import PeriodSeries
    ps = PeriodSeries(np.zeros(44100), sr=44100, method=method)
    ps.calc()
    assert len(ps.periods) > 0
    assert all(len(p.cand_period) == 0 and p.preferred == [] for p in ps.periods)
    assert np.isnan(ps.get_f0()).all()


def test_unsupported_window_raises():
    from pypevoc_amd import PeriodSeries, PvxError
    ps = PeriodSeries(np.zeros(200000), sr=44100, window=40000)
    with pytest.raises(PvxError):
        ps.calc()


def test_large_window_runs_from_global_memory():
    """nwind 16384 (fmin 20 Hz at 96 kHz is 14400 samples): beyond the LDS-resident frame."""
    from pypevoc_amd import PeriodSeries
    sr = 96000
    t = np.arange(sr) / float(sr)
    x = np.sin(2 * np.pi * 110 * t) + 0.5 * np.sin(2 * np.pi * 220 * t)
    ps = PeriodSeries(x, sr=sr, window=16384, fmin=20, method="xcorr")
    ps.calc()
    f0 = ps.get_f0()
    assert len(f0) > 0 and abs(np.nanmedian(f0) - 110.0) < 1.0


def test_per_at_index_out_of_range():
    from pypevoc_amd import PeriodSeries
    ps = PeriodSeries(gen_sin(), method="xcorr")
    with pytest.raises(ValueError):
        ps.per_at_index(10)


def test_threads_on_one_device_give_the_sequential_results():
    """Calls share one per-device workspace (rocFFT plan, execution info, buffers) and take turns on it: two threads with
    equal frame counts get exactly what they get one after the other."""
    import threading
    from pypevoc_amd import PeriodSeries
    sigs = [harmonic(44100, 3.0, seed=s) for s in range(4)]

    def run(x):
        ps = PeriodSeries(x, sr=44100, method="xcorr", cand_method="fft")
        return ps._run(np.arange(ps.nwind, ps.nx - ps.nwind, ps.hop))

    want = [run(x) for x in sigs]
    got = [None] * len(sigs)

    def work(i):
        for _ in range(3):
            got[i] = run(sigs[i])

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(sigs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for w, g in zip(want, got):
        for k in ("period", "strength", "count", "preferred"):
            assert np.array_equal(w[k], g[k], equal_nan=True), k


@pytest.mark.parametrize("nsec", [0.3, 1.7, 4.1])
def test_short_fft_calls_after_long_ones(nsec):
    """The 'fft' plan has a fixed batch per window length; a call with fewer frames transforms the rest of the batch too
    (rows an earlier, longer call left behind) and must not read them."""
    from pypevoc_amd import PeriodSeries
    PeriodSeries(harmonic(44100, 20.0, seed=9), sr=44100).calc()
    x = harmonic(44100, nsec, seed=5)
    ps = PeriodSeries(x, sr=44100)
    ps.calc()
    one = [ps.per_at_index(p.index) for p in ps.periods]
    a = frames(ps, 8)
    ps.periods = one
    for u, v in zip(a, frames(ps, 8)):
        assert np.array_equal(u, v, equal_nan=True)
