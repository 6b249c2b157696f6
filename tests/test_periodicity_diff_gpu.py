"""k_period.hip against tests/period_refs.py, the plain float64 restatement of one frame, at the shapes no fixture holds:
the PeakFinder threshold cases and odd windows (a), more than one 'fft' chunk on the LDS route (b), the global-memory
route with more frames than workgroups and than a chunk (c), the route boundary nwind 6144 / 6145 (d), the search for the
first negative lag past the computed lags on the LDS route (e) and float32 / int16 host signals (f).

count and preferred identical, the NaN pattern identical, periods and strengths within RTOL = 1e-9 relative, without
exceptions: test_period_refs_cpu.py runs the reference alone over every frame compared here and requires every discrete
decision of it to be at least 1e-6 from flipping, a thousand times the kernel's bound (exact index ties apart, which
the kernel must order as the reference does).  The cases and their references are defined here and built once.
Worst errors per case are printed (-s); PERIODICITY.md holds the measured table."""
import collections
import functools

import numpy as np
import pytest

from .period_refs import FrameSimilarity, period_frame_ref
from .test_periodicity_cpu import ctor_kwargs, load_period_golden
from .test_periodicity_gpu import RTOL

pytestmark = pytest.mark.gpu

# sig: the key of signal(); kw: PeriodSeries keywords (window, hop included); frames: None for every frame of calc(), else
# the frame numbers compared with the reference (negative: from the end); split: where the frames are cut for the two
# separate launches that the one launch must equal bit for bit
Case = collections.namedtuple("Case", "sig kw frames split")


def harmonic(sr, n, f0, seed, noise=0.05):
    """Six harmonics of a 3 Hz vibrato around f0, white noise at `noise` of the fundamental; float32-exact."""
    t = np.arange(n) / float(sr)
    ph = 2 * np.pi * np.cumsum(f0 * (1.0 + 0.03 * np.sin(2 * np.pi * 3.0 * t))) / sr
    x = sum(0.5 / h * np.sin(h * ph) for h in range(1, 7)) + noise * 0.5 * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def signal(key):
    if key.startswith("p9"):
        x = load_period_golden("P9_thresholds_odd")[0]["x"]
        if key == "p9_dc":                                           # a DC offset of ten times the amplitude
            return x + 10.0 * np.abs(x).max()
        if key == "p9_float32":
            return x.astype(np.float32)
        if key == "p9_int16":
            return np.round(x * 8000.0).astype(np.int16)
        return x
    if key == "impulses":                                            # +1 every 80 samples, -1 thirty samples later: most lags sum zeros
        x = np.zeros(2000)
        x[0::80], x[30::80] = 1.0, -1.0
        return x
    if key == "chunks":                                              # b: 8276 frames at nwind 1024, hop 2
        return harmonic(16000, 18600, 220.0, seed=21)
    if key == "global":                                              # c: 1030 frames at nwind 8192, hop 4
        return harmonic(48000, 2 * 8192 + 4 * 1030, 150.0, seed=22)
    if key == "route":                                               # d: 11 frames at nwind 6144, hop 37
        return harmonic(48000, 2 * 6145 + 370, 300.0, seed=23)
    if key == "swell":                                               # e: P8a's recipe at a quarter of its rate and window
        t = np.arange(12000) / 24000.0
        x = np.sin(2 * np.pi * 3 * t) + 0.15 * sum(np.sin(2 * np.pi * h * 150 * t) / h for h in range(1, 4))
        return x.astype(np.float32).astype(np.float64)
    raise KeyError(key)


def build_cases():
    cases = collections.OrderedDict()
    g, runs = load_period_golden("P9_thresholds_odd")
    for r in runs:                                                   # a: P9's parameter sets again, every frame
        cases["a_" + r["name"]] = Case("p9", ctor_kwargs(g, r), None, None)
    base = {"sr": 8000, "fmax": 1000}
    for m in ("xcorr", "amdf"):
        for c in ("min", "similar"):
            cases["a_odd481_%s_%s" % (m, c)] = Case("p9", dict(base, threshold=0.3, method=m, cand_method=c, window=np.hanning(481)), None, None)
            cases["a_w479_%s_%s" % (m, c)] = Case("p9", dict(base, fmin=16.72, method=m, cand_method=c, window=479), None, None)
        cases["a_thneg_ncand64_" + m] = Case("p9", dict(base, method=m, threshold=-1.0, ncand=64), None, None)
        cases["a_mindelay_above_maxdelay_" + m] = Case("p9", dict(base, method=m, fmax=40), None, None)
        cases["a_fmax_none_" + m] = Case("p9", dict(base, method=m, fmax=None), None, None)
        cases["a_dc_offset_" + m] = Case("p9_dc", dict(base, method=m), None, None)
        # b: a chunk of the 'fft' plan is 8192 frames at nwind 1024, the grid 1024 workgroups
        cases["b_fft_chunks_" + m] = Case("chunks", dict(sr=16000, fmax=1000, window=1024, hop=2, method=m, cand_method="fft"),
                                          (0, 1023, 1024, 8191, 8192, -1), 5000)
        # d: the last window in LDS and the first in global memory, the same Hann shape at either length (on a pedestal: under
        # a window that ends in zeros amdf's normaliser, taken at the largest lags, leaves every frame unvoiced)
        for n in (6144, 6145):
            cases["d_route_%d_%s" % (n, m)] = Case("route", dict(sr=48000, fmin=100, fmax=1000, threshold=0.5, window=0.5 + 0.5 * np.hanning(n),
                                                                 hop=37, method=m), None, None)
        # f: host signals of other types are widened by np.asarray(x).astype(float)
        cases["f_float32_" + m] = Case("p9_float32", dict(base, method=m), None, None)
        cases["f_int16_" + m] = Case("p9_int16", dict(base, method=m), None, None)
    # a: maxima that begin a plateau, y[k-1] < y[k] == y[k+1].  Every window of 480 holds six impulses of either sign, so its
    # mean is 0 and the correlation exactly 0 off the impulses' distances: the lag after each negative one is such a maximum
    for c in ("min", "similar"):
        cases["a_plateau_xcorr_" + c] = Case("impulses", dict(base, threshold=0, hop=37, method="xcorr", cand_method=c), None, None)
    # c: beyond the LDS a chunk is 1024 frames at nwind 8192 and the grid 512 workgroups; maxdelay 800
    glob = dict(sr=48000, fmin=60, fmax=1000, window=8192, hop=4)
    cases["c_global_xcorr_fft"] = Case("global", dict(glob, method="xcorr", cand_method="fft"), (0, 511, 512, 1023, 1024, -1), 700)
    cases["c_global_amdf_min"] = Case("global", dict(glob, method="amdf", cand_method="min"), (0, 511, 512, 1023, 1024, -1), 700)
    # e: a slow swell under a tone through a window whose first half is zero (fixture P8a at nwind 8192): frames whose first
    # negative lag is early, past maxdelay (unvoiced) or nowhere (the kernel goes on past the lags it computed, to nwind - 1)
    cases["e_firstneg_search"] = Case("swell", dict(sr=24000, fmin=100, fmax=1000, window=np.r_[np.zeros(1024), np.ones(1024)], hop=256), None, None)
    return cases


CASES = build_cases()


def series(case):
    from pypevoc_amd import PeriodSeries
    return PeriodSeries(signal(case.sig), **case.kw)


def frame_params(case):
    """What PeriodSeries derives from its keywords, restated: the widened signal, the window, the delays, the centres."""
    kw = case.kw
    x = np.asarray(signal(case.sig)).astype(np.float64)
    sr = kw.get("sr", 48000)
    fmax = kw.get("fmax", 5000)
    maxdelay = int(sr / kw.get("fmin", 50))
    window = kw.get("window", 3 * maxdelay)
    wind = np.asarray(window, dtype=np.float64) if np.iterable(window) else np.ones(window)
    hop = kw.get("hop", len(wind) // 2)
    return {"x": x, "wind": wind, "centres": np.arange(len(wind), len(x) - len(wind), hop).astype(np.int64),
            "args": (kw.get("method", "xcorr"), kw.get("cand_method", "fft"), 2 if fmax is None else int(sr / fmax), maxdelay,
                     kw.get("threshold", .8), kw.get("vthresh", .2), kw.get("ncand", 8), kw.get("fftthresh", 0.1))}


def fft_chunk(nwind):
    return (64 << 20) // (8 * nwind)


def compared_frames(case, nframes):
    return np.arange(nframes) if case.frames is None else np.array([f % nframes for f in case.frames])


_sims = {}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference on every compared frame of a case: (centres of all frames, compared frame numbers, period and strength
    [compared, ncand] padded with NaN, count, preferred, one margins dict per frame).  Built once per process; the
    similarity sums are shared between the cases that differ only in what they do with them."""
    case = CASES[name]
    fp = frame_params(case)
    x, wind, cen, args = fp["x"], fp["wind"], fp["centres"], fp["args"]
    fr = compared_frames(case, len(cen))
    ncand = args[6]
    per = np.full((len(fr), ncand), np.nan)
    st = np.full((len(fr), ncand), np.nan)
    cnt = np.zeros(len(fr), np.int32)
    pref = np.zeros(len(fr), np.int32)
    margins = []
    for i, f in enumerate(fr):
        key = (case.sig, wind.tobytes(), args[0], int(cen[f]))
        if key not in _sims:
            _sims[key] = FrameSimilarity(x, cen[f], wind, args[0])
        p, s, cnt[i], pref[i], m = period_frame_ref(x, cen[f], wind, *args, sim=_sims[key])
        per[i, :cnt[i]] = p
        st[i, :cnt[i]] = s
        margins.append(m)
    return cen, fr, per, st, cnt, pref, margins


def rel_err(a, b):
    """Worst relative error of a against b; the NaN pattern must be the same."""
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(b)
    return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m]))) if m.any() else 0.0


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_reference(name):
    case = CASES[name]
    ps = series(case)
    cen, fr, per, st, cnt, pref, _ = reference(name)
    got = ps._run(cen)
    assert np.array_equal(got["count"][fr], cnt), (name, got["count"][fr], cnt)
    assert np.array_equal(got["preferred"][fr], pref), (name, got["preferred"][fr], pref)
    eper, est = rel_err(got["period"][fr], per), rel_err(got["strength"][fr], st)
    print("\n%s: %d of %d frames, %d candidates, worst relative error: period %.2e strength %.2e"
          % (name, len(fr), len(cen), int(cnt.sum()), eper, est))
    assert eper <= RTOL and est <= RTOL, (name, eper, est)
    if case.split is not None:                                       # one launch of several chunks == two launches of one chunk each
        chunk = fft_chunk(ps.nwind)
        assert len(cen) > chunk and case.split != chunk and max(case.split, len(cen) - case.split) <= chunk
        parts = [ps._run(cen[:case.split]), ps._run(cen[case.split:])]
        for k in ("period", "strength", "count", "preferred"):
            assert np.array_equal(got[k], np.concatenate([p[k] for p in parts]), equal_nan=True), (name, k)
