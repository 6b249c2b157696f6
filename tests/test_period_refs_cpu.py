"""Pins tests/period_refs.py, the plain float64 frame reference that test_periodicity_diff_gpu.py holds k_period.hip to,
without a GPU:

* it reproduces every run of every recorded P*.npz fixture (count, preferred and NaN pattern identical, periods and
  strengths within 1e-11 relative: a hundredth of the 1e-9 the kernel is allowed, so the reference's own distance from
  the library cannot use up the kernel's budget);
* on every frame the GPU test compares, every discrete decision of the reference is at least 1e-6 from flipping (a
  thousand times the kernel's bound), so those frames have one right answer and the GPU test needs no exceptions;
* the cases built to reach a path do reach it.
PERIODICITY.md holds the measured distances."""
import numpy as np
import pytest

from . import test_periodicity_diff_gpu as diff
from .period_refs import EXACT_TIE, EXTENDED, FrameSimilarity, _total, _wide, failing_margins, period_frame_ref
from .test_periodicity_cpu import ctor_kwargs, load_period_golden, period_golden_names

REF_RTOL = 1e-11
MARGIN_FLOOR = 1e-6
MIN_SHARE = 0.25                                                     # of a run's frames, where a stride is used
P3A_TIE = ("P3a_sin500", "sin500_xcorr", 0)                          # the one documented tie (PERIODICITY.md)

_sims = {}


def fixture_runs():
    out = []
    for name in period_golden_names():
        out += [(name, r["name"]) for r in load_period_golden(name)[1]]
    return out


def checked_frames(cnt):
    """Every frame of a short run; of a long one every third, with the first, the last and every unvoiced frame."""
    F = len(cnt)
    keep = np.zeros(F, bool)
    keep[::3 if F > 40 else 1] = True
    keep[[0, F - 1]] = True
    keep |= cnt == 0
    return np.flatnonzero(keep)


def test_summation_is_extended_or_exact():
    """np.longdouble with a 64-bit mantissa, or math.fsum: either way a lag's sum is rounded to float64 once."""
    assert EXTENDED == bool(np.finfo(np.longdouble).eps < 1e-18)
    x = np.r_[1.0, np.full(4096, 2.0 ** -60)]                        # a float64 running sum loses every small term
    assert float(_total(_wide(x))) == 1.0 + 2.0 ** -48


@pytest.mark.parametrize("name,run", fixture_runs())
def test_reference_reproduces_fixture(name, run):
    from pypevoc_amd import PeriodSeries
    g, runs = load_period_golden(name)
    r = [q for q in runs if q["name"] == run][0]
    ps = PeriodSeries(g["x"], **ctor_kwargs(g, r))                   # only for what it derives from the keywords
    thr = r.get("calc", r.get("pbp", {})).get("threshold")
    thr = ps.threshold if thr is None else thr
    wind = np.asarray(ps.wind, dtype=np.float64)
    cnt, gpref = g[run + "_count"], g[run + "_preferred"]
    gper, gst, index = g[run + "_period"], g[run + "_strength"], g[run + "_index"]
    frames = checked_frames(cnt)
    assert len(frames) >= MIN_SHARE * len(cnt) and frames[0] == 0 and frames[-1] == len(cnt) - 1
    assert np.isin(np.flatnonzero(cnt == 0), frames).all()
    worst = 0.0
    for i in frames:
        key = (name, wind.tobytes(), ps.method, int(np.round(index[i])))
        if key not in _sims:
            _sims[key] = FrameSimilarity(ps.x, index[i], wind, ps.method)
        per, st, c, pref, marg = period_frame_ref(ps.x, index[i], wind, ps.method, ps.cand_method, ps.mindelay, ps.maxdelay, thr,
                                                  ps.vthresh, ps.ncand, ps.fftthresh, sim=_sims[key])
        if "f" in r.get("pbp", {}) and c > 0:                        # the walk along an f0 track prefers the candidate nearest to it
            f = np.interp(index[i] / ps.sr, g[r["pbp"]["tf"]], g[r["pbp"]["f"]])
            pref = int(np.argmin(np.abs(ps.sr / f - per))) if f > 0 else pref
        assert c == cnt[i], (name, run, i)
        assert np.isnan(gper[i, c:]).all() and np.isnan(gst[i, c:]).all(), (name, run, i)
        if c > 0 and not np.allclose(np.sort(per), np.sort(gper[i, :c]), rtol=1e-9, atol=0):
            # as check_against of test_periodicity_gpu.py: the ncand-th and (ncand+1)-th peaks tie to 4 ulp, the last bit of a
            # sum decides which survives; the other candidates and the preferred period must agree
            assert (name, run, i) == P3A_TIE, (name, run, i, per, gper[i])
            assert 0 <= marg["ncand_cap"][0] <= 4 * np.spacing(1.0), marg
            both = [p for p in per if np.isclose(gper[i, :c], p, rtol=1e-9, atol=0).any()]
            assert len(both) == c - 1
            assert abs(per[pref] - gper[i, gpref[i]]) <= 1e-9 * gper[i, gpref[i]]
            continue
        assert pref == gpref[i], (name, run, i)
        if c > 0:
            e = max(np.max(np.abs(per - gper[i, :c]) / np.abs(gper[i, :c])), np.max(np.abs(st - gst[i, :c]) / np.abs(gst[i, :c])))
            worst = max(worst, float(e))
    print("\n%s %s: %d of %d frames, worst relative distance from the recorded library %.2e" % (name, run, len(frames), len(cnt), worst))
    assert worst <= REF_RTOL, (name, run, worst)
    if (name, run) == P3A_TIE[:2]:                                   # the tie is real: 4 ulp at most between the last kept and the first dropped
        assert 0 <= marg["ncand_cap"][0] <= 4 * np.spacing(1.0), marg


@pytest.mark.parametrize("name", list(diff.CASES))
def test_gpu_case_is_decided(name):
    """No frame of any GPU case is left out: each has every decision at least MARGIN_FLOOR from flipping."""
    cen, fr, per, st, cnt, pref, margins = diff.reference(name)
    assert len(fr) == len(margins) > 0
    if diff.CASES[name].frames is None:
        assert np.array_equal(fr, np.arange(len(cen)))
    near = {int(f): failing_margins(m, MARGIN_FLOOR) for f, m in zip(fr, margins) if failing_margins(m, MARGIN_FLOOR)}
    lowest = min([v[0] for m in margins for v in m.values() if isinstance(v, tuple) and v[1] is None], default=np.inf)
    print("\n%s: %d frames, %d candidates, lowest margin %.1e" % (name, len(fr), int(cnt.sum()), lowest))
    assert not near, (name, near)
    assert ((cnt == 0) == (pref == -1)).all()


def outcomes(name):
    return [m.get("firstneg_outcome") for m in diff.reference(name)[6]]


def ties(name, key="ncand_cap"):
    return [int(m.get(key, (None, None))[1] == EXACT_TIE) for m in diff.reference(name)[6]]


def test_gpu_cases_reach_their_paths():
    C = diff.CASES
    count = lambda name: diff.reference(name)[4]                     # noqa: E731
    params = lambda name: diff.frame_params(C[name])                 # noqa: E731
    # e: all three outcomes of the first-negative search, in LDS, with lags left to compute past the first pass
    p = params("e_firstneg_search")
    assert len(p["wind"]) <= 6144 and p["args"][3] < len(p["wind"]) - 1
    assert set(outcomes("e_firstneg_search")) == {"early", "past_maxdelay", "nowhere"}
    seen = set(zip(outcomes("e_firstneg_search"), (count("e_firstneg_search") > 0).tolist()))
    assert {("early", True), ("nowhere", True), ("past_maxdelay", False)} <= seen and ("past_maxdelay", True) not in seen
    for m in ("xcorr", "amdf"):
        # the caps: ncand 1, and th < 0 where the zeros of the non-maxima fill the list, at 8 and at the largest ncand
        assert (count("a_ncand1_" + m) == 1).all()
        for c in ("fft", "min", "similar"):
            assert (count("a_thneg_%s_%s" % (m, c)) == 8).all() and min(ties("a_thneg_%s_%s" % (m, c))) >= 1
            assert (count("a_thr0_%s_%s" % (m, c)) > 0).all() and max(ties("a_thr0_%s_%s" % (m, c))) == 0
        assert (count("a_thneg_ncand64_" + m) == 64).all() and min(ties("a_thneg_ncand64_" + m)) >= 1
        assert params("a_thneg_ncand64_" + m)["args"][6] == 64       # PVX_PERIOD_MAX_NCAND (include/pvx.h)
        assert (count("a_mindelay_above_maxdelay_" + m) == 0).all()
        p = params("a_mindelay_above_maxdelay_" + m)
        assert p["args"][2] > p["args"][3]
        assert params("a_fmax_none_" + m)["args"][2] == 2
        # odd windows; lag counts that are no multiple of four and reach the window's last lags
        assert len(params("a_odd481_" + m)["wind"]) == 481 and (count("a_odd481_" + m) > 0).all()
        p = params("a_w479_" + m)
        assert len(p["wind"]) == 479 and p["args"][3] % 4 != 0 and p["args"][3] >= 479 - 2
        # b: more frames than a chunk of the 'fft' plan and than the grid; the compared frames sit on both edges
        cen, fr = diff.reference("b_fft_chunks_" + m)[:2]
        assert diff.fft_chunk(1024) == 8192 < len(cen) and {0, 1023, 1024, 8191, 8192, len(cen) - 1} == set(fr.tolist())
        assert (count("b_fft_chunks_" + m) > 1).all()
        # d: either side of the LDS limit
        assert len(params("d_route_6144_" + m)["wind"]) == 6144 and len(params("d_route_6145_" + m)["wind"]) == 6145
        assert (count("d_route_6144_" + m) > 1).all() and (count("d_route_6145_" + m) > 1).all()
        assert 9 <= len(count("d_route_6145_" + m)) <= 12
        for k in ("f_float32_", "f_int16_"):
            assert diff.signal(C[k + m].sig).dtype != np.float64 and (count(k + m) > 0).all()
        x = diff.signal("p9")
        assert abs(diff.signal("p9_dc").mean()) > 9 * np.abs(x).max()
    for c in ("min", "similar"):                                     # plateaus: the >= of the peak mask holds with equality
        assert min(ties("a_plateau_xcorr_" + c, "plateau")) == 1 and (count("a_plateau_xcorr_" + c) >= 4).all()
    for name in ("c_global_xcorr_fft", "c_global_amdf_min"):
        cen, fr, _, _, cnt = diff.reference(name)[:5]
        assert len(params(name)["wind"]) == 8192 and 780 <= params(name)["args"][3] <= 820
        assert diff.fft_chunk(8192) == 1024 < len(cen) and {0, 511, 512, 1023, 1024, len(cen) - 1} == set(fr.tolist())
        assert (cnt > 1).all()


def test_p9_fixture_holds_its_cases():
    g, runs = load_period_golden("P9_thresholds_odd")
    names = {r["name"] for r in runs}
    assert g["x"].dtype == np.float64 and len(g["x"]) == 4000 and float(g["sr"]) == 8000
    for m in ("xcorr", "amdf"):
        assert {"ncand1_" + m, "ncand64_" + m, "odd481_" + m, "w479_" + m} <= names
        for c in ("fft", "min", "similar"):
            assert {"thr0_%s_%s" % (m, c), "thneg_%s_%s" % (m, c)} <= names
            assert (g["thneg_%s_%s_count" % (m, c)] == 8).all()
        assert (g["ncand1_%s_count" % m] == 1).all() and g["ncand64_%s_period" % m].shape[1] == 64
        assert len(g["win_odd481_" + m]) == 481
