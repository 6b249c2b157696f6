"""pypevoc_amd.marks (k_marks.hip) against the recorded reference (tests/golden/K*.npz) and the long-double restatement of
tests/marks_refs.py: the same number of marks, the same status, and every mark time within the bound MARKS.md derives.
test_marks_refs_cpu.py checks, without a GPU, that every decision of these walks is far from flipping on the reference alone."""
import functools

import numpy as np
import pytest

from . import marks_refs as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def run_corr(name):
    from pypevoc_amd.marks import period_marks_corr
    c = R.CORR[name]
    return period_marks_corr(R.signal(c["sig"]), sr=c["sr"], t0=c["t0"], tf=c["tf"], f=c["f"], window_size=c["W"], min_per=c["min_per"])


@functools.lru_cache(maxsize=None)
def run_peak(name):
    from pypevoc_amd.marks import period_marks_peak
    c = R.PEAK[name]
    x = R.signal(c["sig"])
    return period_marks_peak(x, sr=c["sr"], tf=c["tf"], f=R.peak_f(c, len(x)), fit_points=c["fit_points"])


def run_rows(c, rows=None, device=False):
    from pypevoc_amd.marks import period_marks_rows
    rows = list(range(len(c["starts"]))) if rows is None else list(rows)
    pick = lambda key: [c[key][r] for r in rows]
    x = c["x"]
    if device:
        import torch
        x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return period_marks_rows(x, pick("starts"), pick("stops"), sr=c.get("sr", 8000), tf=c["tf"], f=c["f"], method="corr", t0=pick("t0"),
                             toff=pick("toff"), window_size=c["W"], min_per=c["min_per"], max_marks=c["max_marks"], max_steps=c["max_steps"])


def row_marks(res, i):
    return res["marks"][i, :res["count"][i]]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_inside(got, ref, what):
    assert len(got) == len(ref.marks), (what, len(got), len(ref.marks))
    err = np.abs(got - ref.marks)
    print("%s: %d marks, worst error %.2e of a bound of %.2e" % (what, len(got), err.max(), ref.bounds[np.argmax(err)]))
    assert np.all(err <= ref.bounds), (what, err.max())


@pytest.mark.parametrize("name", [c["name"] for c in R.CORR_FIXTURES])
def test_corr_fixture(name):
    from pypevoc_amd.marks import marks_last_kernels
    got = run_corr(name)
    assert marks_last_kernels() == "k_marks_corr"
    assert got.dtype == np.float64 and got[0] == R.CORR[name]["t0"]
    ref = R.corr_ref(name)
    assert_inside(got, ref, name)
    want = R.golden("K1_marks_corr")[name + "_marks"]                # the reference's own float64 run lies inside the bounds too
    assert np.all(np.abs(got - want) <= 2 * ref.bounds)


def test_corr_stub_stays_and_points_here():
    import pypevoc_amd
    from pypevoc_amd import Periodicity
    for fn in (Periodicity.period_marks_corr, pypevoc_amd.period_marks_corr, Periodicity.period_marks_peak):
        with pytest.raises(NotImplementedError):
            fn(np.zeros(10))


@pytest.mark.parametrize("kind", R.STATUS_KINDS)
def test_row_status_and_the_rows_beside_it(kind):
    c = R.status_call(kind)
    res = run_rows(c)
    refs = R.rows_ref(c)
    assert list(res["status"]) == c["expect"] == [refs[i].status for i in refs]
    for i in refs:
        assert_inside(row_marks(res, i), refs[i], "%s row %d" % (kind, i))
    for i in (0, 2):                                                 # the healthy rows: what they are in a call of their own
        alone = run_rows(c, [i])
        assert alone["status"][0] == 0 and same_bits(row_marks(alone, 0), row_marks(res, i))
    assert np.all(res["marks"][np.arange(res["marks"].shape[1])[None, :] >= res["count"][:, None]] == 0)


def test_drop_in_raises_where_a_row_reports_a_status():
    from pypevoc_amd.marks import period_marks_corr
    with pytest.raises(ValueError, match="no local maximum"):
        period_marks_corr(np.zeros(2400), sr=8000, tf=R.TRACK[0], f=R.TRACK[1], window_size=256)
    with pytest.raises(ValueError, match="t0 < 0"):
        period_marks_corr(R.signal("v8k"), sr=8000, t0=-0.1, tf=R.TRACK[0], f=R.TRACK[1], window_size=256)
    # a signal shorter than P + W: the loop never runs, the reference returns [t0]
    assert np.array_equal(period_marks_corr(R.signal("v8k")[:200], sr=8000, t0=0.01, tf=R.TRACK[0], f=R.TRACK[1], window_size=256), [0.01])


def test_lds_limit_both_sides():
    from pypevoc_amd import _lib
    from pypevoc_amd.marks import CORR_MAX_LDS
    c = R.lds_limit_call(False)
    assert 3 * c["W"] + int(c["sr"] / min(c["f"])) == CORR_MAX_LDS
    res = run_rows(c)
    ref = R.rows_ref(c)[0]
    assert res["status"][0] == ref.status == 0 and len(ref.marks) >= 3
    assert_inside(row_marks(res, 0), ref, "at the limit")
    past = R.lds_limit_call(True)
    assert 3 * past["W"] + int(past["sr"] / min(past["f"])) == CORR_MAX_LDS + 1
    with pytest.raises(_lib.PvxError, match="status -"):
        run_rows(past)
    assert _lib.load().pvx_marks_last_kernels() == b""               # refused before anything launched


def test_sample_types_widen_exactly():
    from pypevoc_amd.marks import period_marks_corr
    c = R.CORR["w256"]
    x32 = R.golden("K1_marks_corr")["sig_" + c["sig"]]
    assert x32.dtype == np.float32
    got = period_marks_corr(x32, sr=c["sr"], t0=c["t0"], tf=c["tf"], f=c["f"], window_size=c["W"], min_per=c["min_per"])
    assert same_bits(got, run_corr("w256"))
    xi = np.round(x32.astype(np.float64) * 20000).astype(np.int16)
    a = period_marks_corr(xi, sr=c["sr"], tf=c["tf"], f=c["f"], window_size=256)
    b = period_marks_corr(xi.astype(np.float64), sr=c["sr"], tf=c["tf"], f=c["f"], window_size=256)
    assert same_bits(a, b) and len(a) > 10


# ---- period_marks_peak ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in R.PEAK_FIXTURES])
def test_peak_fixture(name):
    c = R.PEAK[name]
    marks, vals = run_peak(name)
    g = R.golden("K2_marks_peak")
    ref = R.peak_ref(name, True)
    x = R.signal(c["sig"])
    assert len(marks) == len(vals) == len(g[name + "_marks"]) == len(ref.marks)
    # the indices behind the marks are the reference's: an unfitted mark is idx / sr to the bit, a fitted one idx + rel
    assert np.array_equal(np.rint(marks * c["sr"] - ref.rel).astype(np.int64), ref.idx)
    plain = ~ref.fitted
    assert same_bits(marks[plain], ref.idx[plain] / float(c["sr"])) and same_bits(vals[plain], x[ref.idx[plain]])
    keep = ref.idx < len(x) - 2                                      # fewer than 3 fit points: the stated deviation
    tol_t, tol_v = R.peak_tolerance(c["sr"], np.abs(marks), np.abs(x).max())
    # 16 times the measured float64 error against the long-double walk; the reference's own run is one such error further
    for want_t, want_v, who, k in ((ref.marks, ref.vals, "restatement", 1.0), (g[name + "_marks"], g[name + "_vals"], "reference", 17.0 / 16.0)):
        et, ev = np.abs(marks - want_t)[keep], np.abs(vals - want_v)[keep]
        print("%s against the %s: times %.2e of %.2e, values %.2e of %.2e" % (name, who, et.max(), k * tol_t.min(), ev.max(), k * tol_v))
        assert np.all(et <= k * tol_t[keep]) and np.all(ev <= k * tol_v), (name, who)


def test_peak_arguments():
    from pypevoc_amd.marks import period_marks_peak, period_marks_rows, BAD_F0
    x = R.signal("v8k")
    with pytest.raises(ValueError):
        period_marks_peak(x, sr=8000, f=151.0, fit_points=2)
    with pytest.raises(ValueError):
        period_marks_peak(x, sr=8000, f=np.full(len(x), np.nan))     # no finite f0
    res = period_marks_rows(x, [0, 0], [len(x), len(x)], sr=8000, tf=[0.0, 1.0], f=[151.0, -3.0], method="peak", toff=[0.0, 2.0])
    assert list(res["status"]) == [0, BAD_F0] and res["count"][1] == 0
    assert res["count"][0] > 10 and res["vals"].shape == res["marks"].shape
