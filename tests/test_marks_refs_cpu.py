"""tests/marks_refs.py against the recorded reference (tests/golden/K*.npz), without a GPU: the restatement reproduces the
goldens, a plain float64 evaluation lies inside the stated bounds, wrong readings of the text fall outside, and every
decision the GPU tests compare is far from flipping -- on the reference alone (a condition on the inputs)."""
import json

import numpy as np
import pytest

from . import marks_refs as R


def test_golden_cases_are_the_fixtures():
    assert json.loads(str(R.golden("K1_marks_corr")["cases"])) == json.loads(json.dumps(R.CORR_FIXTURES))
    assert json.loads(str(R.golden("K2_marks_peak")["cases"])) == json.loads(json.dumps(R.PEAK_FIXTURES))
    for key in R.SIGNALS:
        x = R.golden("K1_marks_corr")["sig_" + key]
        assert x.dtype == np.float32 and len(x) <= 16000


@pytest.mark.parametrize("name", sorted(R.CORR))
def test_corr_restatement_reproduces_the_reference(name):
    want = R.golden("K1_marks_corr")[name + "_marks"]
    for exact in (True, False):
        r = R.corr_ref(name, exact)
        assert r.status == 0
        assert len(r.marks) == len(want)
        assert np.all(np.abs(r.marks - want) <= R.corr_ref(name).bounds), (name, exact)
    assert np.all(np.isfinite(R.corr_ref(name).bounds)) and R.corr_ref(name).bounds.max() < 1e-11


@pytest.mark.parametrize("name", sorted(R.CORR))
def test_corr_decisions_are_far_from_flipping(name):
    r = R.corr_ref(name)
    sr = R.CORR[name]["sr"]
    for m in r.margins:
        assert m.tagged or m.value >= R.MARGIN_FLOOR, m
    for s in r.steps:            # int(next_t sr): the floor is an absolute distance too (next_t sr >= 1), 16 bounds wide
        assert R.KERNEL_FACTOR * sr * s["b_next"] < R.MARGIN_FLOOR, s


def test_corr_fixtures_take_the_paths_they_are_meant_to():
    picks = lambda n: [s["pick"] for s in R.corr_ref(n).steps]
    assert min(abs(k) for k in picks("ring2")) > 128                 # beyond the first ring of lags
    assert min(abs(k) for k in picks("off35")) >= 10
    assert all(s["P"] == 20 for s in R.corr_ref("small_P").steps) and R.CORR["small_P"]["W"] >= 10 * 20
    assert all(s["P"] > R.CORR["P_above_W"]["W"] for s in R.corr_ref("P_above_W").steps)
    c = R.CORR["min_per"]
    assert 0 < sum(1 for s in R.corr_ref("min_per").steps if not s["delay_t"] > c["min_per"]) < len(R.corr_ref("min_per").steps)
    g = R.corr_ref("nan_gap")
    assert len(g.marks) - 1 == len(g.steps) and np.diff(g.marks).max() > 0.05      # the gap is walked without marks


def _outside(good, bad):
    n = min(len(good.marks), len(bad.marks))
    return len(good.marks) != len(bad.marks) or bool(np.any(np.abs(good.marks[:n] - bad.marks[:n]) > good.bounds[:n]))


def test_mark_placed_after_next_t_moves_falls_outside_the_bounds():
    for name in ("w256", "off35", "t0"):
        assert _outside(R.corr_ref(name), R.corr_ref(name, False, "mark_after")), name


def test_nearest_peak_by_value_falls_outside_the_bounds():
    # two equal harmonics under a track 1.5 times too high: P = 2/3 T, the half-period peak at lag +T/6 is the nearest one
    # and the full-period peak at lag -T/3 the highest
    n = np.arange(1500)
    x = (np.sin(2 * np.pi * n / 53.3) + np.sin(4 * np.pi * n / 53.3)).astype(np.float32).astype(np.float64)
    args = (x, 8000, 0.0, [0.0, 0.2], [225.0, 225.5], 256)
    good, plain, bad = R.corr_walk(*args), R.corr_walk(*args, exact=False), R.corr_walk(*args, exact=False, variant="by_value")
    assert good.status == 0 and len(good.marks) > 5
    assert not _outside(good, plain)
    assert _outside(good, bad)


@pytest.mark.parametrize("name", sorted(R.PEAK))
def test_peak_restatement_reproduces_the_reference(name):
    g = R.golden("K2_marks_peak")
    plain, exact = R.peak_ref(name, False), R.peak_ref(name, True)
    x = R.signal(R.PEAK[name]["sig"])
    keep = plain.idx < len(x) - 2                                    # fewer than 3 fit points: the stated deviation
    assert len(plain.marks) == len(g[name + "_marks"])
    assert np.array_equal(plain.marks[keep], g[name + "_marks"][keep])
    assert np.array_equal(plain.vals[keep], g[name + "_vals"][keep])
    assert plain.status & ~R.SHORT_FIT == 0
    # the long-double walk takes the same indices and the same accept / reject decisions
    assert np.array_equal(plain.idx, exact.idx) and np.array_equal(plain.fitted, exact.fitted)
    for m in plain.margins + exact.margins:
        assert m.value >= R.MARGIN_FLOOR, m
    # what the 16-fold allowance of the GPU tests is taken from: measured here, never more than the recorded figures
    drel = np.abs(plain.rel - exact.rel).max()
    dval = np.abs(plain.vals - exact.vals).max() / np.abs(x).max()
    print("%s: |rel(polyfit) - rel(long double)| <= %.2e samples, values %.2e of max |x|" % (name, drel, dval))
    assert drel <= R.PEAK_REL_MEASURED and dval <= R.PEAK_VAL_MEASURED


def test_peak_fixtures_take_the_paths_they_are_meant_to():
    x = R.signal("flat")
    r = R.peak_ref("flat_top")
    assert sum(1 for i in r.idx if x[i] == x[i + 1]) >= 5            # ties: the first of equal maxima is taken
    last = R.peak_walk(R.signal("rising"), 8000, None, 151.0, 5, max_marks=None)
    full = R.golden("K2_marks_peak")["last_sample_marks"]
    assert len(last.marks) == len(full)
    assert int(np.argmax(R.signal("rising"))) == len(R.signal("rising")) - 1
    assert not R.peak_ref("track5").fitted.all() and R.peak_ref("track5").fitted.any()
    assert R.peak_ref("nan_head").idx[0] > 0.06 * 8000 - 60


def test_status_cases_of_the_restatement():
    x = R.signal("v8k")
    tf, f = [0.0, 0.3], [149.0, 153.0]
    assert R.corr_walk(np.zeros(2400), 8000, 0.0, tf, f, 256).status == R.NO_PEAK
    assert R.corr_walk(x, 8000, 0.0, [0.0, 0.255, 0.2551, 0.3], [400.0, 400.0, 60.0, 60.0], 256).status == R.PAST_END
    assert R.corr_walk(x, 8000, 0.0, [0.0, 0.1, 0.1001, 0.3], [149.0, 150.0, -5.0, -5.0], 256).status == R.BAD_F0
    assert R.corr_walk(x, 8000, -0.1, tf, f, 256).status == R.BAD_F0
    assert R.corr_walk(x, 8000, 0.0, tf, f, 256, max_marks=5).status == R.CAPACITY
    assert R.corr_walk(x, 8000, 0.0, tf, f, 256, max_steps=5).status == R.STEPS


def _far(ref):
    return all(m.tagged or m.value >= R.MARGIN_FLOOR for m in ref.margins)


@pytest.mark.parametrize("kind", R.STATUS_KINDS)
def test_status_calls_end_as_stated(kind):
    c = R.status_call(kind)
    refs = R.rows_ref(c)
    assert [refs[i].status for i in refs] == c["expect"]
    assert _far(refs[0]) and _far(refs[2]) and len(refs[0].marks) >= 4 and len(refs[2].marks) >= 3
    if kind in ("past_end", "capacity", "steps"):                    # the row walks a while before it ends
        assert _far(refs[1]) and len(refs[1].marks) >= 5


def test_adhoc_calls_are_far_from_flipping():
    c = R.lds_limit_call(False)
    r = R.rows_ref(c)[0]
    assert r.status == 0 and len(r.marks) >= 3 and _far(r) and np.isfinite(r.bounds).all()
    c = R.many_rows_call()
    for r in R.rows_ref(c, [0, 1, 6, 500, len(c["starts"]) - 1]).values():
        assert r.status == 0 and len(r.marks) >= 4 and _far(r)
    x = R.signal("v8k_long")
    for r in (0, 1, 10, 777, 4199):                                      # test_peak_rows_beyond_the_grid_split_and_shuffled
        s = (7 * r) % 3000
        for exact in (False, True):
            ref = R.peak_walk(x[s:s + 300 + 10 * (r % 5)], 8000, [0.0, 0.5], [149.0, 153.0], 3, exact=exact, toff=s / 8000.0)
            assert ref.status == (R.SHORT_FIT if r == 10 else 0) and len(ref.marks) >= 3 and all(m.value >= R.MARGIN_FLOOR for m in ref.margins)
