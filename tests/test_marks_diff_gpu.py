"""k_marks.hip: what must not change a row's result -- the launch it runs in, the workgroup that takes it, the rows beside it,
the order of the rows, the sample type the signal arrived in, where the signal lives.  All bit for bit."""
import numpy as np
import pytest

from . import marks_refs as R
from .test_marks_gpu import assert_inside, row_marks, run_rows, same_bits

pytestmark = pytest.mark.gpu


def rows_equal(a, ia, b, ib):
    return a["status"][ia] == b["status"][ib] and same_bits(row_marks(a, ia), row_marks(b, ib))


def test_more_rows_than_workgroups_split_and_shuffled():
    c = R.many_rows_call()
    n = len(c["starts"])
    assert n > 1024                                                  # the persistent grid has 1024 workgroups
    assert len(set(b - a for a, b in zip(c["starts"], c["stops"]))) == 7
    one = run_rows(c)
    assert (one["status"] == 0).all() and one["count"].min() >= 4
    order = np.random.default_rng(5).permutation(n)
    a, b = run_rows(c, order[:537]), run_rows(c, order[537:])
    for j, r in enumerate(order[:537]):
        assert rows_equal(a, j, one, r), r
    for j, r in enumerate(order[537:]):
        assert rows_equal(b, j, one, r), r
    sample = [0, 1, 6, 500, n - 1]
    refs = R.rows_ref(c, sample)
    for r in sample:
        assert_inside(row_marks(one, r), refs[r], "row %d" % r)


def test_one_row_and_device_resident_signal():
    c = R.status_call("past_end")
    host = run_rows(c)
    dev = run_rows(c, device=True)
    for i in range(3):
        assert rows_equal(host, i, dev, i)
    assert same_bits(host["marks"], dev["marks"])
    alone = run_rows(c, [2], device=True)
    assert rows_equal(alone, 0, host, 2)


def test_device_signal_in_float32():
    import torch
    from pypevoc_amd.marks import period_marks_corr, period_marks_peak
    c = R.CORR["w256"]
    x32 = R.golden("K1_marks_corr")["sig_" + c["sig"]]
    kw = dict(sr=c["sr"], t0=c["t0"], tf=c["tf"], f=c["f"], window_size=c["W"], min_per=c["min_per"])
    base = period_marks_corr(x32.astype(np.float64), **kw)
    for t in (torch.from_numpy(x32).cuda(), torch.from_numpy(x32.astype(np.float64)).cuda()):
        assert same_bits(period_marks_corr(t, **kw), base), t.dtype
    pm, pv = period_marks_peak(x32.astype(np.float64), sr=8000, f=151.0)
    dm, dv = period_marks_peak(torch.from_numpy(x32).cuda(), sr=8000, f=151.0)
    assert same_bits(pm, dm) and same_bits(pv, dv) and len(pm) > 10


def test_peak_rows_beyond_the_grid_split_and_shuffled():
    from pypevoc_amd.marks import period_marks_rows
    x = R.signal("v8k_long")
    n = 4200                                                         # four rows per workgroup, 1024 workgroups
    starts = np.array([(7 * i) % 3000 for i in range(n)])
    stops = starts + 300 + 10 * (np.arange(n) % 5)
    kw = dict(sr=8000, tf=[0.0, 0.5], f=[149.0, 153.0], method="peak")
    toff = starts / 8000.0
    one = period_marks_rows(x, starts, stops, toff=toff, **kw)
    assert ((one["status"] & ~R.SHORT_FIT) == 0).all() and one["count"].min() >= 3
    assert set(one["status"]) == {0, R.SHORT_FIT}                    # some rows keep a mark one sample off their end
    order = np.random.default_rng(6).permutation(n)
    parts = [order[:1999], order[1999:]]
    for part in parts:
        res = period_marks_rows(x, starts[part], stops[part], toff=toff[part], **kw)
        for j, r in enumerate(part):
            assert res["count"][j] == one["count"][r] and res["status"][j] == one["status"][r]
        assert all(same_bits(row_marks(res, j), row_marks(one, r)) for j, r in enumerate(part))
        assert all(same_bits(res["vals"][j, :res["count"][j]], one["vals"][r, :one["count"][r]]) for j, r in enumerate(part))
    for r in (0, 1, 10, 777, n - 1):                                 # and a row is the single-signal walk of its stretch (row 10: SHORT_FIT)
        ref = R.peak_walk(x[starts[r]:stops[r]], 8000, [0.0, 0.5], [149.0, 153.0], 3, exact=True, toff=toff[r])
        got = row_marks(one, r)
        assert len(got) == len(ref.marks) and one["status"][r] == ref.status
        tol_t, _ = R.peak_tolerance(8000, np.abs(got), 1.0)
        keep = ref.idx < (stops[r] - starts[r]) - 2
        assert np.all(np.abs(got - ref.marks)[keep] <= tol_t[keep])
        assert same_bits(got[~keep], ref.idx[~keep] / 8000.0)        # fewer than 3 fit points: the sample
