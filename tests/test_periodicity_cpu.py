"""Time-domain periodicity (pypevoc_amd.Periodicity): what needs no GPU -- the namespace, the not-mirrored stubs, the P*
fixtures' consistency and the loud failure without a device.  The GPU comparison is test_periodicity_gpu.py."""
import glob
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def period_golden_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "P*.npz")))


def load_period_golden(name):
    """(fixture dict with `x` the float64 signal the reference analysed, list of run descriptions)."""
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    if "x_from" in g:                                                # P6: G7's int16 Perlman samples
        src = np.load(os.path.join(GOLDEN, str(g["x_from"]) + ".npz"))
        g["x"] = src["x"] / src["x_scale"]
    else:
        g["x"] = g["x"].astype(np.float64)
    return g, json.loads(str(g["runs"]))


def ctor_kwargs(g, run):
    kw = dict(run["ctor"])
    w = run["window"]
    if isinstance(w, str):
        kw["window"] = g[w]
    elif w is not None:
        kw["window"] = w
    return kw


def test_reference_import_line_works():
    from pypevoc_amd import PV, PVHarmonic, SinSum, PeriodSeries, period_marks_corr, period_marks_peak, period_marks_amdf  # noqa: F401
    from pypevoc_amd.Periodicity import PeriodTimeSeries, Periodicity, PeriodByPeriod, amdf  # noqa: F401
    assert issubclass(PeriodTimeSeries, PeriodSeries)


@pytest.mark.parametrize("name,where", [("period_marks_corr", "573-618"), ("period_marks_peak", "621-709"),
                                        ("period_marks_amdf", "525-570"), ("amdf", "38-52")])
def test_stubs_name_the_reference_line(name, where):
    from pypevoc_amd import Periodicity as P
    with pytest.raises(NotImplementedError) as e:
        getattr(P, name)(np.zeros(16))
    assert "Periodicity.py:" + where in str(e.value)


def test_period_by_period_stub():
    from pypevoc_amd.Periodicity import PeriodByPeriod
    with pytest.raises(NotImplementedError) as e:
        PeriodByPeriod()
    assert "Periodicity.py:509-522" in str(e.value)


def test_period_fixtures_are_consistent():
    names = period_golden_names()
    assert len(names) >= 7
    total = 0
    for name in names:
        total += os.path.getsize(os.path.join(GOLDEN, name + ".npz"))
        g, runs = load_period_golden(name)
        assert runs
        for r in runs:
            n = r["name"]
            ncand = r["ctor"].get("ncand", 8)
            cnt = g[n + "_count"]
            F = len(cnt)
            for k in ("_period", "_strength"):
                assert g[n + k].shape == (F, ncand)
            for k in ("_preferred", "_index", "_f0", "_f0_05", "_times", "_strength_pref"):
                assert g[n + k].shape == (F,)
            assert ((cnt >= 0) & (cnt <= ncand)).all()
            pref = g[n + "_preferred"]
            assert ((cnt == 0) == (pref == -1)).all() and (pref < np.maximum(cnt, 1)).all()
            for i in range(F):
                assert np.isfinite(g[n + "_period"][i, :cnt[i]]).all() and np.isnan(g[n + "_period"][i, cnt[i]:]).all()
            assert (np.isnan(g[n + "_f0"]) == ~(g[n + "_strength_pref"] > 0)).all()
            if r["mode"] == "calc":
                kw = ctor_kwargs(g, r)
                from pypevoc_amd.Periodicity import PeriodSeries
                ps = PeriodSeries(g["x"], **kw)
                assert np.array_equal(g[n + "_index"], np.arange(ps.nwind, ps.nx - ps.nwind, ps.hop))
    assert total < 2 << 20


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import pypevoc_amd
    x = np.sin(2 * np.pi * 440 / 48000 * np.arange(48000))
    with pytest.raises(pypevoc_amd.PvxError) as e:
        pypevoc_amd.PeriodSeries(x).calc()
    assert "no CPU fallback" in str(e.value)


def test_unknown_method_is_a_value_error():
    from pypevoc_amd import PeriodSeries
    with pytest.raises(ValueError):
        PeriodSeries(np.zeros(48000), method="zc").calc()


def test_per_at_index_outside_the_signal_is_a_value_error():
    from pypevoc_amd import PeriodSeries
    ps = PeriodSeries(np.zeros(48000))
    with pytest.raises(ValueError):
        ps.per_at_index(100)
    with pytest.raises(ValueError):
        ps.per_at_index(48000 - 100)
