"""pypevoc_amd.speech.fricatives without a GPU: the numpy restatement of what the device computes (tests/fricative_refs.py)
against the reference's recorded values (tests/golden/Z*.npz, make_golden_fricatives.py), the status conventions on hand-built
rows, fricative_intervals' window arithmetic, the import lines, the stubs, and the loud failure without a device."""
import json
import os

import numpy as np
import pytest

from . import fricative_refs as R
from .conftest import GOLDEN, ROOT

FILES = ("Z1_rows", "Z2_fused512", "Z3_fused")
_cache = {}


def fixture(name):
    if name not in _cache:
        g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        g["cases"] = json.loads(str(g["cases"]))
        _cache[name] = g
    return _cache[name]


def all_cases():
    return [(f, c["name"]) for f in FILES for c in fixture(f)["cases"]]


def get_case(fname, cname):
    g = fixture(fname)
    return g, [c for c in g["cases"] if c["name"] == cname][0]


def check_values(g, case, got, what=""):
    """got: dict of arrays over the case's rows.  imax identical; every value within the bound computed from the fixture's own
    psd row, rms within its own; returns the worst ratio to the bound per key."""
    cname = case["name"]
    ref, psd, freq = g[cname + "_ref"], g[cname + "_psd"], g[cname + "_freq"]
    x = g[case["x"]].astype(np.float64)
    assert np.array_equal(np.asarray(got["imax"]), g[cname + "_imax"]), (cname, what)
    ratio = dict((k, 0.0) for k in R.REFERENCE_KEYS)
    for r, s in enumerate(case["starts"]):
        bounds = R.value_bounds(freq, psd[r])
        for i, k in enumerate(R.REFERENCE_KEYS):
            want = ref[r, i]
            b = R.rms_bound(x[s:s + case["L"]]) * abs(want) if k == "rms" else bounds[k]
            err = abs(float(got[k][r]) - want)
            assert np.isfinite(err) and err <= b, (cname, what, r, k, float(got[k][r]), want, err, b)
            if b > 0:
                ratio[k] = max(ratio[k], err / b)
    print("%-12s %-22s worst error / bound: " % (cname, what) + "  ".join("%s %.1e" % (k, v) for k, v in ratio.items()))
    return ratio


@pytest.mark.parametrize("fname,cname", all_cases())
def test_restatement_against_the_fixture(fname, cname):
    """The formulas of FRICATIVES.md in plain float64 numpy: the psd within 1e-12 relative per bin of scipy.signal.welch's row,
    the eight values within the propagated bounds of the reference's."""
    g, case = get_case(fname, cname)
    x = g[case["x"]].astype(np.float64)
    freq, psd = R.welch_rows(x, case["starts"], case["L"], case["nwind"], case["sr"])
    assert np.array_equal(freq, g[cname + "_freq"])
    want = g[cname + "_psd"]
    assert psd.shape == want.shape
    err = float(np.max(np.abs(psd - want) / want))
    print("%-12s psd restatement against scipy %.1e" % (cname, err))
    assert err <= 1e-12
    got = dict((k, []) for k in R.REFERENCE_KEYS + ("imax", "status"))
    for s in case["starts"]:
        d = R.fricative_snip(x[s:s + case["L"]], case["nwind"], case["sr"])[0]
        for k in got:
            got[k].append(d[k])
    assert not any(got["status"])
    check_values(g, case, got, "numpy restatement")


def test_fixture_conditions_hold():
    """What the generator refuses a case without: the second-largest bin <= (1 - 1e-6) x the largest; min >= 1e-8 max."""
    for fname, cname in all_cases():
        for S in fixture(fname)[cname + "_psd"]:
            srt = np.sort(S)
            assert srt[-2] <= (1 - 1e-6) * srt[-1] and srt[0] >= 1e-8 * srt[-1], (cname, srt[-2] / srt[-1], srt[0] / srt[-1])


def test_closed_form_sensitivities_are_the_derivatives():
    """The bounds' gradients against central differences in np.longdouble, on a fixture row of 129 bins."""
    g = fixture("Z1_rows")
    freq, S = g["w256_freq"], g["w256_psd"][0]
    a, b = R.sensitivities(freq, S), R.numeric_sensitivities(freq, S)
    for k in R.KEYS:
        assert a[k] > 0 and abs(a[k] - b[k]) <= 1e-6 * a[k], (k, a[k], b[k])


def hand_rows(nb=9):
    """name -> (row, status, the keys that are nan)."""
    f = np.linspace(0.0, 4000.0, nb)
    bump = lambda c: 1.0 + 10.0 * np.exp(-0.5 * ((np.arange(nb) - c) / 1.3) ** 2)      # noqa: E731
    rows = {}
    rows["peak_bin0"] = (np.linspace(5.0, 1.0, nb), 1, ("slope_left",))
    rows["peak_bin1"] = (np.array([2.0, 9.0] + list(np.linspace(3.0, 1.0, nb - 2))), 0, ())
    rows["peak_last"] = (np.linspace(1.0, 5.0, nb), 1, ("slope_right",))
    p = bump(4.0)
    p[5] = p[4]
    rows["plateau"] = (p, 0, ())
    z = bump(5.0)
    z[2] = 0.0
    rows["zero_left"] = (z, 2, ("slope_left",))
    rows["all_zero"] = (np.zeros(nb), 3, R.KEYS)
    rows["regular"] = (bump(4.3), 0, ())
    return f, rows


def check_hand_row(name, f, S, d, status, nans):
    assert int(d["status"]) == status, (name, d["status"])
    for k in R.KEYS:
        assert np.isnan(d[k]) == (k in nans), (name, k, d[k])
    assert int(d["imax"]) == (int(np.argmax(S)) if S.any() else 0), name


def test_status_conventions_on_hand_built_rows():
    f, rows = hand_rows()
    for name, (S, status, nans) in rows.items():
        d = R.descriptors(f, S)
        check_hand_row(name, f, S, d, status, nans)
    d = R.descriptors(f, rows["peak_last"][0])
    assert d["f_max"] == f[-1]                                        # (the reference raises IndexError in refine_max)
    d = R.descriptors(f, rows["peak_bin0"][0])
    assert d["f_max"] == f[1]                                         # refine_max moves a maximum at bin 0 to bin 1
    d = R.descriptors(f, rows["plateau"][0])
    assert d["imax"] == 4 and d["f_max"] == f[4]                      # first index wins, no refinement
    d = R.descriptors(f[:2], np.array([1.0, 3.0]))
    assert d["status"] == 1 and d["f_max"] == f[1] and np.isnan(d["slope_right"]) and not np.isnan(d["slope_left"])
    # the regular rows against numpy's own fit and the package's DistribMoments
    from pypevoc_amd.speech.SpeechAnalysis import DistribMoments
    for name in ("regular", "peak_bin1", "plateau"):
        S = rows[name][0]
        d = R.descriptors(f, S)
        y = 10 * np.log10(S)
        im = int(np.argmax(S))
        assert abs(d["slope_left"] - 1000 * np.polyfit(f[:im + 1], y[:im + 1], 1)[0]) <= 1e-10 * abs(d["slope_left"])
        assert abs(d["slope_right"] - 1000 * np.polyfit(f[im:], y[im:], 1)[0]) <= 1e-10 * abs(d["slope_right"])
        cog, sd, skew, kurt, _ = DistribMoments(f, S)
        for k, v in (("cent", cog), ("stdev", sd), ("skew", skew), ("kurt", kurt)):
            assert abs(d[k] - v) <= 1e-12 * max(abs(v), 1.0), (name, k)


def test_interval_windows_on_hand_worked_intervals():
    from pypevoc_amd.speech.fricatives import interval_windows
    sr, ws = 1000, 100
    # inside: 1.0 .. 2.0 s, middle -> imed 1500, window 1450 .. 1550
    assert interval_windows([(1.0, 2.0)], sr, (0.5,), ws).tolist() == [[1450]]
    # clipped at the start: position 0.02 -> imed 1020, imin 970 < 1000 -> 1000 .. 1100
    assert interval_windows([(1.0, 2.0)], sr, (0.02,), ws).tolist() == [[1000]]
    # clipped at the end: position 0.99 -> imed 1990, imax 2040 > 2000 -> 1900 .. 2000
    assert interval_windows([(1.0, 2.0)], sr, (0.99,), ws).tolist() == [[1900]]
    # an interval shorter than the window (60 ms): imed 1030, 980 < 1000 -> 1000 .. 1100, 1100 > 1060 -> 960 .. 1060
    assert interval_windows([(1.0, 1.06)], sr, (0.5,), ws).tolist() == [[960]]
    # several intervals and positions: [interval][position]
    w = interval_windows([(1.0, 2.0), (3.0, 3.5)], sr, (0.25, 0.5, 0.75), ws)
    assert w.tolist() == [[1200, 1450, 1700], [3075, 3200, 3325]]


def test_geometry_is_scipys():
    from pypevoc_amd.speech.fricatives import geometry, hann_periodic
    assert geometry(1024, 256) == (256, 128, 7, 129)
    assert geometry(300, 333) == (300, 150, 1, 151)
    assert geometry(255, 256) == (255, 128, 1, 128)
    assert geometry(257, 256) == (256, 128, 1, 129)
    assert geometry(4096, 2048) == (2048, 1024, 3, 1025)
    assert geometry(768, 512) == (512, 256, 2, 257)
    # two ways to the same window: each cosine's argument (up to pi) is rounded to 4.4e-16, the window takes half of it, twice
    for n in (255, 256, 300):
        assert np.abs(hann_periodic(n) - R.hann_periodic(n)).max() <= 1e-15


def test_import_lines_and_stubs():
    """The module is imported by the package the way `envelope` is, imports no scipy, and the two stubs of SpeechAnalysis
    still raise."""
    import pypevoc_amd.speech as sp
    from pypevoc_amd.speech import SpeechAnalysis, fricatives
    assert sp.fricatives is fricatives
    init = open(os.path.join(ROOT, "pypevoc_amd", "speech", "__init__.py")).read()
    assert "from . import fricatives  # noqa: F401" in init
    src = open(os.path.join(ROOT, "pypevoc_amd", "speech", "fricatives.py")).read()
    assert "import scipy" not in src and "from scipy" not in src
    for name in ("FricativeDataFromSnip", "FricativeDataFromWav"):
        with pytest.raises(NotImplementedError):
            getattr(SpeechAnalysis, name)(np.zeros(512))
    for name in ("welch_rows", "fricative_desc_rows", "fricative_rows", "FricativeDataFromSnip", "fricative_intervals", "last_kernels"):
        assert callable(getattr(fricatives, name))


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from pypevoc_amd import PvxError
    from pypevoc_amd.speech import fricatives as fr
    x = np.zeros(2048, dtype=np.float32)
    for call in (lambda: fr.welch_rows(x, [0], 1024, 256), lambda: fr.fricative_rows(x, [0, 5], 1024, 256),
                 lambda: fr.fricative_desc_rows(np.ones((2, 9)), np.arange(9.0)), lambda: fr.FricativeDataFromSnip(x),
                 lambda: fr.fricative_intervals(x, 1000, [(0.5, 1.9)], wsize=512)):
        with pytest.raises(PvxError):
            call()
