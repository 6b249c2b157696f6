"""pypevoc_amd.TransferFunctions without a GPU: the fixtures tests/golden/X*.npz (make_golden_transfer.py) against a float64
numpy restatement of mlab's formula, the host side of the mirror -- block starts and times, segment counts, frequencies, the
one-sided scaling, the window_hop=None deviation -- the stubs, and the loud failure without a device.  Also the helpers
test_transfer_gpu.py shares: the restatement, the scales and the bounds of TRANSFER.md."""
import glob
import json
import os

import numpy as np
import pytest

from .conftest import GOLDEN

SELF = 1e-11                                                          # fixture against float64 numpy: both are ~1e-15 from the truth
# bounds of the device results in scaled units (TRANSFER.md): psd relative per bin; csd over sqrt(Pxx Pyy); tfe over
# sqrt(Pyy / Pxx), Pxx the denominator's spectrum; coherence absolute
BOUND = {"psd": 1e-9, "csd": 2e-9, "tfe": 3e-9, "coh": 6e-9}
_CACHE = {}


def golden_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "X*.npz")))


def load(name):
    if name not in _CACHE:
        g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        g["cases"] = json.loads(str(g["cases"]))
        _CACHE[name] = g
    return _CACHE[name]


def all_cases(*funcs, raising=False):
    out = []
    for n in golden_names():
        out += [(n, c["name"]) for c in load(n)["cases"] if (not funcs or c["func"] in funcs) and bool(c["raises"]) == raising]
    return out


def get_case(name, cname):
    g = load(name)
    return g, next(c for c in g["cases"] if c["name"] == cname)


def case_signals(g, case):
    out = []
    for key in (case["x"], case["y"]):
        if key is None:
            out.append(None)
            continue
        x = g[key]
        if case["dtype"] == "float64":
            x = x.astype(np.float64)
        if case.get("slice"):
            x = x[case["slice"][0]:case["slice"][1]]
        assert str(x.dtype) == case["dtype"]
        out.append(x)
    return out


def case_kwargs(g, case):
    kw = dict(case["kw"])
    spec = kw.get("window")
    if spec is not None:
        if "array" in spec:
            kw["window"] = g[spec["array"]].astype(np.float64)
        else:
            f = getattr(np, spec["callable"])
            kw["window"] = lambda x: f(len(x)) * x
    return kw


# ---- float64 numpy restatement (computed once per case and shared) ---------------------------------------------------------
def np_block(x, y, nfft, step, wind):
    """Unscaled means over the segments of conj(Y) X, |X|^2, |Y|^2 of one block (zero-padded to nfft when shorter)."""
    x = np.asarray(x, dtype=np.float64)
    y = x if y is None else np.asarray(y, dtype=np.float64)
    if len(x) < nfft:
        x = np.concatenate([x, np.zeros(nfft - len(x))])
    if len(y) < nfft:
        y = np.concatenate([y, np.zeros(nfft - len(y))])
    nseg = (len(x) - nfft) // step + 1
    idx = np.arange(nseg)[:, None] * step + np.arange(nfft)[None, :]
    X = np.fft.rfft(x[idx] * wind, axis=1)
    Y = np.fft.rfft(y[idx] * wind, axis=1)
    return (np.conj(Y) * X).mean(axis=0), (np.abs(X)**2).mean(axis=0), (np.abs(Y)**2).mean(axis=0)


def np_density(s, nfft, fs, wind):
    c = np.full(nfft // 2 + 1, 2.0)
    c[0] = 1.0
    if not nfft % 2:
        c[-1] = 1.0
    return s * c / fs / (wind**2).sum()


def np_transferogram(source, target, rate, start_time, delta_time, sample_duration, nfft, step):
    """(pxy, pxx, pyy, times) of [nblk][nbins]: the densities of csd(target, source), psd(source), psd(target) per block."""
    wind = np.hanning(nfft)
    slen = int(sample_duration * rate)
    n = len(source) if target is None else min(len(source), len(target))
    s0 = int(start_time * rate)
    i0 = np.arange(s0, n - s0 - slen, int(delta_time * rate))
    rows = [np_block(source[i:i + slen], None if target is None else target[i:i + slen], nfft, step, wind) for i in i0]
    pxy, pxx, pyy = (np_density(np.array([r[j] for r in rows]), nfft, rate, wind) for j in range(3))
    return pxy, pxx, pyy, (i0 + slen / 2) / float(rate)


_REST = {}


def restatement(name, cname):
    """What the case's result is made of, by numpy: dict(pxy, pxx, pyy) for the function's own (x, y) order --
    transferogram: x = source, y = target, pxy = csd(target, source), arrays [nbins][nblk]; the others: pxy = csd(x, y), [nbins]."""
    key = (name, cname)
    if key not in _REST:
        g, case = get_case(name, cname)
        x, y = case_signals(g, case)
        kw = case_kwargs(g, case)
        if case["func"] == "transferogram":
            rate = kw["rate"]
            nfft = 2**int(np.log2(kw["window_duration"] * rate))
            step = 2**int(np.log2(kw["window_hop"] * rate))
            pxy, pxx, pyy, times = np_transferogram(x, y, rate, kw.get("start_time", 0.), kw.get("delta_time", 1.), kw["sample_duration"], nfft, step)
            r = dict(pxy=pxy.T, pxx=pxx.T, pyy=pyy.T, times=times, nfft=nfft, step=step)
        else:
            nfft, fs = kw["NFFT"], kw["Fs"]
            w = kw.get("window")
            wind = np.hanning(nfft) if w is None else (w if isinstance(w, np.ndarray) else w(np.ones(nfft)))
            syx, syy, sxx = np_block(x if y is None else y, None if y is None else x, nfft, nfft - kw.get("noverlap", 0), wind)
            # (np_block's first signal is the unconjugated one: conj(X) Y = csd(x, y))
            r = dict(pxy=np_density(syx, nfft, fs, wind), pxx=np_density(sxx, nfft, fs, wind), pyy=np_density(syy, nfft, fs, wind), nfft=nfft)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REST[key] = r
    return _REST[key]


def worst(got, want, scale):
    """Largest |got - want| / scale over the entries with a positive finite scale.  Everywhere: a nan of `want` is a nan of `got`
    and an exact zero an exact zero; an entry without a scale (a deliberate silence) must be one of the two.  Nothing is left out."""
    got, want, scale = np.asarray(got), np.asarray(want), np.asarray(scale)
    assert got.shape == want.shape == scale.shape, (got.shape, want.shape, scale.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok] == 0, want[ok] == 0)
    with np.errstate(all="ignore"):
        live = ok & (scale > 0) & np.isfinite(scale)
    assert np.all(want[ok & ~live] == 0)
    return float(np.max(np.abs(got[live] - want[live]) / scale[live], initial=0.0))


def compare(name, cname, got, want):
    """Worst scaled differences {quantity: value} between two results of the case (the public functions' return tuples), the
    scales computed with numpy from the fixture's signals."""
    _, case = get_case(name, cname)
    r = restatement(name, cname)
    out = {}
    with np.errstate(all="ignore"):
        if case["func"] == "transferogram":
            if case["y"] is None:
                out["psd"] = worst(got[0], want[0], r["pxx"])
                assert got[3].shape == want[3].shape == (0, want[0].shape[1])
            else:
                out["tfe"] = worst(got[0], want[0], np.sqrt(r["pyy"] / r["pxx"]))
                out["coh"] = worst(got[3], want[3], 1.0 * (r["pxx"] * r["pyy"] > 0))
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            return out
        if case["func"] == "psd":
            out["psd"] = worst(got[0], want[0], r["pxx"])
        elif case["func"] == "csd":
            out["csd"] = worst(got[0], want[0], np.sqrt(r["pxx"] * r["pyy"]))
        elif case["func"] == "cohere":
            out["coh"] = worst(got[0], want[0], 1.0 * (r["pxx"] * r["pyy"] > 0))
        else:                                                         # tfe(y = first, x = second): the denominator is the second's spectrum
            out["tfe"] = worst(got[0], want[0], np.sqrt(r["pxx"] / r["pyy"]))
        assert np.array_equal(got[1], want[1])
    return out


def fixture_result(name, cname):
    g, case = get_case(name, cname)
    if case["func"] == "transferogram":
        return g[cname + "_resp"], g[cname + "_freq"], g[cname + "_times"], g[cname + "_coh"]
    return g[cname + "_out"], g[cname + "_freq"]


def numpy_result(name, cname):
    """The case's result from the restatement, in the public functions' return convention."""
    g, case = get_case(name, cname)
    r = restatement(name, cname)
    ref = fixture_result(name, cname)
    with np.errstate(all="ignore"):
        if case["func"] == "transferogram":
            if case["y"] is None:
                return r["pxx"], ref[1], r["times"], np.zeros((0, r["pxx"].shape[1]))
            return r["pxy"] / r["pxx"], ref[1], r["times"], np.abs(r["pxy"])**2 / (r["pxx"] * r["pyy"])
        if case["func"] == "psd":
            return r["pxx"], ref[1]
        if case["func"] == "csd":
            return r["pxy"], ref[1]
        if case["func"] == "cohere":
            return np.abs(r["pxy"])**2 / (r["pxx"] * r["pyy"]), ref[1]
        return r["pxy"] / r["pyy"], ref[1]                            # tfe(y, x) = csd(y, x) / psd(x): here x is the second signal


SILENT = {"t512_silences": {1: "source", 3: "target", 5: "both"}, "t512_psd_silences": {1: "source", 5: "both"}}


# ---- the fixtures --------------------------------------------------------------------------------------------------------
def test_fixture_list_is_complete():
    assert golden_names() == ["X1_fused", "X2_fused_edges", "X3_rows", "X4_mlab"]
    for n in golden_names():
        assert os.path.getsize(os.path.join(GOLDEN, n + ".npz")) <= 385067
        for k, v in load(n).items():
            if k != "cases" and not k.rsplit("_", 1)[-1] in ("resp", "freq", "times", "coh", "out"):
                assert v.dtype in (np.float32, np.int16), (n, k, v.dtype)
    geo = {}
    for n, cn in all_cases("transferogram"):
        g, case = get_case(n, cn)
        r = restatement(n, cn)
        slen = int(case["kw"]["sample_duration"] * case["kw"]["rate"])
        geo[cn] = dict(nfft=r["nfft"], step=r["step"], nseg=max((slen - r["nfft"]) // r["step"] + 1, 1), nblk=len(r["times"]), slen=slen,
                       delta=int(case["kw"].get("delta_time", 1.) * case["kw"]["rate"]), start=case["kw"].get("start_time", 0.),
                       psd=case["y"] is None, dtype=case["dtype"])
    assert {512, 1024, 2048, 256, 4096} <= {v["nfft"] for v in geo.values() if not v["psd"]}
    assert any(v["step"] * 2 == v["nfft"] for v in geo.values()) and any(v["step"] * 4 == v["nfft"] for v in geo.values())
    assert any(v["nseg"] == 2 and v["slen"] == 2 * v["nfft"] and v["step"] == v["nfft"] for v in geo.values())
    assert any(v["nseg"] >= 5 for v in geo.values())
    assert any(v["delta"] < v["slen"] for v in geo.values()) and any(v["delta"] > v["slen"] for v in geo.values())
    assert any(v["nblk"] >= 14 and v["nfft"] in (512, 1024, 2048) for v in geo.values())
    assert any(v["start"] > 0 for v in geo.values()) and any(v["psd"] for v in geo.values())
    assert any(v["dtype"] == "int16" for v in geo.values()) and any(v["psd"] and v["slen"] < v["nfft"] for v in geo.values())
    funcs = {get_case(n, cn)[1]["func"]: get_case(n, cn)[1]["kw"] for n, cn in all_cases("tfe", "csd", "psd", "cohere") if cn.endswith("333")}
    assert set(funcs) == {"tfe", "csd", "psd", "cohere"} and all(kw["NFFT"] == 333 and kw["noverlap"] == 100 for kw in funcs.values())
    windows = [get_case(n, cn)[1]["kw"].get("window") for n, cn in all_cases("tfe", "csd", "psd", "cohere")]
    assert any(w and "array" in w for w in windows) and any(w and "callable" in w for w in windows)
    assert [cn for _, cn in all_cases(raising=True)] == ["cohere512_too_short"]


@pytest.mark.parametrize("name,cname", all_cases())
def test_fixtures_are_self_consistent(name, cname):
    d = compare(name, cname, fixture_result(name, cname)[:4], numpy_result(name, cname))
    print(name, cname, d)
    assert d and all(v <= SELF for v in d.values()), d


def test_no_scale_is_zero_outside_the_deliberate_silences():
    """The noise floor keeps every bin of every block alive, so that the scaled comparisons leave nothing out; the silent blocks
    give the reference's nan / exact zeros."""
    for name, cname in all_cases():
        r = restatement(name, cname)
        g, case = get_case(name, cname)
        pxx, pyy = np.atleast_2d(r["pxx"].T).T, np.atleast_2d(r["pyy"].T).T          # [nbins][nblk]
        for b in range(pxx.shape[1]):
            quiet = SILENT.get(cname, {}).get(b)
            assert np.all(pxx[:, b] > 0) == (quiet not in ("source", "both")), (cname, b)
            if case["y"] is not None:
                assert np.all(pyy[:, b] > 0) == (quiet not in ("target", "both")), (cname, b)
    g = load("X2_fused_edges")
    resp, coh = g["t512_silences_resp"], g["t512_silences_coh"]
    assert np.all(np.isnan(resp[:, 1])) and np.all(np.isnan(resp[:, 5])) and np.all(resp[:, 3] == 0)
    assert all(np.all(np.isnan(coh[:, b])) for b in (1, 3, 5)) and not np.isnan(coh[:, [0, 2, 4, 6]]).any()
    psd = g["t512_psd_silences_resp"]
    assert np.all(psd[:, [1, 5]] == 0) and np.all(psd[:, [0, 2, 3, 4, 6]] > 0)


def test_coherence_of_the_fixtures_is_neither_zero_nor_one():
    for name, cname in (("X1_fused", "t512"), ("X2_fused_edges", "t2048"), ("X3_rows", "t4096_int16")):
        c = load(name)[cname + "_coh"]
        assert 0.3 < np.median(c) < 0.97 and c.max() <= 1 + 1e-12, (cname, np.median(c))


# ---- the host side of the mirror -----------------------------------------------------------------------------------------
def test_block_starts_and_times():
    from pypevoc_amd import TransferFunctions as tf
    i0, slen, times = tf.block_starts(16000, 8000, 0.5, 0.25, 0.25)   # the start is subtracted twice from the end
    assert slen == 2000 and i0.tolist() == [4000, 6000, 8000] and times.tolist() == [0.625, 0.875, 1.125]
    i0, slen, times = tf.block_starts(1000, 1, 0., 1., .5)
    assert slen == 0 and len(i0) == 1000
    assert len(tf.block_starts(100, 1000, 0., 0.05, 0.2)[0]) == 0
    for name, cname in all_cases("transferogram"):
        g, case = get_case(name, cname)
        kw = case["kw"]
        x, y = case_signals(g, case)
        n = len(x) if y is None else min(len(x), len(y))
        _, _, times = tf.block_starts(n, kw["rate"], kw.get("start_time", 0.), kw.get("delta_time", 1.), kw["sample_duration"])
        assert np.array_equal(times, g[cname + "_times"])
        assert tf.window_geometry(kw["rate"], kw["window_duration"], kw["window_hop"]) == (restatement(name, cname)["nfft"], restatement(name, cname)["step"])


def test_segment_counts_frequencies_and_scaling():
    from pypevoc_amd import TransferFunctions as tf
    for L, nfft, step in ((1024, 512, 512), (1280, 512, 128), (4000, 333, 233), (333, 333, 1), (1000, 256, 256), (2047, 1024, 512)):
        assert tf.nsegments(L, nfft, step) == len(np.lib.stride_tricks.sliding_window_view(np.zeros(L), nfft)[::step])
    assert tf.frequencies(512, 8000)[-1] == 4000.0 and tf.frequencies(333, 8000)[-1] == 166 * (1.0 / (333 * (1 / 8000)))
    assert abs(tf.frequencies(333, 8000)[-1] - 3987.987987987988) < 1e-9 and len(tf.frequencies(333, 8000)) == 167
    for name, cname in all_cases():
        r = restatement(name, cname)
        fs = get_case(name, cname)[1]["kw"].get("Fs", get_case(name, cname)[1]["kw"].get("rate"))
        assert np.array_equal(tf.frequencies(r["nfft"], fs), fixture_result(name, cname)[1])
    assert tf.scaling(8).tolist() == [1, 2, 2, 2, 1] and tf.scaling(7).tolist() == [1, 2, 2, 2] and tf.scaling(2).tolist() == [1, 1]
    assert [tf.nextpow2(v) for v in (1, 2, 3, 1000, 1024, 5512.5)] == [1, 2, 2, 512, 1024, 4096]


def test_window_hop_none_means_half_a_window():
    """The deviation of INTEGRATION.md: the reference's default makes noverlap a float and mlab raises TypeError."""
    from pypevoc_amd import TransferFunctions as tf
    assert tf.window_geometry(8000, 0.128) == (1024, 512) == tf.window_geometry(8000, 0.128, 0.064)
    assert tf.window_geometry(44100, .125, None) == (4096, 2048) and tf.window_geometry(8000, 0.128, 0.128) == (1024, 1024)
    doc = open(os.path.join(os.path.dirname(GOLDEN), "..", "INTEGRATION.md")).read()
    assert "window_hop=None" in doc and "NFFT//2" in doc


def test_argument_checks_need_no_device():
    from pypevoc_amd import TransferFunctions as tf
    x = np.zeros(2000)
    for kw in (dict(detrend="linear"), dict(pad_to=1024), dict(sides="twosided"), dict(scale_by_freq=False)):
        for call in (lambda: tf.psd(x, NFFT=512, **kw), lambda: tf.csd(x, x, NFFT=512, **kw), lambda: tf.tfe(x, x, NFFT=512, **kw),
                     lambda: tf.cohere(x, x, NFFT=512, **kw)):
            with pytest.raises(NotImplementedError):
                call()
    with pytest.raises(ValueError, match="too short"):
        tf.cohere(x[:1000], x[:1000], NFFT=512)
    with pytest.raises(ValueError, match="noverlap"):
        tf.psd(x, NFFT=256, noverlap=256)
    with pytest.raises(NotImplementedError):
        tf.psd(x + 1j, NFFT=256)
    with pytest.raises(NotImplementedError, match="detrend=False"):
        tf.tfe_sig(x, x)
    with pytest.raises(ValueError, match="too short"):              # transferogram with a target: cohere's own complaint
        tf.transferogram(x, x, rate=1000, delta_time=0.1, sample_duration=0.1, window_duration=0.064)
    with pytest.raises(ValueError, match="window length"):
        tf._window(np.ones(100), 256, np.float64)
    w = tf._window(lambda v: np.hamming(len(v)) * v, 64, np.int16)
    assert np.array_equal(w, np.hamming(64)) and np.array_equal(tf._window(None, 64, None), np.hanning(64))


def test_fft_filter_and_its_gains():
    from pypevoc_amd import TransferFunctions as tf
    assert tf.band_gains(8, [(0, 0.5), (0.5, 1.0)], [(1., 1.), (0., 0.)]).tolist() == [1, 1, 0, 0, 0, 0, 0, 1]
    assert tf.band_gains(7, [(0, 0.6)], [(2., 2.)]).tolist() == [2, 2, 0, 0, 0, 0, 2]
    assert tf.band_gains(16, [(0.25, 0.75)], [(1., 4.)]).tolist() == [0, 0, 1, 2, 3, 4, 0, 0, 0, 0, 0, 4, 3, 2, 1, 0]
    assert tf.band_gains(16, [(0, 1.0), (0.25, 0.5)], [(1., 1.), (5., 5.)])[:9].tolist() == [1, 1, 5, 5, 1, 1, 1, 1, 0]   # a later band overrides
    assert tf.band_gains(8, [], []).tolist() == [0] * 8 and tf.band_gains(8, [(0.5, 0.5)], [(1., 1.)]).tolist() == [0] * 8
    for n in (256, 255):
        g = tf.band_gains(n, [(0, 0.3), (0.3, 1.0)], [(1., 0.5), (0.25, 0.)])
        assert g.shape == (n,) and np.array_equal(g[1:], g[1:][::-1])           # bin n - k has the gain of bin k
        x = np.random.default_rng(n).standard_normal(n)
        y = tf.fft_filter(x, [(0, 0.3), (0.3, 1.0)], [(1., 0.5), (0.25, 0.)])
        assert y.shape == (n,) and np.iscomplexobj(y) and np.max(np.abs(y.imag)) < 1e-13
        assert np.allclose(np.fft.fft(y), np.fft.fft(x) * g, atol=1e-10)
    # a tone inside the pass band comes through, one outside does not
    t = np.arange(512)
    lo, hi = np.cos(2 * np.pi * 8 * t / 512), np.cos(2 * np.pi * 100 * t / 512)
    y = tf.fft_filter(lo + hi, [(0, 0.1), (0.1, 1.0)], [(1., 1.), (0., 0.)])
    assert np.max(np.abs(y - lo)) < 1e-12


def test_smthderiv_is_the_windowed_least_squares_slope():
    from pypevoc_amd import TransferFunctions as tf
    ff = np.arange(20.0) * 7 + 1000
    assert np.allclose(tf.smthderiv(ff, 3 * ff + 1, rad=2), 3.0, rtol=1e-12)
    d = tf.smthderiv(ff, 3 * ff + 1)                                   # rad 1: points i - 1 and i; element 0 has one point
    assert np.isnan(d[0]) and np.allclose(d[1:], 3.0, rtol=1e-12)
    rng = np.random.default_rng(5)
    ff, ph = np.cumsum(rng.random(40)) + 50, rng.standard_normal(40)
    for rad in (1, 2, 5, 60):
        d = tf.smthderiv(ff, ph, rad=rad)
        assert d.shape == (40,)
        for i in range(1, 40):
            lo, hi = max(0, i - rad), min(40, i + rad)
            x, y = ff[lo:hi] - ff[lo:hi].mean(), ph[lo:hi] - ph[lo:hi].mean()
            assert abs(d[i] - (x * y).sum() / (x * x).sum()) <= 1e-10 * (1 + abs(d[i])), (rad, i)
    assert tf.smthderiv([], []).shape == (0,)


def test_reference_import_lines_work_without_matplotlib_or_scipy():
    import subprocess
    import sys
    code = ("import sys; from pypevoc_amd import TransferFunctions as tf; "
            "from pypevoc_amd.TransferFunctions import psd, csd, cohere, tfe, tfe_sig, transferogram, nextpow2, smthderiv, fft_filter; "
            "import pypevoc_amd; assert pypevoc_amd.TransferFunctions is tf; "
            "assert not [m for m in sys.modules if m.split('.')[0] in ('matplotlib', 'scipy')]")
    root = os.path.dirname(os.path.dirname(GOLDEN))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("fname,lines", [("determineDelay", "80-109"), ("block_delay", "188-196"), ("maxdelwind", "199-244"),
                                         ("plot_time_freq", "247-261")])
def test_stubs_name_the_reference_lines(fname, lines):
    from pypevoc_amd import TransferFunctions as tf
    with pytest.raises(NotImplementedError) as e:
        getattr(tf, fname)(np.zeros(10), np.zeros(10))
    assert "TransferFunctions.py:" + lines in str(e.value) and "INTEGRATION.md" in str(e.value) and fname in str(e.value)
    assert fname in open(os.path.join(os.path.dirname(os.path.dirname(GOLDEN)), "INTEGRATION.md")).read()


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        return                                                        # (with a device the GPU tests run these calls)
    from pypevoc_amd import PvxError
    from pypevoc_amd import TransferFunctions as tf
    x = np.random.default_rng(0).standard_normal(8000)
    calls = [lambda: tf.psd(x, NFFT=512), lambda: tf.csd(x, x, NFFT=512), lambda: tf.cohere(x, x, NFFT=512), lambda: tf.tfe(x, x, NFFT=333),
             lambda: tf.tfe_sig(x, x, detrend=False), lambda: tf.transferogram(x, x, rate=8000, delta_time=0.1),
             lambda: tf.transferogram(x, None, rate=8000, delta_time=0.1),
             # a call without a block is host arithmetic, but not a CPU fallback either
             lambda: tf.transferogram(x[:100], x[:100], rate=8000)]
    for call in calls:
        with pytest.raises(PvxError) as e:
            call()
        assert "no CPU fallback" in str(e.value)
