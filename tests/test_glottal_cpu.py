"""Glottal inverse filtering (pypevoc_amd.speech.glottal) without a GPU: the fixtures tests/golden/V*.npz
(make_golden_glottal.py) against the float64 numpy restatement of tests/glottal_refs.py, the host side of the mirror --
the high-pass design, frame counts and defaults, the errors raised before the device is touched -- the stubs, and the loud
failure without a device.  Also the helpers test_glottal_gpu.py shares.

The bound of every comparison is 4 * sens_<output> of the case (the factor is SPECDESC.md's): sens is the largest change of
that output when every autocorrelation lag of every LPC moves by up to nwind * 2^-53 * r[0], the worst-case rounding of the
float64 dot product behind it (GLOTTAL.md)."""
import glob
import json
import os

import numpy as np
import pytest

from . import glottal_refs as refs
from .conftest import GOLDEN

OUTPUTS = ("glot", "dglot", "vt", "gc")
_CACHE = {}
_REF = {}


def golden_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "V*.npz")))


def load(name):
    if name not in _CACHE:
        g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        g["cases"] = json.loads(str(g["cases"]))
        for v in g.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[name] = g
    return _CACHE[name]


def all_cases():
    return [(n, c["name"]) for n in golden_names() for c in load(n)["cases"]]


def get_case(name, cname):
    g = load(name)
    return g, next(c for c in g["cases"] if c["name"] == cname)


def case_signal(g, case):
    x = g[case["x"]]
    if case["dtype"] == "float64":
        x = x.astype(np.float64)
    if case["slice"]:
        x = x[case["slice"][0]:case["slice"][1]]
    assert str(x.dtype) == case["dtype"]
    return x


def case_kwargs(case):
    kw = dict(case["kw"])
    if "wind_func" in kw:
        kw["wind_func"] = getattr(np, kw["wind_func"])
    return kw


def bound(g, cname, key):
    return 4.0 * float(g[cname + "_sens_" + key])


def restated(name, cname):
    """(glot, dglot, vt, gc, wins) of the case by tests/glottal_refs.py, computed once"""
    if (name, cname) not in _REF:
        g, case = get_case(name, cname)
        kw = case_kwargs(case)
        nwind = case["nwind"]
        out = refs.ola(case_signal(g, case), nwind, case["nhop"], g[cname + "_hpfilt_b"], np.hanning(nwind),
                       kw.get("wind_func", np.hanning)(nwind), case["tract_order"], case["glottal_order"], 0.99, kw.get("n_it", 1))
        for a in out:
            a.setflags(write=False)
        _REF[(name, cname)] = out
    return _REF[(name, cname)]


# ---- the fixtures --------------------------------------------------------------------------------------------------------
def test_fixture_list_is_complete():
    assert golden_names() == ["V1_11k", "V2_22k", "V3_44k", "V4_edges"]
    for n in golden_names():
        assert os.path.getsize(os.path.join(GOLDEN, n + ".npz")) < 400000
    cases = {cn: get_case(n, cn) for n, cn in all_cases()}
    geo = {(c["Fs"], c["nwind"], len(g[cn + "_hpfilt_b"]), c["tract_order"], c["glottal_order"], c["kw"].get("n_it", 1))
           for cn, (g, c) in cases.items()}
    assert {(11025, 276, 207, 16, 6, 1), (22050, 551, 413, 26, 12, 0), (22050, 551, 413, 26, 12, 1), (22050, 551, 413, 26, 12, 2),
            (44100, 1102, 827, 48, 22, 1), (11025, 256, 207, 16, 6, 1)} <= geo
    assert cases["v11k_w256_h100"][1]["nhop"] == 100
    assert {c["dtype"] for _, c in cases.values()} == {"float32", "float64", "int16"}
    assert cases["e_noframe"][0]["e_noframe_vt"].shape == (0,) and cases["e_oneframe"][0]["e_oneframe_vt"].shape == (1, 17)
    assert cases["e_hamming"][1]["kw"]["wind_func"] == "hamming"
    assert cases["v44k"][1]["nwind"] % cases["v44k"][1]["nhop"] != 0  # the default hop does not divide the window


@pytest.mark.parametrize("name,cname", all_cases())
def test_fixtures_are_self_consistent(name, cname):
    """Shapes, frame counts, the window-sum pattern, the three recorded frames against the full call, and the restatement
    within the bound: the bound admits a correct implementation."""
    g, case = get_case(name, cname)
    x = case_signal(g, case)
    nwind, nhop, pt, pg = case["nwind"], case["nhop"], case["tract_order"], case["glottal_order"]
    n_it = case["kw"].get("n_it", 1)
    starts = refs.frame_starts(len(x), nwind, nhop)
    nfr = len(starts)
    assert g[cname + "_glot"].shape == g[cname + "_dglot"].shape == g[cname + "_winspos"].shape == (len(x),)
    if nfr == 0:
        assert g[cname + "_vt"].shape == g[cname + "_gc"].shape == (0,)
        assert not g[cname + "_glot"].any() and not g[cname + "_dglot"].any() and not g[cname + "_winspos"].any()
        return
    assert g[cname + "_vt"].shape == (nfr, pt + 1) and g[cname + "_gc"].shape == (nfr, (pg if n_it else 1) + 1)
    assert np.all(g[cname + "_vt"][:, 0] == 1.0) and np.all(g[cname + "_gc"][:, 0] == 1.0)
    glot, dglot, vt, gc, wins = restated(name, cname)
    assert np.array_equal(wins > 0, g[cname + "_winspos"])
    assert not g[cname + "_glot"][~g[cname + "_winspos"]].any() and not g[cname + "_dglot"][~g[cname + "_winspos"]].any()
    if "hamming" in cname:
        assert g[cname + "_winspos"][0] and g[cname + "_winspos"][starts[-1] + nwind - 1]
    else:
        assert not g[cname + "_winspos"][0]
    for key, got in zip(OUTPUTS, (glot, dglot, vt, gc)):
        err = float(np.max(np.abs(got - g[cname + "_" + key])))
        print("%s %s: restatement - reference %.3e, bound %.3e" % (cname, key, err, bound(g, cname, key)))
        assert g[cname + "_sens_" + key] > 0 and err <= bound(g, cname, key), (key, err)
    # InverseFilter.apply's frames are the full call's
    frames = [int(q) for q in g[cname + "_frames"]]
    assert frames == sorted(set([0, nfr // 2, nfr - 1]))
    for k, q in enumerate(frames):
        assert np.array_equal(g[cname + "_fvt"][k], g[cname + "_vt"][q]) and np.array_equal(g[cname + "_fgc"][k], g[cname + "_gc"][q])
        fr = refs.frame(x[starts[q]:starts[q] + nwind], g[cname + "_hpfilt_b"], np.hanning(nwind), pt, pg, 0.99, n_it)
        assert np.max(np.abs(fr[0] - g[cname + "_fg"][k])) <= bound(g, cname, "glot")
        assert np.max(np.abs(fr[1] - g[cname + "_fdg"][k])) <= bound(g, cname, "dglot")


def test_fixtures_cannot_be_met_by_zeros():
    for name, cname in all_cases():
        g, case = get_case(name, cname)
        if len(g[cname + "_vt"]):
            for key in OUTPUTS:
                assert np.abs(g[cname + "_" + key]).max() > 1e4 * bound(g, cname, key), (cname, key)


# ---- the host side of the mirror -----------------------------------------------------------------------------------------
def test_highpass_design_is_the_recorded_one():
    from pypevoc_amd.speech import glottal
    seen = set()
    for name, cname in all_cases():
        g, case = get_case(name, cname)
        ref = g[cname + "_hpfilt_b"]
        Fs = case["Fs"]
        if (Fs, len(ref)) in seen:
            continue
        seen.add((Fs, len(ref)))
        b = glottal.firls(int(np.round(300 / 16000 * Fs)), [0, 40, 70, Fs / 2], [0, 0, 1, 1], Fs)
        assert b.shape == ref.shape and np.max(np.abs(b - ref)) <= 1e-14, (Fs, np.max(np.abs(b - ref)))
    assert {t for _, t in seen} == {207, 413, 827}


def test_defaults_and_frame_counts_per_rate():
    from pypevoc_amd import _lib
    from pypevoc_amd.speech import glottal
    assert glottal.default_frame(44100) == (1102, 220, 48, 22)
    assert glottal.default_frame(22050) == (551, 110, 26, 12)
    assert glottal.default_frame(11025) == (276, 55, 16, 6)
    assert glottal.default_frame(16000) == (400, 80, 20, 8)
    for name, cname in all_cases():
        g, case = get_case(name, cname)
        n = len(case_signal(g, case))
        assert _lib.nframes_host(n, case["nwind"], case["nhop"]) == len(g[cname + "_vt"]) == len(refs.frame_starts(n, case["nwind"], case["nhop"]))
    assert _lib.nframes_host(276, 276, 55) == 0 and _lib.nframes_host(277, 276, 55) == 1
    # the constructor's own default orders are not iaif_ola's
    f = glottal.InverseFilter(Fs=11025, nwind=276)
    assert (f.tract_order, f.glottal_order, f.n_pad, f.nwind, f.hpfilt) == (12, 10, 13, 276, 1)
    assert f.leaky_integrator.tolist() == [1, -0.99] and f.id.tolist() == [1] and np.array_equal(f.wind, np.hanning(276))
    assert len(f.hpfilt_b) == 207 and f.init_preliminary_filter(order=101) == 101 and len(f.hpfilt_b) == 101


@pytest.mark.parametrize("Fs", [16000, 48000, 8000])
def test_even_filter_orders_raise_on_the_host(Fs):
    """The reference's firls refuses an even number of taps; the mirror raises before the library is even loaded."""
    from pypevoc_amd.speech import glottal
    for call in (lambda: glottal.InverseFilter(Fs=Fs, nwind=400), lambda: glottal.iaif_ola(np.zeros(4000), Fs=Fs)):
        with pytest.raises(ValueError) as e:
            call()
        assert "numtaps must be odd" in str(e.value)


def test_short_window_warns_and_returns(caplog):
    from pypevoc_amd.speech import glottal
    with caplog.at_level("WARNING"):
        f = glottal.InverseFilter(Fs=11025, nwind=12, tract_order=12)
    assert "Frame not analysed" in caplog.text
    assert not hasattr(f, "nwind") and not hasattr(f, "hpfilt_b") and f.tract_order == 12


def test_lpc_order_check_and_reference_import_lines():
    from pypevoc_amd import speech
    from pypevoc_amd.speech import glottal
    assert speech.glottal is glottal
    for f in ("lpc", "lpc_frames", "iaif_ola", "InverseFilter", "last_kernels"):
        assert callable(getattr(glottal, f))
    with pytest.raises(ValueError):
        glottal.lpc(np.ones(5), 6)


@pytest.mark.parametrize("fname,lines", [("PaddedFilter", "86-126"), ("fir_pre_phase", "129-140"), ("lpcc2pole", "249-272")])
def test_stubs_name_the_reference_lines(fname, lines):
    from pypevoc_amd.speech import glottal
    with pytest.raises(NotImplementedError) as e:
        getattr(glottal, fname)(np.zeros(10), 4)
    assert "glottal.py:" + lines in str(e.value) and "INTEGRATION.md" in str(e.value) and fname in str(e.value)


def test_levinson_restatement_solves_the_toeplitz_system():
    rng = np.random.default_rng(5)
    v = rng.standard_normal(300)
    for p in (1, 7, 48):
        r = refs.autocorr(v, p)
        assert np.allclose(r, np.correlate(v, v, "full")[len(v) - 1:len(v) + p], rtol=1e-13, atol=0)
        a = refs.levinson(r, p)
        T = r[np.abs(np.arange(p)[:, None] - np.arange(p)[None, :])]
        assert a[0] == 1.0 and np.max(np.abs(T @ a[1:] + r[1:])) <= 1e-10 * r[0]
    with pytest.raises(np.linalg.LinAlgError):
        refs.lpc(np.zeros(50), 4)


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from pypevoc_amd import PvxError
    from pypevoc_amd.speech import glottal
    x = np.sin(2 * np.pi * 120 / 11025. * np.arange(3000))
    f = glottal.InverseFilter(Fs=11025, nwind=276)
    calls = [lambda: glottal.iaif_ola(x, Fs=11025), lambda: f.apply(x[:276]), lambda: glottal.lpc(x[:300], 8),
             lambda: glottal.lpc_frames(x, 8, 256, 100, np.hanning(256)),
             # the no-frame result is zeros, but not a CPU fallback either
             lambda: glottal.iaif_ola(x[:200], Fs=11025)]
    for call in calls:
        with pytest.raises(PvxError) as e:
            call()
        assert "no CPU fallback" in str(e.value)
