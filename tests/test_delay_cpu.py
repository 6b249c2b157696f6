"""pypevoc_amd.delay without a GPU: the fixtures tests/golden/Y*.npz (make_golden_delay.py: the reference's maxdelwind,
block_delay and determineDelay) against the numpy restatement of tests/delay_refs.py, the host side of the module -- block
starts and times, the errors that need no device, the imports -- and the loud failure without a device.  Also the helpers
test_delay_gpu.py shares: the fixture cases, and the seeded shapes with their restatement (computed once, read-only)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from . import delay_refs as dr
from .conftest import GOLDEN, ROOT

_CACHE = {}


def load(name):
    if name not in _CACHE:
        g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        g["cases"] = json.loads(str(g["cases"]))
        _CACHE[name] = g
    return _CACHE[name]


def case_names(name):
    return [c["name"] for c in load(name)["cases"]]


def get_case(name, cname):
    g = load(name)
    return g, next(c for c in g["cases"] if c["name"] == cname)


def case_signals(g, case):
    """(source, target) in the case's sample type."""
    out = []
    for key, which in ((case["source"], "slice"), (case["target"], "tslice")):
        x = g[key]
        if case["dtype"] == "float64":
            x = x.astype(np.float64)
        sl = case.get(which) or case.get("slice")
        if sl:
            x = x[sl[0]:sl[1]]
        assert str(x.dtype) == case["dtype"]
        out.append(x)
    return out


def case_window(case, n):
    return None if case.get("window") is None else getattr(np, case["window"])(n)


_REST = {}


def restatement(name, cname):
    """The case by tests/delay_refs.py, computed once: Y1 (delay, strength, times, blocks), Y2 (lag, max, blocks), Y3 (delay,
    blocks of source against source, blocks of target against source)."""
    key = (name, cname)
    if key not in _REST:
        g, case = get_case(name, cname)
        src, tgt = case_signals(g, case)
        if name.startswith("Y1"):
            _REST[key] = dr.maxdelwind(src, tgt, **case["kw"])
        elif name.startswith("Y2"):
            _REST[key] = dr.block_delay(src, tgt, case_window(case, len(src)))
        else:
            _REST[key] = dr.determine_delay(src, tgt, case["maxdel"])
    return _REST[key]


# ---- seeded shapes that are in no fixture (test_delay_gpu.py runs them on the device) --------------------------------------
SHAPES = [(n, n) for n in (1, 2, 63, 64, 65, 300, 512, 513, 2048, 2049)] + [(700, 300), (300, 700), (1, 400), (3000, 5)]
NBLK = 37
# (detrend, window on a, window on v, use_abs with a negated a, sample type): every detrend mode; windows on one signal, both
# and neither; the three sample types
CONFIGS = [("none", False, False, False, "float32"), ("constant", True, False, False, "float64"), ("linear", True, True, False, "int16"),
           ("none", False, True, True, "float32"), ("linear", False, False, False, "float32"), ("constant", True, True, True, "int16")]
_SHAPES = {}


def shape_delta(la, lv):
    return max(1, max(la, lv) // 3)                                   # overlapping blocks


def shape_case(la, lv, ci):
    """dict(a, v, kw, ref) of NBLK overlapping blocks: v seeded noise, a that noise delayed by up to 3 samples through a short
    FIR plus independent noise (negated for use_abs), both float32-exact or int16.  A block side of 1 sample keeps its detrend
    (an exact zero: a silent block); one of 2 samples is not detrended: without their means two pairs (-d, d) and (-e, e)
    correlate to (-de, 2de, -de), an exact tie whenever de < 0, and a line through two points leaves only rounding residue
    (DELAY.md: neither has a defined arg-max)."""
    key = (la, lv, ci)
    if key not in _SHAPES:
        detrend, wa, wv, use_abs, dtype = CONFIGS[ci]
        if min(la, lv) == 2:
            detrend = "none"
        delta = shape_delta(la, lv)
        n = (NBLK - 1) * delta + max(la, lv)
        rng = np.random.default_rng(1000 * la + lv + 7 * ci)
        v = rng.standard_normal(n)
        d = min(3, la - 1, lv - 1)
        a = np.convolve(np.concatenate([np.zeros(d), v])[:n], [1.0, 0.5, 0.25, -0.2, 0.1])[:n] + 0.3 * rng.standard_normal(n) + 0.2
        if use_abs:
            a = -a
        if dtype == "int16":
            a, v = np.round(a * 4000).astype(np.int16), np.round(v * 4000).astype(np.int16)
        else:
            a, v = a.astype(np.float32).astype(dtype), v.astype(np.float32).astype(dtype)
        kw = dict(la=la, lv=lv, start=0, delta=delta, nblk=NBLK, window_a=0.1 + np.hamming(la) if wa else None,
                  window_v=0.1 + np.hamming(lv) if wv else None, detrend=detrend, use_abs=use_abs)
        for x in (a, v):
            x.setflags(write=False)
        _SHAPES[key] = dict(a=a, v=v, kw=kw, ref=dr.xcorr_blocks(a, v, **kw))
    return _SHAPES[key]


# ---- the fixtures --------------------------------------------------------------------------------------------------------
def test_fixture_list_is_complete():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "Y*.npz")))
    assert names == ["Y1_maxdelwind", "Y2_block_delay", "Y3_determine_delay"]
    for n in names:
        assert os.path.getsize(os.path.join(GOLDEN, n + ".npz")) <= 300000
        g = load(n)
        keys = {c[k] for c in g["cases"] for k in ("source", "target")}
        assert all(g[k].dtype in (np.float32, np.int16) for k in keys)
    y1 = {c["name"]: c for c in load("Y1_maxdelwind")["cases"]}
    geo = {}
    for cn, c in y1.items():
        kw = c["kw"]
        d = load("Y1_maxdelwind")[cn + "_delay"]
        geo[cn] = dict(slen=int(kw["sample_duration"] * kw["rate"]), delta=int(kw.get("delta_time", 1.) * kw["rate"]), start=kw.get("start_time", 0.),
                       nblk=len(d), pos=bool(len(d)) and bool(np.all(d > 0)), neg=bool(len(d)) and bool(np.all(d < 0)), dtype=c["dtype"])
    assert geo["positive"]["pos"] and geo["negative"]["neg"]
    assert any(v["delta"] < v["slen"] and v["start"] > 0 for v in geo.values()) and any(v["delta"] > v["slen"] for v in geo.values())
    assert any(v["slen"] > 2048 and v["nblk"] >= 3 for v in geo.values()) and any(v["slen"] <= 2048 for v in geo.values())
    assert geo["no_block"]["nblk"] == 0 and {"int16", "float32", "float64"} == {v["dtype"] for v in geo.values()}
    assert {"silences", "ramp", "sine"} <= set(geo)
    y2 = load("Y2_block_delay")
    lens = {cn: len(case_signals(y2, get_case("Y2_block_delay", cn)[1])[0]) for cn in case_names("Y2_block_delay")}
    assert {300, 2049, 10} == set(lens.values())
    assert {c["window"] for c in y2["cases"]} == {None, "hanning"}
    assert int(y2["b300_identical_lag"]) == -1 and int(y2["b2049_identical_lag"]) == -1
    assert int(y2["zeros10_lag"]) == -10 and float(y2["zeros10_max"]) == 0.0
    y3 = load("Y3_determine_delay")
    md = {c["name"]: c["maxdel"] for c in y3["cases"]}
    assert md["maxdel_16384"] == 2**14 and md["maxdel_beyond_both"] > 5000 and int(y3["negated_3000_delay"]) == 211
    s, t = case_signals(y3, get_case("Y3_determine_delay", "short_target")[1])
    assert len(t) < md["short_target"] <= len(s)


def test_silences_and_the_ramp_are_what_they_claim():
    g, case = get_case("Y1_maxdelwind", "silences")
    delay, strength, times, r = restatement("Y1_maxdelwind", "silences")
    src, tgt = case_signals(g, case)
    quiet = {2: "source", 4: "target", 6: "both"}
    for b in range(len(times)):
        s0 = b * 800
        assert (not src[s0:s0 + 800].any()) == (quiet.get(b) in ("source", "both")) and (not tgt[s0:s0 + 800].any()) == (quiet.get(b) in ("target", "both"))
        assert (r["scale"][b] == 0) == (b in quiet)
    for b in quiet:                                                   # lag 0, and exactly 0.0
        assert g["silences_delay"][b] == -800 / 8000.0 and g["silences_strength"][b] == 0.0 and not np.signbit(g["silences_strength"][b])
    # the detrend matters: without it the ramp's blocks peak elsewhere
    g, case = get_case("Y1_maxdelwind", "ramp")
    src, tgt = case_signals(g, case)
    plain = dr.xcorr_blocks(tgt, src, 800, 800, 0, 1200, 5)
    assert not np.array_equal((plain["lag"] - 800) / 8000.0, g["ramp_delay"])


@pytest.mark.parametrize("cname", case_names("Y1_maxdelwind"))
def test_maxdelwind_fixture_against_the_restatement(cname):
    g = load("Y1_maxdelwind")
    delay, strength, times, r = restatement("Y1_maxdelwind", cname)
    assert np.array_equal(g[cname + "_times"], times) and np.array_equal(g[cname + "_delay"], delay)           # identical lags
    assert g[cname + "_strength"].dtype == np.float64 and g[cname + "_strength"].shape == strength.shape
    if r is None:
        assert len(times) == 0
        return
    assert dr.guard_holds(r)
    assert np.all(np.abs(g[cname + "_strength"] - strength) <= dr.SELF_BOUND * r["scale"])
    # the FFT form of the restatement, which the large GPU cases rely on, agrees with np.correlate
    kw = get_case("Y1_maxdelwind", cname)[1]["kw"]
    f = dr.maxdelwind(*case_signals(g, get_case("Y1_maxdelwind", cname)[1]), fft=True, **kw)[3]
    assert np.array_equal(f["lag"], r["lag"]) and np.all(np.abs(f["corr"] - r["corr"]) <= 1e-13 * r["scale"][:, None] + 1e-300)


@pytest.mark.parametrize("cname", case_names("Y2_block_delay"))
def test_block_delay_fixture_against_the_restatement(cname):
    g = load("Y2_block_delay")
    lag, mx, r = restatement("Y2_block_delay", cname)
    assert int(g[cname + "_lag"]) == lag and dr.guard_holds(r)
    assert abs(float(g[cname + "_max"]) - mx) <= dr.SELF_BOUND * r["scale"][0]


@pytest.mark.parametrize("cname", case_names("Y3_determine_delay"))
def test_determine_delay_fixture_against_the_restatement(cname):
    g = load("Y3_determine_delay")
    delay, rx, ry = restatement("Y3_determine_delay", cname)
    assert int(g[cname + "_delay"]) == delay and dr.guard_holds(rx) and dr.guard_holds(ry)
    assert rx["lag"][0] == len(rx["corr"][0]) // 2                    # a signal against itself peaks at lag la - 1
    if cname.startswith("negated"):
        assert ry["peak"][0] < 0                                      # the abs is what finds it


@pytest.mark.parametrize("la,lv", SHAPES)
def test_the_seeded_shapes_clear_the_guard(la, lv):
    """What test_delay_gpu.py asserts before it compares lags, checked where no device is needed."""
    for ci in range(len(CONFIGS)):
        c = shape_case(la, lv, ci)
        assert dr.guard_holds(c["ref"]), (la, lv, ci)
        one = min(la, lv) == 1 and c["kw"]["detrend"] != "none"
        assert np.all(c["ref"]["scale"] == 0) if one else np.all(c["ref"]["scale"] > 0)
        if c["kw"]["use_abs"] and min(la, lv) >= 63:
            assert np.all(c["ref"]["peak"] < 0)                       # the abs is what finds these


def test_the_restatement_is_numpy_correlate_for_every_order_of_lengths():
    rng = np.random.default_rng(3)
    for la, lv in ((5, 5), (7, 3), (3, 7), (1, 4)):
        a, v = rng.standard_normal(la), rng.standard_normal(lv)
        want = np.array([sum(a[m + k - (lv - 1)] * v[m] for m in range(lv) if 0 <= m + k - (lv - 1) < la) for k in range(la + lv - 1)])
        r = dr.xcorr_blocks(a, v, la, lv)
        assert np.allclose(r["corr"][0], want, atol=1e-14) and np.allclose(dr.correlate_fft(a, v), want, atol=1e-14)
    x = np.arange(50.0) * 0.3 - 2 + np.sin(np.arange(50.0))
    line = np.polyval(np.polyfit(np.arange(50.0), x, 1), np.arange(50.0))
    assert np.allclose(dr.detrended(x, "linear"), x - line, atol=1e-12) and np.allclose(dr.detrended(x, "constant"), x - x.mean(), atol=1e-14)


# ---- the host side of the module -----------------------------------------------------------------------------------------
def test_block_geometry_is_transferograms():
    from pypevoc_amd import TransferFunctions as tf
    for cname in case_names("Y1_maxdelwind"):
        g, case = get_case("Y1_maxdelwind", cname)
        kw = case["kw"]
        src, tgt = case_signals(g, case)
        i0, slen, times = tf.block_starts(min(len(src), len(tgt)), kw["rate"], kw.get("start_time", 0.), kw.get("delta_time", 1.), kw["sample_duration"])
        assert np.array_equal(times, g[cname + "_times"]) and len(i0) == len(g[cname + "_delay"]) and slen == int(kw["sample_duration"] * kw["rate"])


class FakeDeviceArray(object):
    """Enough of a device tensor for the checks that run before the device is touched."""

    def __init__(self, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(4096, False), version=2, strides=None)


def test_stable_errors_need_no_device():
    from pypevoc_amd import delay
    x = np.zeros(100, dtype=np.float32)
    two_d = np.zeros((10, 10), dtype=np.float32)
    for call in (lambda: delay.block_delay(two_d, two_d), lambda: delay.maxdelwind(two_d, two_d), lambda: delay.determineDelay(two_d, two_d),
                 lambda: delay.xcorr_peaks(two_d, x, 10), lambda: delay.xcorr_peaks(FakeDeviceArray((10, 10), "<f4"), FakeDeviceArray((100,), "<f4"), 10),
                 lambda: delay.block_delay(x, x[:50]), lambda: delay.xcorr_peaks(x, x, 10, window_a=np.ones(9)),
                 lambda: delay.xcorr_peaks(x, x, 10, detrend="quadratic"), lambda: delay.xcorr_peaks(x, x, 0)):
        with pytest.raises(ValueError):
            call()
    d32, d64 = FakeDeviceArray((100,), "<f4"), FakeDeviceArray((100,), "<f8")
    for call in (lambda: delay.xcorr_peaks(x, d32, 10), lambda: delay.xcorr_peaks(d32, x, 10), lambda: delay.xcorr_peaks(d32, d64, 10),
                 lambda: delay.maxdelwind(x, d32, rate=100), lambda: delay.maxdelwind(d64, d32, rate=100), lambda: delay.block_delay(d32, d64),
                 lambda: delay.determineDelay(x, d32)):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(NotImplementedError, match="ax"):
        delay.determineDelay(x, x, ax=object())


def test_the_module_imports_neither_scipy_nor_matplotlib():
    code = ("import sys; import pypevoc_amd; from pypevoc_amd import delay; "
            "from pypevoc_amd.delay import determineDelay, block_delay, maxdelwind, xcorr_peaks, last_kernels; "
            "assert pypevoc_amd.delay is delay and 'delay' in pypevoc_amd.__all__; "
            "assert not [m for m in sys.modules if m.split('.')[0] in ('matplotlib', 'scipy')]")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_stubs_of_transferfunctions_stay_stubs():
    from pypevoc_amd import TransferFunctions as tf
    from pypevoc_amd import delay
    for name in ("determineDelay", "block_delay", "maxdelwind"):
        with pytest.raises(NotImplementedError):
            getattr(tf, name)(np.zeros(10), np.zeros(10))
        assert getattr(delay, name) is not getattr(tf, name)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pypevoc_amd.delay" in doc and "PVX_XCORR_FFT" in doc


def test_the_ctypes_table_and_the_header_agree_on_the_constants():
    from pypevoc_amd import _lib
    src = open(os.path.join(ROOT, "include", "pvx.h")).read()
    assert "#define PVX_XCORR_DIRECT_MAX %d\n" % _lib.PVX_XCORR_DIRECT_MAX in src and _lib.PVX_XCORR_DIRECT_MAX == 2048
    assert "#define PVX_XCORR_MAX_P (1 << 20)" in src and _lib.PVX_XCORR_MAX_P == 1 << 20
    assert "PVX_DETREND_NONE = 0, PVX_DETREND_CONSTANT = 1, PVX_DETREND_LINEAR = 2" in src
    assert (_lib.PVX_DETREND_NONE, _lib.PVX_DETREND_CONSTANT, _lib.PVX_DETREND_LINEAR) == (0, 1, 2)


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        return                                                        # (with a device the GPU tests run these calls)
    from pypevoc_amd import PvxError, delay
    x = np.random.default_rng(0).standard_normal(8000)
    calls = [lambda: delay.block_delay(x[:300], x[:300]), lambda: delay.block_delay(x[:300], x[:300], window=np.hanning(300)),
             lambda: delay.maxdelwind(x, x, rate=8000, delta_time=0.1, sample_duration=0.1), lambda: delay.determineDelay(x, x, maxdel=1000),
             lambda: delay.xcorr_peaks(x, x, 100, full=True),
             # a call without a block is host arithmetic, but not a CPU fallback either
             lambda: delay.maxdelwind(x[:100], x[:100], rate=8000), lambda: delay.xcorr_peaks(x, x, 100, nblk=0)]
    for call in calls:
        with pytest.raises(PvxError) as e:
            call()
        assert "no CPU fallback" in str(e.value)
