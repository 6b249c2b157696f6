"""pypevoc_amd.delay on the MI355X (k_xcorr.hip) against the reference's outputs (tests/golden/Y*.npz, make_golden_delay.py)
and, for the shapes no fixture holds, against the numpy restatement of tests/delay_refs.py.

Bounds (DELAY.md): lags identical, no block left out; values, and every lag of the full output, within 2e-9 norm(a') norm(v')
absolute -- the project's 1e-9 relative per spectrum bin over the two factors of a product, then Cauchy-Schwarz and Parseval
over the bins -- on both routes; a silent block gives lag 0 and exactly 0.0.  Before lags are compared the winner's margin is
asserted on the restatement (1e-6 norm norm, 500 times the value bound).  Run with -s for the worst measured values."""
import ctypes

import numpy as np
import pytest

from . import delay_refs as dr
from .test_delay_cpu import CONFIGS, SHAPES, case_names, case_signals, case_window, get_case, restatement, shape_case

pytestmark = pytest.mark.gpu

DIRECT = "k_xcorr_direct"
FFT = "k_xcorr_prep+rocfft+k_xcorr_mul+rocfft+k_xcorr_peak"
ROUTES = ("natural", "fft")


def natural(la, lv):
    return DIRECT if max(la, lv) <= 2048 else FFT


def set_route(monkeypatch, route):
    if route == "fft":
        monkeypatch.setenv("PVX_XCORR_FFT", "1")
    else:
        monkeypatch.delenv("PVX_XCORR_FFT", raising=False)


def check_blocks(what, got, r, full=True):
    """(lag, peak[, corr]) of a device call against the restatement's blocks: the guard first, then identical lags, values
    within the bound, silent blocks exact.  Returns the worst value error in units of the scale."""
    lag, peak = got[0], got[1]
    assert dr.guard_holds(r), what
    assert lag.dtype == np.int64 and peak.dtype == np.float64 and lag.shape == peak.shape == r["lag"].shape, what
    assert np.array_equal(lag, r["lag"]), (what, lag, r["lag"])
    silent = r["scale"] == 0
    assert np.all(peak[silent] == 0.0) and not np.any(np.signbit(peak[silent])), what
    live = ~silent
    w = float(np.max(np.abs(peak[live] - r["peak"][live]) / r["scale"][live], initial=0.0))
    if full:
        corr = got[2]
        assert corr.shape == r["corr"].shape and np.all(corr[silent] == 0.0), what
        w = max(w, float(np.max(np.abs(corr[live] - r["corr"][live]) / r["scale"][live][:, None], initial=0.0)))
        assert np.array_equal(peak, corr[np.arange(len(lag)), lag] + 0.0), what
    print("%-60s worst %.1e (bound %.0e)" % (what, w, dr.VALUE_BOUND))
    assert w <= dr.VALUE_BOUND, (what, w)
    return w


def same_bits(a, b):
    return len(a) == len(b) and all(p.tobytes() == q.tobytes() and p.shape == q.shape for p, q in zip(a, b))


# ---- the fixtures, through the public functions, on both routes ----------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("cname", case_names("Y1_maxdelwind"))
def test_maxdelwind_fixture(cname, route, monkeypatch):
    from pypevoc_amd import delay
    g, case = get_case("Y1_maxdelwind", cname)
    src, tgt = case_signals(g, case)
    kw = case["kw"]
    set_route(monkeypatch, route)
    d, s, t = delay.maxdelwind(src, tgt, **kw)
    assert d.dtype == s.dtype == t.dtype == np.float64
    assert np.array_equal(t, g[cname + "_times"]) and d.shape == s.shape == t.shape
    if len(t) == 0:                                                   # (no device call: last_kernels keeps what ran before)
        return
    slen = int(kw["sample_duration"] * kw["rate"])
    assert delay.last_kernels() == (FFT if route == "fft" else natural(slen, slen))
    assert np.array_equal(d, g[cname + "_delay"]), (d, g[cname + "_delay"])                                   # identical lags, every block
    r = restatement("Y1_maxdelwind", cname)[3]
    assert dr.guard_holds(r)
    silent = r["scale"] == 0
    assert np.all(s[silent] == 0.0) and not np.any(np.signbit(s[silent])) and np.all(d[silent] == -slen / float(kw["rate"]))
    w = float(np.max(np.abs(s - g[cname + "_strength"])[~silent] / r["scale"][~silent], initial=0.0))
    print("%-20s %-8s against the reference: worst %.1e (bound %.0e)" % (cname, route, w, dr.VALUE_BOUND))
    assert w <= dr.VALUE_BOUND


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("cname", case_names("Y2_block_delay"))
def test_block_delay_fixture(cname, route, monkeypatch):
    from pypevoc_amd import delay
    g, case = get_case("Y2_block_delay", cname)
    src, tgt = case_signals(g, case)
    set_route(monkeypatch, route)
    lag, mx = delay.block_delay(src, tgt, window=case_window(case, len(src)))
    assert delay.last_kernels() == (FFT if route == "fft" else natural(len(src), len(tgt)))
    assert lag == int(g[cname + "_lag"]) and isinstance(mx, np.float64)
    r = restatement("Y2_block_delay", cname)[2]
    if r["scale"][0] == 0:
        assert mx == 0.0 and not np.signbit(mx)
        return
    w = abs(mx - float(g[cname + "_max"])) / r["scale"][0]
    print("%-20s %-8s against the reference: %.1e (bound %.0e)" % (cname, route, w, dr.VALUE_BOUND))
    assert w <= dr.VALUE_BOUND


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("cname", case_names("Y3_determine_delay"))
def test_determine_delay_fixture(cname, route, monkeypatch):
    from pypevoc_amd import delay
    g, case = get_case("Y3_determine_delay", cname)
    src, tgt = case_signals(g, case)
    set_route(monkeypatch, route)
    d = delay.determineDelay(src, tgt, maxdel=case["maxdel"])
    lx, ly = min(len(src), case["maxdel"]), min(len(tgt), case["maxdel"])
    assert delay.last_kernels() == (FFT if route == "fft" else natural(ly, lx))
    assert d == int(g[cname + "_delay"])
    # the two correlations themselves, every lag
    _, rx, ry = restatement("Y3_determine_delay", cname)
    check_blocks(cname + " source against source, " + route, delay.xcorr_peaks(src[:lx], src[:lx], lx, nblk=1, use_abs=True, full=True), rx)
    check_blocks(cname + " target against source, " + route, delay.xcorr_peaks(tgt[:ly], src[:lx], ly, lx, nblk=1, use_abs=True, full=True), ry)


# ---- seeded shapes against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("la,lv", SHAPES)
def test_shapes_on_both_routes(la, lv, monkeypatch):
    """Every configuration (detrend modes, windows on one signal, both, neither, use_abs on a negated signal, the three sample
    types) as 37 overlapping blocks and as one block, on the natural route and the forced FFT route; the two routes against
    each other; a block alone against the same block inside the call of 37 (bit for bit)."""
    from pypevoc_amd import delay
    for ci in range(len(CONFIGS)):
        c = shape_case(la, lv, ci)
        got = {}
        for route in ROUTES:
            set_route(monkeypatch, route)
            got[route] = delay.xcorr_peaks(c["a"], c["v"], full=True, **c["kw"])
            assert delay.last_kernels() == (FFT if route == "fft" else natural(la, lv))
            check_blocks("%d x %d config %d %s" % (la, lv, ci, route), got[route], c["ref"])
            one = delay.xcorr_peaks(c["a"], c["v"], full=True, **dict(c["kw"], nblk=1))
            assert same_bits(one, [x[:1] for x in got[route]]), (la, lv, ci, route)
            last = dict(c["kw"], nblk=1, start=(c["kw"]["nblk"] - 1) * c["kw"]["delta"])
            assert same_bits(delay.xcorr_peaks(c["a"], c["v"], full=True, **last), [x[-1:] for x in got[route]]), (la, lv, ci, route)
        # route agreement: same lags, values within the bound
        scale = c["ref"]["scale"]
        live = scale > 0
        assert np.array_equal(got["natural"][0], got["fft"][0])
        assert np.all(np.abs(got["natural"][2] - got["fft"][2])[live] <= dr.VALUE_BOUND * scale[live][:, None])
        assert same_bits(delay.xcorr_peaks(c["a"], c["v"], **c["kw"]), got["fft"][:2])                        # full or not: the same peaks


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("la,lv", [(1, 1), (2, 2), (64, 64), (512, 512), (513, 513), (2048, 2048), (2049, 2049), (700, 300), (300, 700), (1, 400), (3000, 5)])
def test_peaks_at_the_ends(la, lv, route, monkeypatch):
    """An impulse at the last sample of a and the first of v gives lag la + lv - 2, the mirrored pair lag 0: a circular wrap or an
    off-by-one in the padding shows here and nowhere else."""
    from pypevoc_amd import delay
    set_route(monkeypatch, route)
    for dtype in (np.float32, np.int16):
        a, v = np.zeros(la, dtype=dtype), np.zeros(lv, dtype=dtype)
        a[-1], v[0] = 3, 2
        lag, peak, corr = delay.xcorr_peaks(a, v, la, lv, full=True)
        assert delay.last_kernels() == (FFT if route == "fft" else natural(la, lv))
        assert lag[0] == la + lv - 2 and abs(peak[0] - 6.0) <= dr.VALUE_BOUND * 6 and np.all(np.abs(corr[0, :-1]) <= dr.VALUE_BOUND * 6)
        lag, peak, corr = delay.xcorr_peaks(a[::-1].copy(), v[::-1].copy(), la, lv, full=True)
        assert lag[0] == 0 and abs(peak[0] - 6.0) <= dr.VALUE_BOUND * 6 and np.all(np.abs(corr[0, 1:]) <= dr.VALUE_BOUND * 6)
        # the negated pair needs the abs; without it the winner is a zero (direct) or rounding noise (FFT): only the abs is pinned
        lag, peak = delay.xcorr_peaks(-a, v, la, lv, use_abs=True)
        assert lag[0] == la + lv - 2 and abs(peak[0] + 6.0) <= dr.VALUE_BOUND * 6


def test_silent_blocks_are_lag_zero_and_exactly_zero(monkeypatch):
    from pypevoc_amd import delay
    x = np.random.default_rng(5).standard_normal(3000).astype(np.float32)
    z = np.zeros(3000, dtype=np.float32)
    five = np.full(3000, 5, dtype=np.int16)                           # an exactly representable mean: silent once detrended
    for route in ROUTES:
        set_route(monkeypatch, route)
        for a, v, detrend in ((z, x, "none"), (x, z, "linear"), (z, z, "constant"), (five, five, "constant"), (five, five, "linear")):
            for la in (300, 2500):
                lag, peak, corr = delay.xcorr_peaks(a, v, la, nblk=1, detrend=detrend, full=True, use_abs=True)
                assert lag[0] == 0 and peak[0] == 0.0 and not np.signbit(peak[0]) and not corr.any(), (route, detrend, la)


# ---- bit identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("la,lv,ci", [(300, 300, 2), (2049, 2049, 1), (700, 300, 5), (513, 513, 0)])
def test_device_resident_and_chunked_input_are_bit_identical(la, lv, ci, monkeypatch):
    import torch
    from pypevoc_amd import delay
    c = shape_case(la, lv, ci)
    for route in ROUTES:
        set_route(monkeypatch, route)
        got = delay.xcorr_peaks(c["a"], c["v"], full=True, **c["kw"])
        kernels = delay.last_kernels()
        da, dv = (torch.from_numpy(np.array(x)).cuda() for x in (c["a"], c["v"]))
        assert str(da.dtype) == "torch." + CONFIGS[ci][4]
        assert same_bits(delay.xcorr_peaks(da, dv, full=True, **c["kw"]), got) and delay.last_kernels() == kernels
        for limit in (40000, 64, 1 << 19):                            # a few blocks, ONE block, many blocks per batch and chunk
            monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(limit))
            assert same_bits(delay.xcorr_peaks(c["a"], c["v"], full=True, **c["kw"]), got), (route, limit)
            assert same_bits(delay.xcorr_peaks(da, dv, full=True, **c["kw"]), got), (route, limit)
            assert delay.last_kernels() == kernels
        monkeypatch.delenv("PVX_MAX_DEVICE_BYTES")


def test_public_functions_take_device_tensors(monkeypatch):
    import torch
    from pypevoc_amd import delay
    g, case = get_case("Y1_maxdelwind", "overlapping_start")
    src, tgt = case_signals(g, case)
    dsrc, dtgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    assert same_bits(delay.maxdelwind(dsrc, dtgt, **case["kw"]), delay.maxdelwind(src, tgt, **case["kw"]))
    assert delay.block_delay(dsrc[:300], dtgt[:300]) == delay.block_delay(src[:300], tgt[:300])
    assert delay.determineDelay(dsrc, dtgt[:3000], maxdel=4096) == delay.determineDelay(src, tgt[:3000], maxdel=4096)
    # int16 beside float32 goes through float64 on the host; on the device it is refused
    a = delay.maxdelwind(src, np.round(tgt * 1000).astype(np.int16), **case["kw"])
    b = delay.maxdelwind(src.astype(np.float64), np.round(tgt * 1000).astype(np.float64), **case["kw"])
    assert same_bits(a, b)
    with pytest.raises(TypeError):
        delay.maxdelwind(dsrc, dtgt.double(), **case["kw"])


# ---- large cases against the float64 FFT restatement ---------------------------------------------------------------------------
def big_pair(n, seed, delay, ramp=True):
    """A float32 noise source, and it delayed, through a short FIR, plus independent noise and (ramp) a slow ramp."""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(n).astype(np.float32)
    d = np.concatenate([np.zeros(delay), src.astype(np.float64)])[:n]
    tgt = np.convolve(d, [1.0, 0.5, 0.25, -0.2, 0.1])[:n] + 0.6 * rng.standard_normal(n) + (np.linspace(-1.0, 2.0, n) if ramp else 0.0)
    return src, tgt.astype(np.float32)


def test_maxdelwind_at_its_default_block_length():
    """44.1 kHz, blocks of 22050 samples (P = 65536): 3 blocks."""
    from pypevoc_amd import delay
    src, tgt = big_pair(44100 * 3 + 10000, 41, 123)
    kw = dict(rate=44100, delta_time=1., sample_duration=.5)
    want_d, want_s, want_t, r = dr.maxdelwind(src, tgt, fft=True, **kw)
    assert len(want_t) == 3 and dr.guard_holds(r)
    d, s, t = delay.maxdelwind(src, tgt, **kw)
    assert delay.last_kernels() == FFT
    assert np.array_equal(t, want_t) and np.array_equal(d, want_d) and np.all(d == 122 / 44100.0)
    w = float(np.max(np.abs(s - want_s) / r["scale"]))
    print("maxdelwind L = 22050: worst %.1e (bound %.0e)" % (w, dr.VALUE_BOUND))
    assert w <= dr.VALUE_BOUND


def test_determine_delay_at_its_default_maxdel():
    """maxdel = 2**16 on a 1.6 s pair at 44.1 kHz: P = 2**17."""
    from pypevoc_amd import delay
    src, tgt = big_pair(70560, 42, 4321, ramp=False)
    want, rx, ry = dr.determine_delay(src, -tgt, fft=True)
    assert dr.guard_holds(rx) and dr.guard_holds(ry) and want == 4321
    assert delay.determineDelay(src, -tgt) == want and delay.last_kernels() == FFT
    check_blocks("determineDelay maxdel 2**16, target against source", delay.xcorr_peaks(-tgt[:65536], src[:65536], 65536, nblk=1, use_abs=True, full=True), ry)


def test_primitive_at_p_2_to_the_18():
    from pypevoc_amd import delay
    src, tgt = big_pair(100000 + 777, 43, 999)
    kw = dict(la=100000, lv=100000, start=0, delta=777, nblk=2, detrend="linear")
    r = dr.xcorr_blocks(tgt, src, fft=True, **kw)
    assert np.all(r["lag"] == 99999 + 999)
    check_blocks("P = 2**18, 2 blocks", delay.xcorr_peaks(tgt, src, full=True, **kw), r)
    assert delay.last_kernels() == FFT


# ---- entry-point conventions -------------------------------------------------------------------------------------------------
def test_entry_point_conventions():
    from pypevoc_amd import _lib
    lib = _lib.load()
    _lib.init()
    x = np.random.default_rng(9).standard_normal(3000).astype(np.float32)
    lag, peak = np.full(8, -7, dtype=np.int32), np.full(8, -7.0)
    px = ctypes.c_void_p(x.ctypes.data)

    def call(na, nv, la, lv, start, delta, nblk, detrend=0, a=px, v=px):
        return lib.pvx_xcorr_peak(a, v, _lib.PVX_F32, na, nv, la, lv, start, delta, nblk, detrend, None, None, 0, lag.ctypes.data_as(_lib.c_int32_p),
                                  _lib.dptr(peak), None)
    assert call(3000, 3000, 500, 300, 100, 300, 5) == 5                # 100 + 4 * 300 + 500 = 1800 <= 3000
    assert lib.pvx_xcorr_last_kernels() == b"k_xcorr_direct" and np.all(lag[:5] >= 0) and np.all(lag[5:] == -7)
    assert call(1800, 1600, 500, 300, 100, 300, 5) == 5                # the exact boundary of both signals
    assert call(1799, 1600, 500, 300, 100, 300, 5) == _lib.PVX_ERR_SIZE
    assert call(1800, 1599, 500, 300, 100, 300, 5) == _lib.PVX_ERR_SIZE
    assert call(3000, 3000, 500, 300, 1301, 300, 5) == _lib.PVX_ERR_SIZE
    assert call(3000, 3000, 3000, 3000, 0, 0, 3) == 3 and lib.pvx_xcorr_last_kernels() == FFT.encode()        # delta = 0: one block three times
    assert lag[0] == lag[1] == lag[2] == 2999 and peak[0] == peak[1] == peak[2]
    lag[:], peak[:] = -7, -7.0
    assert call(3000, 3000, 500, 300, 100, 300, 0) == 0 and lib.pvx_xcorr_last_kernels() == b"" and np.all(lag == -7) and np.all(peak == -7.0)
    for bad in (dict(la=0), dict(lv=0), dict(delta=-1), dict(start=-1), dict(detrend=3), dict(detrend=-1), dict(nblk=-1)):
        kw = dict(dict(na=3000, nv=3000, la=500, lv=300, start=100, delta=300, nblk=5), **bad)
        assert call(**kw) == -2, bad                                  # PVX_ERR_INVALID
    assert call(3000, 3000, 500, 300, 100, 300, 5, a=None) == -2
    # beyond the length limit: PVX_ERR_UNSUPPORTED and no launch
    big = np.zeros((1 << 19) + 1, dtype=np.float32)
    pb = ctypes.c_void_p(big.ctypes.data)
    assert call(3000, 3000, 500, 300, 100, 300, 5) == 5 and lib.pvx_xcorr_last_kernels() != b""
    lag[:] = -7
    assert call(len(big), len(big), len(big), len(big), 0, 1, 1, a=pb, v=pb) == _lib.PVX_ERR_UNSUPPORTED
    assert lib.pvx_xcorr_last_kernels() == b"" and np.all(lag == -7)
    assert call(len(big), len(big), len(big) - 1, len(big), 0, 1, 1, a=pb, v=pb) == 1 and lag[0] == 0 and peak[0] == 0.0   # P = 2**20 works
