"""pypevoc_amd.TransferFunctions on the MI355X (k_xspec.hip) against the reference's outputs (tests/golden/X*.npz,
make_golden_transfer.py).

Bounds (TRANSFER.md), from the project's 1e-9 relative per spectrum bin: psd 1e-9 relative per bin; csd 2e-9 sqrt(Pxx Pyy)
absolute (modulus of the complex difference); tfe 3e-9 sqrt(Pyy / Pxx) absolute, Pxx the denominator's spectrum; coherence 6e-9
absolute; fused against rows the same.  The scales come from numpy on the fixture's signals; no block, bin or case is left out;
the reference's nan is a nan at the same place and its exact zeros exact zeros.  Run with -s for the worst measured values."""
import ctypes

import numpy as np
import pytest

from .test_transfer_cpu import (BOUND, all_cases, case_kwargs, case_signals, compare, fixture_result, get_case, np_block, np_density,
                                restatement, worst)

pytestmark = pytest.mark.gpu

ROWS = "k_frames+rocfft+k_xspec_rows"
FUSED = (512, 1024, 2048)


def expected_kernels(nfft):
    return "k_xspec_fused<%d>" % nfft if nfft in FUSED else ROWS


def run(name, cname, signals=None):
    """The case through the public function (signals: the host arrays of the fixture unless given)."""
    from pypevoc_amd import TransferFunctions as tf
    g, case = get_case(name, cname)
    x, y = case_signals(g, case) if signals is None else signals
    kw = case_kwargs(g, case)
    if case["func"] == "transferogram":
        return tf.transferogram(x, y, **kw)
    if case["func"] == "psd":
        return tf.psd(x, **kw)
    return getattr(tf, case["func"])(x, y, **kw)


def within(name, cname, got, want, what):
    d = compare(name, cname, got, want)
    print("%-24s %-22s " % (cname, what) + "  ".join("%s %.1e (bound %.0e)" % (k, v, BOUND[k]) for k, v in sorted(d.items())))
    assert d and all(v <= BOUND[k] for k, v in d.items()), (cname, what, d)


def same_bits(a, b):
    return len(a) == len(b) and all(p.tobytes() == q.tobytes() and p.shape == q.shape for p, q in zip(a, b))


def fits_the_device(name, cname):
    """A device-resident signal is read in place: the cases whose signals or blocks mlab zero-pads need host arrays."""
    g, case = get_case(name, cname)
    nfft = restatement(name, cname)["nfft"]
    if case["func"] == "transferogram":
        return int(case["kw"]["sample_duration"] * case["kw"]["rate"]) >= nfft
    return len(case_signals(g, case)[0]) >= nfft


@pytest.mark.parametrize("name,cname", all_cases())
def test_fixture_case(name, cname, monkeypatch):
    """Every case through the public functions on its documented route; the fused windows once more down the rows route."""
    from pypevoc_amd import TransferFunctions as tf
    nfft = restatement(name, cname)["nfft"]
    ref = fixture_result(name, cname)
    got = run(name, cname)
    assert tf.last_kernels() == expected_kernels(nfft)
    assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(got, ref)), [(a.shape, a.dtype) for a in got]
    within(name, cname, got, ref, "against the reference")
    if nfft in FUSED:
        monkeypatch.setenv("PVX_XSPEC_ROWS", "1")
        rows = run(name, cname)
        assert tf.last_kernels() == ROWS
        monkeypatch.delenv("PVX_XSPEC_ROWS")
        within(name, cname, rows, ref, "rows against the reference")
        within(name, cname, rows, got, "rows against fused")


@pytest.mark.parametrize("name,cname", all_cases(raising=True))
def test_reference_exceptions(name, cname):
    _, case = get_case(name, cname)
    with pytest.raises({"ValueError": ValueError}[case["raises"]]):
        run(name, cname)


@pytest.mark.parametrize("name,cname", all_cases())
def test_device_resident_and_chunked_input_are_bit_identical(name, cname, monkeypatch):
    import torch
    from pypevoc_amd import TransferFunctions as tf
    g, case = get_case(name, cname)
    x, y = case_signals(g, case)
    got = run(name, cname)
    route = tf.last_kernels()
    if fits_the_device(name, cname):
        dev = [None if s is None else torch.from_numpy(np.ascontiguousarray(s)).cuda() for s in (x, y)]
        assert str(dev[0].dtype) == "torch." + case["dtype"]
        assert same_bits(run(name, cname, dev), got) and tf.last_kernels() == route
    else:
        with pytest.raises(ValueError, match="zero-padded by the caller"):
            run(name, cname, [None if s is None else torch.from_numpy(np.ascontiguousarray(s)).cuda() for s in (x, y)])
    for limit in (40000, 64, 1 << 19):                                # a few blocks, ONE block, many blocks per chunk
        monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(limit))
        assert same_bits(run(name, cname), got), limit
        assert tf.last_kernels() == route
    monkeypatch.delenv("PVX_MAX_DEVICE_BYTES")


def test_window_hop_none_is_half_a_window():
    from pypevoc_amd import TransferFunctions as tf
    g, case = get_case("X1_fused", "t512_f64_half")
    x, y = case_signals(g, case)
    kw = dict(case["kw"])
    assert kw.pop("window_hop") * kw["rate"] * 2 == 512
    assert same_bits(tf.transferogram(x, y, **kw), run("X1_fused", "t512_f64_half"))


def test_mixed_sample_types_and_callers_conventions():
    """int16 beside float32 goes through float64; tfe's positional arguments are csd's; a block's bits do not depend on its
    neighbours (another grid, another position in the call)."""
    from pypevoc_amd import TransferFunctions as tf
    g, case = get_case("X3_rows", "t512_int16")
    x, y = case_signals(g, case)
    a = tf.transferogram(x, y.astype(np.float32), **case["kw"])
    b = tf.transferogram(x.astype(np.float64), y.astype(np.float64), **case["kw"])
    assert same_bits(a, b)
    g, case = get_case("X4_mlab", "tfe333")
    yy, xx = case_signals(g, case)
    assert same_bits(tf.tfe(yy, xx, 333, 8000, None, None, 100), tf.tfe(yy, xx, NFFT=333, Fs=8000, noverlap=100))
    for name, cname in (("X1_fused", "t512"), ("X3_rows", "t256")):
        g, case = get_case(name, cname)
        src, tgt = case_signals(g, case)
        kw = case["kw"]
        full = tf.transferogram(src, tgt, **kw)
        slen, delta = int(kw["sample_duration"] * kw["rate"]), int(kw["delta_time"] * kw["rate"])
        for b in (0, 5, full[0].shape[1] - 1):
            one = tf.transferogram(src[b * delta: b * delta + slen + 1], tgt[b * delta: b * delta + slen + 1], **kw)
            assert one[0].shape[1] == 1 and one[0][:, 0].tobytes() == np.ascontiguousarray(full[0][:, b]).tobytes(), (cname, b)
            assert one[3][:, 0].tobytes() == np.ascontiguousarray(full[3][:, b]).tobytes()


def test_tfe_sig_against_its_formula():
    """scipy's conventions with detrend=False: periodic Hann window, nperseg 256, hop 128; the ratio needs no scaling."""
    from pypevoc_amd import TransferFunctions as tf
    g, case = get_case("X4_mlab", "tfe333")
    y, x = case_signals(g, case)
    got, f = tf.tfe_sig(y, x, fs=8000, detrend=False)
    wind = np.hanning(257)[:-1]
    sxy, sxx, syy = np_block(x, y, 256, 128, wind)
    assert np.array_equal(f, np.fft.rfftfreq(256, 1 / 8000))
    w = worst(got, sxy / sxx, np.sqrt(syy / sxx))
    print("tfe_sig %.1e (bound %.0e)" % (w, BOUND["tfe"]))
    assert w <= BOUND["tfe"]


def big_pair(n, seed):
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(n).astype(np.float32)
    tgt = (np.convolve(src.astype(np.float64), [1.0, 0.5, 0.25, -0.2, 0.1])[:n] + 0.6 * rng.standard_normal(n)).astype(np.float32)
    return src, tgt


def test_large_call_crosses_workspace_batches(monkeypatch):
    """nwind 256, step 64, blocks of 512 samples every 8 over 150 000 samples: about 18 700 blocks of 5 segments, 14 rocFFT batches
    of whole blocks of both signals; too large for a fixture, so against the numpy restatement; the same bits chunked."""
    from pypevoc_amd import TransferFunctions as tf
    src, tgt = big_pair(150000, 21)
    kw = dict(rate=1, delta_time=8, sample_duration=512, window_duration=256, window_hop=64)
    resp, freq, times, coh = tf.transferogram(src, tgt, **kw)
    assert tf.last_kernels() == ROWS
    nblk = len(np.arange(0, 150000 - 512, 8))
    assert resp.shape == coh.shape == (129, nblk) and nblk > 18600 and nblk * 6 * 2 > 13 * (32 << 20) // (256 * 8)
    wind = np.hanning(256)
    # segment s of block b starts at 8 b + 64 s = 8 (b + 8 s): every distinct frame is transformed once
    frames = (np.arange(nblk + 32) * 8)[:, None] + np.arange(256)[None, :]
    pick = np.arange(nblk)[:, None] + 8 * np.arange(5)[None, :]
    X = np.fft.rfft(src.astype(np.float64)[frames] * wind, axis=1)[pick]
    Y = np.fft.rfft(tgt.astype(np.float64)[frames] * wind, axis=1)[pick]
    pxy, pxx, pyy = (np_density(s, 256, 1, wind).T for s in ((np.conj(Y) * X).mean(axis=1), (np.abs(X)**2).mean(axis=1), (np.abs(Y)**2).mean(axis=1)))
    assert np.all(pxx > 0) and np.all(pyy > 0)
    d = dict(tfe=worst(resp, pxy / pxx, np.sqrt(pyy / pxx)), coh=worst(coh, np.abs(pxy)**2 / (pxx * pyy), np.ones(pxx.shape)))
    print("large call: " + "  ".join("%s %.1e (bound %.0e)" % (k, v, BOUND[k]) for k, v in d.items()))
    assert all(v <= BOUND[k] for k, v in d.items()), d
    assert np.array_equal(times, (np.arange(nblk) * 8 + 256.0) / 1.0)
    monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(1 << 20))
    again = tf.transferogram(src, tgt, **kw)
    monkeypatch.delenv("PVX_MAX_DEVICE_BYTES")
    assert same_bits(again, (resp, freq, times, coh))


@pytest.mark.parametrize("nfft,noverlap,n", [(4096, 3584, 4096 + 599 * 512), (1024, 1023, 1024 + 2999)])
def test_one_block_of_many_segments(nfft, noverlap, n, monkeypatch):
    """tfe over a whole signal is one block: 600 segments of 4096 do not fit a rocFFT batch of both signals (the block is cut
    between segments and carries its sums), 3000 of 1024 run on one wave of the fused kernel and, forced, as rows."""
    from pypevoc_amd import TransferFunctions as tf
    src, tgt = big_pair(n, nfft)
    wind = np.hanning(nfft)
    sxy, sxx, syy = np_block(src, tgt, nfft, nfft - noverlap, wind)
    want = sxy / sxx
    for rows in ((False, True) if nfft in FUSED else (False,)):
        if rows:
            monkeypatch.setenv("PVX_XSPEC_ROWS", "1")
        got, f = tf.tfe(tgt, src, NFFT=nfft, Fs=2, noverlap=noverlap)
        assert tf.last_kernels() == (ROWS if rows else expected_kernels(nfft))
        w = worst(got, want, np.sqrt(syy / sxx))
        print("tfe of one block, NFFT %d, %d segments%s: %.1e (bound %.0e)" % (nfft, (n - nfft) // (nfft - noverlap) + 1, ", rows" if rows else "", w, BOUND["tfe"]))
        assert w <= BOUND["tfe"]
        c, _ = tf.cohere(tgt, src, NFFT=nfft, Fs=2, noverlap=noverlap)
        assert worst(c, np.abs(sxy)**2 / (sxx * syy), np.ones(len(sxx))) <= BOUND["coh"]
    monkeypatch.delenv("PVX_XSPEC_ROWS", raising=False)


# ---- edges -----------------------------------------------------------------------------------------------------------------
def test_no_block_shapes_and_kinds():
    from pypevoc_amd import TransferFunctions as tf
    x = np.ones(100, dtype=np.float32)
    resp, freq, times, coh = tf.transferogram(x, x, rate=8000)
    assert resp.shape == (257, 0) and resp.dtype == np.complex128 and coh.shape == (257, 0) and times.shape == (0,) and len(freq) == 257
    resp, freq, times, coh = tf.transferogram(x, None, rate=8000)
    assert resp.shape == (257, 0) and resp.dtype == np.float64 and coh.shape == (0, 0)


def test_silent_signals():
    from pypevoc_amd import TransferFunctions as tf
    for nfft in (512, 333):
        z = np.zeros(4000, dtype=np.float32)
        x = np.random.default_rng(nfft).standard_normal(4000).astype(np.float32)
        t, _ = tf.tfe(z, x, NFFT=nfft)
        assert np.all(t == 0) and t.dtype == np.complex128
        assert np.isnan(tf.tfe(x, z, NFFT=nfft)[0]).all() and np.isnan(tf.cohere(x, z, NFFT=nfft)[0]).all()
        assert np.all(tf.psd(z, NFFT=nfft)[0] == 0)


def test_blocks_beyond_the_signals_are_refused():
    from pypevoc_amd import _lib
    lib = _lib.load()
    _lib.init()
    x = np.zeros(3000, dtype=np.float32)
    wind = np.hanning(512)
    sxy, sxx, syy = np.zeros(2 * 8 * 257), np.zeros(8 * 257), np.zeros(8 * 257)
    px = ctypes.c_void_p(x.ctypes.data)
    args = lambda n, start, nblk, nseg, two=True: (px, px if two else None, _lib.PVX_F32, n, _lib.dptr(wind), 512, 256, start, 300, nblk, nseg,
                                                   _lib.dptr(sxy) if two else None, _lib.dptr(sxx), _lib.dptr(syy) if two else None)
    assert lib.pvx_xspec(*args(3000, 100, 5, 5)) == 5                 # 100 + 4 * 300 + 4 * 256 + 512 = 2836 <= 3000
    assert lib.pvx_xspec(*args(2836, 100, 5, 5)) == 5
    assert lib.pvx_xspec(*args(2835, 100, 5, 5)) == _lib.PVX_ERR_SIZE
    assert lib.pvx_xspec(*args(3000, 100, 6, 5)) == _lib.PVX_ERR_SIZE
    assert lib.pvx_xspec(*args(3000, 100, 5, 6)) == _lib.PVX_ERR_SIZE
    assert lib.pvx_xspec(*args(3000, 265, 5, 5)) == _lib.PVX_ERR_SIZE
    assert lib.pvx_xspec(*args(3000, 100, 5, 5, two=False)) == 5
    assert lib.pvx_xspec(*args(3000, 100, 0, 5)) == 0 and lib.pvx_xspec_last_kernels() == b""
    assert lib.pvx_xspec(*args(3000, -1, 1, 1)) < 0 and lib.pvx_xspec(*args(3000, 0, 1, 0)) < 0
