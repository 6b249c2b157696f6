"""k_fused_rev at nfft 2048 (fft mode 4): the candidates' phase -- the
interior fast path of the neighbour reads (no candidate within 5 bins of bin 0, of bin M - 1 or of the end of a 256-bin
quarter of the buffer) with the clamped reads as the other branch, ranking only when candidates outnumber npks, and the
long-list branches (more than 64 candidates; a negative threshold term with fewer candidates than npks).

Every case: nfft 2048, hop 512, float32 samples, signals of 12 .. 24 frames (a wave flushes, picks a previous spectrum up
and crosses the start of the signal), against oracle.pvoracle.analyze with the float32 tolerances of
tests/test_hip_parity.py for computed signals (assert_f32(absolute=False): identical peak sets; phase, frequency and
magnitude errors normalised by the frame's largest magnitude).  With the witness library the same input also runs fft
mode 1 (k_fused.hip).  At nfft 2048 mode 4 is another transform (pvx_fft4.h) with its own float32 rounding, so -- as in
test_fused_kernel_variants -- what is identical to mode 1 bit for bit is the selection (binno, and which slots hold a
peak); the values agree to |df| <= 2e-3 Hz.

Which branch a frame takes is decided by its candidate list, so the tests check with a float64 model of the scan
(`candidates`: interior maxima of |X|^2 whose score is above the threshold term, PeakFinder.py:60-70, 155-194) that an
input reaches the branch it is there for.  The salience radius of the analysis is fixed at 5 (PVAnalysis.py:177): no plan
or API setting reaches another one in the fused kernels, so rad = 5 is what is tested.
No test reads kernel assembly or timing."""
import ctypes
import os

import numpy as np
import pytest

from .parity import compare_analysis, pv_result

pytestmark = pytest.mark.gpu

SR, NFFT, HOP, M = 44100.0, 2048, 512, 1024


def nsamp(frames):
    return NFFT + HOP * frames


def tones(frames, bins_amps, phase=0.3):
    t = np.arange(nsamp(frames))
    x = np.zeros(len(t))
    for i, (b, a) in enumerate(bins_amps):
        x += a * np.cos(2 * np.pi * b * t / NFFT + phase * (i + 1))
    return x.astype(np.float32)


def candidates(oracle, x, thr=0.005):
    """Per frame: (candidate bins in ascending order, threshold term th) of the scan, from the oracle's float64 spectra."""
    x = np.asarray(x, dtype=np.float64)
    out = []
    for j in range(oracle.nframes(len(x), NFFT, HOP)):
        y = np.abs(oracle.stft_frame(x, j * HOP, NFFT)) ** 2
        minamp = np.sqrt(y.max()) * thr
        th = minamp * minamp - y.min() if minamp != 0.0 else 0.0
        k = np.arange(1, M - 1)
        c = (y[k - 1] < y[k]) & (y[k] >= y[k + 1]) & ((y[k] - y.min() > th) | (th < 0))
        out.append((k[c], th))
    return out


def interior(bins):
    """The kernel's test: every candidate on bins 6 .. 249 of its quarter."""
    q = np.asarray(bins, dtype=np.int64) & 255
    return bool(np.all((q >= 6) & (q <= 249)))


@pytest.fixture(scope="module")
def amd():
    import pypevoc_amd
    from pypevoc_amd import _lib
    _lib.init()
    return pypevoc_amd


def assert_f32(c):
    # tests/test_hip_parity.py: assert_f32(c, absolute=False)
    assert c["bad_peaks"] <= 1e-3 * max(c["ref_peaks"], 1), c
    assert c["ph_norm"] <= 2e-6 and c["realph_norm"] <= 2e-5 and c["f_norm"] <= 2e-5 and c["mag_norm"] <= 1e-6, c
    assert c["totalmag_rel"] <= 1e-6, c


def run(amd, x, K, thr=0.005, mode=None):
    from pypevoc_amd import _lib
    if mode is not None:
        os.environ["PVX_FFT_MODE"] = str(mode)
    try:
        p = amd.PV(x, SR, nfft=NFFT, hop=HOP, npks=K, pkthresh=thr, progress=False, precision=32)
        p.run_pv()
    finally:
        if mode is not None:
            del os.environ["PVX_FFT_MODE"]
    assert _lib.load().pvx_plan_get_fft_mode(p._plan.handle) == (4 if mode is None else mode)
    return p


def check(amd, oracle, x, K, thr=0.005):
    """Mode 4 against the oracle and, the selection bit for bit, against mode 1 (the `witness` fixture has loaded that library)."""
    assert x.dtype == np.float32 and 12 <= oracle.nframes(len(x), NFFT, HOP) <= 24
    o = oracle.analyze(x.astype(np.float64), SR, NFFT, HOP, K, thr)
    p = run(amd, x, K, thr)
    assert p.nframes == len(o["t"])
    assert_f32(compare_analysis(pv_result(p), o, NFFT, HOP, SR))
    w = run(amd, x, K, thr, mode=1)
    assert np.array_equal(p.binno, w.binno) and np.array_equal(p.f > 0, w.f > 0)
    assert np.abs(p.f - w.f).max() <= 2e-3
    return p, o


# ------------------------------------------------------------------ edge peaks: the clamped branch
EDGE_BINS = [1, 2, 5, 6, M - 6, M - 5, M - 2, M - 1]
INTERIOR_TONES = [(100.3, 0.5), (300.0, 0.25), (700.6, 0.4)]      # candidates on bins 100, 300 and 701


@pytest.mark.parametrize("mixed", [False, True], ids=["alone", "mixed"])
@pytest.mark.parametrize("edge", EDGE_BINS)
def test_tones_at_the_ends_of_the_spectrum(amd, oracle, witness, edge, mixed):
    """A pure tone centred on bin 1, 2, 5, 6, M - 6, M - 5, M - 2 or M - 1, alone and beside interior tones: a candidate whose
    salience window or 3-bin energy is cut by the spectrum's end sends the whole frame through the clamped reads, the frame's
    interior tones included.  (Bin M - 1 is no interior bin: a tone there is nobody's candidate, and bin 6 is the first
    that leaves a frame on the fast path.)"""
    x = tones(16, [(float(edge), 0.3)] + (INTERIOR_TONES if mixed else []))
    want = ([] if edge == M - 1 else [edge]) + ([100, 300, 701] if mixed else [])
    for b, _ in candidates(oracle, x):
        assert sorted(b) == sorted(want)
    assert interior(want) == (edge in (6, M - 1))
    p, o = check(amd, oracle, x, 8)
    if mixed:
        assert ((o["f"] > 0).sum(axis=1) >= 3).all()


def test_tones_beside_a_quarter_boundary(amd, oracle, witness):
    """The buffer keeps the spectrum in four quarters of 256 bins, 16 slots apart: a candidate within 5 bins of a quarter's end
    has neighbours in two quarters and takes the clamped reads, an index at a time; the frames of the second half of the
    signal hold the interior tones only."""
    half = nsamp(16) // 2
    x = tones(16, INTERIOR_TONES)
    t = np.arange(nsamp(16))
    for b, a in ((250.0, 0.3), (255.4, 0.2), (256.0, 0.35), (261.0, 0.15), (511.3, 0.3), (767.0, 0.2), (773.0, 0.3)):
        x[:half] += (a * np.cos(2 * np.pi * b * t[:half] / NFFT)).astype(np.float32)
    cand = candidates(oracle, x)
    assert not any(interior(b) for b, _ in cand[:9]) and all(interior(b) for b, _ in cand[-5:])
    assert {250, 256, 261, 767, 773} <= set(cand[2][0])
    check(amd, oracle, x, 8)
    check(amd, oracle, x, 20)


# the bound of the interior test itself.  A weak tone centred on bin w (Hann: bins w - 1 .. w + 1 and nothing else) next to a
# quarter's end, and a strong tone s on the other side of it whose peak bin IS interior, so that the weak tone is the frame's only
# candidate that can leave the fast path.  The strong tone's side lobes rise monotonically towards it; the weak tone's level is set
# between the strong tone's |X| on bin d = w +- 5 (the outermost bin of the weak candidate's salience window) and on the bin before
# it, so the salience verdict of the weak candidate hangs on bin d alone.  Where d lies across the quarter's end (q = 251, q = 4)
# a fast path that admitted the frame would read the padding between the quarters instead of bin d; where it does not (q = 249,
# q = 6: the last bins the test admits) the fast path's outermost read is what decides.
BOUND_CASES = [(qb + w, qb + s) for qb in (256, 512, 768) for w, s in ((-5, 6.4), (-7, 6.4), (4, -6.6), (6, -6.6))]


@pytest.mark.parametrize("w,s", BOUND_CASES, ids=lambda v: str(v))
def test_salience_window_across_a_quarter_boundary(amd, oracle, witness, w, s):
    up = s > w
    d = w + 5 if up else w - 5
    strong = tones(16, [(s, 1.0)])
    ys = np.abs(oracle.stft_frame(strong.astype(np.float64), 4 * HOP, NFFT))
    level = np.sqrt(ys[d] * ys[d - 1 if up else d + 1])              # between the decisive bin and the one before it
    unit = np.abs(oracle.stft_frame(tones(16, [(float(w), 1.0)]).astype(np.float64), 4 * HOP, NFFT))[w]
    x = (strong + tones(16, [(float(w), level / unit)])).astype(np.float32)
    thr = 0.2 * level / ys.max()                                     # the weak tone is a candidate, the far side lobes are not
    decisive = []                                                    # frames whose verdict on bin w hangs on bin d alone
    cand = candidates(oracle, x, thr)
    assert interior([w]) == ((w & 255) in (249, 6))
    for j in range(len(cand)):
        y = np.abs(oracle.stft_frame(x.astype(np.float64), j * HOP, NFFT))
        lo, hi = (w - 5, d - 1) if up else (d + 1, w + 5)
        others = np.delete(y[lo:hi + 1], w - lo)
        b = cand[j][0]
        if w in b and interior([c for c in b if c != w]) and y[d] > 1.05 * y[w] and y[w] > 1.05 * others.max():
            decisive.append(j)
    assert len(decisive) >= 4, decisive
    p, o = check(amd, oracle, x, 8, thr)
    assert all(w not in o["binno"][j] for j in decisive)             # ... and there the weak tone is not salient


# ------------------------------------------------------------------ candidate counts around the limits
def _count_signal(ntones):
    """ntones steady tones of distinct levels, all above a threshold of 0.1 of the maximum (and their Hann side lobes, -31 dB,
    below it), with two silent stretches: frames 5, 6 and 14 have no candidate at all."""
    x = tones(20, [(60.25 + 83.0 * i, 1.0 - 0.04 * i) for i in range(ntones)])
    x[HOP * 5: HOP * 5 + NFFT + HOP] = 0.0
    x[HOP * 14: HOP * 14 + NFFT] = 0.0
    return x


@pytest.mark.parametrize("K", [8, 1, 20])
@pytest.mark.parametrize("ntones", [1, 8, 9])
def test_few_candidates(amd, oracle, witness, ntones, K):
    """npks 8 with 0 candidates (silent frames between bursts), 1, exactly 8 (nothing is cut: no ranking, bins ascending) and 9
    (one is cut: ranking); npks 1; npks 20 (the dense staging's instantiation)."""
    x = _count_signal(ntones)
    counts = [len(b) for b, _ in candidates(oracle, x, 0.1)]
    assert [counts[j] for j in (5, 6, 14)] == [0, 0, 0] and [counts[j] for j in (0, 10, 19)] == [ntones] * 3
    p, o = check(amd, oracle, x, K, 0.1)
    assert (p.f[5] == 0).all() and (p.f[14] == 0).all()
    assert (o["f"][10] > 0).sum() == min(ntones, K)
    assert np.all(np.diff(p.binno[10][p.f[10] > 0]) > 0)             # a frame's peaks leave in ascending bin order


# white noise, threshold 0.55 of the maximum: the first seed of 0 .. 199 whose 16 frames hold, by `candidates`, 63 and 64
# candidates (one per lane, ranking) and 65 (the long-list branch); the frames around them hold 10 .. 137
NOISE_SEED, NOISE_THR = 132, 0.55


def _noise(seed):
    return (0.1 * np.random.default_rng(seed).standard_normal(nsamp(16))).astype(np.float32)


@pytest.mark.parametrize("K", [8, 20, 64])
def test_candidate_counts_around_64(amd, oracle, witness, K):
    x = _noise(NOISE_SEED)
    counts = [len(b) for b, _ in candidates(oracle, x, NOISE_THR)]
    assert {63, 64, 65} <= set(counts) and min(counts) < 16 and max(counts) > 96, counts
    check(amd, oracle, x, K, NOISE_THR)


# ------------------------------------------------------------------ equal magnitudes
def test_equal_magnitudes_keep_their_order(amd, oracle, witness):
    """Two tones of the same amplitude, mirrored about the middle of the spectrum (0.2 bins above bin 200, 0.2 below bin M - 200): with npks 8 and 2 + 5 candidates nothing is cut
    and no ranking runs; with npks 4 the ranking meets the two equal scores at the top, well above the cut.  Both ways
    the frame's peaks leave in ascending bin order with both tones among them."""
    x = tones(16, [(200.2, 0.5), (M - 200.2, 0.5)] + [(330.3 + 57 * i, 0.2 - 0.03 * i) for i in range(5)])
    for b, _ in candidates(oracle, x, 0.05):
        assert len(b) == 7 and {200, M - 200} <= set(b) and interior(b)
    for K in (8, 4):
        p, o = check(amd, oracle, x, K, 0.05)
        for j in range(p.nframes):
            kept = p.binno[j][p.f[j] > 0]
            assert len(kept) == min(K, 7) and {200, M - 200} <= set(kept) and np.all(np.diff(kept) > 0)


# ------------------------------------------------------------------ th < 0 and fewer candidates than npks
def test_flat_spectrum_with_fewer_candidates_than_npks(amd, oracle, witness):
    """Two unequal clicks d samples apart: |X|^2 ripples between (a - b)^2 and (a + b)^2 with d / 2 maxima, so its minimum
    exceeds the threshold term (th < 0) and there are fewer candidates than npks: the frames that see the clicks leave the
    one-candidate-per-lane branch.  The tone that follows brings ordinary frames into the same wave's range."""
    x = tones(16, [(90.4, 0.3)])
    x[: HOP * 9] = 0.0
    x[3000], x[3006] = 1.0, 0.6
    cand = candidates(oracle, x)
    flat = [j for j, (b, th) in enumerate(cand) if th < 0]
    assert len(flat) == 4 and all(0 < len(cand[j][0]) < 8 for j in flat)
    assert any(th > 0 and len(b) > 0 for b, th in cand)
    check(amd, oracle, x, 8)
    x[3010] = 0.5                                                    # (a third click: another ripple, still flat)
    assert sum(th < 0 for _, th in candidates(oracle, x)) == 4
    check(amd, oracle, x, 8)


# ------------------------------------------------------------------ a batch: zero row inside a wave's range, wire formats
@pytest.mark.parametrize("blocks", [None, "1"], ids=["grid", "one_workgroup"])
def test_batch_and_wire_formats(amd, oracle, monkeypatch, blocks):
    """Two signals of 20 frames in one call: 42 rows, row 21 the zero row of the second signal -- with one workgroup of twelve
    waves (PVX_FUSED_BLOCKS=1) inside the range of the wave that walks rows 22 .. 19.  Signal 0 has edge, quarter-boundary and
    interior candidates and silent frames; signal 1 is noise around 64 candidates.  The plain output against the oracle,
    signal by signal; the wire blocks the kernel writes itself (pvx_analyze_dev_wire, formats 1 and 2) decode to the plain
    output bit for bit."""
    import torch
    from pypevoc_amd import _lib
    from pypevoc_amd.batch import ResultWire
    lib = _lib.load()
    if blocks:
        monkeypatch.setenv("PVX_FUSED_BLOCKS", blocks)
    F, K = 20, 8
    x0 = tones(F, [(2.0, 0.45), (255.0, 0.44), (100.3, 0.5), (700.6, 0.48)])
    x0[HOP * 7: HOP * 7 + NFFT + HOP] = 0.0
    c0 = [list(b) for b, _ in candidates(oracle, x0, NOISE_THR)]
    assert c0.count([2, 100, 255, 701]) >= 12 and [] in c0
    x1 = (0.1 * np.random.default_rng(NOISE_SEED).standard_normal(nsamp(F))).astype(np.float32)
    xb = np.stack([x0, x1])
    thr = NOISE_THR
    counts = [len(b) for b, _ in candidates(oracle, x1, thr)]
    assert min(counts) < 64 < max(counts)
    dev = torch.device("cuda", 0)
    dx = torch.from_numpy(xb).to(dev)
    plan = ctypes.c_void_p()
    _lib.check(lib.pvx_plan_create(ctypes.byref(plan), SR, NFFT, HOP, K, thr, _lib.dptr(np.hanning(NFFT)), 32, 0), "pvx_plan_create")
    try:
        assert lib.pvx_plan_get_fft_mode(plan) == 4 and int(lib.pvx_nframes(xb.shape[1], NFFT, HOP)) == F
        rows = 2 * F
        n = rows * K
        wire = ResultWire(plan, rows, K)
        res = torch.zeros(wire.result_numel() + rows, dtype=torch.float64, device=dev)
        rp = wire.result_ptrs(res.data_ptr())
        _lib.check(lib.pvx_analyze_dev(plan, dx.data_ptr(), _lib.PVX_F32, xb.shape[1], 2, xb.shape[1], rp[0], rp[1], rp[2], rp[3], rp[4],
                                       res.data_ptr() + wire.result_numel() * 8, rp[5], None, None), "pvx_analyze_dev")
        torch.cuda.synchronize()
        plain = res[: wire.result_numel()].cpu().numpy()
        arr = {k: plain[i * n:(i + 1) * n].reshape(2, F, K) for i, k in enumerate(("f", "mag", "ph", "realph", "binno"))}
        tm = plain[5 * n:].reshape(2, F)
        for b in range(2):
            o = oracle.analyze(xb[b].astype(np.float64), SR, NFFT, HOP, K, thr)
            got = dict({k: v[b] for k, v in arr.items()}, totalmag=tm[b])
            assert_f32(compare_analysis(got, o, NFFT, HOP, SR))
        assert (arr["f"][0] > 0).sum() > F and (arr["f"][1] > 0).sum() > F
        for fmt in (1, 2):
            _lib.check(lib.pvx_plan_set_wire_format(plan, fmt), "pvx_plan_set_wire_format")
            wf = ResultWire(plan, rows, K)
            w = torch.full((wf.nbytes,), 0xAB, dtype=torch.uint8, device=dev)
            r = lib.pvx_analyze_dev_wire(plan, dx.data_ptr(), _lib.PVX_F32, xb.shape[1], 2, xb.shape[1], w.data_ptr(), None)
            assert r == F, (r, lib.pvx_last_error())
            out = torch.full((wf.result_numel(),), np.nan, dtype=torch.float64, device=dev)
            wf.unpack(w.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.int64), plain.view(np.int64)), fmt
    finally:
        lib.pvx_plan_destroy(plan)
