"""The three segmenter stages' entry points (pvx_seg_detect, pvx_seg_refine, pvx_seg_transitions) on hand-built tables
against tests/segment_refs.py, at the shapes where k_segment.hip changes path: tile seams, chunk and accumulator
boundaries of the band sum, lanes with and without a fourth element, empty sides, every status.

Every table is built so that each choice rests on a difference of at least MARGIN dB, or on values that are the same
bits by construction (a repeated row, a repeated energy); the builders assert it, so a logarithm's last bits cannot flip a
choice and the discrete outputs must be equal everywhere.  A continuous output may differ from the float64 restatement by
eight times that restatement's own distance from its np.longdouble evaluation on the same table (SEGMENT.md: the
device's log10 may be a couple of ulp looser than the host's; its documented accuracy is not on the build machine, so the
second, analytic bound of the design is not used).  That distance is measured here on the CPU and never from the kernel.
A table on which it happens to be under a quarter of an ulp of the values says nothing about rounding: the builder draws
the next seed."""
import ctypes

import numpy as np
import pytest

from . import segment_refs as R

pytestmark = pytest.mark.gpu

MARGIN = 1e-6
EPS = np.finfo(np.float64).eps
LD = np.longdouble


def lib():
    from pypevoc_amd import _lib
    _lib.init()
    return _lib, _lib.load()


def i32p(a):
    from pypevoc_amd import _lib
    return a.ctypes.data_as(_lib.c_int32_p)


def energy(db):
    return 10.0 ** (np.asarray(db, dtype=np.float64) / 10.0)


def distance(a64, ald):
    """The largest |float64 - long double| over the finite entries, and the scale an ulp is taken at."""
    a64, ald = np.asarray(a64, dtype=np.float64), np.asarray(ald, dtype=LD)
    fin = np.isfinite(a64)
    assert np.array_equal(fin, np.isfinite(ald.astype(np.float64)))
    if not fin.any():
        return 0.0, 0.0
    return float(np.abs(a64[fin].astype(LD) - ald[fin]).max()), float(np.abs(a64[fin]).max())


def lucky(pairs):
    """True when some quantity's float64 evaluation sits within a quarter ulp of the long double one on the whole table."""
    return any(scale > 0 and d < 0.25 * EPS * scale for d, scale in (distance(a, b) for a, b in pairs))


def within(got, want64, wantld, what):
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want64)), what
    inf = np.isinf(want64)
    assert np.array_equal(got[inf], want64[inf]), what
    fin = np.isfinite(want64)
    d, _ = distance(want64, wantld)
    err = float(np.abs(got[fin] - want64[fin]).max()) if fin.any() else 0.0
    print("%s: max err %.3e, bound 8 x %.3e" % (what, err, d))
    assert err <= 8 * d, (what, err, d)


# ---- detect -------------------------------------------------------------------------------------------------------------
def det_table(steps, nband, rng, zero_rows=()):
    """Energies [len(steps) + 1][nband] whose detection function is about `steps` (dB, > 0): every band moves by steps[i] /
    nband from row i to row i + 1, up and down in turn.  steps[i] = None repeats row i - 1 in row i + 1 (the same bits), so
    det[i] == det[i - 1] exactly."""
    db = np.empty((len(steps) + 1, nband))
    db[0] = rng.uniform(-60.0, -20.0, nband)
    flat = []
    for i, s in enumerate(steps):
        if s is None:
            db[i + 1] = db[i - 1]
            flat.append(i)
        else:
            db[i + 1] = db[i] + (1 if i % 2 == 0 else -1) * s / nband
    spec = energy(db)
    for i, s in enumerate(steps):
        if s is None:
            spec[i + 1] = spec[i - 1]
    for r in zero_rows:
        spec[r] = 0.0
    return spec, set(flat)


def det_margins(spec, thresh, flat):
    det = R.detect(spec, thresh)[0]
    with np.errstate(invalid="ignore"):
        d = np.abs(np.diff(det))
    for i in range(len(d)):
        if np.isfinite(d[i]):
            assert d[i] >= MARGIN or (d[i] == 0.0 and (i + 1) in flat), (i, d[i])
    t = np.abs(det[np.isfinite(det)] - thresh)
    assert t.size == 0 or t.min() >= MARGIN


def run_detect(spec, thresh, maxseg, expect_size=False):
    L, lb = lib()
    spec = np.ascontiguousarray(spec, dtype=np.float64)
    nfr, nband = spec.shape
    det = np.full(max(nfr - 1, 1), -7.0)
    idx, fpos = np.full(max(maxseg, 1), -7, dtype=np.int32), np.full(max(maxseg, 1), -7.0)
    cnt = ctypes.c_int64(-1)
    rc = lb.pvx_seg_detect(L.dptr(spec), nfr, nband, float(thresh), maxseg, L.dptr(det), i32p(idx), L.dptr(fpos), ctypes.byref(cnt))
    if expect_size:
        assert rc == L.PVX_ERR_SIZE, rc
        k = maxseg
    else:
        assert rc == cnt.value >= 0, (rc, cnt.value)
        k = rc
    assert np.all(idx[k:] == -7) and np.all(fpos[k:] == -7.0)         # nothing beyond the count is written
    return det[:nfr - 1], idx[:k], fpos[:k], cnt.value


def check_detect(spec, thresh, flat, what):
    det_margins(spec, thresh, flat)
    det64, pk64, fp64 = R.detect(spec, thresh)
    detld, pkld, fpld = R.detect(spec, thresh, LD)
    assert np.array_equal(pk64, pkld)
    det, idx, fpos, cnt = run_detect(spec, thresh, max((len(det64) - 1) // 2, 0))
    assert cnt == len(pk64) and np.array_equal(idx, pk64), what
    within(det, det64, detld, what + " det")
    within(fpos, fp64, fpld, what + " fpos")
    return len(pk64)


def random_steps(nd, rng):
    """Steps in 0.5 .. 6 dB, neighbours at least 1e-3 apart."""
    s = rng.uniform(0.5, 6.0, nd)
    for i in range(1, nd):
        while abs(s[i] - s[i - 1]) < 1e-3 or abs(s[i] - 2.0) < 1e-3:
            s[i] = rng.uniform(0.5, 6.0)
    return list(s)


@pytest.mark.parametrize("nband", [1, 2, 5, 8, 9, 128])
def test_detect_sizes(nband):
    for nd in (1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4097):
        for seed in range(100):
            rng = np.random.default_rng(1000 * nband + nd + 100000 * seed)
            spec, flat = det_table(random_steps(nd, rng), nband, rng)
            d64, ld = R.detect(spec, 2.0), R.detect(spec, 2.0, LD)
            if not lucky([(d64[0], ld[0])] + ([(d64[2], ld[2])] if len(d64[1]) else [])):
                break
        n = check_detect(spec, 2.0, flat, "nd %d nband %d" % (nd, nband))
        assert nd < 63 or n > 0


def test_detect_flat_plateaus_seams_and_dense_peaks():
    rng = np.random.default_rng(7)
    # two rows in turn: the detection function is the same bits everywhere, no index is a peak
    spec, flat = det_table([3.0] + [None] * 1200, 5, rng)
    det, idx, fpos, cnt = run_detect(spec, 0.5, 600)
    assert cnt == 0 and len(set(det.tolist())) == 1 and det[0] > 2.9
    assert len(R.detect(spec, 0.5)[1]) == 0
    # plateaus beside rises: 1, 3, 3, 1 -- PeakFinder's rule (prev < cur >= next) would take the first 3
    steps = []
    for k in range(150):
        steps += [1.0 + 0.01 * k, 3.0 + 0.01 * k, None, 1.5 + 0.01 * k]
    spec, flat = det_table(steps, 4, rng)
    assert check_detect(spec, 0.5, flat, "plateaus") == 0
    # every other index a peak, at both parities: the seams of the 512-value tiles are crossed by peaks at 511, 512, 513
    for parity in (0, 1):
        steps = [(4.0 if i % 2 == parity else 1.0) + 1e-3 * (i % 7) for i in range(1100)]
        spec, flat = det_table(steps, 3, rng)
        n = check_detect(spec, 2.0, flat, "dense parity %d" % parity)
        assert n == len([i for i in range(1, 1099) if i % 2 == parity])
    # single peaks exactly at the seams
    steps = [1.0 + 1e-3 * (i % 5) for i in range(1600)]
    for i in (510, 512, 1023, 1025, 1535):
        steps[i] = 5.0
    spec, flat = det_table(steps, 2, rng)
    det_margins(spec, 4.0, flat)
    det, idx, fpos, cnt = run_detect(spec, 4.0, 16)
    assert list(idx) == [510, 512, 1023, 1025, 1535] and np.array_equal(idx, R.detect(spec, 4.0)[1])
    # no peak at all: a monotone detection function
    spec, flat = det_table([1.0 + 0.01 * i for i in range(700)], 2, rng)
    assert check_detect(spec, 0.5, flat, "monotone") == 0


def test_detect_overflow_reports_the_full_count():
    rng = np.random.default_rng(8)
    steps = [(4.0 if i % 2 else 1.0) + 1e-3 * (i % 7) for i in range(41)]
    spec, flat = det_table(steps, 3, rng)
    want = R.detect(spec, 2.0)
    det, idx, fpos, cnt = run_detect(spec, 2.0, 4, expect_size=True)
    assert cnt == len(want[1]) == 20 and np.array_equal(idx, want[1][:4])
    within(fpos, want[2][:4], R.detect(spec, 2.0, LD)[2][:4], "overflow fpos")
    det, idx, fpos, cnt = run_detect(spec, 2.0, 20)                   # exactly enough room
    assert cnt == 20 and np.array_equal(idx, want[1])


def test_detect_rows_of_zeros():
    rng = np.random.default_rng(9)
    spec, flat = det_table(random_steps(300, rng), 5, rng, zero_rows=(0, 40, 41, 42, 100, 299, 300))
    spec[200, 2] = 0.0                                                # one band of a row
    det64, pk64, fp64 = R.detect(spec, 2.0)
    assert np.isnan(det64).sum() == 3 and np.isinf(det64).sum() >= 8
    detld, _, fpld = R.detect(spec, 2.0, LD)
    det, idx, fpos, cnt = run_detect(spec, 2.0, 150)
    assert np.array_equal(idx, pk64)
    within(det, det64, detld, "zeros det")
    within(fpos, fp64, fpld, "zeros fpos")


# ---- refine -------------------------------------------------------------------------------------------------------------
def run_refine(spec, ranges, tseg, hop, half, tsr, sr, thr):
    L, lb = lib()
    spec = np.ascontiguousarray(spec, dtype=np.float64)
    ranges = np.ascontiguousarray(ranges, dtype=np.int32).reshape(-1, 6)
    tseg = np.ascontiguousarray(tseg, dtype=np.float64)
    nseg, nband = len(tseg), spec.shape[1]
    valb, vala = np.full((nseg, nband), -7.0), np.full((nseg, nband), -7.0)
    cross, out = np.full((nseg, nband), -7, dtype=np.int32), np.full(nseg, -7.0)
    rc = lb.pvx_seg_refine(L.dptr(spec), spec.shape[0], nband, i32p(ranges), L.dptr(tseg), nseg, hop, half, tsr, sr, float(thr) if thr else 0.0,
                           1 if thr else 0, L.dptr(valb), L.dptr(vala), i32p(cross), L.dptr(out))
    assert rc == nseg, rc
    return valb, vala, cross, out


GEO = (128, 128.0, 16000.0, 16000.0)                                  # hop, half, tsr, sr


def side_table(m, nband, rng, levels=None):
    """[2m + 1][nband] dB: m frames around -40, one at -25, m around -20; `levels`: values drawn from that short list instead
    (duplicates across lanes).  One segment: ibef [0, m), iaft [m + 1, 2m + 1), iall [0, 2m + 1)."""
    def draw(base, k):
        if levels is not None:
            return base + rng.choice(levels, size=(k, nband))
        return base + rng.uniform(-3.0, 3.0, (k, nband))
    db = np.vstack([draw(-40.0, m), np.full((1, nband), -25.0), draw(-20.0, m)])
    return db, np.array([[0, m, m + 1, 2 * m + 1, 0, 2 * m + 1]], dtype=np.int32)


def refine_margins(spec, ranges, tseg, thr):
    """No dB value within MARGIN of its cell's valm (values that equal it bit for bit apart)."""
    valb, vala, cross, bandpk, weight, out = R.refine(spec, ranges, tseg, *GEO, thr)
    with np.errstate(divide="ignore", invalid="ignore"):
        db = 10 * np.log10(spec)
        for s in range(len(tseg)):
            for b in range(spec.shape[1]):
                vb, va = valb[s, b], vala[s, b]
                valm = (vb + va) / 2. if not thr else min(va, vb) + thr
                d = np.abs(db[ranges[s, 4]:ranges[s, 5], b] - valm)
                d = d[np.isfinite(d) & (d != 0.0)]
                assert d.size == 0 or d.min() >= MARGIN


def check_refine(spec, ranges, tseg, thr, what):
    refine_margins(spec, ranges, tseg, thr)
    r64 = R.refine(spec, ranges, tseg, *GEO, thr)
    rld = R.refine(spec, ranges, tseg, *GEO, thr, LD)
    assert np.array_equal(r64[2], rld[2])
    valb, vala, cross, out = run_refine(spec, ranges, tseg, *GEO, thr)
    assert np.array_equal(cross, r64[2]), what
    within(valb, r64[0], rld[0], what + " valb")
    within(vala, r64[1], rld[1], what + " vala")
    within(out, r64[5], rld[5], what + " out")
    return r64, (valb, vala, cross, out)


@pytest.mark.parametrize("thr", [None, 0, 3.0])
def test_refine_side_lengths(thr):
    for m in (0, 1, 2, 31, 32, 33, 63, 64, 65, 128, 255, 256):
        for seed in range(100):
            rng = np.random.default_rng(17 * m + 5 + 100000 * seed)
            db, ranges = side_table(m, 3, rng)
            spec = energy(db)
            tseg = np.array([(m * 128 + 128.0) / 16000.0])
            r64, rld = R.refine(spec, ranges, tseg, *GEO, thr), R.refine(spec, ranges, tseg, *GEO, thr, LD)
            if m == 0 or not lucky([(r64[0], rld[0]), (r64[1], rld[1])]):
                break
        r64, got = check_refine(spec, ranges, tseg, thr, "side %d thr %s" % (m, thr))
        if m == 0:
            assert np.all(got[2] == -1) and np.isnan(got[3]).all()    # NaN medians: no crossing, a NaN weight, a NaN result
        elif not thr:
            assert np.all(got[2] >= 0)


def test_refine_duplicates_ties_no_crossing_and_specials():
    rng = np.random.default_rng(21)
    # duplicate values across lanes: three levels only
    for m in (32, 65, 200):
        db, ranges = side_table(m, 4, rng, levels=[-1.0, 0.0, 1.0])
        check_refine(energy(db), ranges, np.array([1.0]), None, "duplicates %d" % m)
    # crossings at equal distance on both sides of len(ibef): the earlier one
    m = 32
    db, ranges = side_table(m, 2, rng)
    db[m] = -42.0
    db[m - 2] = -18.0                                                 # up at m - 3, down at m - 2
    db[m + 1], db[m + 2] = -41.0, -43.0                              # first value above valm after the centre: m + 3
    r64, got = check_refine(energy(db), ranges, np.array([1.0]), None, "tie")
    assert np.all(got[2] == m - 2)
    valm = (r64[0] + r64[1]) / 2
    assert np.all((db[m + 2] - valm) * (db[m + 3] - valm) < 0)       # the later one, also 2 away
    # no crossing with a finite weight: out is tseg, seconds among samples
    db = np.vstack([-40.0 + rng.uniform(-0.5, 0.5, (20, 2)), np.full((1, 2), -39.0), -38.0 + rng.uniform(-0.5, 0.5, (20, 2))])
    ranges = np.array([[0, 20, 21, 41, 0, 41]], dtype=np.int32)
    r64, got = check_refine(energy(db), ranges, np.array([0.3125]), 3.0, "no crossing")
    assert np.all(got[2] == -1) and got[3][0] == r64[5][0] and abs(got[3][0] - 0.3125) < 1e-12
    # one energy everywhere: every dB value equals valm bit for bit, no product is negative
    spec = np.full((41, 2), 3.7e-5)
    r64, got = check_refine(spec, ranges, np.array([0.5]), None, "constant")
    assert np.all(got[2] == -1) and np.isnan(got[3][0])              # weights 0: 0 / 0
    # -inf inside a side is ordered like a number; a NaN makes its side's median NaN
    db, ranges = side_table(33, 3, rng)
    spec = energy(db)
    spec[3, 0] = 0.0
    spec[40:60, 1] = 0.0                                              # most of the after side: its median is -inf
    spec[5, 2] = np.nan
    r64, got = check_refine(spec, ranges, np.array([1.0]), None, "specials")
    assert np.isfinite(got[0][0, 0]) and got[1][0, 1] == -np.inf and np.isnan(got[0][0, 2]) and got[2][0, 2] == -1


@pytest.mark.parametrize("nband", [1, 128])
def test_refine_bands_segments_and_batch_independence(nband):
    rng = np.random.default_rng(23 + nband)
    m, nfine = 8, 300
    db = rng.uniform(-60.0, -10.0, (nfine, nband))
    spec = energy(db)
    L, lb = lib()
    for nseg in ((0, 1, 257) if nband == 1 else (1, 9)):
        c = np.linspace(m, nfine - m - 1, max(nseg, 1)).astype(np.int32)[:nseg]
        ranges = np.stack([c - m, c, c + 1, c + m + 1, c - m, c + m + 1], axis=1).astype(np.int32).reshape(nseg, 6)
        tseg = (c * 128 + 128.0) / 16000.0
        if nseg == 0:
            valb, vala, cross, out = run_refine(spec, np.zeros((0, 6), dtype=np.int32), tseg, *GEO, None)
            assert out.shape == (0,) and lb.pvx_segment_last_kernels() == b""
            continue
        r64, got = check_refine(spec, ranges, tseg, 3.0 if nseg == 1 else None, "nband %d nseg %d" % (nband, nseg))
        assert lb.pvx_segment_last_kernels() == b"k_seg_refine"
    # a segment alone gives the bits it gives inside the batch
    for s in (0, nseg // 2, nseg - 1):
        one = run_refine(spec, ranges[s:s + 1], tseg[s:s + 1], *GEO, None)
        for a, b in zip(one, got):
            assert R.same(a[0], b[s])


def test_refine_limit_is_refused_without_a_launch():
    L, lb = lib()
    spec = np.ones((600, 2))
    rg = np.array([[0, 257, 258, 515, 0, 515]], dtype=np.int32)
    out = np.empty(1)
    lb.pvx_seg_detect(L.dptr(spec), 600, 2, 0.0, 0, None, None, None, None)
    assert lb.pvx_segment_last_kernels() == b"k_seg_detect"
    assert lb.pvx_seg_refine(L.dptr(spec), 600, 2, i32p(rg), L.dptr(np.array([1.0])), 1, 128, 128.0, 16000.0, 16000.0, 0.0, 0, None, None, None,
                             L.dptr(out)) == L.PVX_ERR_UNSUPPORTED
    assert lb.pvx_segment_last_kernels() == b""
    rg[0] = [0, 256, 257, 513, 0, 513]                                # exactly at the limit
    assert lb.pvx_seg_refine(L.dptr(spec), 600, 2, i32p(rg), L.dptr(np.array([1.0])), 1, 128, 128.0, 16000.0, 16000.0, 0.0, 0, None, None, None,
                             L.dptr(out)) == 1


# ---- transitions --------------------------------------------------------------------------------------------------------
MODES = {"minmax": (0, 0.0), "median": (1, 0.0), "mean": (2, 0.0), "pct0": (3, 0.0), "pct10": (3, 10.0), "pct50": (3, 50.0),
         "pct100": (3, 100.0)}


def run_trans(v, tx, trt, mode, thr=0.5, escale=0.0):
    L, lb = lib()
    v = np.ascontiguousarray(v, dtype=np.float64)
    tx = np.ascontiguousarray(tx, dtype=np.float64)
    nser, n = v.shape
    trt = np.ascontiguousarray(np.broadcast_to(np.asarray(trt, dtype=np.float64), (nser,)))
    o = [np.full(nser, -7.0) for _ in range(3)]
    st = np.full(nser, -7, dtype=np.int32)
    code, pct = MODES[mode]
    rc = lb.pvx_seg_transitions(L.dptr(v), nser, n, n, 1, escale, L.dptr(tx), n if tx.ndim == 2 else 0, L.dptr(trt), code, pct, thr, L.dptr(o[0]),
                                L.dptr(o[1]), L.dptr(o[2]), i32p(st))
    assert rc == nser, rc
    return o[0], o[1], o[2], st


def step_series(n, nser, rng, falling):
    """dB series that step between about -40 and -20 in the middle, with a ramp point or two, and a far dip that crosses the
    level once more: the nearest crossing has to be chosen."""
    k = n // 2
    lo, hi = -40.0 + rng.uniform(-3, 3, (nser, n)), -20.0 + rng.uniform(-3, 3, (nser, n))
    x = np.where(np.arange(n)[None, :] < k, lo, hi)
    if n >= 64:
        x[:, n - 5] = -41.0                                           # a dip far after the step
    return -60.0 - x if falling else x


def trans_margins(x, tx, trt, mode, thr):
    trts = np.broadcast_to(np.asarray(trt, dtype=np.float64), (len(x),))
    for r in range(len(x)):
        t, trt = tx if tx.ndim == 1 else tx[r], trts[r]
        ttr, vbef, vaft, st = R.transitions_row(x[r], t, trt, mode, thr)
        if st in (R.OUTSIDE, R.EMPTY_SIDE) or np.isnan(vbef) or np.isnan(vaft):    # (a NaN compares false whatever its bits)
            continue
        assert abs(vaft - vbef) >= MARGIN or vaft == vbef
        vtran = vbef * thr + vaft * (1 - thr) if vaft > vbef else vaft * thr + vbef * (1 - thr)
        d = np.abs(x[r] - vtran)
        d = d[d != 0.0]
        assert d.size == 0 or d.min() >= MARGIN
        if mode == "minmax" or mode.startswith("pct"):
            dm = abs(np.median(x[r][t < trt]) - np.median(x[r][t > trt]))
            assert dm >= MARGIN or dm == 0.0                          # (0: one value on both sides, the same bits)


def check_trans(x, tx, trt, mode, thr, as_energy, what):
    """as_energy: the kernel takes 10 ** (x / 10) / 4 with escale 4 and the logarithm itself."""
    if as_energy:
        v = energy(x) / 4.0
        with np.errstate(divide="ignore"):
            x64, xld = 10 * np.log10(v * 4.0), 10 * np.log10(v.astype(LD) * 4.0)
    else:
        v, x64, xld = x, x, x.astype(LD)
    trans_margins(x64, tx, trt, mode, thr)
    w64 = R.transitions(x64, tx, trt, mode, thr)
    wld = R.transitions(xld, tx, trt, mode, thr, LD)
    assert np.array_equal(w64[3], wld[3])
    got = run_trans(v, tx, trt, mode, thr, 4.0 if as_energy else 0.0)
    assert np.array_equal(got[3], w64[3]), (what, got[3], w64[3])
    for j, name in enumerate(("ttr", "vbef", "vaft")):
        if as_energy:
            within(got[j], w64[j], wld[j], "%s %s" % (what, name))
        else:
            assert R.same(got[j], w64[j]), (what, name)               # no logarithm: numpy's operations in numpy's order
    return w64, got


@pytest.mark.parametrize("mode", sorted(MODES))
def test_transitions_sizes_modes_and_directions(mode):
    for n in (2, 3, 64, 65, 129, 4096):
        for falling in (False, True):
            for as_energy in (False, True):
                for seed in range(100):
                    rng = np.random.default_rng(n + 7 * falling + 100000 * seed + 13 * len(mode))
                    x = step_series(n, 3, rng, falling)
                    tx = np.arange(n) * 0.008
                    trt = tx[n // 2] - 0.004 if n != 3 else tx[1]
                    if not as_energy:
                        break
                    v = energy(x) / 4.0
                    w64 = R.transitions(10 * np.log10(v * 4.0), tx, trt, mode, 0.5)
                    wld = R.transitions(10 * np.log10(v.astype(LD) * 4.0), tx, trt, mode, 0.5, LD)
                    if not lucky([(w64[1], wld[1]), (w64[2], wld[2])]):
                        break
                w64, got = check_trans(x, tx, trt, mode, 0.5, as_energy, "%s n %d falling %d energy %d" % (mode, n, falling, as_energy))
                assert np.all(got[3] == R.OK)
                if mode != "pct100":                                  # (there the dip is the after side's typical value)
                    assert np.all(np.abs(got[0] - trt) < 0.008 * 1.01)    # the step's crossing, not the far dip's


def test_transitions_every_status_and_own_times():
    rng = np.random.default_rng(31)
    n = 65
    x = step_series(n, 6, rng, False)
    x[5] = -33.0                                                      # a constant series: vbef == vaft, nothing crosses
    tx = np.tile(np.arange(n) * 0.01, (6, 1))
    tx[1] += 0.5                                                      # every series with times of its own
    trt = np.array([0.315, 0.815, 5.0, tx[3, -1], 0.0, 0.315])       # ok, ok, outside, no point after, none before, no crossing
    for mode in ("minmax", "mean", "pct10"):
        w64, got = check_trans(x, tx, trt, mode, 0.5, False, "statuses " + mode)
        assert list(got[3]) == [R.OK, R.OK, R.OUTSIDE, R.EMPTY_SIDE, R.EMPTY_SIDE if mode != "mean" else R.NO_CROSSING, R.NO_CROSSING]
        assert got[0][2] == 5.0 and got[1][2] == 0.0 and got[2][2] == 0.0
    # two crossings at the same distance in time: the earlier one
    x1 = np.full((1, 9), -40.0)
    x1[0, 3] = -20.0
    x1[0, 6:] = -20.0                                                 # up at 2 and at 5: both 1.5 from trt = 4
    w64, got = check_trans(x1, np.arange(9.0), 4.0, "mean", 0.5, False, "time tie")
    assert got[3][0] == R.OK and 2.0 < got[0][0] < 3.0


def test_transitions_series_alone_and_in_a_batch():
    rng = np.random.default_rng(33)
    n = 129
    x = step_series(n, 7, rng, False)
    x[3] = -60.0 - x[3]
    tx = np.arange(n) * 0.008
    trt = tx[n // 2] - 0.004
    v = energy(x) / 4.0
    for mode in ("minmax", "median", "mean", "pct10"):
        batch = run_trans(v, tx, trt, mode, 0.5, 4.0)
        for r in range(7):
            one = run_trans(v[r:r + 1], tx, trt, mode, 0.5, 4.0)
            for a, b in zip(one, batch):
                assert R.same(a[0], b[r]), (mode, r)
