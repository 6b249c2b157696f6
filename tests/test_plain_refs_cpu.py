"""The plain references of tests/plain_refs.py, pinned on the CPU before they judge a kernel (tests/test_consumers_gpu.py):
against values recorded from the reference (D1, W1, W2), against the oracle, and against the product's host path.  The
inputs of the GPU module's harmonic sweep are built here too, and checked with the oracle alone: that every case reaches
the branch of k_harmonic.hip it was added for, and that none of them spends the float32 comparison's allowance of bin
flips through the choice of its f0 track."""
import os

import numpy as np
import pytest

from .conftest import GOLDEN
from .plain_refs import calc_f0_ref, funcwind_ref, harmonic_power_ref, heterodyne_ref, rms_ref

SR = 22050.0
EPS = 2.0 ** -52


def hpower_bound(K):
    """Relative bound between two float64 evaluations of hpower: all terms are non-negative, a row has at most K squares
    and a sum at most K rows, and each side rounds once per operation (unit roundoff 2**-53): < (2K + 2) * 2**-52."""
    return (2 * K + 2) * EPS


# ------------------------------------------------------------------ descriptors
def test_descriptor_references_match_the_recorded_values():
    """D1: calc_f0 with the default and a non-default argument set, calc_harmonic_power with two thresholds, recorded from
    the reference on its own (F, 8) arrays."""
    g = np.load(os.path.join(GOLDEN, "D1_descriptors.npz"))
    fm, idx = calc_f0_ref(g["f"], g["mag"])
    assert np.array_equal(fm, g["f0"]) and np.array_equal(idx, g["fundamental_idx"])
    fm, idx = calc_f0_ref(g["f"], g["mag"], fmin=300, fmax=2000, thr=0.3)
    assert np.array_equal(fm, g["f0_b"]) and np.array_equal(idx, g["fundamental_idx_b"])
    K = g["f"].shape[1]
    for thr, tag in ((0.01, ""), (0.002, "_b")):
        hp, nh = harmonic_power_ref(g["f"], g["mag"], thr)
        assert np.array_equal(nh, g["nharmonics" + tag])
        assert np.array_equal(hp == 0, g["hpower" + tag] == 0)
        assert (np.abs(hp - g["hpower" + tag]) <= hpower_bound(K) * g["hpower" + tag]).all()


def random_result_arrays(seed, F, K):
    """(F, K) arrays like an analysis result, but with what an analysis rarely gives: empty slots between valid ones,
    frequencies and magnitudes that tie exactly, and all-empty frames."""
    rng = np.random.default_rng(seed)
    f = np.round(rng.uniform(40.0, 6000.0, (F, K)), 0)              # whole Hz: exact ties and exact integer ratios
    mag = np.round(rng.uniform(0.0, 1.0, (F, K)), 2)
    f[rng.random((F, K)) < 0.3] = 0.0
    mag[f == 0] = 0.0
    if K > 1:
        f[:, -1] = f[:, 0]                                           # a tie on the lowest candidate: the first one wins
        mag[:, -1] = mag[:, 0]
    if F > 2:
        f[2] = 0.0
        mag[2] = 0.0
    return f, mag


@pytest.mark.parametrize("F,K", [(1, 1), (7, 3), (40, 8), (70, 66), (3, 20)])
def test_descriptor_references_match_the_host_path(F, K):
    """PV's numpy branch (arrays assigned on the host: no GPU) on seeded arrays with zeros, holes and ties; a row with a
    NaN magnitude has no fundamental on either side; F < K with a valid slot >= F raises on both."""
    import pypevoc_amd
    f, mag = random_result_arrays(1000 * F + K, F, K)
    p = pypevoc_amd.PV(np.zeros(4096), SR, nfft=1024, hop=256, npks=K, progress=False)
    p.f, p.mag = f, mag
    assert not p._on_device()
    for args in ((50, 10000, 0.1), (300, 2000, 0.3), (0, 1e9, 0.0), (50, 10000, 1.0), (2000, 300, 0.1)):
        fm = p.calc_f0(*args)
        rfm, ridx = calc_f0_ref(f, mag, *args)
        assert np.array_equal(fm, rfm) and np.array_equal(p.fundamental_idx, ridx), args
        if args[2] == 1.0 or args[0] > args[1]:
            assert not rfm.any() and not ridx.any()
    raises = bool((f[:, F:] > 0).any())
    assert raises == ((F, K) == (3, 20))
    for thr in (0.01, 0.05, 0.5, 0.0):
        if raises:
            with pytest.raises(IndexError):
                harmonic_power_ref(f, mag, thr)
            with pytest.raises(IndexError):
                p.calc_harmonic_power(thr)
            continue
        hp, nh = harmonic_power_ref(f, mag, thr)
        p.calc_harmonic_power(thr)
        assert np.array_equal(nh, p.nharmonics), thr
        assert np.array_equal(hp == 0, p.hpower == 0) and (np.abs(hp - p.hpower) <= hpower_bound(K) * hp).all(), thr
        if thr == 0.0:
            assert not nh.any()                                      # |x| < 0 never holds: not even the peak itself
    # a NaN among finite magnitudes: np.max is NaN, no peak passes the limit
    mn = mag.copy()
    mn[0, K // 2] = np.nan
    p.mag = mn
    fm = p.calc_f0()
    rfm, ridx = calc_f0_ref(f, mn)
    assert rfm[0] == 0.0 and ridx[0] == 0
    assert np.array_equal(fm, rfm) and np.array_equal(p.fundamental_idx, ridx)


# ------------------------------------------------------------------ reductions
REDUCERS = ("sum", "mean", "max", "min", "std", "var")


def _c2(z):
    return np.stack([z.real, z.imag], axis=1)


def test_reduction_references_match_the_recorded_values():
    """W1 (heterodyne, RMSWind) and W2 (FuncWind: six reducers x power 0 / 1 / 2, an odd window and hop, a complex signal)
    as recorded from the reference.  numpy sums pairwise, these loops left to right: the fixtures' own 1e-13 / 1e-14."""
    g = dict(np.load(os.path.join(GOLDEN, "W1_windowed.npz")))
    x = g["x"].astype(np.float64)
    hetsig = np.exp(-2j * np.pi * np.cumsum(g["het_fvec"]))
    h, ic = heterodyne_ref(x, hetsig, np.hanning(1024), 256)
    assert np.array_equal(ic, g["het_icent"]) and np.abs(_c2(h) - g["het"]).max() <= 1e-13
    h, ic = heterodyne_ref(x, hetsig, np.ones(256), 100)
    assert np.array_equal(ic, g["het_rect_icent"]) and np.abs(_c2(h) - g["het_rect"]).max() <= 1e-13
    assert np.abs(rms_ref(x, np.blackman(1024), 512) - g["rms"]).max() <= 1e-14
    assert np.abs(rms_ref(x, np.hanning(1000), 333) - g["rms_odd"]).max() <= 1e-14
    g = dict(np.load(os.path.join(GOLDEN, "W2_funcwind.npz")))
    x = g["x"].astype(np.float64)
    for name in REDUCERS:
        tol = 0.0 if name in ("max", "min") else 1e-13
        for power in (0, 1, 2):
            want = g["%s_p%d" % (name, power)]
            got = funcwind_ref(name, x, np.blackman(1024), 512, power)
            assert got.shape == want.shape and np.abs(got - want).max() <= tol, (name, power)
        assert np.abs(funcwind_ref(name, x, np.hanning(1000), 333, 1) - g["%s_odd" % name]).max() <= tol, name
    xc = x * np.exp(2j * np.pi * np.arange(len(x)) * 1000.0 / float(g["sr"]))
    for name in ("sum", "mean"):
        assert np.abs(_c2(funcwind_ref(name, xc, np.blackman(1024), 256, 1)) - g["c_%s" % name]).max() <= 1e-13, name
    for name in ("std", "var"):
        got = funcwind_ref(name, xc, np.blackman(1024), 256, 1)
        assert got.dtype == np.float64 and np.abs(got - g["c_%s" % name]).max() <= 1e-13, name
    with pytest.raises(TypeError):
        funcwind_ref("max", xc, np.blackman(1024), 256, 1)


def reduction_signal(n, cpx=False):
    """The seeded signal of the reduction sweeps (CPU here, GPU in test_consumers_gpu.py): a prefix of 6000 samples."""
    rng = np.random.default_rng(77)
    x = rng.standard_normal(6000)
    if cpx:
        x = x + 1j * rng.standard_normal(6000)
    return x[:n].copy()


# (wlen, hop) of the sweep and, for each, the signal lengths: n - wlen an exact multiple of hop (the frame at n - wlen must
# not exist) first, then lengths for 1, 2, 3 and 5 frames (a block holds 4 waves: the last one ragged), then a longer one
REDUCTION_SHAPES = [
    (1, 1, (1 + 5, 2, 3, 4, 4000)),
    (7, 3, (7 + 3 * 5, 8, 11, 14, 3001)),
    (63, 64, (63 + 64 * 2, 64, 63 + 65, 63 + 64 * 2 + 1, 63 + 64 * 4 + 9, 4000)),
    (64, 1, (64 + 5, 65, 66, 67, 64 + 300)),
    (65, 200, (65 + 200 * 3, 66, 65 + 201, 65 + 401, 65 + 801, 4000)),
    (1000, 1000, (1000 + 1000 * 2, 1001, 2001, 3001, 5001)),
]


def reduction_cases():
    out = []
    for wlen, hop, lengths in REDUCTION_SHAPES:
        for i, n in enumerate(lengths):
            out.append(pytest.param(wlen, hop, n, i == 0, id="w%d-h%d-n%d" % (wlen, hop, n)))
    return out


def test_reduction_shapes_cover_the_frame_counts():
    """Every (wlen, hop) has a length with n - wlen an exact multiple of hop, and frame counts 1, 2, 3 and 5."""
    for wlen, hop, lengths in REDUCTION_SHAPES:
        assert (lengths[0] - wlen) % hop == 0 and lengths[0] > wlen
        counts = {len(range(0, n - wlen, hop)) for n in lengths}
        assert {1, 2, 3, 5} <= counts, (wlen, hop, sorted(counts))


@pytest.mark.parametrize("wlen,hop,n,exact", reduction_cases())
def test_reduction_references_match_the_oracle(oracle, wlen, hop, n, exact):
    """The same sweep the kernels get, references against the oracle's C loops: windows shorter than a wave, hop > wlen,
    hop = 1, the strict frame rule.  Both add left to right in float64, so they agree to the last bit or two."""
    x = reduction_signal(n)
    w = np.hanning(wlen)
    nfr = len(range(0, n - wlen, hop))
    hs = np.exp(-2j * np.pi * 0.0123 * np.arange(n))
    h, ic = heterodyne_ref(x, hs, w, hop)
    oh, oi = oracle.heterodyne(x, hs, w, hop)
    assert len(h) == nfr == len(oh) and np.array_equal(ic, oi)
    assert np.abs(h - oh).max() <= 1e-14 * max(1.0, np.abs(oh).max())
    if exact:
        assert ic[-1] - wlen // 2 == n - wlen - hop                 # no frame at n - wlen
    r = rms_ref(x, w, hop)
    orr = oracle.rms_frames(x, w, hop)
    assert len(r) == nfr and np.abs(r - orr).max() <= 1e-14 * max(1.0, np.abs(orr).max())
    xc = reduction_signal(n, cpx=True)
    for name in REDUCERS:
        for power in (1, 2):
            got = funcwind_ref(name, x, w, hop, power)
            want = oracle.funcwind(name, x, w, hop, power)
            tol = 0.0 if name in ("max", "min") else 1e-14 * max(1.0, np.abs(want).max())
            assert got.shape == want.shape == (nfr,) and np.abs(got - want).max() <= tol, (name, power)
        if name not in ("max", "min"):
            got = funcwind_ref(name, xc, w, hop, 1)
            want = oracle.funcwind(name, xc, w, hop, 1)
            assert got.dtype == want.dtype and np.abs(got - want).max() <= 1e-14 * max(1.0, np.abs(want).max()), name


def test_reduction_references_propagate_nan_and_inf(oracle):
    """min / max of a frame with a NaN is NaN in exactly the frames that hold it; -inf / +inf come through min / max where
    the window does not multiply them by an exact zero (np.hanning's end samples)."""
    wlen, hop = 63, 20
    x = reduction_signal(400)
    w = np.hanning(wlen)
    starts = np.arange(0, len(x) - wlen, hop)
    for name in ("min", "max"):
        xn = x.copy()
        xn[150] = np.nan
        got = funcwind_ref(name, xn, w, hop, 1)
        holds = (starts <= 150) & (150 < starts + wlen)
        assert np.array_equal(np.isnan(got), holds) and holds.sum() >= 3
        assert np.array_equal(got, oracle.funcwind(name, xn, w, hop, 1), equal_nan=True)
        xi = x.copy()
        xi[150] = -np.inf if name == "min" else np.inf
        assert not ((starts == 150) | (starts + wlen - 1 == 150)).any()                   # never under a zero end sample
        got = funcwind_ref(name, xi, w, hop, 1)
        assert np.array_equal(got == xi[150], holds) and np.isfinite(got[~holds]).all()
        assert np.array_equal(got, oracle.funcwind(name, xi, w, hop, 1))


# ------------------------------------------------------------------ inputs of the harmonic sweep (k_harmonic.hip)
def _with_gaps(f0, rng, nzero=4, nnan=3):
    f0 = f0.copy()
    f0[rng.choice(len(f0), nzero, replace=False)] = 0.0
    f0[rng.choice(len(f0), nnan, replace=False)] = np.nan
    return f0


def harmonic_case(name, frames=40):
    """Signal, parameters and per-frame f0 track of one row of the harmonic sweep; sr 22050, float64, PVHarmonic's own
    fmin = 30 Hz.  With N2 = nfft // 2 and f0bin = f0 * nfft / sr a frame has nh = ceil((N2 - 1 - f0bin) / f0bin) harmonics.

    deep:  nfft 4096, f0 ~ 27 Hz: f0bin ~ 5, nh ~ 400, K = 100.  Seven trips of the 64-wide harmonic loop, stored harmonics
           past lane 63, a residual over hundreds of partial sums.  The measured first harmonic stays below fmin.
    few:   nfft 512, f0 ~ 3 kHz: nh = 3 < K = 10, the trailing slots keep the zeros written at the top of the kernel.
    bin1:  nfft 1024, f0 in 22.5 .. 31.5 Hz: f0bin 1.04 .. 1.47 (above the half bin the host rejects), the first harmonic
           sits on bin 1 where the 3-bin sum is clamped on the left; the tone itself is at 31 Hz, so that the measured first
           harmonic exceeds fmin and the other K = 80 stored harmonics are re-centred.
    nyq:   nfft 999 (N2 = 499), nh = 20 and 20 * f0bin in 497.5 .. 498: the last harmonic lands on bin N2 - 1 = 498 and
           the 3-bin sum is clamped on the right; K = 24 > nh keeps it among the stored ones."""
    rng = np.random.default_rng({"deep": 21, "few": 22, "bin1": 23, "nyq": 24}[name])
    if name == "deep":
        nfft, hop, K, tone, nharm = 4096, 1024, 100, 27.0, 80
    elif name == "few":
        nfft, hop, K, tone, nharm = 512, 128, 10, 3000.0, 3
    elif name == "bin1":
        nfft, hop, K, tone, nharm = 1024, 256, 80, 31.0, 10
    else:
        nfft, hop, K, tone, nharm = 999, 250, 24, 24.8875 * SR / 999, 20
    n = nfft + hop * (frames - 1) + 1
    t = np.arange(n) / SR
    x = sum(0.3 / h * np.sin(2 * np.pi * tone * h * t + h) for h in range(1, nharm + 1)) + 0.01 * rng.standard_normal(n)
    if name == "deep":
        f0 = tone * (1 + 0.02 * rng.standard_normal(frames))
    elif name == "few":
        f0 = tone * (1 + 0.01 * rng.standard_normal(frames))
    elif name == "bin1":
        f0 = rng.uniform(22.5, 31.5, frames)
    else:
        f0 = rng.uniform(24.877, 24.898, frames) * SR / nfft
    f0 = _with_gaps(f0, rng)
    if name == "few":
        # The first analysed frame is measured against an all-zero previous spectrum; with hop = nfft / 4 its first harmonic
        # then comes out at a whole number of half bins, which puts its third harmonic exactly on a half-integer.  An f0
        # above the last bin gives frame 0 no harmonic at all (nh = 0, one more branch) and a spectrum for frame 1.
        f0[0] = 12000.0
        f0[1] = tone
    return dict(x=x, sr=SR, nfft=nfft, hop=hop, K=K, f0=f0, fmin=30.0, frames=frames)


def _bin_positions(c, o):
    """Per valid frame the (fractional) bin position every harmonic's bin is rounded from: (h + 1) * f0bin, or, once the
    first harmonic measured by the ORACLE (o["f"][:, 0]) exceeds fmin, (h + 1) times its bin where that stays below
    N2 - 1.  Returns a list of (frame, nh, positions[nh])."""
    nfft, N2 = c["nfft"], c["nfft"] // 2
    out = []
    for fr, f0 in enumerate(c["f0"]):
        if not f0 > 0:
            continue
        f0bin = f0 / c["sr"] * nfft
        nh = len(np.arange(f0bin, N2 - 1, f0bin))
        pos = f0bin * np.arange(1, nh + 1)
        f1 = o["f"][fr, 0]
        if nh > 0 and f1 > c["fmin"]:
            corr = f1 / c["sr"] * nfft * np.arange(1, nh + 1)
            take = corr < N2 - 1
            take[0] = False
            pos[take] = corr[take]
        out.append((fr, nh, pos))
    return out


def _famp(oracle, c, fr):
    return np.abs(oracle.stft_frame(c["x"], fr * c["hop"], c["nfft"]))


@pytest.mark.parametrize("name", ["deep", "few", "bin1", "nyq"])
def test_harmonic_cases_reach_their_branches(oracle, name):
    """With the oracle alone: the number of harmonics per frame is what the case was built for (counted on the oracle's
    own output with room for all of them), and the magnitudes the oracle reports at the ends of the spectrum are the
    clamped 2-bin sums of its own spectrum -- so the bins are 1 and N2 - 1."""
    c = harmonic_case(name)
    N2 = c["nfft"] // 2
    o = oracle.harmonic(c["x"], c["sr"], c["f0"], c["nfft"], c["hop"], N2 + 2, c["fmin"])
    valid = c["f0"] > 0
    assert 30 <= valid.sum() < c["frames"] and np.isnan(c["f0"]).any() and (c["f0"] == 0).any()
    if name == "bin1":
        # harmonics 1.0 .. 1.5 bins apart: their 3-bin sums overlap, the harmonic energy exceeds the total and the residual
        # is the square root of a negative number in most frames, as in the reference
        assert np.isnan(o["residuals"][~valid]).all() and np.isnan(o["residuals"][valid]).sum() > 0.5 * valid.sum()
    else:
        assert np.array_equal(np.isnan(o["residuals"]), ~valid)
    nh = (o["f"] != 0).sum(axis=1)
    rows = _bin_positions(c, o)
    assert [r[1] for r in rows] == list(nh[valid])
    if name == "deep":
        assert nh[valid].min() > 6 * 64 and nh[valid].max() < 7 * 64 and c["K"] > 64      # seven trips, stored ones past lane 63
        assert (o["f"][valid, 0] <= c["fmin"]).sum() > 0.75 * valid.sum()                 # bins from the f0 given, mostly
    elif name == "few":
        assert nh[0] == 0 and (nh[valid][1:] == 3).all() and c["K"] > 3
    elif name == "bin1":
        assert nh[valid].min() > 5 * 64 and c["K"] > 64
        assert (o["f"][valid, 0] > c["fmin"]).sum() > 0.75 * valid.sum()                  # most frames re-centre
        for fr, _, pos in rows:
            assert np.rint(pos[0]) == 1
        for fr, _, pos in rows[:5]:
            a = _famp(oracle, c, fr)
            two, three = np.sqrt(a[1] ** 2 + a[2] ** 2), np.sqrt(a[0] ** 2 + a[1] ** 2 + a[2] ** 2)
            assert abs(o["mag"][fr, 0] - two) <= 1e-12 * two and abs(three - two) > 1e-6 * two
    else:
        assert (nh[valid] == 20).all() and c["K"] > 20 and N2 == 499
        # (the first frame, and one that follows a gap, measure their first harmonic against an older spectrum and may
        # re-centre elsewhere)
        hit = [fr for fr, _, pos in rows if N2 - 1.5 < pos[-1] < N2 - 1]
        assert len(hit) > 0.75 * valid.sum()
        for fr in hit[:5]:
            a = _famp(oracle, c, fr)
            two, three = np.sqrt(a[N2 - 2] ** 2 + a[N2 - 1] ** 2), np.sqrt(a[N2 - 3] ** 2 + a[N2 - 2] ** 2 + a[N2 - 1] ** 2)
            assert abs(o["mag"][fr, 19] - two) <= 1e-12 * two and abs(three - two) > 1e-6 * two


@pytest.mark.parametrize("name", ["deep", "few", "bin1"])
def test_harmonic_cases_leave_the_float32_allowance_alone(oracle, name):
    """The float32 comparison tolerates 1 % of harmonics on a neighbouring bin (a bin position within float32 error of a
    half-integer rounds either way).  In the oracle's float64 run of the cases compared at float32, fewer than 0.2 % of
    the stored harmonics have their bin position within 1e-3 of a half-integer: the inputs do not use the allowance up."""
    c = harmonic_case(name)
    o = oracle.harmonic(c["x"], c["sr"], c["f0"], c["nfft"], c["hop"], c["K"], c["fmin"])
    near = total = 0
    for fr, nh, pos in _bin_positions(c, o):
        p = pos[: min(nh, c["K"])]
        total += len(p)
        near += int((np.abs(p - np.floor(p) - 0.5) <= 1e-3).sum())
    assert total == (o["f"] != 0).sum() and near < 0.002 * total, (near, total)
