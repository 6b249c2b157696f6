"""Plain float64 numpy restatement of HeterodyneHarmonic's fixed-resolution path, frame by frame and harmonic by harmonic:
what pypevoc_amd/Heterodyne.py and k_hetharm.hip compute, written from the formulas (HETHARM.md), with no import of the
reference and none of the package.  tests/test_hetharm_cpu.py holds it against the recorded Q*.npz.

Below it, the exact-phase reference (HETHARM.md, "Exact-phase tests"): on a track fvec[t] = k[t] * 2**-q with integer k the running
phase is an integer over 2**q, so the carrier of any harmonic at any sample comes from integer arithmetic, correct to an ulp
however long the signal is; and a numpy model of the device's three-launch scan with switchable slips."""
import numpy as np


def nframes(nsamp, nwind, nhop):
    """frames start at 0, nhop, .. while the start is < nsamp - nwind"""
    return len(range(0, nsamp - nwind, nhop))


def frame_times(nsamp, sr, nwind, nhop):
    """th: centre time of every frame; idxh: the centres as samples (one more than th when nwind is odd and the last fits)"""
    c = nwind // 2
    th = np.arange(c, nsamp - (nwind - c), nhop) / sr
    idxh = np.arange(c, nsamp - c, nhop).astype('i')
    return th, idxh


def track(nsamp, sr, f, tf=None, fmin=0.1):
    """(fvec in cycles per sample, fmin raised to the track's minimum) from a number, a per-sample array or tf / f pairs"""
    tvec = np.arange(nsamp) / sr
    hz = np.interp(tvec, tf, f) if tf is not None else np.asarray(f, dtype=float) * np.ones(nsamp)
    return hz / sr, max(fmin, hz.min())


def hetsig(fvec, n):
    return np.exp(1j * np.cumsum(fvec * n * 2 * np.pi))


def extract(x, fvec, n, wind, hop):
    """harmonic n: 2 * windowed mean of x * hetsig per frame, and the frames' centre samples"""
    hs = hetsig(fvec, n)
    wlen, norm = len(wind), np.sum(wind)
    out, icent = [], []
    for start in range(0, len(x) - wlen, hop):
        seg = x[start:start + wlen] * hs[start:start + wlen] * wind
        out.append(2 * np.sum(seg) / norm)
        icent.append(start + wlen // 2)
    return np.array(out, dtype=complex), np.array(icent, dtype=np.int64)


def extract_all(x, fvec, nharm, wind, hop):
    ah = np.zeros((nframes(len(x), len(wind), hop), nharm), dtype=complex)
    for n in range(nharm):
        ah[:, n] = extract(x, fvec, n, wind, hop)[0]
    ah[:, 0] /= 2
    return ah


def interp_amp(nsamp, nwind, nhop, col):
    """the frame values `col` linearly interpolated to every sample, clamped to the end values outside the frame centres"""
    t = np.arange(nsamp)
    if len(col) == 1:
        return np.full(nsamp, col[0], dtype=complex)
    r = t - nwind // 2
    i0 = np.clip(r // nhop, 0, len(col) - 2)
    fr = np.clip((r - i0 * nhop) / nhop, 0.0, 1.0)
    return col[i0] + (col[i0 + 1] - col[i0]) * fr


def filter_mask(hf, f0, n, sr, fmin, fmax, ampthr):
    """the four terms of the mask, each as a boolean array"""
    return {"fmin": f0 < fmin, "fmax": f0 > fmax, "nyquist": f0 * n > sr / 2.2, "amp": np.abs(hf) < np.max(np.abs(hf)) * ampthr}


def filter_harmonic(ah, fvec, n, sr, nwind, nhop, fmin, fmax, ampthr):
    hf = interp_amp(len(fvec), nwind, nhop, ah[:, n])
    m = filter_mask(hf, fvec * sr, n, sr, fmin, fmax, ampthr)
    hf[m["fmin"] | m["fmax"] | m["nyquist"] | m["amp"]] = 0
    return hf


def resynth_partial(ah, fvec, n, sr, nwind, nhop, filter=False, fmin=None, fmax=None, ampthr=None):
    hf = filter_harmonic(ah, fvec, n, sr, nwind, nhop, fmin, fmax, ampthr) if filter else interp_amp(len(fvec), nwind, nhop, ah[:, n])
    return np.real(np.conj(hetsig(fvec, n)) * hf)


def resynth(ah, fvec, sr, nwind, nhop):
    y = np.zeros(len(fvec))
    for n in range(ah.shape[1]):
        y += resynth_partial(ah, fvec, n, sr, nwind, nhop)
    return y


def calc_adjusted_freq(x, fvec, sr, wind, nhop):
    h, ic = extract(x, fvec, 1, wind, nhop)
    dph = np.concatenate(([0], np.diff(np.unwrap(np.angle(h)))))
    return fvec[ic] - dph / nhop / 2 / np.pi, ic / sr


def f_cols(fvec, sr, th, nharm, include_dc):
    f0t = np.interp(th, np.arange(len(fvec)) / sr, fvec * sr)
    return np.array([f0t * n for n in range(0 if include_dc else 1, nharm)]).T


def angle_ratios(ah, include_dc):
    camp = ah if include_dc else ah[:, 1:]
    ang = np.angle(camp / camp[:, :1])
    return np.hstack((np.zeros((len(ang), 1)), ang)) if include_dc else ang


def partial_frequencies(ah, fcols, sr, nhop, include_dc):
    camp = ah if include_dc else ah[:, 1:]
    newf = fcols[1:, :] - np.diff(np.unwrap(np.angle(camp)), axis=0) / (nhop / sr) / 2 / np.pi
    return np.hstack((np.zeros((len(newf), 1)), newf)) if include_dc else newf


# ---- exact phase on dyadic tracks --------------------------------------------------------------------------------------
def dyadic_track(rng, n, lo, hi, q=30):
    """(k, fvec): integers k[t] drawn from [lo * 2**q, hi * 2**q) and fvec[t] = k[t] * 2**-q, exact in float64.  With
    sr a power of two the track in Hz, fvec * sr, is exact too.  Every partial sum of up to 2**21 such values fits 53 bits
    (q + 21 < 53 for hi < 1): np.cumsum(fvec), and any other order of adding, carries no rounding at all."""
    k = rng.integers(int(lo * 2 ** q), int(hi * 2 ** q), size=n, dtype=np.int64)
    return k, k * 2.0 ** -q


def cumphase(k, q=30):
    """K[t] = (k[0] + .. + k[t]) mod 2**q: the running phase of the fundamental in units of 2**-q cycles"""
    return np.cumsum(np.asarray(k, dtype=np.int64)) % (1 << q)


def cis_units(fr, q=30):
    """exp(2j * pi * fr / 2**q) for integers fr in [0, 2**q): the argument is brought to [-pi, pi) before the one rounded
    product with pi, so the value is within about 2 ulp of the true one whatever the phase was before the reduction"""
    fr = np.where(fr >= 1 << (q - 1), fr - (1 << q), fr)
    a = 2 * np.pi * (fr / float(1 << q))
    return np.cos(a) + 1j * np.sin(a)


def carrier_exact(k, h, q=30, K=None):
    """exp(+2j * pi * h * cumsum(k) / 2**q) per sample.  K is reduced mod 2**q before the product with h (h < 2**33 stays in
    int64).  K: cumphase(k, q) where the caller has it already."""
    K = cumphase(k, q) if K is None else K
    return cis_units((int(h) * K) % (1 << q), q)


def extract_exact(x, k, h, wind, hop, frames, q=30, K=None):
    """harmonic h at the frames `frames` only (frame i starts at i * hop): (2 / sum(wind) * sum_j x w z  [len(frames)] complex,
    S = 2 / sum(wind) * sum_j |x w|  [len(frames)]).  sum(wind) is the correctly rounded sum (math.fsum).  Not halved for h = 0."""
    import math
    x, wind, frames = np.asarray(x, dtype=float), np.asarray(wind, dtype=float), np.asarray(frames, dtype=np.int64)
    idx = frames[:, None] * int(hop) + np.arange(len(wind))
    K = cumphase(k, q) if K is None else K
    z = cis_units((int(h) * K[idx]) % (1 << q), q)
    xw = x[idx] * wind
    scale = 2 / math.fsum(wind)
    return scale * np.sum(xw * z, axis=1), scale * np.sum(np.abs(xw), axis=1)


def extract_all_exact(x, k, harmonics, wind, hop, frames, halve_dc=True, q=30, K=None):
    """(ah [len(frames), len(harmonics)], S of the same shape); with halve_dc the column of harmonic 0 and its S are halved, as
    extract_all halves it (an exact operation)"""
    K = cumphase(k, q) if K is None else K
    cols = [extract_exact(x, k, h, wind, hop, frames, q, K) for h in harmonics]
    ah, S = np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1)
    for j, h in enumerate(harmonics):
        if h == 0 and halve_dc:
            ah[:, j] /= 2
            S[:, j] /= 2
    return ah, S


def extract_bound(S, wlen, G=8):
    """|device - exact| per frame and harmonic: two sincospi and at most G - 1 rotations give each term (G + 4) * 2**-52, a lane
    adds wlen / 64 terms by fma, the wave sum has six levels; the leading 2 is the reference's own share"""
    return 2 * (G + 10 + wlen / 64) * 2.0 ** -52 * S


def knots(nsamp, nwind, nhop, nfr):
    """(i0, i1): the frames whose centres lie either side of each sample, both clamped to the first and the last frame"""
    r = np.arange(nsamp) - nwind // 2
    i0 = np.clip(r // nhop, 0, nfr - 1)
    return i0, np.minimum(i0 + 1, nfr - 1)


def resynth_bound(ah, nsamp, nwind, nhop, G=8):
    """|device - exact| per sample for the sum of the columns of ah: 2 * (G + 8) * 2**-52 * sum_h (|ah[i0, h]| + |ah[i0 + 1, h]|)"""
    i0, i1 = knots(nsamp, nwind, nhop, len(ah))
    mag = np.sum(np.abs(ah), axis=1)
    return 2 * (G + 8) * 2.0 ** -52 * (mag[i0] + mag[i1])


def resynth_partial_exact(ah, k, n, sr, nwind, nhop, filter=False, fmin=None, fmax=None, ampthr=None, col=None, q=30, K=None):
    """resynth_partial with the exact carrier; harmonic n is column `col` of ah (n itself unless given)"""
    fvec = np.asarray(k) * 2.0 ** -q
    c = n if col is None else col
    hf = filter_harmonic(ah, fvec, n, sr, nwind, nhop, fmin, fmax, ampthr) if filter else interp_amp(len(fvec), nwind, nhop, ah[:, c])
    z = carrier_exact(k, n, q, K)
    return z.real * hf.real + z.imag * hf.imag


def resynth_exact(ah, k, harmonics, sr, nwind, nhop, q=30, K=None):
    """sum over the harmonics `harmonics` (column j of ah is harmonics[j]), unfiltered: (y, the bound of resynth_bound)"""
    K = cumphase(k, q) if K is None else K
    y = np.zeros(len(K))
    for j, h in enumerate(harmonics):
        y += resynth_partial_exact(ah, k, h, sr, nwind, nhop, col=j, q=q, K=K)
    return y, resynth_bound(ah, len(K), nwind, nhop)


# ---- which frames see the seams of the device's phase scan, and a model of that scan -------------------------------------
def scan_frames(n, wlen, hop, tile=2048, lanes=256):
    """frames checked on a long signal: the first, the last, and every frame whose window holds a sample that starts a tile of the
    scan, for the first three tiles after tile 0, the last two, and every tile that starts a round of `lanes` tile sums"""
    nfr = nframes(n, wlen, hop)
    last = (n - 1) // tile
    marks = {tile * j for j in (1, 2, 3, last - 1, last) if j >= 1} | set(range(lanes * tile, n, lanes * tile))
    sel = {0, nfr - 1}
    for b in marks:
        if b < n:
            sel.update(i for i in range(max(0, -(-(b - wlen + 1) // hop)), b // hop + 1) if i < nfr)
    return np.array(sorted(sel), dtype=np.int64)


SCAN_SLIPS = ("carry", "inclusive", "last_tile", "index")


def scan_model(fvec, tile=2048, lanes=256, slip=None):
    """np.cumsum(fvec) the way the device adds it: sums of `tile` samples, an exclusive scan of those sums in rounds of `lanes`
    with a running carry, every tile scanned on top of its offset.  slip (one of SCAN_SLIPS) makes one deliberate mistake:
    'carry' drops the carry from the second round on, 'inclusive' uses inclusive tile offsets, 'last_tile' gives a partial
    last tile the offset of the tile before it, 'index' is off by one element (cyc[t] = sum(fvec[:t]))."""
    assert slip is None or slip in SCAN_SLIPS
    fvec = np.asarray(fvec, dtype=float)
    n = len(fvec)
    nt = -(-n // tile)
    tiles = np.zeros(nt * tile)
    tiles[:n] = fvec
    tiles = tiles.reshape(nt, tile)
    tsum = np.sum(tiles, axis=1)
    off, carry = np.zeros(nt), 0.0
    for base in range(0, nt, lanes):
        inc = np.cumsum(tsum[base:base + lanes])
        ex = inc if slip == "inclusive" else np.concatenate(([0.0], inc[:-1]))
        off[base:base + lanes] = (0.0 if slip == "carry" and base > 0 else carry) + ex
        carry += inc[-1]
    if slip == "last_tile" and n % tile and nt > 1:
        off[-1] = off[-2]
    cyc = (off[:, None] + np.cumsum(tiles, axis=1)).reshape(-1)[:n]
    return np.concatenate(([0.0], cyc[:-1])) if slip == "index" else cyc


# ---- the seeded inputs that the CPU sensitivity test and the GPU test of the scan share -----------------------------------
SR = 8192
SCAN_NS = (2047, 2048, 2049, 4097, 524287, 524288, 524289, 1048581)
SCAN_WLEN, SCAN_HOP, SCAN_NHARM = 511, 100, 9


def random_ah(rng, nfr, nharm):
    return rng.standard_normal((nfr, nharm)) + 1j * rng.standard_normal((nfr, nharm))


def scan_case(n):
    """k, fvec, the signal x and a random ah for the scan test of n samples (seeded by n)"""
    rng = np.random.default_rng(n)
    k, fvec = dyadic_track(rng, n, 0.01, 0.06)
    x = rng.standard_normal(n)
    return {"k": k, "fvec": fvec, "x": x, "ah": random_ah(rng, nframes(n, SCAN_WLEN, SCAN_HOP), SCAN_NHARM),
            "frames": scan_frames(n, SCAN_WLEN, SCAN_HOP)}
