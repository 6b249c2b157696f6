"""Long-double reference of the windowed half spectrum, the derived bound on a float64 FFT of it, the cases and the one
comparator that test_spectrum_refs_cpu.py and test_spectrum_diff_gpu.py share (SPECTRA.md).

The four spectral kernels (k_fbank.hip, k_specdesc.hip, k_xspec.hip, k_fric.hip) each carry their own copy of the float64
single-wave transform and each have a rows route through rocFFT.  None of them exposes the transform, but each can be
driven to report one bin's magnitude; those magnitudes are held here to a direct DFT in np.longdouble at an absolute,
frame-scaled bound, so a bin without signal is compared like any other.

fft_tol (derived, not measured).  Higham, "Accuracy and Stability of Numerical Algorithms", Theorem 24.2: a Cooley-Tukey
FFT of length N = 2^t in floating point has
    ||fl(X) - X||_2 <= t eta / (1 - t eta) ||X||_2,     eta = mu + gamma_4 (sqrt 2 + mu),
mu the absolute error of the stored twiddles and gamma_4 = 4u / (1 - 4u) the cost of one complex multiply-add.  Twiddles
good to one ulp have mu <= u, so eta <= u + 4u (1.415 + u) < 7u; rounded up to 8u.  Two more stages of the same size are
allowed for: one for the untangle of the real transform (a twiddle multiply and two butterflies per bin pair), one for the
window multiply x*w before the transform and the 0.5* / fma steps after it.  With Parseval, ||X||_2 = sqrt(N) ||x w||_2:
    |X_got[k] - X[k]|  <=  ||fl(X) - X||_2  <=  8u (ceil(log2 N) + 2) sqrt(N) ||x w||_2     for every bin k.
A mixed-radix factorisation into 2, 3 and 5 has fewer levels than ceil(log2 N) radix-2 ones, each level one twiddle
multiply and one small DFT whose adds are covered by gamma_4 per radix-2-equivalent level, so the bound stands for every
length whose prime factors are 2, 3 and 5.  A length rocFFT handles by Bluestein's algorithm (333, 999) has no such
derivation here and stays with the 1e-9 tests.  u = 2^-53.

Amplitudes.  The kernels return powers, magnitudes or products, so amplitudes are compared:
    | sqrt(P_got[k]) - |X[k]| |  <=  tol + 4u |X[k]|
(the reverse triangle inequality, and 4u for squaring, adding, scaling and the square root).  For a mean over nseg
segments sqrt(P_got) is nseg^-1/2 times the Euclidean norm over the segments of the magnitudes the kernel had; it is held
to nseg^-1/2 ||(|X_s[k]|)_s|| at sqrt(mean_s tol_s^2), the reverse triangle inequality in R^nseg.

The mean term (fricatives).  The segment mean is removed before the window: the reference is dft_ld(x - mean_ld, w), and a
float64 mean that is off by d moves bin k by d |W[k]|, W the spectrum of the window.  A mean summed as a lane's chain of
N/64 adds, six levels of a wave sum and one division is within gamma_n mean|x| of the true one, n = N/64 + 7,
gamma_n = n u / (1 - n u); int16 samples sum exactly and n = 1 (the division)."""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
PI = LD("3.14159265358979323846264338327950288")                       # 36 digits
FUSED = (512, 1024, 2048)
ROWS_ONLY = (256, 1000, 375)                                           # 375 = 3 5^3: odd and smooth, no Nyquist bin
LENGTHS = FUSED + ROWS_ONLY
DTYPES = {"f64": np.float64, "f32": np.float32, "i16": np.int16}

_TABLE = {}
_MATS = {}                                                             # the twiddle matrices of one N at a time
_REFS = {}


# ---- the reference ---------------------------------------------------------------------------------------------------
def twiddles(N):
    """(cos, sin) of 2 pi m / N for m = 0 .. N-1 in long double."""
    t = _TABLE.get(N)
    if t is None:
        a = (LD(2) * PI * np.arange(N, dtype=LD)) / LD(N)
        t = _TABLE[N] = (np.cos(a), np.sin(a))
    return t


def _matrices(N):
    if N not in _MATS:
        _MATS.clear()
        c, s = twiddles(N)
        m = (np.arange(N // 2 + 1, dtype=np.int64)[:, None] * np.arange(N, dtype=np.int64)[None, :]) % N
        _MATS[N] = (c[m], s[m])
    return _MATS[N]


def dft_ld(frames, wind):
    """(re, im) [F][N//2 + 1] in long double of the half spectrum of frames * wind by the defining sum.  Samples and
    window are converted to long double before the multiply: the rounding of x*w is the implementation's, not the
    reference's.  The twiddles come from the N-entry table, indexed by (k n) % N in integers; any N, odd included.  A bin's
    sum runs over blocks of 128 terms, the blocks added in order: at most 144 long-double roundings deep, 0.07 u."""
    f = np.atleast_2d(np.asarray(frames)).astype(LD)
    xw = f * np.asarray(wind).astype(LD)
    N = xw.shape[1]
    C, S = _matrices(N)
    re = np.zeros((N // 2 + 1, len(xw)), dtype=LD)
    im = np.zeros_like(re)
    for j in range(0, N, 128):
        re += C[:, j:j + 128] @ xw[:, j:j + 128].T
        im -= S[:, j:j + 128] @ xw[:, j:j + 128].T
    return re.T.copy(), im.T.copy()


def fft_tol(N, xw_norm):
    """The absolute bound on |X_got[k] - X[k]| of every bin of a float64 FFT of x*w (the module's docstring):
    8u (ceil(log2 N) + 2) sqrt(N) ||x w||_2.  Only for N whose prime factors are 2, 3 and 5."""
    n = int(N)
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    assert n == 1, "fft_tol is derived for lengths with prime factors 2, 3 and 5 only (got %d)" % N
    return 8.0 * U * (math.ceil(math.log2(N)) + 2) * math.sqrt(N) * np.asarray(xw_norm, dtype=np.float64)


def gamma(n):
    return n * U / (1.0 - n * U)


def mean_chain(N, exact_sums):
    """n of the mean term's gamma_n: N/64 adds of a lane, six levels of the wave sum, the division."""
    return 1.0 if exact_sums else N / 64.0 + 7.0


class Ref(object):
    """re, im, amp [F][K] (long double), xnorm [F] = ||X||_2 = sqrt(N) ||x w||_2, tol [F][1] or [F][K] (float64)."""

    def __init__(self, re, im, xnorm, tol):
        self.re, self.im, self.xnorm, self.tol = re, im, xnorm, tol
        self.amp = np.sqrt(re * re + im * im)


def window_spectrum(wind):
    """|W[k]| of the window, long double."""
    re, im = dft_ld(np.ones(len(wind)), wind)
    return np.sqrt(re * re + im * im)[0]


def spectrum_ref(key, values, wind, demean=False, exact_sums=False):
    """The reference of the frames `values` [F][N] (the sample values the implementation sees) under `wind`, computed once
    per key.  demean: every frame's long-double mean is removed first and the bound carries the mean term."""
    r = _REFS.get(key)
    if r is None:
        v = np.atleast_2d(np.asarray(values, dtype=np.float64)).astype(LD)
        N = v.shape[1]
        w = np.asarray(wind, dtype=np.float64)
        if demean:
            v = v - v.mean(axis=1, keepdims=True)
        re, im = dft_ld(v, w)
        xw = v * w.astype(LD)
        xwn = np.sqrt((xw * xw).sum(axis=1)).astype(np.float64)
        tol = fft_tol(N, xwn)[:, None]
        if demean:
            absmean = np.abs(np.atleast_2d(np.asarray(values, dtype=np.float64))).mean(axis=1)
            tol = tol + gamma(mean_chain(N, exact_sums)) * absmean[:, None] * window_spectrum(w).astype(np.float64)[None, :]
        r = _REFS[key] = Ref(re, im, math.sqrt(N) * xwn, tol)
    return r


def mean_amp(amp):
    """nseg^-1/2 ||(|X_s[k]|)_s||: [S][K] -> [K]."""
    return np.sqrt((amp * amp).mean(axis=0))


def mean_tol(tol, K):
    """sqrt(mean_s tol_s^2): [S][1 or K] -> [K]."""
    t = np.broadcast_to(np.asarray(tol, dtype=np.float64), (len(tol), K))
    return np.sqrt((t * t).mean(axis=0))


# ---- the comparator --------------------------------------------------------------------------------------------------
def check_bins(what, got, ref, tol, scale, rel=None):
    """Asserts |got - ref| <= tol + rel on every bin of every frame, snippet or block (rel: 4u |ref| unless given) and
    returns the worst error in units of u * scale, scale being the frame's ||X||_2 (or whatever the caller measures in).
    got and ref: amplitudes [F][K] (or complex values); tol: absolute, broadcast against them.  Nothing is left out: a
    bin whose reference is exactly zero is compared like any other."""
    cplx = np.iscomplexobj(got) or np.iscomplexobj(ref)
    kind = np.clongdouble if cplx else LD
    got = np.atleast_2d(np.asarray(got).astype(kind))
    ref = np.atleast_2d(np.asarray(ref).astype(kind))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), (what, "not finite")
    err = np.abs(got - ref).astype(LD)
    bound = np.asarray(tol, dtype=np.float64) + (4.0 * U * np.abs(ref).astype(np.float64) if rel is None else np.asarray(rel, dtype=np.float64))
    bound = np.broadcast_to(bound, err.shape)
    assert (bound >= 0).all(), what
    sc = np.broadcast_to(np.asarray(scale, dtype=np.float64).reshape(-1, 1) if np.ndim(scale) == 1 else np.asarray(scale, dtype=np.float64),
                         err.shape)
    over = err > bound
    if over.any():
        f, k = np.unravel_index(int(np.argmax(np.where(over, err / np.maximum(bound, np.finfo(np.float64).tiny), 0))), err.shape)
        raise AssertionError("%s: %d of %d bins beyond the bound; worst frame %d bin %d: got %.17g ref %.17g err %.3e bound %.3e (%.1f u of scale)"
                             % (what, int(over.sum()), err.size, f, k, float(np.abs(got[f, k])), float(np.abs(ref[f, k])),
                                float(err[f, k]), float(bound[f, k]), float(err[f, k] / (U * sc[f, k]))))
    errd = err.astype(np.float64)                                     # (a frame without signal, such as a constant with its mean removed,
    units = np.where(sc > 0, errd / np.where(sc > 0, U * sc, 1.0), np.where(errd > 0, np.inf, 0.0))      # has scale 0: any error there is inf)
    return float(np.max(units))


# ---- the cases -------------------------------------------------------------------------------------------------------
def rect(N):
    return np.ones(N)


def ramp(N):
    """w[n] = 1 + n/N: no symmetry, no zero, exactly representable for N a power of two"""
    return 1.0 + np.arange(N) / float(N)


def asym_window(N):
    w = 0.25 + (np.arange(N) / float(N)) ** 2
    assert np.abs(w - w[::-1]).max() > 0.1 and np.abs(w - w[(N - np.arange(N)) % N]).max() > 0.1
    return w


def tone_bins(N):
    """37, 1, the bin below the last one, and 64 with the bin the untangle pairs it with (N/2 - 64)"""
    h = N // 2
    out = []
    for k in (37, 1, h - 1, 64, h - 64):
        if k not in out:
            out.append(k)
    return out


def impulse_positions(N):
    out = []
    for n0 in (0, 1, 63, 64, 127, 128, N // 2 - 1, N // 2, N - 2, N - 1):
        if n0 not in out:
            out.append(n0)
    return out


def _cos(N, k, scale=1.0):
    n = np.arange(N)
    return scale * np.cos(2 * np.pi * ((k * n) % N) / N)


class Case(object):
    """frames [F][N] float64 sample values; wind [N]; dtypes the sample types the case runs in (the values are rounded to
    the type first and the reference sees the rounded ones); y [F][N] for the cross-spectrum case."""

    def __init__(self, name, N, frames, wind, dtypes, y=None):
        self.name, self.N, self.frames, self.wind, self.dtypes, self.y = name, N, np.atleast_2d(np.asarray(frames, dtype=np.float64)), wind, dtypes, y

    def samples(self, dtype, which="x"):
        """the frames as an array of the sample type"""
        src = self.frames if which == "x" else self.y
        out = src.astype(DTYPES[dtype])
        if dtype == "i16":
            assert np.array_equal(out.astype(np.float64), src), self.name
        return out

    def key(self, dtype, which="x"):
        """the reference's key: sample types that hold the float64 values exactly share one"""
        src = self.frames if which == "x" else self.y
        same = np.array_equal(self.samples(dtype, which).astype(np.float64), src)
        return (self.N, self.name, which, "f64" if same else dtype)

    def ref(self, dtype, which="x", demean=False):
        v = self.samples(dtype, which).astype(np.float64)
        exact = demean and dtype == "i16"                              # (the mean term is the one thing that knows the type)
        return spectrum_ref(self.key(dtype, which) + (demean, exact), v, self.wind, demean=demean, exact_sums=exact)


CASE_NAMES = ("tone", "dc", "nyquist", "impulses", "asym", "i16_full", "dc_tiny")
XSPEC_ONLY = ("loud_quiet",)
_CASES = {}


def _full_scale_tone(N, kf):
    x = np.round(32767.5 * _cosf(N, kf) - 0.5)
    x[np.argmax(x)] = 32767.0
    x[np.argmin(x)] = -32768.0
    return x


def _cosf(N, kf):
    return np.cos(2 * np.pi * kf * np.arange(N) / N)


def get_case(name, N):
    c = _CASES.get((name, N))
    if c is not None:
        return c
    n = np.arange(N)
    all3, two = ("f64", "f32", "i16"), ("f64", "f32")
    if name == "tone":                                                 # every other bin is empty
        c = Case(name, N, [_cos(N, k) for k in tone_bins(N)], rect(N), two)
    elif name == "dc":
        c = Case(name, N, np.ones(N), rect(N), all3)
    elif name == "nyquist":                                            # (odd N: no Nyquist bin, |X[k]| = 1 / |cos(pi k / N)|)
        c = Case(name, N, 1.0 - 2.0 * (n % 2), rect(N), all3)
    elif name == "impulses":                                           # flat at w[n0], one frame per position
        c = Case(name, N, [(n == n0).astype(np.float64) for n0 in impulse_positions(N)], ramp(N), all3)
    elif name == "asym":
        c = Case(name, N, np.random.default_rng(1000 + N).standard_normal((4, N)), asym_window(N), two)
    elif name == "i16_full":                                           # between bins, -32768 and +32767 included
        c = Case(name, N, [_full_scale_tone(N, N // 5 + 0.37), _full_scale_tone(N, N // 3 + 0.61)], np.hanning(N), all3)
        assert c.frames.min() == -32768 and c.frames.max() == 32767
    elif name == "dc_tiny":
        # frame 0: the stress case itself (its mean is 30000 exactly for even N); frame 1: one more on every fifth sample,
        # a mean that float32 cannot hold
        t = 30000.0 + np.round(_cos(N, 11, 3.0))
        c = Case(name, N, [t, t + (n % 5 == 0)], np.hanning(N), all3)
    elif name == "loud_quiet":                                         # x as asym; y: bin-centred tones of amplitude 2^-40
        a = get_case("asym", N)
        c = Case(name, N, a.frames, a.wind, two, y=np.array([_cos(N, 37 + 3 * i, 2.0 ** -40) for i in range(len(a.frames))]))
    else:
        raise KeyError(name)
    _CASES[(name, N)] = c
    return c


def peak_bin(ref_amp_row):
    return int(np.argmax(ref_amp_row))


def probe_bins(N, k0):
    """the bins the ratio and flux tails are probed at"""
    h = N // 2
    out = []
    for k in (0, 1, 63, 64, k0 - 1, k0, k0 + 1, h - 1, h):
        if 0 <= k <= h and k not in out:
            out.append(k)
    return out
