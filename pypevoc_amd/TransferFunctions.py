"""Drop-ins for pypevoc/TransferFunctions.py: transferogram (:112-185), tfe (:21-26), tfe_sig (:10-15), nextpow2, fft_filter,
smthderiv, and the three names the reference takes from matplotlib.mlab -- psd, csd, cohere -- with mlab's argument order and
return conventions.  Neither matplotlib nor scipy is imported.

What runs per segment -- window, transform, conj(Y) X, |X|^2, |Y|^2 and their means over the segments of a block -- is one call
of pvx_xspec (k_xspec.hip, include/pvx.h; TRANSFER.md) for all the blocks of a call; the scaling, the two divisions and the
transposes are one numpy expression over the (nblk, nbins) result (nothing runs per block in Python), so the nan / zero
patterns of silence are numpy's own.
Signals are host arrays or 1-D float32 / float64 / int16 tensors already on the GPU.  No CPU fallback."""
import ctypes

import numpy as np

from . import _lib

_REF = "pypevoc/TransferFunctions.py"


def nextpow2(number):
    """The largest power of two that does not exceed `number` (>= 1)."""
    return 2 ** int(np.log2(number))


# ---- the device call -------------------------------------------------------------------------------------------------
def last_kernels():
    """The kernels the calling thread's last device call of psd / csd / cohere / tfe / transferogram ran: 'k_xspec_fused<1024>',
    'k_frames+rocfft+k_xspec_rows' (a transferogram without a block makes no device call)."""
    return _lib.load().pvx_xspec_last_kernels().decode()


def nsegments(length, nfft, step):
    """Segments of mlab's sliding window over `length` >= nfft samples."""
    return (int(length) - int(nfft)) // int(step) + 1


def scaling(nfft):
    """mlab's one-sided factor per bin 0 .. nfft//2: 2, but 1 at DC and, for even nfft, at the Nyquist bin."""
    c = np.full(int(nfft) // 2 + 1, 2.0)
    c[0] = 1.0
    if not nfft % 2:
        c[-1] = 1.0
    return c


def frequencies(nfft, fs):
    """mlab's one-sided frequencies (np.fft.fftfreq's own arithmetic; the last one positive)."""
    f = np.fft.fftfreq(int(nfft), 1 / fs)[:int(nfft) // 2 + 1]
    if not nfft % 2:
        f[-1] *= -1
    return f


def block_starts(nsamples, rate, start_time, delta_time, sample_duration):
    """transferogram's blocks (:139-149, :165): their first samples, their length and their times.  The start is subtracted
    twice from the end, as the reference does."""
    sample_start = int(start_time * rate)
    sample_delta = int(delta_time * rate)
    sample_len = int(sample_duration * rate)
    sample_end = nsamples - sample_start - sample_len
    i0 = np.arange(sample_start, sample_end, sample_delta)
    return i0, sample_len, (i0 + sample_len / 2) / float(rate)


def window_geometry(rate, window_duration, window_hop=None):
    """(NFFT, step) of transferogram (:152-158).  window_hop=None means NFFT//2 (the reference's float
    noverlap raises TypeError in mlab)."""
    nfft = nextpow2(window_duration * rate)
    step = nextpow2(window_hop * rate) if window_hop else nfft // 2
    return nfft, step


def _siglen(x):
    return int(_lib.DeviceSignal(x).shape[0]) if _lib.is_device_array(x) else len(x)


def _sigdtype(x):
    return _lib.DeviceSignal(x).dtype if _lib.is_device_array(x) else np.asarray(x).dtype


def _window(window, nfft, dtype):
    if window is None:
        return np.hanning(nfft)
    if not np.iterable(window):
        window = window(np.ones(nfft, dtype))                        # mlab: the callable sees ones of the signal's type
    window = np.ascontiguousarray(window, dtype=np.float64)
    if len(window) != nfft:
        raise ValueError("The window length must match the data's first dimension")
    return window


def _pad(x, nfft):
    """mlab zero-pads a signal shorter than NFFT to one segment."""
    if _lib.is_device_array(x):
        if _siglen(x) < nfft:
            raise ValueError("a device-resident signal shorter than NFFT has to be zero-padded by the caller")
        return x
    x = np.asarray(x)
    if np.iscomplexobj(x):
        raise NotImplementedError("complex signals (mlab's two-sided spectra) are not mirrored (INTEGRATION.md)")
    if x.ndim != 1:
        raise ValueError("a 1-D signal is expected")
    if len(x) < nfft:
        n = len(x)
        x = np.resize(x, nfft)
        x[n:] = 0
    return x


def xspec_run(x, y, wind, step, start, delta, nblk, nseg):
    """pvx_xspec: (sxy, sxx, syy) as host arrays [nblk][nwind//2 + 1], the unscaled means over the nseg segments of every
    block of conj(Y) X (complex128), |X|^2 and |Y|^2; y None: (None, sxx, None).  x, y: host arrays, or both 1-D float32 /
    float64 / int16 signals of one type already on the GPU, read in place.  Raises PvxError without a GPU."""
    lib = _lib.load()
    _lib.init()
    wind = np.ascontiguousarray(wind, dtype=np.float64)
    nwind, step, start, delta, nblk, nseg = len(wind), int(step), int(start), int(delta), max(int(nblk), 0), int(nseg)
    nb = nwind // 2 + 1
    two = y is not None
    if two and _lib.is_device_array(x) != _lib.is_device_array(y):
        raise TypeError("both signals must be host arrays, or both device-resident")
    if _lib.is_device_array(x):
        import torch
        sx = _lib.DeviceSignal(x)
        sy = _lib.DeviceSignal(y) if two else None
        if len(sx.shape) != 1 or (two and len(sy.shape) != 1):
            raise ValueError("1-D signals are expected")
        if two and sy.dtype_code != sx.dtype_code:
            raise TypeError("device-resident signals must share one sample type (got %s and %s)" % (sx.dtype, sy.dtype))
        dev = _lib.bound_torch_device()                              # the outputs and the stream must be the bound device's
        n = min(sx.shape[0], sy.shape[0]) if two else sx.shape[0]
        dxx = torch.empty(max(nblk * nb, 1), dtype=torch.float64, device=dev)
        dyy = torch.empty(max(nblk * nb, 1), dtype=torch.float64, device=dev) if two else None
        dxy = torch.empty(max(2 * nblk * nb, 1), dtype=torch.float64, device=dev) if two else None
        stream = torch.cuda.current_stream()
        got = _lib.check(lib.pvx_xspec_dev(ctypes.c_void_p(sx.ptr), ctypes.c_void_p(sy.ptr) if two else None, sx.dtype_code, n, _lib.dptr(wind),
                                           nwind, step, start, delta, nblk, nseg, ctypes.c_void_p(dxy.data_ptr()) if two else None,
                                           ctypes.c_void_p(dxx.data_ptr()), ctypes.c_void_p(dyy.data_ptr()) if two else None,
                                           ctypes.c_void_p(stream.cuda_stream)), "pvx_xspec_dev")
        sxx = dxx.cpu().numpy()[:nblk * nb]
        syy = dyy.cpu().numpy()[:nblk * nb] if two else None
        sxy = dxy.cpu().numpy()[:2 * nblk * nb] if two else None
    else:
        xs, code = _lib.as_signal(x)
        ys = None
        if two:
            ys, codey = _lib.as_signal(y)
            if codey != code:                                        # one sample type for both: the wider one holds either exactly
                xs, ys, code = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(ys, dtype=np.float64), _lib.PVX_F64
        if xs.ndim != 1 or (two and ys.ndim != 1):
            raise ValueError("1-D signals are expected")
        n = min(len(xs), len(ys)) if two else len(xs)
        sxx = np.empty(nblk * nb)
        syy = np.empty(nblk * nb) if two else None
        sxy = np.empty(2 * nblk * nb) if two else None
        got = _lib.check(lib.pvx_xspec(ctypes.c_void_p(xs.ctypes.data), ctypes.c_void_p(ys.ctypes.data) if two else None, code, n, _lib.dptr(wind),
                                       nwind, step, start, delta, nblk, nseg, _lib.dptr(sxy) if two else None, _lib.dptr(sxx),
                                       _lib.dptr(syy) if two else None), "pvx_xspec")
    if got != nblk:
        raise _lib.PvxError("pvx_xspec returned %d blocks for %d" % (got, nblk))
    sxx = sxx.reshape(nblk, nb)
    if not two:
        return None, sxx, None
    return sxy.view(np.complex128).reshape(nblk, nb), sxx, syy.reshape(nblk, nb)


# ---- mlab's psd / csd / cohere ---------------------------------------------------------------------------------------
def _mlab_args(NFFT, Fs, detrend, noverlap, pad_to, sides, scale_by_freq):
    NFFT = 256 if NFFT is None else int(NFFT)
    Fs = 2 if Fs is None else Fs
    noverlap = 0 if noverlap is None else noverlap
    if noverlap >= NFFT:
        raise ValueError("noverlap must be less than NFFT")
    if int(noverlap) != noverlap:
        raise TypeError("noverlap must be an integer")
    if not (detrend is None or detrend == "none" or getattr(detrend, "__name__", "") == "detrend_none"):
        raise NotImplementedError("detrend other than none is not mirrored (INTEGRATION.md)")
    if not (pad_to is None or pad_to == NFFT):
        raise NotImplementedError("pad_to other than NFFT is not mirrored (INTEGRATION.md)")
    if sides not in (None, "default", "onesided"):
        raise NotImplementedError("sides other than onesided is not mirrored (INTEGRATION.md)")
    if not (scale_by_freq is None or scale_by_freq is True):
        raise NotImplementedError("scale_by_freq=False is not mirrored (INTEGRATION.md)")
    return NFFT, Fs, NFFT - int(noverlap)


def _density(s, nfft, fs, wind):
    """mlab's density of the unscaled mean s [.., nbins], in mlab's order of operations."""
    p = s * scaling(nfft)
    p /= fs
    p /= (wind**2).sum()
    return p


def _one_block(x, y, NFFT, Fs, window, step):
    """The three spectra of whole signals as one block: (sxy, sxx, syy, freqs, wind), each of [nbins]."""
    x = _pad(x, NFFT)
    wind = _window(window, NFFT, _sigdtype(x))
    nseg = nsegments(_siglen(x), NFFT, step)
    if y is not None:
        y = _pad(y, NFFT)
        if nsegments(_siglen(y), NFFT, step) != nseg:
            raise ValueError("the two signals give different numbers of segments (%d and %d)" % (nsegments(_siglen(y), NFFT, step), nseg))
    sxy, sxx, syy = xspec_run(x, y, wind, step, 0, 1, 1, nseg)
    return (None if sxy is None else sxy[0]), sxx[0], (None if syy is None else syy[0]), frequencies(NFFT, Fs), wind


def psd(x, NFFT=None, Fs=None, detrend=None, window=None, noverlap=None, pad_to=None, sides=None, scale_by_freq=None):
    """matplotlib.mlab.psd: (Pxx, freqs), Welch's average periodogram of x as a one-sided density."""
    NFFT, Fs, step = _mlab_args(NFFT, Fs, detrend, noverlap, pad_to, sides, scale_by_freq)
    _, sxx, _, freqs, wind = _one_block(x, None, NFFT, Fs, window, step)
    return _density(sxx, NFFT, Fs, wind), freqs


def csd(x, y, NFFT=None, Fs=None, detrend=None, window=None, noverlap=None, pad_to=None, sides=None, scale_by_freq=None):
    """matplotlib.mlab.csd: (Pxy, freqs), the mean over the segments of conj(X) Y as a one-sided density."""
    NFFT, Fs, step = _mlab_args(NFFT, Fs, detrend, noverlap, pad_to, sides, scale_by_freq)
    sxy, _, _, freqs, wind = _one_block(y, x, NFFT, Fs, window, step)       # the device's first signal is the unconjugated one
    return _density(sxy, NFFT, Fs, wind), freqs


def cohere(x, y, NFFT=256, Fs=2, detrend=None, window=None, noverlap=0, pad_to=None, sides="default", scale_by_freq=None):
    """matplotlib.mlab.cohere: (Cxy, freqs), |Pxy|^2 / (Pxx Pyy)."""
    if _siglen(x) < 2 * NFFT:
        raise ValueError("Coherence is calculated by averaging over *NFFT* length "
                         "segments.  Your signal is too short for your choice of *NFFT*.")
    NFFT, Fs, step = _mlab_args(NFFT, Fs, detrend, noverlap, pad_to, sides, scale_by_freq)
    sxy, syy, sxx, freqs, wind = _one_block(y, x, NFFT, Fs, window, step)   # (device x = y here: its |X|^2 is Pyy)
    with np.errstate(all="ignore"):
        Cxy = np.abs(_density(sxy, NFFT, Fs, wind))**2 / (_density(sxx, NFFT, Fs, wind) * _density(syy, NFFT, Fs, wind))
    return Cxy, freqs


def tfe(y, x, *args, **kwargs):
    """(Pyx / Pxx, freqs): the transfer function from x to y, csd(y, x) over psd(x), in one device pass.  After the two signals
    the arguments are csd's, by position or by name."""
    names = ("NFFT", "Fs", "detrend", "window", "noverlap", "pad_to", "sides", "scale_by_freq")
    if len(args) > len(names):
        raise TypeError("tfe takes at most %d arguments after the signals" % len(names))
    kw = dict(zip(names, args))
    for k in kwargs:
        if k not in names or k in kw:
            raise TypeError("tfe got an unexpected or repeated argument %r" % k)
    kw.update(kwargs)
    window = kw.pop("window", None)
    NFFT, Fs, step = _mlab_args(kw.get("NFFT"), kw.get("Fs"), kw.get("detrend"), kw.get("noverlap"), kw.get("pad_to"), kw.get("sides"),
                                kw.get("scale_by_freq"))
    sxy, sxx, _, freqs, wind = _one_block(x, y, NFFT, Fs, window, step)     # conj(Y) X = csd(y, x); |X|^2 = psd(x)
    with np.errstate(all="ignore"):
        return _density(sxy, NFFT, Fs, wind) / _density(sxx, NFFT, Fs, wind), freqs


def tfe_sig(y, x, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None, detrend="constant", return_onesided=True,
            scaling="density", axis=-1, average="mean"):
    """estimate transfer function from x to y with scipy.signal.csd's conventions (periodic Hann window, nperseg 256, hop
    nperseg//2): csd(y, x) / csd(x, x), returned as (ratio, freqs).  detrend=False is required: scipy's default removes every
    segment's mean, which the device pass does not."""
    if detrend is not False:
        raise NotImplementedError("tfe_sig on the device needs detrend=False: scipy's default detrend='constant' is not mirrored "
                                  "(%s:10-15, INTEGRATION.md)" % _REF)
    if not return_onesided or axis != -1 or average != "mean":
        raise NotImplementedError("tfe_sig: return_onesided=False, axis and average='median' are not mirrored (INTEGRATION.md)")
    n = min(_siglen(x), _siglen(y))
    if isinstance(window, str):
        if window not in ("hann", "hanning"):
            raise NotImplementedError("tfe_sig: named windows other than 'hann' are not mirrored; pass the window as an array")
        nperseg = min(256 if nperseg is None else int(nperseg), n)
        wind = np.hanning(nperseg + 1)[:-1]                            # scipy's get_window('hann', n): periodic
    else:
        wind = np.ascontiguousarray(window, dtype=np.float64)
        if nperseg is not None and int(nperseg) != len(wind):
            raise ValueError("value specified for nperseg is different from length of window")
        nperseg = len(wind)
    if not (nfft is None or int(nfft) == nperseg):
        raise NotImplementedError("tfe_sig: nfft other than nperseg is not mirrored (INTEGRATION.md)")
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if noverlap >= nperseg:
        raise ValueError("noverlap must be less than nperseg.")
    step = nperseg - noverlap
    sxy, sxx, _ = xspec_run(x, y, wind, step, 0, 1, 1, nsegments(n, nperseg, step))
    with np.errstate(all="ignore"):
        return sxy[0] / sxx[0], np.fft.rfftfreq(nperseg, 1 / fs)


# ---- transferogram ---------------------------------------------------------------------------------------------------
def transferogram(source, target, rate=1, start_time=0., delta_time=1.,
                  sample_duration=.5, window_duration=.125, window_hop=None):
    """resp, freqs, times, coherence = transferogram(source, target, rate, ...)

    The transfer function from `source` to `target` as it changes over time: one Welch estimate (tfe and coherence) per block
    of `sample_duration` seconds, a new block every `delta_time` seconds from `start_time` on.  Within a block the segments are
    `window_duration` seconds long, rounded down to a power of two samples (NFFT), Hann-windowed, and `window_hop` seconds apart,
    rounded down likewise (None: NFFT//2).  All times are in seconds at `rate` samples per second.

    resp       complex128 [NFFT//2 + 1, nblocks]: csd(target, source) / psd(source) of every block
    freqs      [NFFT//2 + 1] in the unit of `rate`
    times      [nblocks]: the middle of every block
    coherence  float64 [NFFT//2 + 1, nblocks]

    target=None: resp is the real power spectral density of `source` per block and coherence has shape (0, nblocks).
    The signals are host arrays or 1-D tensors already on the GPU.  All blocks of the call are one pass of pvx_xspec."""
    n_samples = _siglen(source) if target is None else min(_siglen(source), _siglen(target))
    i0, sample_len, times = block_starts(n_samples, rate, start_time, delta_time, sample_duration)
    nfft, step = window_geometry(rate, window_duration, window_hop)
    if step < 1 or nfft < 2:
        raise ValueError("window_duration and window_hop must span at least two and one samples")
    freq = frequencies(nfft, rate)
    nblk = len(i0)
    if nblk == 0:
        _lib.init()                                                   # host arithmetic, but no CPU fallback either
        return (np.zeros((len(freq), 0), dtype=np.float64 if target is None else np.complex128), freq, times,
                np.zeros((0 if target is None else len(freq), 0)))
    if target is not None and sample_len < 2 * nfft:
        raise ValueError("Coherence is calculated by averaging over *NFFT* length "
                         "segments.  Your signal is too short for your choice of *NFFT*.")
    wind = _window(None, nfft, None)
    start, delta = int(i0[0]), (int(i0[1] - i0[0]) if nblk > 1 else 1)
    if sample_len < nfft:
        # psd of blocks shorter than NFFT: mlab zero-pads each to one segment.  The blocks are laid side by side, padded
        if _lib.is_device_array(source):
            raise ValueError("device-resident blocks shorter than NFFT have to be zero-padded by the caller")
        src = _lib.as_signal(source)[0]
        padded = np.zeros((nblk, nfft), dtype=src.dtype)
        padded[:, :sample_len] = src[i0[:, None] + np.arange(sample_len)[None, :]]
        source, start, delta, nseg = padded.reshape(-1), 0, nfft, 1
    else:
        nseg = nsegments(sample_len, nfft, step)
    sxy, sxx, syy = xspec_run(source, target, wind, step, start, delta, nblk, nseg)
    if target is None:
        return _density(sxx, nfft, rate, wind).T, freq, times, np.zeros((0, nblk))
    with np.errstate(all="ignore"):
        pxy, pxx, pyy = (_density(s, nfft, rate, wind) for s in (sxy, sxx, syy))
        resp = pxy / pxx                                              # tfe(target, source) = csd(target, source) / psd(source)
        coherence = np.abs(pxy)**2 / (pyy * pxx)
    return resp.T, freq, times, coherence.T


# ---- host functions: one numpy pass per call -------------------------------------------------------------------------------
def band_gains(n, bands, gains):
    """The gain of every bin of an n-point FFT for fft_filter: band (lo, hi), in units of the Nyquist rate, covers the bins
    int(lo*n/2) .. int(hi*n/2) - 1 with a linear ramp from its first gain to its second; a later band overrides an earlier one,
    bins no band covers get 0 (the Nyquist bin too, unless hi > 1).  Bin n - k has the gain of bin k, so a real signal stays
    real."""
    n = int(n)
    half = np.zeros(n // 2 + 1)
    for (lo, hi), (g_lo, g_hi) in zip(bands, gains):
        k0, k1 = int(lo * (n / 2)), int(hi * (n / 2))
        ramp = np.linspace(g_lo, g_hi, max(k1 - k0, 0))
        k1 = min(k1, len(half))
        if k1 > k0:
            half[k0:k1] = ramp[:k1 - k0]
    return np.concatenate([half, half[1:(n + 1) // 2][::-1]])


def fft_filter(x, bands, gains):
    """x filtered in the frequency domain: ifft(fft(x) * band_gains(len(x), bands, gains)), returned complex as the reference
    returns it.  fft_filter(x, [(0, 0.1), (0.1, 1.0)], [(1., 1.), (0., 0.)]) is a low pass at a tenth of the Nyquist rate.
    The gains are mirrored exactly onto the negative frequencies; the reference's ramp on that side is one point shorter
    for a band that starts at 0, which only shows where such a band's two gains differ."""
    x = np.asarray(x)
    return np.fft.ifft(np.fft.fft(x) * band_gains(len(x), bands, gains))


def smthderiv(ff, ph, rad=1):
    """d ph / d ff, smoothed: element i is the slope of the least-squares line through the points max(0, i - rad) ..
    min(len, i + rad) - 1 (the reference's window, which ends before i + rad).  Every window at once: an [n, 2 rad] table of
    the points, centred per window.  A window of a single point (element 0 at rad = 1) has no slope: nan."""
    ff = np.asarray(ff, dtype=np.float64)
    ph = np.asarray(ph, dtype=np.float64)
    n = len(ph)
    if n == 0:
        return np.zeros(0)
    rad = min(max(int(rad), 0), n)
    idx = np.arange(n)[:, None] + np.arange(-rad, rad)[None, :]
    live = (idx >= 0) & (idx < n)
    idx = np.clip(idx, 0, n - 1)
    count = live.sum(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        x = np.where(live, ff[:n][idx], 0.0)
        y = np.where(live, ph[idx], 0.0)
        x = np.where(live, x - x.sum(axis=1, keepdims=True) / count, 0.0)
        y = np.where(live, y - y.sum(axis=1, keepdims=True) / count, 0.0)
        return (x * y).sum(axis=1) / (x * x).sum(axis=1)


# ---- not mirrored ------------------------------------------------------------------------------------------------------
def _stub(name, lines, why):
    def f(*args, **kwargs):
        raise NotImplementedError("%s is not mirrored on the device (%s:%s: %s; INTEGRATION.md, 'Not mirrored')" % (name, _REF, lines, why))
    f.__name__ = name
    f.__doc__ = "Not mirrored: %s:%s (%s)." % (_REF, lines, why)
    return f


determineDelay = _stub("determineDelay", "80-109", "full-length time-domain correlations of two signals")
block_delay = _stub("block_delay", "188-196", "a full time-domain correlation per block")
maxdelwind = _stub("maxdelwind", "199-244", "a detrend and a full time-domain correlation per block")
plot_time_freq = _stub("plot_time_freq", "247-261", "a matplotlib image")
