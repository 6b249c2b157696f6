"""Drop-ins for the hop-strided windowed measures of pypevoc/SoundUtils.py that share the analysis
framing: RMSWind (:71-103), Heterodyn (:106-117), HeterodynWithF0Track (:120-138).  The per-frame
reductions run as HIP kernels (k_reduce.hip); building the heterodyning signal is host numpy as in the
reference.  FuncWind (:42-69) runs on the device for the named reducers np.sum / np.mean / np.max / np.min / np.std /
np.var (k_funcwind); an arbitrary Python callable has no device form and raises TypeError.
SpecCentWind (:142-160) and SpecFlux (:196-231) run in k_specdesc.hip (pvx_specdesc, include/pvx.h; SPECDESC.md): the host
folds the reference's bin ranges of the full spectrum onto weights per half-spectrum bin, everything per frame is on the
device.  AvgWind (:163-193) is FuncWind's sum.  aubio_f0yin (:234-261) runs YIN in k_yin.hip (pvx_yin; YIN.md) without the
aubio package; f0yin and f0yin_rows are its wider forms.  No CPU fallback."""
import ctypes

import numpy as np

from . import _lib
from .Heterodyne import heterodyne


def _frame_times(nsam, sr, nwind, nhop):
    nfr = int(_lib.load().pvx_nframes(int(nsam), int(nwind), int(nhop)))
    ist = np.arange(nfr) * int(nhop)
    return (ist + ist + int(nwind)) / 2.0 / float(sr)                # SoundUtils.py:64, 98


_FW_OPS = {"sum": 0, "mean": 1, "max": 2, "amax": 2, "min": 3, "amin": 3, "std": 4, "var": 5}


def _funcwind_op(func):
    """PVX_FW_* of a numpy reducer (np.sum, np.mean, np.max / np.amax, np.min / np.amin, np.std, np.var; the builtins sum /
    max / min count as their numpy namesakes) or a TypeError: other callables would have to run in Python per frame."""
    if isinstance(func, str):
        name = func
    elif any(func is b for b in (sum, max, min)):                    # (identity: `in` would compare an array-like elementwise)
        name = func.__name__
    elif (getattr(func, "__module__", None) or "").split(".")[0] == "numpy" and getattr(np, getattr(func, "__name__", ""), None) is func:
        name = func.__name__
    else:
        name = None
    if name not in _FW_OPS:
        raise TypeError("FuncWind on the device takes np.sum, np.mean, np.max, np.min, np.std or np.var (got %r): "
                        "an arbitrary callable has no device form (INTEGRATION.md)" % (func,))
    return _FW_OPS[name]


def FuncWind(func, x, sr=1, nwind=1024, nhop=512, power=1, windfunc=np.blackman):
    '''
    Applies a function window by window to a time series
    (func: np.sum, np.mean, np.max, np.min, np.std or np.var)
    '''
    op = _funcwind_op(func)
    lib = _lib.load()
    _lib.init()
    x = np.asarray(x)
    cpx = np.iscomplexobj(x)
    x = np.ascontiguousarray(x, dtype=np.complex128 if cpx else np.float64)
    wind = np.ascontiguousarray(windfunc(nwind), dtype=np.float64)
    if power > 0:
        wsumpow = sum(wind ** power)                                 # SoundUtils.py:55-58
    else:
        wsumpow = 1.
    t = _frame_times(len(x), sr, nwind, nhop)
    cout = cpx and op in (0, 1)
    out = np.zeros(len(t), dtype=np.complex128 if cout else np.float64)
    if len(t):
        r = lib.pvx_funcwind(x.view(np.float64).ctypes.data_as(_lib.c_double_p), int(cpx), len(x), _lib.dptr(wind), int(nwind), int(nhop), op,
                             float(wsumpow), out.view(np.float64).ctypes.data_as(_lib.c_double_p))
        _lib.check(r, "pvx_funcwind")
    return out, t


def RMSWind(x, sr=1, nwind=1024, nhop=512, windfunc=np.blackman):
    '''
    Calculates the RMS amplitude amplitude of x, in frames of
    length nwind, and in steps of nhop. windfunc is used as
    windowing function.
    '''
    lib = _lib.load()
    _lib.init()
    x = np.ascontiguousarray(x, dtype=np.float64)
    wind = np.ascontiguousarray(windfunc(nwind), dtype=np.float64)
    t = _frame_times(len(x), sr, nwind, nhop)
    out = np.zeros(len(t))
    if len(t):
        _lib.check(lib.pvx_rms_frames(_lib.dptr(x), len(x), _lib.dptr(wind), int(nwind), int(nhop), _lib.dptr(out)),
                   "pvx_rms_frames")
    return out, t


def _het(x, sinsig, sr, nwind, nhop, windfunc):
    # FuncWind(np.sum, x*sinsig, power=1) * 2 = heterodyne(x, sinsig, windfunc(nwind), nhop)
    hamp, _ = heterodyne(x, sinsig, wind=windfunc(nwind), hop=nhop)
    return hamp, _frame_times(len(x), sr, nwind, nhop)


def Heterodyn(x, f, sr=1, nwind=1024, nhop=512, windfunc=np.blackman):
    '''
    Calculates the amplitude near frequency f in x
    '''
    sinsig = np.exp(2j * np.pi * np.arange(len(x)) * f / float(sr))
    return _het(x, sinsig, sr, nwind, nhop, windfunc)


def HeterodynWithF0Track(x, tf0, f0, sr=1, nwind=1024, nhop=512, windfunc=np.blackman):
    '''
    Calculates the amplitude near frequency f0 in x
    (f0 is time-varying, values given at tf0)
    '''
    tf0 = np.asarray(tf0)
    f0 = np.asarray(f0)
    valid_idx = np.logical_not(np.isnan(f0))
    tx = np.arange(len(x)) / float(sr)
    f0s = np.interp(tx, tf0[valid_idx], f0[valid_idx])
    phs = np.cumsum(2 * np.pi * f0s / sr)
    return _het(x, np.exp(1j * phs), sr, nwind, nhop, windfunc)


# ---- windowed spectral measures (k_specdesc.hip) --------------------------------------------------------------------
SD_RATIO, SD_FLUX, SD_PSD = 0, 1, 2                                   # pvx_specdesc_measure of include/pvx.h
SD_BLOCK = 16                                                         # PVX_SPECDESC_BLOCK


def fold_bins(bins, nwind):
    """How many of the full-spectrum bins `bins` (indexes into range(nwind)) fall onto each half-spectrum bin 0 .. nwind//2:
    bin k and bin nwind - k of a real frame's spectrum share a magnitude."""
    bins = np.asarray(bins, dtype=np.int64)
    c = np.zeros(int(nwind) // 2 + 1)
    np.add.at(c, np.minimum(bins, int(nwind) - bins), 1.0)
    return c


def specdesc_run(x, wind, hop, nfr, measure, a=None, b=None):
    """pvx_specdesc on x: nfr values (ratio, flux) or the mean power of nfr frames over bins 0 .. nwind//2 - 1 (psd), as a
    host float64 array.  x: a host array, or a float32 / float64 / int16 1-D signal already on the GPU (a torch tensor,
    anything with __cuda_array_interface__), read in place.  Raises PvxError without a GPU.  nfr <= 0: an empty array; the
    library is told (last_kernels() is '' afterwards) and launches nothing."""
    lib = _lib.load()
    _lib.init()
    wind = np.ascontiguousarray(wind, dtype=np.float64)
    nwind, hop, nfr = len(wind), int(hop), max(int(nfr), 0)
    nout = nwind // 2 if measure == SD_PSD else nfr
    tabs = [None if t is None else np.ascontiguousarray(t, dtype=np.float64) for t in (a, b)]
    for t in tabs:
        if t is not None and t.shape != (nwind // 2 + 1,):
            raise ValueError("weights per half-spectrum bin must be [%d]: got %r" % (nwind // 2 + 1, t.shape))
    pa, pb = [None if t is None else _lib.dptr(t) for t in tabs]
    if _lib.is_device_array(x):
        import torch
        sig = _lib.DeviceSignal(x)
        if len(sig.shape) != 1:
            raise ValueError("a 1-D signal is expected")
        dout = torch.empty(max(nout, 1), dtype=torch.float64, device=_lib.bound_torch_device())   # the output and the stream must be the bound device's
        stream = torch.cuda.current_stream()
        got = _lib.check(lib.pvx_specdesc_dev(ctypes.c_void_p(sig.ptr), sig.dtype_code, sig.shape[0], _lib.dptr(wind), nwind, hop, nfr, measure,
                                              pa, pb, ctypes.c_void_p(dout.data_ptr()), ctypes.c_void_p(stream.cuda_stream)), "pvx_specdesc_dev")
        out = dout.cpu().numpy()[:nout]
    else:
        xs, code = _lib.as_signal(x)
        if xs.ndim != 1:
            raise ValueError("a 1-D signal is expected")
        out = np.empty(nout)
        got = _lib.check(lib.pvx_specdesc(ctypes.c_void_p(xs.ctypes.data), code, len(xs), _lib.dptr(wind), nwind, hop, nfr, measure, pa, pb,
                                          _lib.dptr(out)), "pvx_specdesc")
    assert got == nfr, (got, nfr)
    return out if nfr else np.zeros(0)


def _siglen(x):
    return int(_lib.DeviceSignal(x).shape[0]) if _lib.is_device_array(x) else len(x)


def last_kernels():
    """The kernels the calling thread's last SpecCentWind / SpecFlux / SpectralMoments ran: 'k_specdesc_fused<1024>',
    'k_frames+rocfft+k_specdesc_rows' ('' when it had no frame)."""
    return _lib.load().pvx_specdesc_last_kernels().decode()


def SpecCentWind(x, sr=1, nwind=1024, nhop=512, windfunc=np.blackman):
    '''
    Calculates the SpectralCentroid of x, in frames of
    length nwind, and in steps of nhop.

    The frames are windowed by np.blackman(nwind) whatever windfunc is: the reference does not hand windfunc on to
    FuncWind (SoundUtils.py:157-158).  Bins 0 .. nwind//2 - 1, frequencies k/nwind*sr.
    '''
    nwind, nhop = int(nwind), int(nhop)
    half = nwind // 2
    a = np.zeros(half + 1)
    b = np.zeros(half + 1)
    a[:half] = np.arange(half) / float(nwind) * sr                    # :150
    b[:half] = 1.0
    nfr = _lib.nframes_host(_siglen(x), nwind, nhop)
    ist = np.arange(nfr) * nhop
    t = (ist + ist + nwind) / 2.0 / float(sr)                         # :66
    return specdesc_run(x, np.blackman(nwind), nhop, nfr, SD_RATIO, a, b), t


def flux_band(sr, nwind, minf=0, maxf=np.inf):
    """The full-spectrum bins SpecFlux sums over (SoundUtils.py:211-216, 225): range(nwind)[minbin:maxbin]."""
    minbin = int(minf / sr * nwind)
    maxbinf = (float(maxf) / sr * nwind)
    if maxbinf > nwind:
        maxbin = nwind
    else:
        maxbin = int(maxbinf)
    return np.arange(nwind)[minbin:maxbin]


def SpecFlux(x, sr=1, nwind=1024, nhop=512, minf=0, maxf=np.inf, windfunc=np.blackman):
    '''
    Calculates the spectral flux between the frames at ist and ist + nhop: the norm of the difference of their magnitude
    spectra over the bins from minf to maxf (bins of the full spectrum: a band above sr/2 counts the mirrored bins)
    '''
    nwind, nhop = int(nwind), int(nhop)
    c = fold_bins(flux_band(sr, nwind, minf, maxf), nwind)
    nfr = _lib.nframes_host(_siglen(x) - nhop, nwind, nhop)          # :218: while iend < nsam - nhop
    ist = np.arange(nfr) * nhop
    t = (ist + ist + nwind + nhop) / 2.0 / float(sr)                  # :226
    return specdesc_run(x, windfunc(nwind), nhop, nfr, SD_FLUX, c), t


def AvgWind(x, sr=1, nwind=1024, nhop=512, windfunc=np.blackman):
    '''
    Calculates the windowed average of x, in frames of
    length nwind, and in steps of nhop: sum(xw)/sum(wind)
    '''
    return FuncWind(np.sum, x, sr=sr, nwind=nwind, nhop=nhop, power=1, windfunc=windfunc)


# ---- YIN f0 tracking (k_yin.hip) ------------------------------------------------------------------------------------
YIN_FALLBACK, YIN_SILENT = 1, 2                                       # PVX_YIN_* of include/pvx.h
YIN_MAX_NWIND = 8192                                                  # PVX_YIN_MAX_NWIND
YIN_DEFAULT_TOLERANCE = 0.15


def yin_lags(nwind, sr, fmin=None, fmax=None):
    """The lag range [lo, hi] f0yin searches (YIN.md, step 3): lo = 2, raised to floor(sr / fmax); hi = nwind//2 - 2, lowered
    to ceil(sr / fmin).  ValueError for nwind < 8 and for an empty range."""
    nwind = int(nwind)
    if nwind < 8:
        raise ValueError("f0yin needs a window of at least 8 samples (got %d)" % nwind)
    L = nwind // 2
    lo, hi = 2, L - 2
    if fmin is not None:
        if not fmin > 0:
            raise ValueError("fmin must be positive (got %r)" % (fmin,))
        hi = min(int(np.ceil(sr / float(fmin))), L - 2)
    if fmax is not None:
        if not fmax > 0:
            raise ValueError("fmax must be positive (got %r)" % (fmax,))
        lo = max(2, int(np.floor(sr / float(fmax))))
    if lo > hi:
        raise ValueError("no lag to search: fmax %r gives lo = %d, fmin %r and nwind %d give hi = %d" % (fmax, lo, fmin, nwind, hi))
    return lo, hi


def yin_frames(nsamp, sr, nwind=1024, hop=512):
    """Frame starts and times of aubio_f0yin's loop (SoundUtils.py:255, 258): starts range(0, nsamp - nwind, hop), times
    (start + nwind/2) / sr."""
    if int(hop) < 1:
        raise ValueError("hop must be at least 1 (got %r)" % (hop,))
    starts = np.arange(0, int(nsamp) - int(nwind), int(hop), dtype=np.int64)
    return starts, (starts + int(nwind) / 2.0) / float(sr)


def _yin_tolerance(tolerance):
    if tolerance is not None:
        if tolerance > 0.0 and tolerance < 1.0:                      # SoundUtils.py:243-247
            return float(tolerance)
        import sys
        sys.stderr.write('Tolerance not set: Out of bounds\n')
    return YIN_DEFAULT_TOLERANCE


def _yin_run(y, starts, nwind, lo, hi, tol, sr):
    """One pvx_yin launch over the frames y[s : s + nwind] for s in starts; host arrays back."""
    nwind = int(nwind)
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    nf = len(starts)
    dev = _lib.is_device_array(y)
    if dev:
        sig = _lib.DeviceSignal(y)
        if len(sig.shape) != 1:
            raise ValueError("a 1-D signal is expected")
        nx = sig.shape[0]
    else:
        y = np.asarray(y)
        if y.ndim != 1:
            raise ValueError("a 1-D signal is expected")
        nx = len(y)
    if nf and (starts.min() < 0 or starts.max() > nx - nwind):
        bad = starts[(starts < 0) | (starts > nx - nwind)][0]
        raise ValueError("the frame starting at %d leaves the signal (%d samples, window %d)" % (int(bad), nx, nwind))
    res = {"freq": np.zeros(nf), "conf": np.zeros(nf), "tau": np.zeros(nf), "flag": np.zeros(nf, dtype=np.int32),
           "pick": np.zeros(nf, dtype=np.int32)}
    if nf == 0:
        return res
    lib = _lib.load()
    _lib.init()
    args = (starts.ctypes.data_as(_lib.c_int64_p), nf, nwind, int(lo), int(hi), float(tol), float(sr))
    if dev:
        import torch
        tdev = _lib.bound_torch_device()                             # the outputs and the stream must be the bound device's
        if sig.dtype != np.float64:                                  # float32 / int16: every value is a float64 value
            y = torch.as_tensor(y, device=tdev).to(torch.float64)
            sig = _lib.DeviceSignal(y)
        dd = torch.empty((3, nf), dtype=torch.float64, device=tdev)
        di = torch.empty((2, nf), dtype=torch.int32, device=tdev)
        stream = torch.cuda.current_stream()
        _lib.check(lib.pvx_yin_dev(ctypes.c_void_p(sig.ptr), nx, *args, ctypes.c_void_p(dd[0].data_ptr()), ctypes.c_void_p(dd[1].data_ptr()),
                                   ctypes.c_void_p(dd[2].data_ptr()), ctypes.c_void_p(di[0].data_ptr()), ctypes.c_void_p(di[1].data_ptr()),
                                   ctypes.c_void_p(stream.cuda_stream)), "pvx_yin_dev")
        hd, hi_ = dd.cpu().numpy(), di.cpu().numpy()
        res.update(freq=hd[0].copy(), conf=hd[1].copy(), tau=hd[2].copy(), flag=hi_[0].copy(), pick=hi_[1].copy())
    else:
        x = np.ascontiguousarray(y, dtype=np.float64)                # float32 / int16 widen exactly
        _lib.check(lib.pvx_yin(_lib.dptr(x), nx, *args, _lib.dptr(res["freq"]), _lib.dptr(res["conf"]), _lib.dptr(res["tau"]),
                               res["flag"].ctypes.data_as(_lib.c_int32_p), res["pick"].ctypes.data_as(_lib.c_int32_p)), "pvx_yin")
    return res


def f0yin_rows(y, starts, nwind, sr, tolerance=None, fmin=None, fmax=None):
    """YIN on the frames y[s : s + nwind] for s in starts (any order, repeats allowed), one launch: a dict of freq, conf,
    tau (the refined period in samples), pick (its integer lag) and flag (YIN_FALLBACK: no dip below the tolerance, the
    arg-min was taken; YIN_SILENT: a silent or constant frame, freq = conf = 0), one entry per start.  y: a host array
    (float64, float32, int16, ...) or a 1-D signal already on the GPU."""
    lo, hi = yin_lags(nwind, sr, fmin, fmax)
    return _yin_run(y, starts, nwind, lo, hi, _yin_tolerance(tolerance), sr)


def f0yin(y, sr, nwind=1024, hop=512, tolerance=None, fmin=None, fmax=None, full=False):
    """f0 by YIN (YIN.md) over the frames of aubio_f0yin's loop: (freq, time, conf), one entry per frame; full=True: a
    dict that adds tau, pick, flag and starts.  tolerance: the threshold of the first-dip rule (None or outside (0, 1):
    0.15); fmin / fmax bound the lags searched."""
    lo, hi = yin_lags(nwind, sr, fmin, fmax)
    nsamp = int(_lib.DeviceSignal(y).shape[0]) if _lib.is_device_array(y) else len(y)
    starts, time = yin_frames(nsamp, sr, nwind, hop)
    res = _yin_run(y, starts, nwind, lo, hi, _yin_tolerance(tolerance), sr)
    if full:
        res.update(time=time, starts=starts)
        return res
    return res["freq"], time, res["conf"]


def aubio_f0yin(y, sr, nwind=1024, hop=512, method='yin', tolerance=None):
    ''' Applies f0 detection to a numpy vector: the reference's entry (SoundUtils.py:234-261) without the aubio package;
    method 'yin' runs f0yin, aubio's other methods are not mirrored
    '''
    if method != 'yin':
        raise NotImplementedError("aubio_f0yin: method %r is not mirrored by pypevoc_amd, only 'yin' (INTEGRATION.md)" % (method,))
    return f0yin(y, sr, nwind=nwind, hop=hop, tolerance=tolerance)


def yin_last_kernels():
    """The kernel the calling thread's last f0yin / f0yin_rows launch ran: 'k_yin', 'k_yin/seg2' or 'k_yin/seg4' (a call without a
    frame launches nothing and leaves this as it was)."""
    return _lib.load().pvx_yin_last_kernels().decode()
