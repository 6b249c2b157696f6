"""Fricative descriptors on the GPU: FricativeDataFromSnip of pypevoc/speech/SpeechAnalysis.py (:349-384) for many snippets
of one signal in one call, and the two batched primitives under it -- a Welch power spectrum with scipy's conventions
(scipy.signal.welch's defaults: periodic Hann window, half overlap, every segment's mean removed, one-sided density) and the
descriptors of a power-spectrum row (refined position of the maximum, the spectral slopes either side of it in dB/kHz, the
four distribution moments).  The stubs of FricativeDataFromSnip and FricativeDataFromWav in SpeechAnalysis stay as they
are; the working functions live here.

Everything per snippet runs in libpvx_hip (pvx_welch, pvx_fric_desc, pvx_fricative; k_fric.hip, FRICATIVES.md): nothing per
snippet or per segment happens in Python, no scipy is imported, and there is no CPU fallback.  welch_rows is the detrended
auto spectrum; the detrended cross spectrum (TransferFunctions.tfe_sig's default) is still open.

Deviations from the reference.  Nothing is clamped; `status` carries, per row,
  1  the maximum is at an end bin: the side of the fit that has one point gives nan for its slope (numpy returns a
     rank-deficient minimum-norm answer there); with the maximum at the last bin the reference raises IndexError in
     refine_max, here f_max = freq[-1];
  2  a bin of the spectrum is zero, negative or not finite: every output that reads that bin's logarithm is nan; a row whose
     sum is zero is nan throughout, except rms;
  4  (fricative_intervals) the window does not lie inside the signal: the row is all nan, and nothing is read.
A snippet shorter than nwind uses nper = len(w), as scipy does, without the warning."""
import ctypes

import numpy as np

from .. import _lib

KEYS = ("f_max", "slope_left", "slope_right", "cent", "stdev", "skew", "kurt")      # the columns of pvx_fricative's desc
REFERENCE_KEYS = ("f_max", "rms", "slope_left", "slope_right", "cent", "stdev", "skew", "kurt")
STATUS_END_PEAK, STATUS_BAD_BIN, STATUS_OUTSIDE = 1, 2, 4


def last_kernels():
    """The kernels the calling thread's last device call of this module ran: 'k_fric_fused<1024>+k_fric_desc+k_fric_rms',
    'k_fric_frames+rocfft+k_fric_acc', 'k_fric_desc' ('' when it had no row)."""
    return _lib.load().pvx_fric_last_kernels().decode()


def geometry(length, nwind):
    """(nper, step, nseg, nbins) of scipy.signal.welch's defaults on `length` samples: nper = min(nwind, length), half
    overlap, nseg = (length - noverlap) // step."""
    nper = min(int(nwind), int(length))
    nov = nper // 2
    step = nper - nov
    return nper, step, (int(length) - nov) // step, nper // 2 + 1


def hann_periodic(n):
    """scipy.signal.get_window('hann', n): the periodic Hann window, with general_cosine's own arithmetic."""
    fac = np.linspace(-np.pi, np.pi, int(n) + 1)
    return (0.5 + 0.5 * np.cos(fac))[:-1]


def _window(window, nper):
    if window is None:
        return hann_periodic(nper)
    window = np.ascontiguousarray(window, dtype=np.float64)
    if window.shape != (nper,):
        raise ValueError("the window must have nper = min(nwind, length) = %d values" % nper)
    return window


def _i32p(a):
    return None if a is None else a.ctypes.data_as(_lib.c_int32_p)


def _f64p(a):
    return None if a is None else _lib.dptr(a)


def _run(x, starts, length, nwind, sr, window, want_psd, want_desc):
    """pvx_welch / pvx_fricative (or their _dev forms for a signal on the GPU): (freq, psd or None, desc, imax, status, rms)
    as host arrays, the last four None unless want_desc."""
    lib = _lib.load()
    _lib.init()
    starts = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
    nrows, length, nwind, sr = len(starts), int(length), int(nwind), float(sr)
    if length < 2 or nwind < 2:                                      # (the library's own answer: no geometry to size the arrays by)
        raise _lib.PvxError("pvx_fricative failed (status %d): snippets of %d samples, nwind %d (at least 2 are needed)"
                            % (_lib.PVX_ERR_SIZE, length, nwind))
    nper, _, _, nb = geometry(length, nwind)
    win = _window(window, nper)
    freq = np.fft.rfftfreq(nper, 1 / sr)
    sp = starts.ctypes.data_as(_lib.c_int64_p)
    if _lib.is_device_array(x):
        import torch
        sx = _lib.DeviceSignal(x)
        if len(sx.shape) != 1:
            raise ValueError("a 1-D signal is expected")
        dev = _lib.bound_torch_device()   # the outputs and the stream must be the bound device's
        n = int(sx.shape[0])
        dpsd = torch.empty(max(nrows * nb, 1), dtype=torch.float64, device=dev) if want_psd else None
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        pp = ctypes.c_void_p(dpsd.data_ptr()) if want_psd else None
        if want_desc:
            ddesc = torch.empty(max(nrows * 7, 1), dtype=torch.float64, device=dev)
            dimax = torch.empty(max(nrows, 1), dtype=torch.int32, device=dev)
            dstat = torch.empty(max(nrows, 1), dtype=torch.int32, device=dev)
            drms = torch.empty(max(nrows, 1), dtype=torch.float64, device=dev)
            got = _lib.check(lib.pvx_fricative_dev(ctypes.c_void_p(sx.ptr), sx.dtype_code, n, sp, nrows, length, nwind, _lib.dptr(win), sr,
                                                   _lib.dptr(freq), pp, *[ctypes.c_void_p(t.data_ptr()) for t in (ddesc, dimax, dstat, drms)],
                                                   stream), "pvx_fricative_dev")
            desc = ddesc.cpu().numpy()[:nrows * 7].reshape(nrows, 7)
            imax, status, rms = dimax.cpu().numpy()[:nrows], dstat.cpu().numpy()[:nrows], drms.cpu().numpy()[:nrows]
        else:
            got = _lib.check(lib.pvx_welch_dev(ctypes.c_void_p(sx.ptr), sx.dtype_code, n, sp, nrows, length, nwind, _lib.dptr(win), sr, pp,
                                               stream), "pvx_welch_dev")
            desc = imax = status = rms = None
        psd = dpsd.cpu().numpy()[:nrows * nb].reshape(nrows, nb) if want_psd else None
    else:
        xs, code = _lib.as_signal(x)
        if xs.ndim != 1:
            raise ValueError("a 1-D signal is expected")
        n = len(xs)
        psd = np.empty((nrows, nb)) if want_psd else None
        if want_desc:
            desc, imax, status, rms = np.empty((nrows, 7)), np.empty(nrows, dtype=np.int32), np.empty(nrows, dtype=np.int32), np.empty(nrows)
            got = _lib.check(lib.pvx_fricative(ctypes.c_void_p(xs.ctypes.data), code, n, sp, nrows, length, nwind, _lib.dptr(win), sr,
                                               _lib.dptr(freq), _f64p(psd), _lib.dptr(desc), _i32p(imax), _i32p(status), _lib.dptr(rms)),
                             "pvx_fricative")
        else:
            desc = imax = status = rms = None
            got = _lib.check(lib.pvx_welch(ctypes.c_void_p(xs.ctypes.data), code, n, sp, nrows, length, nwind, _lib.dptr(win), sr, _f64p(psd)),
                             "pvx_welch")
    if got != nrows:
        raise _lib.PvxError("pvx_fricative returned %d rows for %d" % (got, nrows))
    return freq, psd, desc, imax, status, rms


def welch_rows(x, starts, length, nwind=256, sr=1.0, window=None):
    """scipy.signal.welch(x[s : s + length], fs=sr, nperseg=nwind) for every s of starts, in one device call: (freq [nb],
    psd [len(starts)][nb]), nb = min(nwind, length) // 2 + 1.  x: a host array (float64 / float32 / int16) or a 1-D signal
    already on the GPU; window: None for the periodic Hann window, or an array of min(nwind, length) values."""
    freq, psd = _run(x, starts, length, nwind, sr, window, True, False)[:2]
    return freq, psd


def _as_dict(desc, imax, status):
    d = dict((k, np.ascontiguousarray(desc[:, i])) for i, k in enumerate(KEYS))
    d["imax"] = imax
    d["status"] = status
    return d


def fricative_desc_rows(psd, freq):
    """The descriptors of every row of psd [n][nb] over the common axis freq [nb], nb >= 2: a dict of arrays with the keys
    f_max, slope_left, slope_right, cent, stdev, skew, kurt, imax and status.  On the psd rows of fricative_rows it returns
    that call's values bit for bit."""
    psd = np.ascontiguousarray(psd, dtype=np.float64)
    freq = np.ascontiguousarray(freq, dtype=np.float64)
    if psd.ndim != 2 or freq.shape != (psd.shape[1],):
        raise ValueError("rows [n][nb] and their axis [nb] are expected")
    lib = _lib.load()
    _lib.init()
    n, nb = psd.shape
    desc, imax, status = np.empty((n, 7)), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    got = _lib.check(lib.pvx_fric_desc(_lib.dptr(psd), n, nb, _lib.dptr(freq), _lib.dptr(desc), _i32p(imax), _i32p(status)), "pvx_fric_desc")
    assert got == n, (got, n)
    return _as_dict(desc, imax, status)


def fricative_rows(x, starts, length, nwind=256, sr=1.0, window=None, return_psd=False):
    """FricativeDataFromSnip(x[s : s + length], nwind, sr) for every s of starts, in one device call: a dict of arrays
    [len(starts)] with the reference's eight keys (f_max, rms, slope_left, slope_right, cent, stdev, skew, kurt) plus imax
    and status (the module's docstring), and psd [len(starts)][nb] / freq [nb] with return_psd."""
    freq, psd, desc, imax, status, rms = _run(x, starts, length, nwind, sr, window, bool(return_psd), True)
    d = _as_dict(desc, imax, status)
    d["rms"] = rms
    if return_psd:
        d["psd"], d["freq"] = psd, freq
    return d


def FricativeDataFromSnip(w, nwind=256, sr=1):
    """The reference's dict of eight Python floats for the snippet w: row 0 of fricative_rows(w, [0], len(w), nwind, sr)."""
    n = int(_lib.DeviceSignal(w).shape[0]) if _lib.is_device_array(w) else len(w)
    rows = fricative_rows(w, [0], n, nwind, sr)
    return dict((k, float(rows[k][0])) for k in REFERENCE_KEYS)


def interval_windows(intervals, sr, pos=(0.5,), wsize=1024):
    """The windows FricativeDataFromWav (:386-423) evidently means, as sample indices: imin [len(intervals)][len(pos)] (every
    window is wsize samples long).  For (st, end) and pp: imed = int((st + (end - st) pp) sr), imin = int(imed - wsize/2),
    imax = int(imed + wsize/2); if imin < st sr: imin = int(st sr), imax = imin + wsize; if imax > end sr: imax = int(end sr),
    imin = imax - wsize."""
    out = np.empty((len(intervals), len(pos)), dtype=np.int64)
    for i, (st, end) in enumerate(intervals):
        for j, pp in enumerate(pos):
            imed = int((st + (end - st) * pp) * sr)
            imin = int(imed - wsize / 2)
            imax = int(imed + wsize / 2)
            if imin < st * sr:
                imin = int(st * sr)
                imax = imin + wsize
            if imax > end * sr:
                imax = int(end * sr)
                imin = imax - wsize
            out[i, j] = imin
    return out


def fricative_intervals(w, sr, intervals, pos=(0.5,), wsize=1024):
    """What FricativeDataFromWav evidently means, on an array -- a restatement of intent: the reference's function cannot run
    (undefined names, a list as a dict key).  One window of wsize samples per (st, end) of intervals (seconds) and per
    relative position pp of pos (interval_windows), all of them through one fricative_rows call with nwind = wsize:
    {pp: dict of arrays over the intervals}.  A window that does not lie inside the signal gives a row of nan with status 4.
    Pre-emphasis stays with the caller (pypevoc_amd.FFTFilters.preemph); reading the wav file is not mirrored."""
    wsize = int(wsize)
    pos = tuple(pos)
    n = int(_lib.DeviceSignal(w).shape[0]) if _lib.is_device_array(w) else len(w)
    imin = interval_windows(intervals, sr, pos, wsize)
    inside = (imin >= 0) & (imin + wsize <= n)
    rows = fricative_rows(w, imin[inside], wsize, wsize, sr)
    out = {}
    for j, pp in enumerate(pos):
        d = {}
        for k in REFERENCE_KEYS + ("imax", "status"):
            full = np.full(imin.shape, -1 if k == "imax" else (STATUS_OUTSIDE if k == "status" else np.nan),
                           dtype=rows[k].dtype)
            full[inside] = rows[k]
            d[k] = full[:, j]
        out[pp] = d
    return out
