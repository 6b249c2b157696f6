"""The spectral-envelope half of pypevoc/speech/SpeechAnalysis.py's formant tracker on the GPU: lpc2form_full (:211-218) and
Formants(full=True) (:298-311), and the batched PeakFinder(y, x).refine_all() (pypevoc/PeakFinder.py:331-413) they rest on.
The stubs of those names in SpeechAnalysis and formants.Formants(full=True) stay as they are; the working functions live
here.

The envelope |1 / A(e^jw)| of every frame's LPC polynomial on npts points, the scan for its peaks and their three-point
refinement run in libpvx_hip (pvx_lpc_envelope, pvx_peaks_refine; k_lpcenv.hip, pvx_peakref.h, ENVELOPE.md), one wave per
frame: nothing per frame or per peak happens in Python, no scipy is imported, and there is no CPU fallback.  The host
matches the formants to the peaks as one numpy pass over [frames][columns].

Formants(full=True) runs formants' device half with the LPC rows kept, then the envelope pass on them.  For a signal on the
GPU the rows stay there and pvx_lpc_envelope_dev reads them in place; for a host signal they cross the link twice, at
(order + 1) * 8 bytes per frame each way.

Deviations from the reference, beyond formants': a frame whose envelope has more than `order` peaks (rounding noise on a
flat stretch; |A|^2 is a polynomial of degree `order` in cos w, so an envelope has fewer than `order` interior maxima)
raises PvxError naming the frame; a root of A on the unit circle at a grid point gives inf there, as in scipy, and is not
handled."""
import ctypes

import numpy as np

from .. import _lib
from . import formants
from .SpeechAnalysis import hamming

ENV_MAX_NPTS = 16384                                                  # PVX_ENV_MAX_NPTS of include/pvx.h
ROOTS_MAX_ORDER = formants.ROOTS_MAX_ORDER


def last_kernels():
    """The kernels the calling thread's last envelope / peak call ran: 'k_lpc_envelope', 'k_peaks_refine' ('' when it
    launched nothing)."""
    return _lib.load().pvx_envelope_last_kernels().decode()


def _check(rc, what, over):
    if rc == _lib.PVX_ERR_SIZE:
        raise _lib.PvxError("%s failed (status %d): row %d has more peaks than its list holds: %s"
                            % (what, rc, over.value, (_lib.load().pvx_last_error() or b"").decode()))
    return _lib.check(rc, what)


def _i32p(a):
    return None if a is None else a.ctypes.data_as(_lib.c_int32_p)


def _f64p(a):
    return None if a is None else _lib.dptr(a)


def _lists(n, maxpk):
    return (np.empty(n, dtype=np.int32), np.empty((n, maxpk), dtype=np.int32), np.empty((n, maxpk)), np.empty((n, maxpk)))


def _rows(coef):
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    if coef.ndim != 2 or coef.shape[1] < 2:
        raise ValueError("coefficient rows [n][order + 1] with order >= 1 are expected")
    return coef


def _envelope_run(coef, npts, Fs, maxpk, want_env, want_peaks):
    """pvx_lpc_envelope on host coefficient rows [n][order + 1]: (env or None, (npk, idx, pos, val) or None)."""
    coef = _rows(coef)
    lib = _lib.load()
    _lib.init()
    n, order = coef.shape[0], coef.shape[1] - 1
    env = np.empty((n, int(npts))) if want_env else None
    npk, idx, pos, val = _lists(n, maxpk) if want_peaks else (None,) * 4
    over = ctypes.c_int64(-1)
    rc = lib.pvx_lpc_envelope(_lib.dptr(coef), n, order, int(npts), float(Fs), int(maxpk), _f64p(env), _i32p(npk), _i32p(idx), _f64p(pos),
                              _f64p(val), ctypes.byref(over))
    _check(rc, "pvx_lpc_envelope", over)
    assert rc == n, (rc, n)
    return env, ((npk, idx, pos, val) if want_peaks else None)


def _envelope_run_dev(d_coef, n, order, npts, Fs, maxpk):
    """pvx_lpc_envelope_dev on the flat float64 device tensor d_coef of n rows [order + 1]: npk, idx, pos, val as host arrays."""
    import torch
    lib = _lib.load()
    dev = d_coef.device
    npk = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    idx = torch.empty(max(n * maxpk, 1), dtype=torch.int32, device=dev)
    pos = torch.empty(max(n * maxpk, 1), dtype=torch.float64, device=dev)
    val = torch.empty(max(n * maxpk, 1), dtype=torch.float64, device=dev)
    over = ctypes.c_int64(-1)
    rc = lib.pvx_lpc_envelope_dev(ctypes.c_void_p(d_coef.data_ptr()), n, order, int(npts), float(Fs), int(maxpk), None,
                                  *[ctypes.c_void_p(t.data_ptr()) for t in (npk, idx, pos, val)], ctypes.byref(over),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _check(rc, "pvx_lpc_envelope_dev", over)
    assert rc == n, (rc, n)
    return (npk.cpu().numpy()[:n], idx.cpu().numpy()[:n * maxpk].reshape(n, maxpk), pos.cpu().numpy()[:n * maxpk].reshape(n, maxpk),
            val.cpu().numpy()[:n * maxpk].reshape(n, maxpk))


def envelope_frames(coef, npts=1024):
    """abs(freqz([1], row, worN=npts)[1]) of every row of coef [n][order + 1] ([1, a_1 .. a_order], order <= 64; the
    leading coefficient need not be 1 but must not be 0): [n][npts], 3 <= npts <= 16384."""
    return _envelope_run(coef, npts, 1.0, 0, True, False)[0]


def envelope_peaks_frames(coef, Fs=1.0, npts=1024):
    """The refined peaks of every row's envelope on the axis k Fs / (2 npts): npk [n], idx [n][order] (-1 beyond npk), pos
    and val [n][order] (NaN beyond npk).  A row with more than `order` peaks raises PvxError."""
    coef = _rows(coef)
    return _envelope_run(coef, npts, Fs, coef.shape[1] - 1, False, True)[1]


def peaks_frames(y, x=None, sel=None):
    """PeakFinder(row, x).refine_all() of every row of y [n][npts]: npk [n], idx [n][maxpk] (-1 beyond npk), pos and val
    [n][maxpk] (NaN beyond npk), maxpk = (npts - 1) // 2.  x: the rows' common axis [npts] (None: arange).  sel [n][maxpk']
    (int, -1 padded): these indices are refined instead of the scan's, slot by slot, and maxpk = maxpk'."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim != 2:
        raise ValueError("rows [n][npts] are expected")
    n, npts = y.shape
    if x is not None:
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (npts,):
            raise ValueError("the axis must have the rows' length")
    if sel is not None:
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        if sel.ndim != 2 or sel.shape[0] != n:
            raise ValueError("sel [n][maxpk] is expected")
        maxpk = sel.shape[1]
    else:
        maxpk = max(npts - 1, 0) // 2
    lib = _lib.load()
    _lib.init()
    npk, idx, pos, val = _lists(n, maxpk)
    over = ctypes.c_int64(-1)
    rc = lib.pvx_peaks_refine(_lib.dptr(y), n, npts, _f64p(x), maxpk, _i32p(sel), _i32p(npk), _i32p(idx), _f64p(pos), _f64p(val),
                              ctypes.byref(over))
    _check(rc, "pvx_peaks_refine", over)
    assert rc == n, (rc, n)
    return npk, idx, pos, val


def lpc2form_full(a, Fs=1.0, npts=1024):
    '''
    Convert all-pole coefficients to resonance frequencies and bandwidths (formants.lpc2form), and the refined peaks of the
    spectral envelope on npts points (SpeechAnalysis.py:211-218)

    a: LPC coefficients (all-pole coefficients excluding order 0)
    Fs: sampling rate

    returns FreqS, BW, the peaks' frequencies and their amplitudes
    '''
    a = np.asarray(a, dtype=np.float64)
    FreqS, BW = formants.lpc2form(a, Fs)
    if len(a) == 0:                                                   # a constant envelope has no peak
        return FreqS, BW, np.zeros(0), np.zeros(0)
    npk, _, pos, val = envelope_peaks_frames(np.concatenate(([1.0], a))[None, :], Fs, npts)
    return FreqS, BW, pos[0, :npk[0]], val[0, :npk[0]]


def match_peaks(Form, npk, pkF, pkA):
    """Peaks, Amplitudes [frames][cols] of Formants(full=True) (SpeechAnalysis.py:307-311): for each formant Form[f, c] that
    is not NaN the frequency and amplitude of the peak of frame f nearest to it -- the first of equally near ones, as
    np.argmin --, NaN where the frame has no peak.  pkF, pkA [frames][maxpk], a row's first npk entries valid."""
    Form = np.asarray(Form, dtype=np.float64)
    pkF, pkA = np.asarray(pkF, dtype=np.float64), np.asarray(pkA, dtype=np.float64)
    npk = np.asarray(npk).astype(np.int64)
    Peaks = np.nan * np.ones(Form.shape)
    Amplitudes = np.nan * np.ones(Form.shape)
    if Form.size == 0 or pkF.shape[1] == 0:
        return Peaks, Amplitudes
    valid = np.arange(pkF.shape[1])[None, :] < npk[:, None]           # [frames][maxpk]
    with np.errstate(invalid="ignore"):
        dist = np.abs(pkF[:, None, :] - Form[:, :, None])            # [frames][cols][maxpk]
    dist = np.where(valid[:, None, :], dist, np.inf)
    # np.argmin returns the first NaN where there is one: a NaN distance of a valid peak must win as it does there
    key = np.where(np.isnan(dist), -1.0, dist)
    pick = np.argmin(key, axis=2)                                     # [frames][cols]
    ok = ~np.isnan(Form) & (npk[:, None] > 0)
    rows = np.arange(Form.shape[0])[:, None]
    Peaks[ok] = pkF[rows, pick][ok]
    Amplitudes[ok] = pkA[rows, pick][ok]
    return Peaks, Amplitudes


def Formants(w, Fs, tWind=0.025, tHop=0.0125,
             fMin=50, fMax=5500, bwMax=400,
             modelOrd=10, hpFreq=50, full=False):
    '''Estimate formants from waveform w with sample rate Fs

       w:          signal (a host array, or a float32 / float64 / int16 signal on the GPU); not modified
       tWind:      window length in seconds
       tHop:       hop length in seconds
       fMin:       minimum frequency of formant in Hz
       fMax:       maximum frequency of formant in Hz
                    (determines resampling rate)
       bwMax:      maximum bandwidth (Hz)
       modelOrder: model order for linear prediction (LPC)
       hpFreq:     > 0 switches the pre-emphasis w[i] - w[i+1] on (its value
                    is not used, as in the reference)
       full:       also the frequency and amplitude of the peak of the LPC spectral envelope
                    (1024 points) nearest to each formant

       returns Time [frames], Form and BandWidths [frames][int(modelOrd/2)], NaN where a frame has fewer formants;
       with full also Peaks and Amplitudes of the same shape
    '''
    if not full:
        return formants.Formants(w, Fs, tWind, tHop, fMin, fMax, bwMax, modelOrd, hpFreq)
    n = formants.glottal._signal(w)[2]
    down, wLen, FsN, nwind, hop, nFrames, Time = formants.geometry(n, Fs, tWind, tHop, fMax)
    ncols = int(modelOrd / 2)
    if nFrames == 0:
        return (Time,) + tuple(np.nan * np.ones((0, ncols)) for _ in range(4))
    if modelOrd > nwind:
        raise ValueError('Order must be smaller than size of vector')
    dev_rows = {"lpc": None}                                          # on the GPU the rows stay there
    rows = formants._formants_run(w, hpFreq > 0, down, formants.firwin_np(down) if down > 1 else None, hamming(nwind), hop, nFrames,
                                  modelOrd, FsN, want=("nkept", "freq", "bw", "lpc"), dev_rows=dev_rows)
    order = int(modelOrd)
    if dev_rows["lpc"] is not None:
        npk, _, pkF, pkA = _envelope_run_dev(dev_rows["lpc"], nFrames, order, 1024, FsN, order)
    else:
        npk, _, pkF, pkA = _envelope_run(rows["lpc"], 1024, FsN, order, False, True)[1]
    Form, BandWidths = formants.select(rows["nkept"], rows["freq"], rows["bw"], fMin, fMax, bwMax, ncols)
    Peaks, Amplitudes = match_peaks(Form, npk, pkF, pkA)
    return Time, Form, BandWidths, Peaks, Amplitudes
