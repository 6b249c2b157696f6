"""The formant tracker of pypevoc/speech/SpeechAnalysis.py on the GPU: Formants (:220-319), lpc (:9-24) and lpc2form
(:186-209), and lpcc2pole of pypevoc/speech/glottal.py (:249-272).  The stubs of those names in SpeechAnalysis and glottal
stay as they are; the working functions live here.

The pre-emphasis, the decimation, the windowed frames, their LPCs and the roots of every frame's polynomial run in
libpvx_hip (pvx_formants, pvx_polyroots; k_formant.hip, pvx_lpc.h, pvx_roots.h, FORMANTS.md), one workgroup per frame, one
wave per polynomial: nothing per frame happens in Python, no scipy is imported, and there is no CPU fallback.  The host
computes, once per call, the frame geometry with the reference's own expressions, the decimation filter (a numpy
restatement of scipy.signal.firwin as resample_poly calls it), the window, and the selection of the formants as one numpy
pass over [frames][order].

Mirrored behaviour worth knowing (FORMANTS.md, "lpc2form's shift"): lpc2form drops the frequencies that are not > 0 but
keeps every bandwidth, so with k roots at angle 0 (positive real or zero roots) frequency j is returned beside the
bandwidth of the root k places before its own.  Formants selects on those pairs.  This module reproduces it.

Deviations from the reference:
  * the caller's array is not modified (the reference pre-emphasises it in place);
  * float32 and int16 samples are widened to float64 before the difference (the reference filters float32 in float32 and
    lets int16 wrap);
  * Formants(full=True) raises NotImplementedError here: it needs PeakFinder.refine_all, and speech/envelope.py's Formants
    runs it (ENVELOPE.md);
  * a polynomial with a zero leading coefficient is refused (np.roots strips leading zeros)."""
import ctypes

import numpy as np

from .. import _lib
from . import glottal
from .SpeechAnalysis import hamming

ROOTS_MAX_ORDER = 64                                                  # PVX_ROOTS_MAX_ORDER of include/pvx.h
LPC_MAX_NWIND = glottal.LPC_MAX_NWIND


def firwin_np(down):
    """The filter of scipy.signal.resample_poly(x, 1, down): firwin(2 * half + 1, 1 / down, window=('kaiser', 5.0)) with
    half = 10 * down, normalised to unit gain at 0 Hz."""
    down = int(down)
    half = 10 * down
    L = 2 * half + 1
    m = np.arange(L) - (L - 1) / 2.0
    c = 1.0 / down
    h = c * np.sinc(c * m) * np.kaiser(L, 5.0)
    return h / h.sum()


def geometry(n, Fs, tWind=0.025, tHop=0.0125, fMax=5500):
    """(underSample, decimated length, Fs, nwind, hop, nFrames, Time) of Formants on n samples at rate Fs, with the
    reference's expressions (SpeechAnalysis.py:251-277).  underSample 0 raises scipy's ValueError, a negative frame count
    numpy's."""
    underSample = int(Fs / fMax / 2)
    if underSample < 1:
        raise ValueError("up and down must be >= 1")
    wLen = -(-int(n) // underSample)
    FsN = int(Fs * wLen / float(n))
    Fsf = float(FsN)
    hop = int(round(FsN * tHop))
    nwind = int(round(FsN * tWind))
    nFrames = int(np.floor((wLen - nwind - 1) / hop))
    if nFrames < 0:
        raise ValueError("negative dimensions are not allowed")
    Time = np.arange(nFrames + 0) * hop / Fsf + nwind / Fsf / 2
    return underSample, wLen, FsN, nwind, hop, nFrames, Time


def select(nkept, freq, bw, fMin, fMax, bwMax, ncols):
    """Form, BandWidths [frames][ncols] from the frames' kept roots: freq / bw [frames][order] in ascending angle, the
    first nkept of a row valid.  lpc2form's FreqS is freq[k0:nkept], k0 the count of frequencies that are not > 0, beside
    BW = bw[:nkept] (unshifted: the reference's pairing); row by row the accepted pairs fill the columns from the left."""
    nkept = np.asarray(nkept).astype(np.int64)
    nfr, order = freq.shape
    j = np.arange(order)[None, :]
    valid = j < nkept[:, None]
    with np.errstate(invalid="ignore"):
        k0 = np.sum(valid & ~(freq > 0), axis=1)
        src = np.minimum(j + k0[:, None], max(order - 1, 0))
        F = np.take_along_axis(freq, src, axis=1)
        cand = (j + k0[:, None]) < nkept[:, None]
        ok = cand & (F > fMin) & (F < fMax - fMin) & (bw < bwMax)
    col = np.cumsum(ok, axis=1) - 1
    Form = np.nan * np.ones((nfr, ncols))
    BandWidths = np.nan * np.ones((nfr, ncols))
    if ok.any() and col[ok].max() >= ncols:
        raise IndexError("index %d is out of bounds for axis 1 with size %d" % (ncols, ncols))
    r = np.nonzero(ok)
    Form[r[0], col[ok]] = F[ok]
    BandWidths[r[0], col[ok]] = bw[ok]
    return Form, BandWidths


def last_kernels():
    """The kernels the calling thread's last Formants / lpc2form / lpcc2pole / roots_frames ran:
    'k_preemph_decim+k_formant_frames', 'k_polyroots' ('' when it launched nothing)."""
    return _lib.load().pvx_formants_last_kernels().decode()


def _check(rc, what, sing, noconv):
    if rc == _lib.PVX_ERR_SINGULAR:
        raise np.linalg.LinAlgError("Singular principal minor (frame %d)" % sing.value)
    if rc == _lib.PVX_ERR_NOCONV:
        raise _lib.PvxError("%s: the root iteration of row %d did not converge" % (what, noconv.value))
    return _lib.check(rc, what)


def _formants_run(x, preemph, down, taps, wind, hop, nfr, order, Fs, want=("nkept", "freq", "bw"), dev_rows=None):
    """pvx_formants on x (a host array, or a float32 / float64 / int16 1-D signal on the GPU, read in place): a dict of
    the rows in `want` (nkept int32 [nfr]; freq, bw, re, im [nfr][order]; lpc [nfr][order + 1]) as host arrays.  dev_rows: a
    dict whose keys name rows that, for a signal on the GPU, are not copied to the host: it receives their flat device
    tensors instead (speech/envelope.py reads the lpc rows there).  For a host signal it is left as it is."""
    lib = _lib.load()
    _lib.init()
    ptr, code, n, keep, on_dev = glottal._signal(x)
    nfr, order, nwind = int(nfr), int(order), len(wind)
    wind = np.ascontiguousarray(wind, dtype=np.float64)
    taps = None if taps is None else np.ascontiguousarray(taps, dtype=np.float64)
    names = ("nkept", "freq", "bw", "re", "im", "lpc")
    shapes = dict(nkept=(nfr,), freq=(nfr, order), bw=(nfr, order), re=(nfr, order), im=(nfr, order), lpc=(nfr, order + 1))
    sing, noconv = ctypes.c_int64(-1), ctypes.c_int64(-1)
    head = (ctypes.c_void_p(ptr), code, n, int(bool(preemph)), int(down), None if taps is None else _lib.dptr(taps),
            0 if taps is None else len(taps), _lib.dptr(wind), nwind, int(hop), nfr, order, float(Fs))
    if on_dev:
        import torch
        dev = _lib.bound_torch_device()   # the outputs and the stream must be the bound device's
        outs = {k: torch.empty(max(int(np.prod(shapes[k])), 1), dtype=torch.int32 if k == "nkept" else torch.float64, device=dev)
                for k in want}
        rc = lib.pvx_formants_dev(*head, *[ctypes.c_void_p(outs[k].data_ptr()) if k in outs else None for k in names],
                                  ctypes.byref(sing), ctypes.byref(noconv), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _check(rc, "pvx_formants_dev", sing, noconv)
        stay = dev_rows if dev_rows is not None else {}
        res = {k: outs[k].cpu().numpy()[:int(np.prod(shapes[k]))].reshape(shapes[k]) for k in want if k not in stay}
        stay.update({k: outs[k] for k in stay if k in outs})
    else:
        res = {k: np.empty(shapes[k], dtype=np.int32 if k == "nkept" else np.float64) for k in want}
        args = [None if k not in res else (res[k].ctypes.data_as(_lib.c_int32_p) if k == "nkept" else _lib.dptr(res[k])) for k in names]
        rc = lib.pvx_formants(*head, *args, ctypes.byref(sing), ctypes.byref(noconv))
        _check(rc, "pvx_formants", sing, noconv)
    assert rc == nfr, (rc, nfr)
    return res


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
       full:       NotImplementedError here; pypevoc_amd.speech.envelope.Formants runs it

       returns Time [frames], Form and BandWidths [frames][int(modelOrd/2)], NaN where a frame has fewer formants
    '''
    if full:
        raise NotImplementedError("Formants(full=True) (pypevoc/speech/SpeechAnalysis.py:298-311) needs PeakFinder.refine_all, "
                                  "which this function does not run: pypevoc_amd.speech.envelope.Formants(full=True) does "
                                  "(see INTEGRATION.md)")
    n = glottal._signal(w)[2]
    down, wLen, FsN, nwind, hop, nFrames, Time = geometry(n, Fs, tWind, tHop, fMax)
    ncols = int(modelOrd / 2)
    if nFrames == 0:
        return Time, np.nan * np.ones((0, ncols)), np.nan * np.ones((0, ncols))
    if modelOrd > nwind:
        raise ValueError('Order must be smaller than size of vector')
    rows = _formants_run(w, hpFreq > 0, down, firwin_np(down) if down > 1 else None, hamming(nwind), hop, nFrames, modelOrd, FsN)
    Form, BandWidths = select(rows["nkept"], rows["freq"], rows["bw"], fMin, fMax, bwMax, ncols)
    return Time, Form, BandWidths


def lpc(w, order, axis=-1):
    """The LPC coefficients of the vector w without the leading 1 (SpeechAnalysis.py:9-24): one device call."""
    return glottal.lpc(w, order)[1:]


def _roots_run(coef, want_status=False):
    """pvx_polyroots on coefficient rows [n][order + 1] (host): re, im [n][order], nkept [n]."""
    lib = _lib.load()
    _lib.init()
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    if coef.ndim != 2 or coef.shape[1] < 2:
        raise ValueError("coefficient rows [n][order + 1] with order >= 1 are expected")
    n, order = coef.shape[0], coef.shape[1] - 1
    re, im = np.empty((n, order)), np.empty((n, order))
    nkept, status = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    noconv = ctypes.c_int64(-1)
    rc = lib.pvx_polyroots(_lib.dptr(coef), n, order, _lib.dptr(re), _lib.dptr(im), nkept.ctypes.data_as(_lib.c_int32_p),
                           status.ctypes.data_as(_lib.c_int32_p), ctypes.byref(noconv))
    _check(rc, "pvx_polyroots", noconv, noconv)
    assert rc == n, (rc, n)
    return re, im, nkept


def roots_frames(coef):
    """The roots of every row of coef [n][order + 1] (np.roots' coefficient order, order <= 64) as complex [n][order],
    canonical: a real root has imaginary part +0.0, complex roots are exact conjugate pairs.  Per row first the roots with
    imag >= 0 by ascending angle (equal angles by ascending modulus), then their conjugates in the partners' order."""
    re, im, _ = _roots_run(coef)
    return re + 1j * im


def lpc2form(a, Fs=1.0):
    '''
    Convert all-pole coefficients to resonance frequencies
    and bandwidths (SpeechAnalysis.py:186-209, its pairing included: see the module's docstring)

    a: LPC coefficients (all-pole coefficients excluding order 0)
    Fs: sampling rate
    '''
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError("a 1-D coefficient vector is expected")
    _lib.load()
    _lib.init()
    if len(a) == 0:
        return np.zeros(0), np.zeros(0)
    re, im, nkept = _roots_run(np.concatenate(([1.0], a))[None, :])
    RTS = (re[0] + 1j * im[0])[:nkept[0]]                              # imag >= 0, already in ascending angle
    nFreq = np.arctan2(np.imag(RTS), np.real(RTS)) * (Fs / (2 * np.pi))
    FreqS = nFreq[nFreq > 0]
    with np.errstate(divide="ignore"):
        BW = -1 / 2 * (Fs / (2 * np.pi)) * np.log(np.abs(RTS))
    return FreqS, BW


def lpcc2pole(b, sr=1):
    """Pole frequencies and bandwidths of the all-pole filter(s) b (glottal.py:249-272), b with its leading coefficient:
    1-D: (fp, bw) of the roots with imag >= 0 in ascending frequency; 2-D [rows][order + 1] (iaif_ola's vt): two arrays
    [rows][order + 2], a row's values from the left, zeros behind them."""
    b = np.asarray(b, dtype=np.float64)
    _lib.load()
    _lib.init()
    rows = b if b.ndim > 1 else b[None, :]
    if rows.ndim != 2:
        raise ValueError("a coefficient vector or rows of them are expected")
    if rows.shape[1] < 2 or rows.shape[0] == 0:
        re = im = np.zeros((rows.shape[0], 0))
        nkept = np.zeros(rows.shape[0], dtype=np.int32)
    else:
        re, im, nkept = _roots_run(rows)
    rts = re + 1j * im
    fp = np.arctan2(rts.imag, rts.real) * sr / 2 / np.pi
    with np.errstate(divide="ignore"):
        bw = -1 / 2 * (sr / 2 / np.pi) * np.log(np.abs(rts))
    if b.ndim == 1:
        return fp[0, :nkept[0]], bw[0, :nkept[0]]
    keep = np.arange(rts.shape[1])[None, :] < nkept[:, None]
    poles = np.zeros((b.shape[0], int(b.shape[1] + 1)))
    bws = np.zeros((b.shape[0], int(b.shape[1] + 1)))
    poles[:, :rts.shape[1]][keep] = fp[keep]
    bws[:, :rts.shape[1]][keep] = bw[keep]
    return poles, bws
