"""Drop-in for pypevoc/speech/glottal.py: lpc (:32-34), iaif_ola (:36-84) and InverseFilter (:143-246), Alku's iterative
adaptive inverse filtering.

Every frame of a call -- the high-pass FIR, the LPCs, the inverse filters, the leaky integrators -- and the overlap-add
run in libpvx_hip (pvx_iaif, pvx_lpc; k_iaif.hip, pvx_lpc.h, GLOTTAL.md), one workgroup per frame, all frames of a call in
one launch: nothing per frame happens in Python, and there is no CPU fallback.  The host designs the high-pass filter once
per InverseFilter (a numpy restatement of scipy.signal.firls with unit weights: this package imports no scipy).

lpc_frames is the batched form of lpc the reference does not have.  PaddedFilter, fir_pre_phase and lpcc2pole are not
mirrored here and raise NotImplementedError; a working lpcc2pole is in pypevoc_amd.speech.formants."""
import ctypes
import logging

import numpy as np

from .. import _lib

LPC_MAX_ORDER = 128                                                   # PVX_LPC_MAX_ORDER of include/pvx.h
LPC_MAX_NWIND = 16384                                                 # PVX_LPC_MAX_NWIND
IAIF_MAX_NWIND = 4096                                                 # PVX_IAIF_MAX_NWIND
IAIF_MAX_TAPS = 4095                                                  # PVX_IAIF_MAX_TAPS


def firls(numtaps, bands, desired, fs):
    """scipy.signal.firls(numtaps, bands, desired, fs=fs) with unit weights: the least-squares linear-phase FIR of the
    piecewise linear gain `desired` over the frequency pairs `bands`, from the Toeplitz-plus-Hankel normal equations."""
    numtaps = int(numtaps)
    if numtaps % 2 == 0 or numtaps < 1:
        raise ValueError("numtaps must be odd and >= 1")
    M = (numtaps - 1) // 2
    bands = np.asarray(bands, dtype=np.float64).flatten() / (0.5 * float(fs))
    desired = np.asarray(desired, dtype=np.float64).flatten()
    if len(bands) % 2 or bands.size != desired.size or (bands < 0).any() or (bands > 1).any() or (np.diff(bands.reshape(-1, 2)) <= 0).any():
        raise ValueError("bands must be increasing frequency pairs between 0 and fs/2, with one gain per frequency")
    bands = bands.reshape(-1, 2)
    desired = desired.reshape(-1, 2)
    weight = np.ones(len(desired))
    n = np.arange(numtaps)[:, np.newaxis, np.newaxis]
    q = np.dot(np.diff(np.sinc(bands * n) * bands, axis=2)[:, :, 0], weight)
    k = np.arange(M + 1)
    Q = q[np.abs(k[:, None] - k[None, :])] + q[k[:, None] + k[None, :]]   # toeplitz(q[:M+1]) + hankel(q[:M+1], q[M:])
    n = n[:M + 1]
    m = np.diff(desired, axis=1) / np.diff(bands, axis=1)
    c = desired[:, [0]] - bands[:, [0]] * m
    b = bands * (m * bands + c) * np.sinc(bands * n)
    b[0] -= m * bands * bands / 2.
    b[1:] += m * np.cos(n[1:] * np.pi * bands) / (np.pi * n[1:]) ** 2
    b = np.dot(np.diff(b, axis=2)[:, :, 0], weight)
    a = np.linalg.solve(Q, b)
    return np.hstack((a[:0:-1], 2 * a[0], a[1:]))


def default_frame(Fs):
    """(nwind, nhop, tract_order, glottal_order) of iaif_ola's None arguments (glottal.py:41-48)."""
    nwind = int(np.round(25 / 1000 * Fs))
    return nwind, int(nwind / 5), 2 * int(np.round(Fs / 2000)) + 4, 2 * int(np.round(Fs / 4000))


def last_kernels():
    """The kernels the calling thread's last iaif_ola / InverseFilter.apply / lpc / lpc_frames ran: 'k_iaif_frames+k_iaif_ola',
    'k_iaif_frames', 'k_lpc_frames' ('' when it had no frame)."""
    return _lib.load().pvx_iaif_last_kernels().decode()


def _signal(x):
    """(pointer, dtype code, length, keep-alive, on the device?) of a 1-D host or device signal."""
    if _lib.is_device_array(x):
        sig = _lib.DeviceSignal(x)
        if len(sig.shape) != 1:
            raise ValueError("a 1-D signal is expected")
        return sig.ptr, sig.dtype_code, int(sig.shape[0]), sig, True
    xs, code = _lib.as_signal(x)
    if xs.ndim != 1:
        raise ValueError("a 1-D signal is expected")
    return xs.ctypes.data, code, len(xs), xs, False


def _check(rc, what, sing):
    if rc == _lib.PVX_ERR_SINGULAR:
        raise np.linalg.LinAlgError("Singular principal minor (frame %d)" % sing.value)
    return _lib.check(rc, what)


def _device_outputs(shapes):
    """float64 device blocks (torch tensors on the bound device) of the given element counts, and torch's current stream."""
    import torch
    dev = _lib.bound_torch_device()                                  # the outputs and the stream must be the bound device's
    outs = [None if c is None else torch.empty(max(c, 1), dtype=torch.float64, device=dev) for c in shapes]
    return outs, torch.cuda.current_stream()


def _iaif_run(x, nwind, hop, nfr, hp_b, lpc_wind, ola_wind, tract_order, glottal_order, leak, n_it, ola, frames):
    """pvx_iaif on x: (glot, dglot, g, dg, vt, gc) as host float64 arrays; glot / dglot None without `ola`, g / dg None
    without `frames`.  x: a host array, or a float32 / float64 / int16 1-D signal already on the GPU, read in place."""
    lib = _lib.load()
    _lib.init()
    ptr, code, n, keep, on_dev = _signal(x)
    nwind, hop, nfr, n_it = int(nwind), int(hop), max(int(nfr), 0), int(n_it)
    pt, pg = int(tract_order), int(glottal_order)
    hp_b = np.ascontiguousarray(hp_b, dtype=np.float64)
    lpc_wind = np.ascontiguousarray(lpc_wind, dtype=np.float64)
    ola_wind = np.ascontiguousarray(ola_wind, dtype=np.float64) if ola else None
    if lpc_wind.shape != (nwind,) or (ola and ola_wind.shape != (nwind,)):
        raise ValueError("the windows must have nwind = %d samples" % nwind)
    gcw = (pg if n_it > 0 else 1) + 1
    counts = [n if ola else None, n if ola else None, nfr * nwind if frames else None, nfr * nwind if frames else None,
              nfr * (pt + 1), nfr * gcw]
    sing = ctypes.c_int64(-1)
    head = (ctypes.c_void_p(ptr), code, n, nwind, hop, nfr, _lib.dptr(hp_b), len(hp_b), _lib.dptr(lpc_wind),
            _lib.dptr(ola_wind) if ola else None, pt, pg, float(leak), n_it)
    if on_dev:
        douts, stream = _device_outputs(counts)
        rc = lib.pvx_iaif_dev(*head, *[None if t is None else ctypes.c_void_p(t.data_ptr()) for t in douts], ctypes.byref(sing),
                              ctypes.c_void_p(stream.cuda_stream))
        _check(rc, "pvx_iaif_dev", sing)
        outs = [None if t is None else t.cpu().numpy()[:c] for t, c in zip(douts, counts)]
    else:
        outs = [None if c is None else np.empty(c) for c in counts]
        rc = lib.pvx_iaif(*head, *[None if a is None else _lib.dptr(a) for a in outs], ctypes.byref(sing))
        _check(rc, "pvx_iaif", sing)
    assert rc == nfr, (rc, nfr)
    glot, dglot, g, dg, vt, gc = outs
    if frames:
        g, dg = g.reshape(nfr, nwind), dg.reshape(nfr, nwind)
    return glot, dglot, g, dg, vt.reshape(nfr, pt + 1), gc.reshape(nfr, gcw)


def lpc_frames(x, order, nwind, hop, wind=None):
    """[1, a_1 .. a_order] of every whole frame x[i*hop : i*hop+nwind] * wind (wind None: the bare frames), i <
    (len(x) - nwind) // hop + 1, as a host array [frames][order + 1]: one device call, a workgroup per frame.
    order <= 128, nwind <= 16384.  A frame whose autocorrelation is singular (silence) raises np.linalg.LinAlgError."""
    lib = _lib.load()
    _lib.init()
    ptr, code, n, keep, on_dev = _signal(x)
    order, nwind, hop = int(order), int(nwind), int(hop)
    if order > nwind:
        raise ValueError('Order must be smaller than size of vector')
    if wind is not None:
        wind = np.ascontiguousarray(wind, dtype=np.float64)
        if wind.shape != (nwind,):
            raise ValueError("the window must have nwind = %d samples" % nwind)
    pw = None if wind is None else _lib.dptr(wind)
    nfr = (n - nwind) // hop + 1 if n >= nwind and nwind > 0 else 0
    sing = ctypes.c_int64(-1)
    if on_dev:
        (dout,), stream = _device_outputs([nfr * (order + 1)])
        rc = lib.pvx_lpc_dev(ctypes.c_void_p(ptr), code, n, pw, nwind, hop, nfr, order, ctypes.c_void_p(dout.data_ptr()), ctypes.byref(sing),
                             ctypes.c_void_p(stream.cuda_stream))
        _check(rc, "pvx_lpc_dev", sing)
        out = dout.cpu().numpy()[:nfr * (order + 1)]
    else:
        out = np.empty(nfr * (order + 1))
        rc = lib.pvx_lpc(ctypes.c_void_p(ptr), code, n, pw, nwind, hop, nfr, order, _lib.dptr(out), ctypes.byref(sing))
        _check(rc, "pvx_lpc", sing)
    assert rc == nfr, (rc, nfr)
    return out.reshape(nfr, order + 1)


def lpc(x, n):
    """[1, a_1 .. a_n] of the whole vector x (glottal.py:32-34: SpeechAnalysis.lpc with the leading 1 a filter needs)."""
    ptr, code, nsamp, keep, on_dev = _signal(x)
    if n > nsamp:
        raise ValueError('Order must be smaller than size of vector')
    return lpc_frames(x, n, nsamp, 1)[0]


def iaif_ola(x, Fs=1, nwind=None, nhop=None,
             tract_order=None, glottal_order=None,
             leaky_integration=0.99, wind_func=np.hanning,
             n_it=1):
    """Glottal flow and its derivative of x by overlap-add of the inverse-filtered frames (glottal.py:36-84): returns
    glot, dglot [len(x)] and the frames' vocal-tract and glottal filters [frames][order + 1] (two arrays of shape (0,)
    when x has no frame).  x: a host array, or a float32 / float64 / int16 signal on the GPU."""
    def_nwind, _, def_tract, def_glottal = default_frame(Fs)
    if nwind is None:
        nwind = def_nwind
    if nhop is None:
        nhop = int(nwind / 5)
    if tract_order is None:
        tract_order = def_tract
    if glottal_order is None:
        glottal_order = def_glottal

    wind = wind_func(nwind)

    iaif = InverseFilter(Fs=Fs, nwind=nwind,
                         tract_order=tract_order,
                         glottal_order=glottal_order,
                         leaky_integration=leaky_integration)

    n = _signal(x)[2]
    nfr = _lib.nframes_host(n, nwind, nhop)                          # ist = 0, nhop, ... while ist < len(x) - nwind
    if nfr > 0 and not hasattr(iaif, "hpfilt_b"):                     # 'Frame not analysed': the reference fails in apply
        raise AttributeError("'InverseFilter' object has no attribute 'hpfilt_b'")
    if nfr == 0:
        # nothing is launched and the library zeroes glot and dglot; with no frame it reads neither the filter nor the
        # windows (a half-built InverseFilter has none), only their lengths must be valid
        nw = max(int(nwind), 2)
        glot, dglot, _, _, _, _ = _iaif_run(x, nw, max(int(nhop), 1), 0, np.zeros(1), np.zeros(nw), np.zeros(nw), 0, 0, leaky_integration,
                                            n_it, True, False)
        return glot, dglot, np.array([]), np.array([])
    glot, dglot, _, _, vt, gc = _iaif_run(x, nwind, nhop, nfr, iaif.hpfilt_b, iaif.wind, wind, tract_order, glottal_order,
                                          -iaif.leaky_integrator[1], n_it, True, False)
    return glot, dglot, vt, gc


def _not_mirrored(name, where):
    def stub(*args, **kwargs):
        raise NotImplementedError("%s (pypevoc/speech/glottal.py:%s) is not mirrored: see INTEGRATION.md" % (name, where))
    stub.__name__ = name
    return stub


PaddedFilter = _not_mirrored("PaddedFilter", "86-126")
fir_pre_phase = _not_mirrored("fir_pre_phase", "129-140")
lpcc2pole = _not_mirrored("lpcc2pole", "249-272")


class InverseFilter(object):
    """Alku's iterative adaptive inverse filtering of one frame of nwind samples (glottal.py:143-246).  The constructor's
    default orders are the reference's own (tract 2*round(Fs/2000), glottal 2*round(Fs/4000) + 4: not those of iaif_ola).
    Attributes as in the reference: Fs, nwind, tract_order, glottal_order, hpfilt, hpfilt_b, wind, n_pad,
    leaky_integrator, id.  hpfilt > 1 repeats the high-pass filter on the frame itself there, which changes nothing."""

    def __init__(self, Fs=1, nwind=1024, wind_func=np.hanning,
                 tract_order=None, glottal_order=None,
                 leaky_integration=0.99, hpfilt=1):
        if tract_order is None:
            tract_order = 2 * int(np.round(Fs / 2000))
        if glottal_order is None:
            glottal_order = 2 * int(np.round(Fs / 4000)) + 4
        self.Fs = Fs
        self.tract_order = tract_order
        self.glottal_order = glottal_order
        if not nwind > self.tract_order:                              # the reference warns and leaves the object half built
            logging.warning('Frame not analysed')
            return
        self.nwind = int(nwind)
        self.hpfilt = hpfilt
        self.leaky_integrator = np.array([1, -leaky_integration])
        self.wind = wind_func(self.nwind)
        self.init_preliminary_filter()                                # even orders: ValueError, before any device call
        self.n_pad = tract_order + 1
        self.id = np.array([1])

    def apply(self, x, n_it=1):
        """g, dg, Hvt, Hg of the one frame x (nwind samples; a host array or a signal on the GPU): one device call, the
        LPCs windowed by self.wind."""
        if self.hpfilt < 1:
            raise UnboundLocalError("hpfilt = %r: the reference applies no high-pass filter and fails on its unassigned y" % (self.hpfilt,))
        n = _signal(x)[2]
        if n != self.nwind:
            raise ValueError("operands could not be broadcast together with shapes (%d,) (%d,)" % (n, self.nwind))
        _, _, g, dg, vt, gc = _iaif_run(x, self.nwind, self.nwind, 1, self.hpfilt_b, self.wind, None, self.tract_order, self.glottal_order,
                                        -self.leaky_integrator[1], n_it, False, True)
        return g[0], dg[0], vt[0], gc[0]

    def init_preliminary_filter(self, order=None, freq_stop=40, freq_pass=70):
        """Designs hpfilt_b, the high-pass FIR in front of the analysis (least squares: stop below freq_stop, pass above
        freq_pass); returns its length.  order None: round(300 / 16000 * Fs) taps, which must be odd."""
        if order is None:
            order = int(np.round(300 / 16000 * self.Fs))
        logging.info('Preliminary high-pass filter order set to %d' % order)
        self.hpfilt_b = firls(order, [0, freq_stop, freq_pass, self.Fs / 2], [0, 0, 1, 1], self.Fs)
        return len(self.hpfilt_b)
