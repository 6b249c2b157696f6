"""Drop-in for pypevoc.Heterodyne (pypevoc/Heterodyne.py): heterodyne(), the windowed complex demodulation against a
given heterodyning signal (:35-60; pvx_heterodyne, k_reduce.hip), and HeterodyneHarmonic (:261-542), the decomposition of a
signal into the harmonics of one f0 track and its resynthesis (pvx_hetharm / pvx_hetharm_resynth, k_hetharm.hip; HETHARM.md).

HeterodyneHarmonic follows the reference's fixed-resolution path.  What cannot run in the reference for any input raises
NotImplementedError here: nper= (variable resolution), set_fvec(adjust=True), get_voice_component, harmonic_frequencies, the
older class Heterodyne and heterodyne_corr ('not mirrored')."""
import collections.abc
import copy
import ctypes

import numpy as np

from . import _lib


def heterodyne(x, hetsig, wind=None, hop=None):
    """
    Heterodyner: calculates the complex amplitude of a sine wave centered at f

    Arguments:
        x: signal
        hetsig: complex heterodyning signal, same length as x (exp(-2j*pi*cumsum(f/sr)))
        wind: window (array, defaults to 256 point rectangular)
        hop: samples between windows (required, as in the reference where None fails in range())
    Returns (2 * windowed mean of x*hetsig per frame, centre sample of each frame).
    """
    if wind is None:
        wind = np.ones(2 ** 8)
    if hop is None:
        raise TypeError("'NoneType' object cannot be interpreted as an integer")   # range(0, n, None)
    lib = _lib.load()
    _lib.init()
    x = np.ascontiguousarray(x, dtype=np.float64)
    h = np.ascontiguousarray(hetsig, dtype=np.complex128)
    if len(h) != len(x):
        raise ValueError("operands could not be broadcast together with shapes (%d,) (%d,)" % (len(x), len(h)))
    wind = np.ascontiguousarray(wind, dtype=np.float64)
    wlen = len(wind)
    nfr = int(lib.pvx_nframes(len(x), wlen, int(hop)))
    out = np.zeros(nfr, dtype=np.complex128)
    icent = np.zeros(nfr, dtype=np.int64)
    if nfr > 0:
        r = lib.pvx_heterodyne(_lib.dptr(x), h.view(np.float64).ctypes.data_as(_lib.c_double_p), len(x), _lib.dptr(wind),
                               wlen, int(hop), out.view(np.float64).ctypes.data_as(_lib.c_double_p),
                               icent.ctypes.data_as(_lib.c_int64_p))
        _lib.check(r, "pvx_heterodyne")
    return out, icent


def _unsupported(name, where, why):
    def fn(*args, **kwargs):
        raise NotImplementedError(
            "%s (Heterodyne.py:%s) does not run in the reference for any input (%s) and is not mirrored by pypevoc_amd "
            "(see INTEGRATION.md, 'not mirrored')" % (name, where, why))
    fn.__name__ = name.split(".")[-1]
    fn.__doc__ = "Not mirrored: Heterodyne.py:%s (%s)." % (where, why)
    return fn


heterodyne_corr = _unsupported("heterodyne_corr", "63-99", "it uses a module `ts` that is never imported")


class Heterodyne(object):
    """Not mirrored (Heterodyne.py:101-256; its __init__ reads an undefined name)."""

    def __init__(self, *args, **kwargs):
        _unsupported("Heterodyne", "101-256", "its constructor raises NameError")()


def _cplx_ptr(a):
    return a.view(np.float64).ctypes.data_as(_lib.c_double_p)


class HeterodyneHarmonic(object):
    """
    Sine sum decomposition of a signal along one f0 track (Heterodyne.py:261-542, fixed resolution)
    """

    def __init__(self, x, sr=1.0, tf=None, f=None, nper=None, nwind=1024, nhop=None,
                 wfun=np.hanning, ampthr=0.1, nharm=5, fmin=0.1, fmax=1000, include_dc=False):
        """
        Arguments:
            * x:        signal: a host array, or a float64 1-D tensor already on the GPU (read in place)
            * sr:       sampling rate
            * f:        frequency track in Hz (a number, or an array: one value per sample, or per entry of tf)
            * tf:       time values of f (host)
            * nwind:    window length
            * nhop:     interval between estimations (defaults to nwind // 2)
            * nper:     variable resolution: not mirrored (raises NotImplementedError)
            * wfun:     windowing function
            * nharm:    number of harmonics, the DC term (harmonic 0) included
            * ampthr:   amplitude threshold of filter_harmonic, relative to the harmonic's maximum
            * fmin, fmax: f0 range kept by filter_harmonic (fmin is raised to the track's minimum)
            * include_dc: camp, f, angle_ratios and partial_frequencies keep the DC column
        All nharm columns of `ah` come from one kernel launch; nothing is computed on the host.
        """
        if nper is not None:
            _unsupported("HeterodyneHarmonic(nper=...)", "356-359, 466-467", "OverflowError / TypeError in the window length")()
        self._xdev = None
        if _lib.is_device_array(x):
            self._xdev = _lib.DeviceSignal(x)
            if len(self._xdev.shape) != 1 or self._xdev.dtype != np.float64:
                raise ValueError("HeterodyneHarmonic takes a 1-D float64 device signal")
            self.x = x
            self.nsamp = self._xdev.shape[0]
        else:
            self.x = np.ascontiguousarray(x, dtype=np.float64)
            if self.x.ndim != 1:
                raise ValueError("HeterodyneHarmonic takes a 1-D signal")
            self.nsamp = len(self.x)
        self.sr = sr
        self.nper = nper
        self.variable_resolution = False
        self.nwind = nwind
        self.nhop = nwind // 2 if nhop is None else nhop
        self.tf = tf
        self.fvals = f
        self.nharm = nharm
        self.wfun = wfun
        self.ampthr = ampthr
        self.fmin = fmin
        self.fmax = fmax
        self.include_dc = include_dc
        self.wind = wfun(self.nwind)
        self.set_fvec(self.fvals, self.tf)
        self.extract_partials()

    # ---- the launches ------------------------------------------------------------------------------------------
    def _nframes(self, wlen, hop):
        return _lib.nframes_host(self.nsamp, wlen, hop)

    def _track(self, fvec):
        fvec = np.ascontiguousarray(fvec, dtype=np.float64)
        if fvec.shape != (self.nsamp,):
            raise ValueError("operands could not be broadcast together with shapes (%d,) %s" % (self.nsamp, fvec.shape))
        return fvec

    def _device(self):
        """torch, its device object and current stream for the `_dev` entries (the signal lives on the bound device)"""
        import torch
        return torch, _lib.bound_torch_device(), torch.cuda.current_stream()

    def _extract(self, fvec, wind, hop, first, count, halve_dc):
        """pvx_hetharm: harmonics first .. first+count-1 of the normalised track fvec -> (ah [nfr, count], icent [nfr])"""
        first, count, hop = int(first), int(count), int(hop)
        if first < 0:
            raise ValueError("harmonic numbers start at 0 (got %d)" % first)
        wind = np.ascontiguousarray(wind, dtype=np.float64)
        wlen = len(wind)
        nfr = self._nframes(wlen, hop) if wlen > 0 and hop > 0 else 0
        ah = np.zeros((nfr, count), dtype=np.complex128)
        icent = np.zeros(nfr, dtype=np.int64)
        if nfr == 0 and wlen > 0 and hop > 0:
            return ah, icent
        fvec = self._track(fvec)
        lib = _lib.load()
        _lib.init()
        if self._xdev is None:
            r = lib.pvx_hetharm(_lib.dptr(self.x), self.nsamp, _lib.dptr(fvec), _lib.dptr(wind), wlen, hop, first, count, int(bool(halve_dc)),
                                _cplx_ptr(ah), icent.ctypes.data_as(_lib.c_int64_p))
            _lib.check(r, "pvx_hetharm")
        else:
            torch, dev, stream = self._device()
            dfv = torch.from_numpy(fvec).to(dev)
            dah = torch.empty(nfr * count * 2, dtype=torch.float64, device=dev)
            dic = torch.empty(nfr, dtype=torch.int64, device=dev)
            r = lib.pvx_hetharm_dev(ctypes.c_void_p(self._xdev.ptr), self.nsamp, ctypes.c_void_p(dfv.data_ptr()), _lib.dptr(wind), wlen, hop,
                                    first, count, int(bool(halve_dc)), ctypes.c_void_p(dah.data_ptr()), ctypes.c_void_p(dic.data_ptr()),
                                    ctypes.c_void_p(stream.cuda_stream))
            _lib.check(r, "pvx_hetharm_dev")
            ah = dah.cpu().numpy().view(np.complex128).reshape(nfr, count)
            icent = dic.cpu().numpy()
        return ah, icent

    def _resynth(self, first, count, filter, want_hf=False):
        """pvx_hetharm_resynth on self.ah: (y [nsamp], hf [nsamp] complex or None)"""
        first, count = int(first), int(count)
        ah = np.ascontiguousarray(self.ah, dtype=np.complex128)
        nfr, ntot = ah.shape
        if first < 0 or count < 1 or first + count > ntot:
            raise IndexError("harmonics %d .. %d of %d" % (first, first + count - 1, ntot))
        y = np.zeros(self.nsamp)
        hf = np.zeros(self.nsamp, dtype=np.complex128) if want_hf else None
        if nfr == 0 and self._nframes(int(self.nwind), int(self.nhop)) == 0:
            return y, hf
        fvec = self._track(self.fvec)
        lib = _lib.load()
        _lib.init()
        args = (nfr, ntot, int(self.nwind), int(self.nhop), first, count, int(bool(filter)), float(self.sr), float(self.fmin), float(self.fmax),
                float(self.ampthr))
        if self._xdev is None:
            r = lib.pvx_hetharm_resynth(_lib.dptr(fvec), self.nsamp, _cplx_ptr(ah), *args, _lib.dptr(y), _cplx_ptr(hf) if want_hf else None)
            _lib.check(r, "pvx_hetharm_resynth")
        else:
            torch, dev, stream = self._device()
            dfv = torch.from_numpy(fvec).to(dev)
            dah = torch.from_numpy(ah.view(np.float64).reshape(-1)).to(dev)
            dy = torch.empty(self.nsamp, dtype=torch.float64, device=dev)
            dhf = torch.empty(2 * self.nsamp, dtype=torch.float64, device=dev) if want_hf else None
            r = lib.pvx_hetharm_resynth_dev(ctypes.c_void_p(dfv.data_ptr()), self.nsamp, ctypes.c_void_p(dah.data_ptr()), *args,
                                            ctypes.c_void_p(dy.data_ptr()), ctypes.c_void_p(dhf.data_ptr()) if want_hf else None,
                                            ctypes.c_void_p(stream.cuda_stream))
            _lib.check(r, "pvx_hetharm_resynth_dev")
            y = dy.cpu().numpy()
            if want_hf:
                hf = dhf.cpu().numpy().view(np.complex128)
        return y, hf

    # ---- the track ---------------------------------------------------------------------------------------------
    def set_fvec(self, f0c, th=None, adjust=False):
        """Set the f0 track (Hz): per sample, a number, or values f0c at times th (Heterodyne.py:431-457).  Resets ah.

        adjust=True is not mirrored: the reference hands calc_adjusted_freq a vector in Hz where it expects cycles per
        sample.  Call `f0c, th = h.calc_adjusted_freq(h.fvec)` and `h.set_fvec(f0c * h.sr, th)` instead."""
        if adjust:
            _unsupported("HeterodyneHarmonic.set_fvec(adjust=True)", "446-448",
                         "calc_adjusted_freq gets Hz for cycles per sample; use calc_adjusted_freq(self.fvec) and set_fvec(f0c*sr, th)")()
        tvec = np.arange(self.nsamp) / self.sr
        fvec = f0c if th is None else np.interp(tvec, th, f0c)
        if not isinstance(fvec, collections.abc.Sequence):          # a number, or an array (which is no Sequence)
            fvec = fvec * np.ones(self.nsamp)
        self.fvec = fvec / self.sr
        self.fmin = max(self.fmin, min(fvec))
        c = int(self.nwind) // 2
        self.th = np.arange(c, self.nsamp - (self.nwind - c), self.nhop) / self.sr
        self.idxh = np.arange(c, self.nsamp - c, self.nhop).astype('i')
        self.ah = np.zeros((self.th.shape[0], self.nharm), dtype='complex')

    @property
    def f0(self):
        """the track in Hz, per sample"""
        return self.fvec * self.sr

    @property
    def t(self):
        return self.th

    @property
    def camp(self):
        """complex amplitudes [frame, harmonic], without the DC column unless include_dc"""
        return self.ah if self.include_dc else self.ah[:, 1:]

    @camp.setter
    def camp(self, mx):
        self.ah = mx

    @property
    def f(self):
        """nominal frequency of each column at the frame times (Heterodyne.py:310-317)"""
        f0t = np.interp(self.t, np.arange(self.nsamp) / self.sr, self.f0)
        first = 0 if self.include_dc else 1
        return np.array([f0t * n for n in range(first, self.nharm)]).T

    @property
    def angle_ratios(self):
        """phase of every column relative to the first one of camp (Heterodyne.py:319-324)"""
        camp = self.camp
        ang = np.angle(camp / np.tile(camp[:, :1], (1, camp.shape[1])))
        if self.include_dc:
            ang = np.hstack((np.zeros((ang.shape[0], 1)), ang))
        return ang

    @property
    def partial_frequencies(self):
        """nominal frequencies corrected by the frame-to-frame phase drift (Heterodyne.py:326-332)"""
        dt = self.nhop / self.sr
        newf = self.f[1:, :] - np.diff(np.unwrap(np.angle(self.camp)), axis=0) / dt / 2 / np.pi
        if self.include_dc:
            newf = np.hstack((np.zeros((newf.shape[0], 1)), newf))
        return newf

    def harmonic_times(self, n=1):
        return self.th

    def harmonic_amplitudes(self, n=1):
        return self.ah[:, n]

    harmonic_frequencies = _unsupported("HeterodyneHarmonic.harmonic_frequencies", "377-381", "a 2-D array indexed by idxh: IndexError")
    get_voice_component = _unsupported("HeterodyneHarmonic.get_voice_component", "501-519",
                                       "it calls heterodyne with a signature that does not exist")

    def heterodyner_signal(self, n=1):
        """exp(1j * cumsum(2*pi*n*fvec)) as a host array (the kernels never build it)"""
        return self.heterodyner_signal_from_f(self.fvec * n)

    def heterodyner_signal_from_f(self, f):
        """heterodyning signal of a normalised frequency vector (cycles per sample), host array"""
        return np.exp(1j * np.cumsum(f * 2 * np.pi))

    def calc_adjusted_freq(self, fvec, nwind=None, nhop=None):
        """
        Refine a normalised frequency track (cycles per sample) by a first-pass heterodyne: the frame-to-frame phase
        drift of the demodulated signal corrects it (Heterodyne.py:403-429).  Returns (f0c, th), f0c normalised.
        """
        wind = self.wind if nwind is None else self.wfun(nwind)
        if nhop is None:
            nhop = len(wind) // 2
        tvec = np.arange(self.nsamp) / self.sr
        h, ih = self._extract(fvec, wind, nhop, 1, 1, False)
        th = ih / self.sr
        dph = np.concatenate(([0], np.diff(np.unwrap(np.angle(h[:, 0])))))
        f0c = np.interp(th, tvec, fvec) - dph / nhop / 2 / np.pi
        return f0c, th

    # ---- analysis / resynthesis --------------------------------------------------------------------------------
    def extract_partial(self, n):
        """complex amplitude of harmonic n per frame and the frames' centre samples (the DC term is not halved here)"""
        if int(n) != n:
            raise TypeError("harmonic number must be an integer, got %r" % (n,))
        h, ic = self._extract(self.fvec, self.wind, self.nhop, n, 1, False)
        return h[:, 0], ic

    def extract_partials(self):
        """all harmonics 0 .. nharm-1 in one launch -> (ah [frame, harmonic] with the DC column halved, th)"""
        if self.nharm < 1:
            raise IndexError("index 0 is out of bounds for axis 1 with size 0")
        ah, _ = self._extract(self.fvec, self.wind, self.nhop, 0, self.nharm, True)
        self.ah[:, :] = ah
        return self.ah, self.th

    def filter_harmonic(self, n):
        """amplitude of harmonic n per sample, zeroed where f0 leaves [fmin, fmax], the harmonic passes sr/2.2 or it is weak"""
        return self._resynth(n, 1, True, want_hf=True)[1]

    def resynth_partial(self, n, filter=False):
        """harmonic n as a signal, from its (optionally filtered) interpolated amplitude"""
        return self._resynth(n, 1, filter)[0]

    def resynth(self):
        """sum of all harmonics' signals, unfiltered"""
        return self._resynth(0, self.nharm, False)[0]

    def clone(self):
        return copy.copy(self)
