"""Drop-in for pypevoc/FFTFilters.py: FFT filter banks and mel cepstra.

FilterBank.specout (:274-292), MelFilterBank.mfcc / mfcc_and_mel (:352-374) run in libpvx_hip (pvx_filterbank,
include/pvx.h; k_fbank.hip): every frame of a call in one launch at nwind 512 / 1024 / 2048, nothing per frame in
Python, no CPU fallback.  Filter construction (PiecewiseFilterSpec, the FilterBank constructors: setup work) stays on the
host in numpy and reproduces the reference's arrays bit for bit, its quirks included: fvec = linspace(0, sr, nwind) puts
bin k at k*sr/(nwind-1) (:262), f_to_mel adds where the mel formula multiplies (:61-63), TriangularFilterBank rounds its
band limits to float32 (:327), preemph returns float32 and subtracts the NEXT sample (:55-56).  fft_filter (:376-405) is
not mirrored: it raises NotImplementedError.  Design and numbers: FILTERBANK.md."""
import ctypes

import numpy as np

from . import _lib

MAX_NBAND = 128                                                       # PVX_FBANK_MAX_NBAND of include/pvx.h
_CEP_MODES = {"DCT1": 1, "DCT2": 2, "DCT3": 3, "DCT4": 4, "IFFT": 5}


class BandError(Exception):
    """A band of a filter specification cannot be realised on the frequency vector (FFTFilters.py:27-37)."""

    def __init__(self, message):
        self.message = message
        Exception.__init__(self, message)


def preemph(w, hpFreq=0, Fs=1):
    """Pre-emphasis above the cut-on frequency hpFreq (FFTFilters.py:40-59): float32 copy of w with a times the
    following sample subtracted from every sample but the last, a = exp(-2 pi hpFreq / Fs); w itself for hpFreq <= 0."""
    if not hpFreq > 0:
        return w
    a = np.exp(-2. * np.pi * hpFreq / float(Fs))
    wo = w.astype('f')
    wo[:-1] -= wo[1:] * a
    return wo


def _f_to_mel_py(freq):
    return 1125. + np.log(1. + freq / 700.)                           # FFTFilters.py:63 (a sum, as the reference has it)


def _mel_to_f_py(mel):
    return 700. * (np.exp(mel - 1125.) - 1)                           # FFTFilters.py:66


f_to_mel = np.vectorize(_f_to_mel_py)
mel_to_f = np.vectorize(_mel_to_f_py)


def peaks(x):
    """Indexes of the interior local maxima of x (FFTFilters.py:72-77)."""
    mid = x[1:-1]
    return np.flatnonzero(np.logical_and(x[:-2] < mid, x[2:] < mid)) + 1


def nearest(a, b):
    """For every element of a, the element of b nearest to it (FFTFilters.py:80-86)."""
    out = np.zeros(len(a))
    for i, v in enumerate(a):
        out[i] = b[np.argmin(np.abs(b - v))]
    return out


def nextpow2(x):
    return 2**(np.ceil(np.log2(x)))                                   # FFTFilters.py:337-338


class PiecewiseFilterSpec(object):
    """Piecewise-linear gain over frequency (FFTFilters.py:88-231): rows of bandf are the bands' [start, end] as
    fractions of sr, rows of bandg the gains at those two ends."""
    bandf = np.array([0.0, 0.5])
    bandg = np.array([1.0, 1.0])
    sr = 1.0
    label = ''

    def __init__(self, mode='', cutoff=0.5, freq=np.array([0.0, 0.5]), gain=np.array([1.0, 1.0]), sr=1.0, label=''):
        """mode 'lp' / 'lowpass', 'hp' / 'hipass' / 'highpass' (freq: the corner), 'bp' / 'bandpass', 'bs' / 'bandstop'
        (freq: the two corners); any other mode: vertices freq with gains gain, and `label`.  Frequencies in the unit of sr."""
        self.sr = sr
        m = mode.lower()
        if m in ('lp', 'lowpass'):
            self.set_lowpass_cutoff(freq / float(sr))
        elif m in ('hp', 'hipass', 'highpass'):
            self.set_hipass_cutoff(freq / float(sr))
        elif m in ('bp', 'bandpass'):
            self.set_bandpass_freqs(freq[0] / float(sr), freq[-1] / float(sr))
        elif m in ('bs', 'bandstop'):
            self.set_bandstop_freqs(freq[0] / float(sr), freq[-1] / float(sr))
        else:
            assert len(freq) == len(gain)
            self.set_triangular_filter(freq, gain)
            self.label = label
        if not self.label:
            self.label = 'Piecewise filter with {} bands'.format(len(self.bandf) - 1)

    def _two(self, f, glow, ghigh, name):
        self.bandf = np.array([[0.0, f], [f, 0.5]])
        self.bandg = np.array([[glow, glow], [ghigh, ghigh]])
        self.label = '{} filter, fc={}'.format(name, f * self.sr)

    def _three(self, f1, f2, gout, gin, name):
        self.bandf = np.array([[0.0, f1], [f1, f2], [f2, 0.5]])
        self.bandg = np.array([[gout, gout], [gin, gin], [gout, gout]])
        self.label = '{} filter, fc={}'.format(name, (f1 / 2 + f2 / 2) * self.sr)

    def set_lowpass_cutoff(self, f):
        self._two(f, 1.0, 0.0, 'Lowpass')                             # FFTFilters.py:137-140

    def set_hipass_cutoff(self, f):
        self._two(f, 0.0, 1.0, 'Hipass')                              # :142-145

    def set_bandpass_freqs(self, f1, f2):
        self._three(f1, f2, 0.0, 1.0, 'Bandpass')                     # :147-150

    def set_bandstop_freqs(self, f1, f2):
        self._three(f1, f2, 1.0, 0.0, 'Bandstop')                     # :152-155

    def set_triangular_filter(self, freq, gain):
        """Bands between neighbouring vertices in ascending frequency (FFTFilters.py:157-166)."""
        order = np.argsort(freq)
        self.bandf = np.array([[freq[i] / self.sr, freq[j] / self.sr] for i, j in zip(order[:-1], order[1:])])
        self.bandg = np.array([[gain[i], gain[j]] for i, j in zip(order[:-1], order[1:])])

    def __repr__(self):
        rep = '{}:\n'.format(self.label)
        for f, g in zip(self.bandf, self.bandg):
            span = '  Freq = [{},{}]: '.format(f[0] * self.sr, f[1] * self.sr)
            rep += span + ('gain = {}\n'.format(g[0]) if g[0] == g[1] else 'gain = [{},{}]\n'.format(g[0], g[1]))
        return rep

    def get_frequency_gains(self):
        """(band edges in the unit of sr, gains), both N x 2 (FFTFilters.py:182-191)."""
        return np.array(self.bandf) * self.sr, np.array(self.bandg)

    def get_frequency_edges(self):
        """The distinct band edges in the unit of sr (FFTFilters.py:193-197)."""
        return np.unique((np.array(self.bandf).flatten() * self.sr))

    def apply_to_freq_vector(self, fvec, align_edges=False):
        """Gain at the frequencies fvec (FFTFilters.py:200-231).  align_edges moves every band edge to the nearest
        element of fvec first; a band whose two edges then coincide raises BandError."""
        fvec = np.array(fvec)
        edge = {}
        for ff in self.get_frequency_edges():
            edge[ff] = fvec[np.argmin(np.abs(fvec - ff))] if align_edges else ff
        mask = np.zeros(len(fvec))
        for f, g in zip(self.bandf * self.sr, self.bandg):
            fst, fend = edge[f[0]], edge[f[1]]
            inside = np.logical_and(fvec >= fst, fvec <= fend)
            if fend == fst:
                raise BandError('Band is too narrow: try increasing nwind')
            mask[inside] = (fvec[inside] - fst) / (fend - fst) * (g[1] - g[0]) + g[0]
        return mask


class FilterBank(object):
    """FFT filter bank (FFTFilters.py:235-298).  fb [bands][nwind] holds the weights over the full spectrum; it is read
    when specout is called, so it may be edited."""
    label = []
    fvec = np.zeros(0)
    fb = np.zeros((0, 0))
    sr = 1.

    def __init__(self, fspec_list=None, sr=1.0, nwind=256, windfunc=np.hanning, nhop=None, align_edges=True):
        """fspec_list: PiecewiseFilterSpec objects (default: low-pass and high-pass at the frequency 0.25, which is
        sr/4 at the default sr = 1 only, :264-267); nhop default nwind/2."""
        self.sr = sr
        self.wind = windfunc(nwind)
        self.nwind = int(nwind)
        self.hop = nhop if nhop else int(nwind / 2)
        self.fvec = np.linspace(0., sr, nwind)                        # :262: endpoint included
        if not fspec_list:
            fspec_list = [PiecewiseFilterSpec(mode='lowpass', freq=0.25, sr=sr),
                          PiecewiseFilterSpec(mode='hipass', freq=0.25, sr=sr)]
        self.fb = np.zeros((len(fspec_list), len(self.fvec)))
        self.label = []
        for i, fspec in enumerate(fspec_list):
            self.fb[i, :] = fspec.apply_to_freq_vector(self.fvec, align_edges=align_edges)
            self.label.append(fspec.label)

    # ---- the launch -------------------------------------------------------------------------------------------
    def _run(self, w, cep_mode):
        """pvx_filterbank on w: (spec [nfr][nband], cep or None, nfr); host arrays back."""
        fb = np.ascontiguousarray(self.fb, dtype=np.float64)
        wind = np.ascontiguousarray(self.wind, dtype=np.float64)
        nwind = int(self.nwind)
        if fb.ndim != 2 or fb.shape[1] != nwind or len(wind) != nwind:
            raise ValueError("fb must be [bands][nwind] and wind [nwind] (nwind = %d): got %r and %r" % (nwind, fb.shape, wind.shape))
        nband = fb.shape[0]
        if nband > MAX_NBAND:
            raise NotImplementedError("a filter bank of %d bands: the kernels take up to %d (PVX_FBANK_MAX_NBAND)" % (nband, MAX_NBAND))
        if nband < 1:
            raise ValueError("a filter bank without bands")
        hop = int(self.hop)
        cpx = 2 if cep_mode == 5 else 1
        lib = _lib.load()
        if _lib.is_device_array(w):
            import torch
            sig = _lib.DeviceSignal(w)
            if len(sig.shape) != 1:
                raise ValueError("specout takes a 1-D signal")
            n = sig.shape[0]
            nfr = _lib.nframes_host(n, nwind, hop)
            dev = _lib.bound_torch_device()   # the outputs and the stream must be the bound device's
            dspec = torch.empty(max(nfr * nband, 1), dtype=torch.float64, device=dev)
            dcep = torch.empty(max(nfr * nband * cpx, 1) if cep_mode else 1, dtype=torch.float64, device=dev)
            stream = torch.cuda.current_stream()
            got = _lib.check(lib.pvx_filterbank_dev(ctypes.c_void_p(sig.ptr), sig.dtype_code, n, _lib.dptr(wind), nwind, hop, _lib.dptr(fb),
                                                    nband, cep_mode, ctypes.c_void_p(dspec.data_ptr()), ctypes.c_void_p(dcep.data_ptr()),
                                                    ctypes.c_void_p(stream.cuda_stream)), "pvx_filterbank_dev")
            spec = dspec.cpu().numpy()[:nfr * nband]
            cep = dcep.cpu().numpy()[:nfr * nband * cpx] if cep_mode else None
        else:
            x, code = _lib.as_signal(w)
            if x.ndim != 1:
                raise ValueError("specout takes a 1-D signal")
            n = len(x)
            nfr = _lib.nframes_host(n, nwind, hop)
            _lib.init()
            spec = np.empty(nfr * nband)
            cep = np.empty(nfr * nband * cpx) if cep_mode else None
            got = _lib.check(lib.pvx_filterbank(ctypes.c_void_p(x.ctypes.data), code, n, _lib.dptr(wind), nwind, hop, _lib.dptr(fb), nband,
                                                cep_mode, _lib.dptr(spec), _lib.dptr(cep) if cep_mode else None), "pvx_filterbank")
        assert got == nfr, (got, nfr)
        return spec.reshape(nfr, nband), (None if cep is None else cep), nfr

    def _tout(self, nfr):
        # :290: (float(n) + nwind/2.) / float(sr) for n = 0, hop, ...
        return (np.arange(nfr, dtype=np.int64) * int(self.hop) + self.nwind / 2.) / float(self.sr)

    def specout(self, w):
        """Output of the filter bank on w (FFTFilters.py:274-292): (band energies [frames][bands], frame centre times).
        w: a host array, or a float32 / float64 / int16 1-D signal already on the GPU (a torch tensor, anything with
        __cuda_array_interface__), read in place.  No frame (len(w) <= nwind): two arrays of shape (0,), as the
        reference returns."""
        spec, _, nfr = self._run(w, 0)
        if nfr == 0:
            return np.array([]), np.array([])
        return spec, self._tout(nfr)

    def __repr__(self):
        return 'FilterBank with filters:\n' + ''.join('  ' + ll + '\n' for ll in self.label)


class TriangularFilterBank(FilterBank):
    """Bank of triangular filters (FFTFilters.py:300-334): band n rises from flim[n] to 1 at flim[n+1] and falls to
    flim[n+2]."""
    label = []
    fvec = np.zeros(0)
    fb = np.zeros((0, 0))
    sr = 1.

    def __init__(self, flim=[0, .5, 1.], nwind=256, sr=1., nhop=None):
        """flim: band limits (in the unit of sr; as fractions of the rate for sr = 1), rounded to float32 as the
        reference does; nwind: FFT window; nhop: hop between frames (default nwind/2)."""
        unit = 'Hz' if sr > 1.0 else ''
        flim = np.sort(flim).astype('f')
        specs = []
        for n, centre in enumerate(flim[1:-1]):
            lab = '{}{} band ({}-{}{})'.format(centre, unit, flim[n], flim[n + 2], unit)
            specs.append(PiecewiseFilterSpec(freq=flim[n:n + 3], gain=np.array([0.0, 1.0, 0.0]), label=lab, sr=sr))
        super(TriangularFilterBank, self).__init__(fspec_list=specs, nwind=nwind, sr=sr, nhop=nhop)


class MelFilterBank(TriangularFilterBank):
    """n triangular bands evenly spaced on the reference's mel scale between fmin and fmax (FFTFilters.py:342-374);
    nwind = the power of two nearest to twind * sr, hop = int(thop * sr)."""

    def __init__(self, n=26, fmin=300., fmax=8000., twind=.025, sr=44100., thop=.01):
        nwind = int(2**np.round(np.log2(twind * sr)))
        nhop = int(thop * sr)
        fc = mel_to_f(np.linspace(f_to_mel(fmin), f_to_mel(fmax), n + 2))
        super(MelFilterBank, self).__init__(flim=fc, nwind=nwind, sr=sr, nhop=nhop)

    def _cepstra(self, w, mode):
        if mode not in _CEP_MODES:
            raise NotImplementedError("mfcc mode %r (FFTFilters.py:355-362 knows DCT1 .. DCT4 and IFFT)" % (mode,))
        code = _CEP_MODES[mode]
        if code == 1 and np.shape(self.fb)[0] < 2:
            raise ValueError("DCT type 1 needs at least 2 bands")
        spec, cep, nfr = self._run(w, code)
        if nfr == 0:
            # the reference hands log(np.array([])) to the transform: scipy's dct and np.fft.ifft both refuse it
            raise ValueError("no frame: the signal is not longer than the window (%d samples)" % self.nwind)
        nband = spec.shape[1]
        cep = cep.reshape(nfr, nband, 2).view(np.complex128)[:, :, 0] if code == 5 else cep.reshape(nfr, nband)
        return cep, spec, self._tout(nfr)

    def mfcc(self, w, mode='DCT2'):
        """(cepstra [frames][bands], times): the DCT of type 1..4 (scipy.fftpack's, norm=None) or, for 'IFFT', the
        inverse FFT (complex) of the log band energies (FFTFilters.py:352-362).  No floor: a band without energy is -inf."""
        cep, _, t = self._cepstra(w, mode)
        return cep, t

    def mfcc_and_mel(self, w, mode='DCT2'):
        """(cepstra, band energies, times) (FFTFilters.py:364-374)."""
        return self._cepstra(w, mode)


def last_kernels():
    """The kernels the calling thread's last specout / mfcc ran: 'k_fbank_fused<1024>', 'k_frames+rocfft+k_fbank_rows'."""
    return _lib.load().pvx_filterbank_last_kernels().decode()


def fft_filter(x, bands, gains):
    raise NotImplementedError("fft_filter (FFTFilters.py:376-405, a whole-signal FFT / IFFT filter that prints per band) is not "
                              "mirrored: see INTEGRATION.md")
