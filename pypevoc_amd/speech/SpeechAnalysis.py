"""Drop-in for pypevoc/speech/SpeechAnalysis.py: SpectralMoments (:82-139), Periodogram (:141-184), DistribMoments (:54-80)
and rmsWind (:321-346).

The mean power spectrum over the frames runs in libpvx_hip (pvx_specdesc, measure PSD; k_specdesc.hip, SPECDESC.md): the
frames are added in fixed blocks, nothing per frame happens in Python, no CPU fallback.  The moments of the nwind//2
numbers that come back are host numpy, once per call.  rmsWind is the device's windowed standard deviation (k_funcwind).

Deviations from the reference, which cannot run these two as written under Python 3:
  Periodogram  raises TypeError there (np.zeros of a float length, :168); here it has the evident meaning, SpectralMoments'
               own frame count, window and specLen = nwind//2.
  rmsWind      without nhop raises TypeError there (a float hop, :327); here nhop=None means nwind//2.
lpc, lpc2form, lpc2form_full, Formants, refine_max and FricativeData* are not mirrored here and raise NotImplementedError;
working lpc, lpc2form and Formants are in pypevoc_amd.speech.formants (FORMANTS.md)."""
import numpy as np

from .. import _lib
from ..SoundUtils import SD_PSD, FuncWind, specdesc_run, _siglen


def hamming(M):
    """scipy.signal.windows.hamming(M) (symmetric), bit for bit: general_cosine's sum 0.54 + (1. - 0.54) * cos(fac) over
    fac = linspace(-pi, pi, M).  np.hamming(M) differs from it in the last bit of some samples."""
    M = int(M)
    if M <= 1:
        return np.ones(M)
    fac = np.linspace(-np.pi, np.pi, M)
    w = np.zeros(M)
    for k, ak in enumerate([0.54, 1. - 0.54]):
        w += ak * np.cos(k * fac)
    return w


def DistribMoments(x, f, MaxMoments=4):
    '''Calculate the moments in a distribution f(x)
       x: abcissa - values at which distribution is given
       f: value -   values of the distribution
       MaxMoments: maximum moment order to return

       returns:
       COG: center of gravity
       StDev: standard deviation
       skew: skewness
       kurt: kurtosis
       Moments: array with all raw central moments
    '''
    moments = []
    m0 = np.sum(f)
    m1 = np.sum(f * x) / m0
    moments.append(m1)
    for mn in range(1, MaxMoments):
        moments.append(np.sum((x - m1)**(mn + 1) * f) / m0)
    cog = m1
    stdev = np.sqrt(moments[1])
    skew = moments[2] / moments[1]**1.5
    kurt = moments[3] / moments[1]**2 - 3.
    return cog, stdev, skew, kurt, moments


def frame_geometry(wLen, Fs, tWind, tHop):
    """(window, hop, frame count) of SpectralMoments (SpeechAnalysis.py:105-111); the count may be zero or negative."""
    hop = int(np.round(Fs * tHop))
    nwind = int(np.round(Fs * tWind))
    return nwind, hop, int((wLen - nwind - 1) / hop)


def _mean_power(w, Fs, tWind, tHop):
    """(mean over the frames of |fft(frame * hamming)|^2 at bins 0 .. nwind//2 - 1, their frequencies, the frame count).
    No frame: the reference's zeros / float(nFrames) (:114, :128), computed here, nothing launched."""
    _lib.load()
    _lib.init()
    nwind, hop, nfr = frame_geometry(_siglen(w), Fs, tWind, tHop)
    specLen = int(nwind / 2)
    freqS = (np.arange(specLen)) * float(Fs) / nwind
    if nfr <= 0:
        specdesc_run(w, hamming(nwind), hop, 0, SD_PSD)
        with np.errstate(all='ignore'):
            return np.zeros(specLen) / float(nfr), freqS, nfr
    return specdesc_run(w, hamming(nwind), hop, nfr, SD_PSD), freqS, nfr


def SpectralMoments(w, Fs, tWind=0.025, tHop=0.0125, windFunc=None, fCut=300, maxMoments=4):
    '''Calculates spectral moments in short windows  of signal w

        w:          signal (a host array, or a float32 / float64 / int16 signal on the GPU)
        Fs:         sample rate
        tWind:      window length in seconds
        tHop:       hop length in seconds
        windFunc:   accepted and ignored, as the reference ignores it: the frames are
                    windowed by scipy.signal.windows.hamming (SpeechAnalysis.py:122)
        fCut:       high-pass cutoff
        MaxMoments: maximum moment order to return

       returns a dict of
        cog:     center of gravity
        std:     standard deviation
        skew:    skewness
        kurt:    kurtosis
        level:   sqrt of the mean power
    '''
    P, freqS, _ = _mean_power(w, Fs, tWind, tHop)
    with np.errstate(all='ignore'):
        SxxS = np.sqrt(P)                                             # :128
        intens = np.sqrt(np.mean(P))                                  # :131
        idx = freqS > fCut
        cog, std, skew, kurt, mm = DistribMoments(freqS[idx], SxxS[idx], maxMoments)
    return dict(cog=cog, std=std, skew=skew, kurt=kurt, level=intens)


def Periodogram(w, Fs, tWind=0.025, tHop=0.0125, windFunc=None):
    '''Mean power spectrum of the hamming-windowed frames of w

       returns:
        Sxx:       power spectrum, bins 0 .. nwind//2 - 1
        f:         frequency values
    '''
    P, freqS, _ = _mean_power(w, Fs, tWind, tHop)
    return P, freqS


def rmsWind(w, nwind=256, nhop=None, windfunc=np.ones, sr=1):
    '''
    calculate RMS values in window chunks of data: (times, np.std of the frame times the window
    normalised to unit mean square)
    '''
    nwind = int(nwind)
    if not nhop:
        nhop = nwind // 2
    nhop = int(nhop)
    wvr = windfunc(nwind)
    wvnorm = np.sqrt(sum(wvr**2) / nwind)
    wv = wvr / wvnorm
    r, _ = FuncWind(np.std, w, sr=sr, nwind=nwind, nhop=nhop, power=0, windfunc=lambda n: wv)
    t = (np.arange(len(r)) * nhop + nwind / 2) / float(sr)            # :343
    return t, r


def _not_mirrored(name, where):
    def stub(*args, **kwargs):
        raise NotImplementedError("%s (pypevoc/speech/SpeechAnalysis.py:%s) is not mirrored: see INTEGRATION.md" % (name, where))
    stub.__name__ = name
    return stub


lpc = _not_mirrored("lpc", "9-24")
refine_max = _not_mirrored("refine_max", "26-51")
lpc2form = _not_mirrored("lpc2form", "186-209")
lpc2form_full = _not_mirrored("lpc2form_full", "211-218")
Formants = _not_mirrored("Formants", "220-319")
FricativeDataFromSnip = _not_mirrored("FricativeDataFromSnip", "349-384")
FricativeDataFromWav = _not_mirrored("FricativeDataFromWav", "386-423")
