"""pypevoc/speech/SpeechChunker.py's SilenceDetector with the percentile discriminator (:40-164): the frame amplitudes come
from the mirror's rmsWind (the plain detector) or from a one-band FilterBank of the mirror (fmin / fmax), both on the GPU;
20 log10, the two percentiles and the walk over the frames' clusters -- a sequential pass over tens of frames -- are host
numpy, as in the reference.

method='kmeans' (sklearn), to_textgrid (pympi), recognise (speech_recognition), MultiChannelSegmenter, analyse_rec,
process_file_list and the command line are not mirrored.  pypevoc_amd.speech does not export
SilenceDetector itself: import it from here."""
import numpy as np

from .. import _lib
from .SpeechAnalysis import rmsWind


def _not_mirrored(name, where):
    def stub(*args, **kwargs):
        raise NotImplementedError("%s (pypevoc/speech/SpeechChunker.py:%s) is not mirrored: see INTEGRATION.md" % (name, where))
    stub.__name__ = name
    return stub


def _decibels(ampl):
    with np.errstate(divide="ignore"):                                # (digital silence: -inf, as in the reference)
        return 20 * np.log10(np.asarray(ampl, dtype=np.float64).reshape(-1))


def _sounding_runs(sound, min_gap):
    """(first, stop) frame indices of the stretches of True in sound, after stretches parted by fewer than min_gap False
    frames are joined; stop is one past a stretch's last True frame."""
    edges = np.diff(np.concatenate(([0], np.asarray(sound, dtype=np.int8), [0])))
    first, stop = np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)
    if len(first) > 1:
        parted = first[1:] - stop[:-1] >= min_gap
        first, stop = first[np.concatenate(([True], parted))], stop[np.concatenate((parted, [True]))]
    return first, stop


class SilenceDetector(object):
    """The sounding regions of a signal (:40-164): tst and tend, their starts and ends in seconds.

    x: the signal, a host array or a 1-D signal on the GPU (FilterBank.specout reads it in place; the plain detector copies
    it to the host for rmsWind).  wind_sec: the amplitude window, hopped by half its length.  method 'pctYY': a frame
    sounds when its level in dB lies above the midpoint of the frames' percentiles YY and 100 - YY.  min_len: the shortest
    silence, in seconds, that parts two regions.  max_len is accepted and has no effect, as in the reference.  fmin, fmax:
    take the amplitude in that band (either may be None: a low-pass or a high-pass).  Also sets at, ax, amin, amax, ath,
    clusters, nwind and nfr."""

    def __init__(self, x, sr=1, wind_sec=0.92, method='pct05', min_len=0.1, max_len=5, fmin=None, fmax=None):
        if method[:3].lower() != 'pct':
            if method == 'kmeans':
                raise NotImplementedError("SilenceDetector(method='kmeans') (pypevoc/speech/SpeechChunker.py:100-110, sklearn) is not "
                                          "mirrored: see INTEGRATION.md")
            raise ValueError("method %r: 'pctYY' is known" % (method,))   # (the reference: AttributeError on self.clusters)
        self.x, self.sr = x, sr
        self.nwind = int(wind_sec * sr)
        if fmin is None and fmax is None:
            self._calc_amplitude(nwind=self.nwind)
        else:
            self._calc_band_amplitude(nwind=self.nwind, fmin=fmin, fmax=fmax)
        self._percentile_discriminator(pct=int(method[3:5]))
        self.tst, self.tend = self._clusters_to_time_int(min_int=min_len, max_int=max_len)

    def _calc_amplitude(self, nwind=4096):
        """at, ax: the frames' times and RMS level in dB (:71-78).  The window is self.nwind whatever nwind says; nwind
        sets the hop, nfr -- both as in the reference."""
        self.nfr = nwind // 2
        x = self.x
        if _lib.is_device_array(x):                                   # (rmsWind takes host arrays; the band route reads the GPU's in place)
            import torch
            x = torch.as_tensor(x).cpu().numpy()
        self.at, ampl = rmsWind(x, sr=self.sr, nwind=self.nwind, nhop=self.nfr)
        self.ax = _decibels(ampl)

    def _calc_band_amplitude(self, nwind=4096, fmin=50, fmax=5000):
        """at, ax from a FilterBank of one band (:80-98): fmin .. fmax, below fmax (fmin None) or above fmin (fmax None)."""
        from ..FFTFilters import FilterBank, PiecewiseFilterSpec
        self.nfr = nwind // 2
        freq, mode = {(True, False): (fmax, 'lp'), (False, True): (fmin, 'hp')}.get((fmin is None, fmax is None), ([fmin, fmax], 'bp'))
        bank = FilterBank([PiecewiseFilterSpec(freq=freq, mode=mode, sr=self.sr)], sr=self.sr, nwind=self.nwind, nhop=self.nfr)
        ampl, self.at = bank.specout(self.x)
        self.ax = _decibels(ampl)

    def _percentile_discriminator(self, pct=5):
        """amin, amax: the percentiles pct and 100 - pct of ax; ath: their midpoint; clusters: 1 for the frames above ath,
        0 for the others (:114-126)."""
        self.amin, self.amax = np.percentile(self.ax, pct), np.percentile(self.ax, 100 - pct)
        self.ath = (self.amin + self.amax) / 2
        self.clusters = (self.ax > self.ath).astype(int)

    def _clusters_to_time_int(self, min_int=0.0, max_int=None):
        """(tst, tend), lists of seconds, from clusters (:128-164).  The reference walks the frames; what the walk yields
        is stated here on the runs of cluster 1.  With gap = round(min_int / hop time) frames: runs parted by fewer than gap
        silent frames are one region; a region is reported when it begins before the last gap frames; it starts at the
        frame before its first sounding frame; it ends at its first silent frame when that lies before the last gap frames
        as well, else at the last frame."""
        gap = int(np.round(min_int / (self.nfr / float(self.sr))))     # (this order of division: a tie rounds as the reference's)
        at = np.asarray(self.at)
        first, stop = _sounding_runs(np.asarray(self.clusters) > 0, gap)
        watched = len(self.clusters) - gap                            # the walk looks at the frames before this one
        kept = first < watched
        first, stop = first[kept], stop[kept]
        tst = at[np.maximum(first - 1, 0)]
        tend = at[np.where(stop < watched, np.minimum(stop, len(at) - 1), len(at) - 1)]
        return list(tst), list(tend)

    _k_means_discriminator = _not_mirrored("SilenceDetector._k_means_discriminator", "100-110")
    to_textgrid = _not_mirrored("SilenceDetector.to_textgrid", "166-175")
    output = _not_mirrored("SilenceDetector.output", "177-179")
    recognise = _not_mirrored("SilenceDetector.recognise", "181-214")


MultiChannelSegmenter = _not_mirrored("MultiChannelSegmenter", "216-398")
output_results = _not_mirrored("output_results", "400-408")
analyse_rec = _not_mirrored("analyse_rec", "411-441")
process_file_list = _not_mirrored("process_file_list", "444-494")
main = _not_mirrored("main", "497-524")
