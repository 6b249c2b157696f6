"""pypevoc/speech/SpeechSegmenter.py's SpeechSegmenter on the GPU: the detection function of the rough filter bank and its
peaks (process :203-222, the parabolic fit :224-260), the band-wise refinement of every segment on the fine bank
(refine_segment_all_bands :262-302, refine_all_all_bands :304-314) and the refinement of an interval's two edges
(refine_interval :316-389 on refine_transition_points :39-124).

Both banks are the mirror's TriangularFilterBank as it stands; pvx_filterbank_dev leaves their band energies in device
memory and the kernels of k_segment.hip (pvx_seg_detect, pvx_seg_refine, pvx_seg_transitions; SEGMENT.md) read them
there: the energies cross to the host only when `fine_spec` or `finespec` is asked for.  A signal is a host array or a
float32 / float64 / int16 1-D signal already on the GPU, as FilterBank.specout takes it.  Nothing per frame, per
segment or per band happens in Python and there is no CPU fallback.  refine_all_all_bands computes the fine bank once
per call, where the reference computes it once per segment.

Deviations from the reference (SEGMENT.md has the list): the constructor copies the band list instead of appending
sr/2 to the caller's (and so to its own shared default); mode 'pctYY' reads YY with float(), where the reference's
np.float raises AttributeError on numpy >= 1.24; a transition without a point after trt raises ValueError, not
IndexError; SyllableSegmenter and MultiChannelSegmenter are not mirrored (SilenceDetector: speech.chunker)."""
import ctypes

import numpy as np

from .. import FFTFilters as ff
from .. import _lib

SEG_MAX_SIDE = 256                                                    # PVX_SEG_MAX_SIDE of include/pvx.h
SEG_MAX_SERIES = 4096                                                 # PVX_SEG_MAX_SERIES
SEG_OK, SEG_OUTSIDE, SEG_EMPTY_SIDE, SEG_NO_CROSSING = 0, 1, 2, 3     # pvx_seg_status
_MODES = {"minmax": 0, "median": 1, "mean": 2}                        # pvx_seg_mode; 'pctYY' is 3


def last_kernels():
    """The kernel the calling thread's last segmenter stage ran: 'k_seg_detect', 'k_seg_refine', 'k_seg_transitions'
    ('' when it launched nothing)."""
    return _lib.load().pvx_segment_last_kernels().decode()


def _check(rc, what):
    if rc == _lib.PVX_ERR_UNSUPPORTED:
        raise NotImplementedError("%s: %s" % (what, (_lib.load().pvx_last_error() or b"").decode()))
    if rc == _lib.PVX_ERR_INVALID:
        raise ValueError("%s: %s" % (what, (_lib.load().pvx_last_error() or b"").decode()))
    return _lib.check(rc, what)


def _i32p(a):
    return a.ctypes.data_as(_lib.c_int32_p)


peaks = ff.peaks                                                      # SpeechSegmenter.py:32-37 is FFTFilters.py:72-77: strict interior maxima


def _mode_code(mode):
    """(pvx_seg_mode, pct) of a mode string of refine_transition_points."""
    if mode in _MODES:
        return _MODES[mode], 0.0
    if isinstance(mode, str) and mode[:3] == 'pct':
        pct = float(mode[3:])                                         # (the reference: np.float, SpeechSegmenter.py:86)
        if not 0.0 <= pct <= 100.0:
            raise ValueError("Percentiles must be in the range [0, 100]")
        return 3, pct
    raise ValueError("mode %r: 'minmax', 'median', 'mean' or 'pctYY' are known" % (mode,))


def transition_points_rows(x, tx=None, trt=None, mode='minmax', thr=0.5):
    """refine_transition_points of every row of x [rows][n] (host array) in one launch: (ttr, vbef, vaft, status), each
    [rows].  tx: the rows' common times [n] or their own [rows][n] (None: arange(n)), sorted here as the reference sorts
    them, the rows with them; trt: a scalar or [rows].  status: SEG_OK; SEG_OUTSIDE, trt outside tx: (trt, 0, 0);
    SEG_EMPTY_SIDE, no point after trt, or none before it in modes 'minmax' and 'pctYY'; SEG_NO_CROSSING.  Nothing is
    raised for a row's status: refine_transition_points does that for its one row."""
    code, pct = _mode_code(mode)
    x = np.array(x, dtype=np.float64, ndmin=2)
    if x.ndim != 2:
        raise ValueError("rows [rows][n] are expected")
    rows, n = x.shape
    if n < 1:
        raise ValueError("an empty series")
    if n > SEG_MAX_SERIES:
        raise NotImplementedError("a series of %d points: the kernel takes up to %d (PVX_SEG_MAX_SERIES)" % (n, SEG_MAX_SERIES))
    if tx is None:
        tx = np.arange(n, dtype=np.float64)
    else:
        tx = np.array(tx, dtype=np.float64)
        if tx.shape == (n,):
            istx = np.argsort(tx)                                     # :62-64
            tx, x = tx[istx], x[:, istx]
        elif tx.shape == (rows, n):
            istx = np.argsort(tx, axis=1)
            tx, x = np.take_along_axis(tx, istx, axis=1), np.take_along_axis(x, istx, axis=1)
        else:
            raise ValueError("tx must be [n] or [rows][n]")
    if not np.all(np.isfinite(tx)):
        raise ValueError("tx must be finite")
    trt = np.ascontiguousarray(np.broadcast_to(np.asarray(trt, dtype=np.float64), (rows,)))
    x, tx = np.ascontiguousarray(x), np.ascontiguousarray(tx)
    ttr, vbef, vaft = np.empty(rows), np.empty(rows), np.empty(rows)
    status = np.empty(rows, dtype=np.int32)
    lib = _lib.load()
    _lib.init()
    rc = lib.pvx_seg_transitions(_lib.dptr(x), rows, n, n, 1, 0.0, _lib.dptr(tx), n if tx.ndim == 2 else 0, _lib.dptr(trt), code, pct,
                                 float(thr), _lib.dptr(ttr), _lib.dptr(vbef), _lib.dptr(vaft), _i32p(status))
    _check(rc, "pvx_seg_transitions")
    return ttr, vbef, vaft, status


def _raise_status(st, what):
    if st == SEG_EMPTY_SIDE:
        raise ValueError("%s: no point on one side of the rough transition" % what)
    if st == SEG_NO_CROSSING:
        raise ValueError("%s: the series does not cross the level between the values before and after" % what)


def refine_transition_points(x, tx=None, trt=None, mode='minmax', thr=0.5):
    """One row of transition_points_rows with the reference's outcomes (SpeechSegmenter.py:39-124): (ttr, vbef, vaft), the
    time at which the series x over the times tx (None: its indices) crosses the level vbef thr + vaft (1 - thr) -- or, where
    x falls, vaft thr + vbef (1 - thr) -- nearest to the rough time trt, and the typical values of x before and after trt
    that set the level: 'minmax' the extreme values on the far sides (the medians say which way x goes), 'median', 'mean',
    'pctYY' the percentiles YY and 100 - YY.  (trt, 0, 0) when trt lies outside tx; ValueError for an empty side or when
    nothing crosses the level."""
    ttr, vbef, vaft, status = transition_points_rows(np.asarray(x, dtype=np.float64)[None, :], tx, trt, mode, thr)
    if status[0] == SEG_OUTSIDE:
        return trt, 0, 0
    _raise_status(status[0], "refine_transition_points")
    return ttr[0], vbef[0], vaft[0]


class _DeviceBank(object):
    """The band energies of one specout call, left on the GPU: a flat float64 torch tensor of nfr * nband values."""

    def __init__(self, fb, w):
        import torch
        bank = np.ascontiguousarray(fb.fb, dtype=np.float64)
        wind = np.ascontiguousarray(fb.wind, dtype=np.float64)
        nwind, hop = int(fb.nwind), int(fb.hop)
        if bank.ndim != 2 or bank.shape[1] != nwind or len(wind) != nwind:
            raise ValueError("fb must be [bands][nwind] and wind [nwind] (nwind = %d): got %r and %r" % (nwind, bank.shape, wind.shape))
        self.nband = bank.shape[0]
        if self.nband > ff.MAX_NBAND:
            raise NotImplementedError("a filter bank of %d bands: the kernels take up to %d (PVX_FBANK_MAX_NBAND)" % (self.nband, ff.MAX_NBAND))
        if self.nband < 1:
            raise ValueError("a filter bank without bands")
        self.device = _lib.bound_torch_device()
        if _lib.is_device_array(w):
            sig = _lib.DeviceSignal(w)
        else:
            x, _ = _lib.as_signal(w)
            sig = _lib.DeviceSignal(torch.from_numpy(x).to(self.device))
        if len(sig.shape) != 1:
            raise ValueError("a 1-D signal is expected")
        n = sig.shape[0]
        self.nfr = _lib.nframes_host(n, nwind, hop)
        self.spec = torch.empty(max(self.nfr * self.nband, 1), dtype=torch.float64, device=self.device)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        got = _lib.check(_lib.load().pvx_filterbank_dev(ctypes.c_void_p(sig.ptr), sig.dtype_code, n, _lib.dptr(wind), nwind, hop, _lib.dptr(bank),
                                                        self.nband, 0, ctypes.c_void_p(self.spec.data_ptr()), None, self.stream),
                         "pvx_filterbank_dev")
        assert got == self.nfr, (got, self.nfr)
        self.kernels = ff.last_kernels()
        self.times = fb._tout(self.nfr)

    def host(self):
        return self.spec.cpu().numpy()[:self.nfr * self.nband].reshape(self.nfr, self.nband)

    def new(self, n, dtype):
        import torch
        return torch.empty(max(int(n), 1), dtype=dtype, device=self.device)


def _ptr(t, offset_bytes=0):
    return ctypes.c_void_p(t.data_ptr() + offset_bytes)


class SpeechSegmenter(object):
    """Mirror of SpeechSegmenter (SpeechSegmenter.py:127-389): rough boundaries from the rate of change of a coarse filter
    bank's dB levels, then refinement on a fine bank.  Attributes are the reference's: detection_func, detection_func_times,
    detection_func_indexes_int, detection_function_indexes_ref, segments, fine_spec, fine_time, tfine, finespec, bandtrans,
    trans."""

    def __init__(self, sr=44100., bands=[225., 2000., 4000., 8000., 15000.], refine_bands=None, detect_thresh=0.7, rough_window=2048,
                 fine_window=256):
        """sr: sampling rate; bands: band limits of the rough bank (Hz), sr/2 is added when absent, to a copy (:147-150
        adds it to the caller's list); refine_bands: limits of the fine bank (None: the rough ones); rough_window,
        fine_window: the banks' FFT windows; detect_thresh: threshold on the detection function, scaled here, once, by
        sr / rough_window (:157) -- set_signal changes sr and leaves the threshold."""
        limits = list(bands)
        nyquist = sr / 2.
        if nyquist not in limits:
            limits.append(nyquist)
        self.sr = sr
        self.rough_window, self.fine_window = rough_window, fine_window
        self.pkthresh = self.sr / self.rough_window * detect_thresh
        self.bands = self.rough_bands = limits
        self.refine_bands = refine_bands
        self._fine_seg = self._fine_iv = None                         # the fine banks on the GPU behind fine_spec / finespec
        self._fpos = self._details = None

    def set_bands(self, bands):
        """Both banks at the current sr (:186-199).  Without refine_bands the fine bank takes these limits, and keeps
        them from then on."""
        self.bands = bands
        if not self.refine_bands:
            self.refine_bands = bands
        self.rough_fb = ff.TriangularFilterBank(flim=bands, sr=self.sr, nwind=self.rough_window)
        self.fine_fb = ff.TriangularFilterBank(flim=self.refine_bands, sr=self.sr, nwind=self.fine_window)

    def set_signal(self, signal, sr=1):
        """The signal the refinements read and its rate; the banks are rebuilt at that rate (:163-170)."""
        self.sig, self.sr = signal, sr
        self.set_bands(self.bands)
        self.tmax = len(signal) / float(sr)

    def set_soundfile(self, filename):
        """set_signal on a WAV file's samples at the file's rate (:172-184; scipy.io.wavfile, imported here only)."""
        from scipy.io import wavfile
        rate, samples = wavfile.read(filename)
        self.set_signal(samples, rate)

    # ---- rough segmentation ---------------------------------------------------------------------------------------
    def process(self, w):
        """Rough boundaries of w (:203-222): the frame times of the rough bank at which the detection function -- the
        bands' summed |change of dB level| from frame to frame -- has a strict peak above pkthresh.  One launch behind the
        bank's.  ValueError when w gives no rough frame."""
        import torch
        self.sig = w
        bank = _DeviceBank(self.rough_fb, w)
        nfr = bank.nfr
        if nfr == 0:
            # the reference: np.log10 of specout's empty 1-D array, then np.diff(axis=0) / np.sum(axis=1): AxisError
            raise ValueError("no rough frame: the signal is not longer than the rough window (%d samples)" % self.rough_fb.nwind)
        nd = nfr - 1
        maxseg = max((nd - 1) // 2, 0)                                # strict interior maxima of nd points: no overflow
        ddet, didx, dfpos = bank.new(nd, torch.float64), bank.new(maxseg, torch.int32), bank.new(maxseg, torch.float64)
        count = ctypes.c_int64(0)
        got = _check(_lib.load().pvx_seg_detect_dev(_ptr(bank.spec), nfr, bank.nband, float(self.pkthresh), maxseg, _ptr(ddet), _ptr(didx),
                                                    _ptr(dfpos), ctypes.byref(count), bank.stream), "pvx_seg_detect_dev")
        assert got == count.value, (got, count.value)
        self._kernels = (bank.kernels, last_kernels())
        kept = didx.cpu().numpy()[:got].astype(np.intp)
        self.detection_func = ddet.cpu().numpy()[:nd]
        self.detection_func_times = bank.times[:-1] + self.rough_fb.hop / 2 / float(self.sr)
        self.detection_func_indexes_int = kept
        self._fpos = (kept, dfpos.cpu().numpy()[:got])               # the kernel's parabolic positions of these indices
        self.segments = bank.times[kept]                              # (the frames' own times, not detection_func_times: :220)
        return self.segments

    def refine_segment_parabolic_fit(self, pos):
        """(position, value) of the vertex of the parabola through the detection function at pos - 1, pos, pos + 1 where pos
        is a strict peak, else (pos, its value) (:224-250).  Host arithmetic on three numbers, in k_seg_detect's order."""
        around = self.detection_func[pos - 1:pos + 2]
        if len(around) < 3:
            raise IndexError("refine_segment_parabolic_fit: index %d has no neighbour on both sides" % pos)
        left, top, right = around
        if not (top > left and top > right):
            return pos, top.tolist()
        slope = (right - left) / 2
        curv = (right + left) / 2 - top
        shift = - slope / 2 / curv
        return float(pos) + shift, (curv * shift * shift + slope * shift + top).tolist()

    def refine_segments_parabolic(self):
        """The segments at the vertices of the parabolas through the detection function's peaks (:252-260): the
        positions k_seg_detect found with the peaks; indices set by hand since process go through
        refine_segment_parabolic_fit."""
        if self._fpos is not None and self._fpos[0] is self.detection_func_indexes_int:
            self.detection_function_indexes_ref = self._fpos[1].tolist()
        else:
            self.detection_function_indexes_ref = [self.refine_segment_parabolic_fit(pk)[0] for pk in self.detection_func_indexes_int]
        axis = self.detection_func_times
        self.segments = np.interp(self.detection_function_indexes_ref, np.arange(len(axis)), axis)

    # ---- band-wise refinement -----------------------------------------------------------------------------------
    @property
    def fine_spec(self):
        """dB of the fine bank of the last refine_segment_all_bands / refine_all_all_bands [frames][bands] (:272), fetched
        from the GPU when asked for."""
        if self._fine_seg is None:
            raise AttributeError("fine_spec: no segment refinement has run")
        with np.errstate(divide="ignore"):
            return 10 * np.log10(self._fine_seg.host())

    @property
    def finespec(self):
        """The fine bank's energies of the last refine_interval [frames][bands] (:385), fetched when asked for."""
        if self._fine_iv is None:
            raise AttributeError("finespec: no refine_interval has run")
        return self._fine_iv.host()

    def _side_ranges(self, tfine, tsegs):
        """ibef, iaft, iall of refine_segment_all_bands (:276-278) as [first, last + 1) rows of tfine, [nseg][6]: the strict
        comparisons against the reference's own float bounds, by bisection on the ascending tfine."""
        intbef = (self.rough_window * 2) / float(self.sr)
        r = np.empty((len(tsegs), 6), dtype=np.int32)
        lo = np.searchsorted(tfine, tsegs - intbef, side='right')    # the first tfine > tseg - intbef
        hi = np.searchsorted(tfine, tsegs + intbef, side='left')     # the first tfine >= tseg + intbef
        hi = np.maximum(hi, lo)                                       # (a NaN tseg: three empty ranges at the end)
        r[:, 0] = r[:, 4] = lo
        r[:, 3] = r[:, 5] = hi
        r[:, 1] = np.clip(np.searchsorted(tfine, tsegs, side='left'), lo, hi)    # the first tfine >= tseg
        r[:, 2] = np.clip(np.searchsorted(tfine, tsegs, side='right'), lo, hi)   # the first tfine > tseg
        return r

    def _refine_all_bands(self, tsegs, thr):
        """refine_segment_all_bands of every tseg on one fine bank: the weighted means [nseg], in samples."""
        import torch
        tsegs = np.ascontiguousarray(tsegs, dtype=np.float64)
        bank = _DeviceBank(self.fine_fb, self.sig)
        if bank.nfr == 0:
            raise ValueError("no fine frame: the signal is not longer than the fine window (%d samples)" % self.fine_fb.nwind)
        self._fine_seg = bank
        self.fine_time = tfine = bank.times
        nseg, nband = len(tsegs), bank.nband
        ranges = np.ascontiguousarray(self._side_ranges(tfine, tsegs))
        dvalb, dvala = bank.new(nseg * nband, torch.float64), bank.new(nseg * nband, torch.float64)
        dcross, dout = bank.new(nseg * nband, torch.int32), bank.new(nseg, torch.float64)
        fb = self.fine_fb
        _check(_lib.load().pvx_seg_refine_dev(_ptr(bank.spec), bank.nfr, nband, _i32p(ranges), _lib.dptr(tsegs), nseg, int(fb.hop), fb.nwind / 2.,
                                              float(fb.sr), float(self.sr), float(thr) if thr else 0.0, 1 if thr else 0, _ptr(dvalb),
                                              _ptr(dvala), _ptr(dcross), _ptr(dout), bank.stream), "pvx_seg_refine_dev")
        self._kernels = (bank.kernels, last_kernels() if nseg else "")
        self._details = (ranges, dvalb, dvala, dcross, nseg, nband)  # stay on the GPU: _refine_details() fetches them
        return dout.cpu().numpy()[:nseg]

    def _refine_details(self):
        """The last refinement's per-(segment, band) values, for the tests: ranges [nseg][6], valb, vala, cross [nseg][nband]."""
        ranges, dvalb, dvala, dcross, nseg, nband = self._details
        return {"ranges": ranges, "valb": dvalb.cpu().numpy()[:nseg * nband].reshape(nseg, nband),
                "vala": dvala.cpu().numpy()[:nseg * nband].reshape(nseg, nband),
                "cross": dcross.cpu().numpy()[:nseg * nband].reshape(nseg, nband)}

    def refine_segment_all_bands(self, tseg, thr=None):
        """The refined position of the boundary near tseg, in samples (:262-302): per band of the fine bank the crossing,
        nearest to tseg, of the level between the medians of 2 rough windows before and after; the bands' positions
        weighted by their |step|.  thr: the level is the lower median + thr dB instead of the mean of the two.  A band
        without a crossing contributes tseg itself, in seconds, as in the reference."""
        return self._refine_all_bands(np.array([tseg], dtype=np.float64), thr)[0]

    def refine_all_all_bands(self, thr=None):
        """refine_segment_all_bands of every segment on one fine bank and one launch, in seconds (:304-314): the new
        self.segments, a list."""
        refined = list(self._refine_all_bands(np.asarray(self.segments, dtype=np.float64), thr) / self.sr)
        self.segments = refined
        return refined

    def refine_interval(self, tstart, tend, marg=0.1, thr=0.5, mode='minmax'):
        """The two edges of the sound that fills the rough interval [tstart, tend] seconds (:316-389): the fine bank of the
        signal from marg before to marg after it, and per band and edge refine_transition_points with that mode and thr
        on the frames up to the other edge; an edge is the bands' transition times weighted by their |step|.  Returns
        self.trans = [start, end]; self.bandtrans [2][bands], self.tfine and self.finespec go with it."""
        import torch
        code, pct = _mode_code(mode)
        dur = tend - tstart
        first = max(0, int((tstart - marg) * self.sr))
        last = min(len(self.sig), int((tend + marg) * self.sr))
        x = self.sig[first:last] if not _lib.is_device_array(self.sig) else torch.as_tensor(self.sig)[first:last]
        bank = _DeviceBank(self.fine_fb, x)
        if bank.nfr == 0:
            raise ValueError("no fine frame in the interval: it is not longer than the fine window (%d samples)" % self.fine_fb.nwind)
        self._fine_iv = bank
        tfine = bank.times
        nband = bank.nband
        escale = float((self.rough_window / self.fine_window)**2)    # dB of finespec * (rough / fine)^2, :342

        edges = []
        kernels = ""
        for name, t0, t1, trt in (("start", 0, marg + dur, marg), ("end", marg, 2 * marg + dur, dur + marg)):
            i0 = int(np.searchsorted(tfine, t0, side='left'))         # tfine >= t0 and tfine <= t1, :347-350
            i1 = int(np.searchsorted(tfine, t1, side='right'))
            n = i1 - i0
            if n < 1:
                raise ValueError("refine_interval: no fine frame around the interval's %s" % name)
            if n > SEG_MAX_SERIES:
                raise NotImplementedError("refine_interval: %d fine frames around the interval's %s: the kernel takes up to %d "
                                          "(PVX_SEG_MAX_SERIES)" % (n, name, SEG_MAX_SERIES))
            tx = np.ascontiguousarray(tfine[i0:i1])
            trts = np.full(nband, trt, dtype=np.float64)
            dt, db_, da = (bank.new(nband, torch.float64) for _ in range(3))
            dst = bank.new(nband, torch.int32)
            _check(_lib.load().pvx_seg_transitions_dev(_ptr(bank.spec, i0 * nband * 8), nband, n, 1, nband, escale, _lib.dptr(tx), 0,
                                                       _lib.dptr(trts), code, pct, float(thr), _ptr(dt), _ptr(db_), _ptr(da), _ptr(dst),
                                                       bank.stream), "pvx_seg_transitions_dev")
            kernels = last_kernels()
            ttr, vbef, vaft = (t.cpu().numpy()[:nband] for t in (dt, db_, da))
            status = dst.cpu().numpy()[:nband]
            for ibd in range(nband):
                _raise_status(status[ibd], "refine_interval: band %d, the interval's %s" % (ibd, name))
            outside = status == SEG_OUTSIDE
            ttr = np.where(outside, trt, ttr)
            weights = np.abs(np.where(outside, 0.0, vaft) - np.where(outside, 0.0, vbef))
            edges.append((ttr, np.sum(ttr * weights) / np.sum(weights)))
        self._kernels = (bank.kernels, kernels)

        self.tfine = tfine + (tstart - marg)
        self.bandtrans = np.vstack([edges[0][0], edges[1][0]])
        self.trans = np.array([edges[0][1], edges[1][1]]) + tstart - marg   # (tstart - marg, not first / sr: :382)
        return self.trans

    def last_kernels(self):
        """(the bank's kernels, the segmenter stage's kernel) of this object's last process / refinement."""
        return self._kernels

    def plot_last(self):
        raise NotImplementedError("SpeechSegmenter.plot_last (pypevoc/speech/SpeechSegmenter.py:391-416, matplotlib) is not mirrored: "
                                  "see INTEGRATION.md")
