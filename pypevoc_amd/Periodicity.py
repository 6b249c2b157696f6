"""Drop-in for pypevoc/Periodicity.py's time-domain f0 tracker: PeriodSeries (:251-503), its Periodicity frames
(:55-248) and PeriodTimeSeries (:505-506).  Every frame's similarity function (xcorr or amdf), normalisation,
voicing test, candidate peaks, preferred candidate and sort by strength run in one launch of k_period.hip
(pvx_periodicity, include/pvx.h); there is no CPU fallback.  The scalar period-mark walks (period_marks_*,
the module-level amdf, PeriodByPeriod) are not mirrored: they raise NotImplementedError.
Design and numbers: PERIODICITY.md."""
import ctypes

import numpy as np

from . import _lib

_METHODS = {"xcorr": 0, "amdf": 1}
_CAND_METHODS = {"fft": 0, "min": 1, "similar": 2}            # anything else: preferred stays 0 (:189-197), code 3


class Periodicity(object):
    """Single period object, including multiple periodicity candidates (Periodicity.py:55-248).

    Constructed by PeriodSeries; Periodicity(parent, index) runs the one frame centred at round(index) on the GPU."""

    def __init__(self, parent, index=0, _row=None):
        self.parent = parent
        self.nwind = parent.nwind
        self.wind = parent.wind
        self.sr = parent.sr
        self.mindelay = parent.mindelay
        self.maxdelay = int(parent.maxdelay)
        self.method = parent.method
        self.threshold = parent.threshold
        self.vthresh = parent.vthresh
        self.ncand = parent.ncand
        self.fftthresh = parent.fftthresh
        self.cand_method = parent.cand_method
        self.index = index
        if _row is None:
            res = parent._run(np.array([_centre(index)], dtype=np.int64))
            _row = (res["period"][0], res["strength"][0], int(res["count"][0]), int(res["preferred"][0]))
        per, st, cnt, pref = _row
        # as _calc leaves them (candidates in position order) is not observable: the frames come back sorted by
        # strength (sort_strength, :223-236), which is what per_at_index / calc hand out
        self.cand_period = np.array(per[:cnt], dtype=np.float64)
        self.cand_strength = np.array(st[:cnt], dtype=np.float64)
        self.preferred = pref if cnt > 0 else ([] if pref < 0 else 0)

    def set_time_properties(self, index):
        self.index = float(index)
        self.time = float(index) / self.sr

    def sort_strength(self):
        """Sort candidates by periodicity strength (the frames already are: this is idempotent)."""
        idx = np.argsort(self.cand_strength)[::-1]
        self.cand_period = self.cand_period[idx]
        self.cand_strength = self.cand_strength[idx]
        pref = np.flatnonzero(idx == self.preferred)
        self.preferred = pref[0] if len(pref) > 0 else []

    def get_preferred_period(self):
        if len(self.cand_period) > 0:
            return self.cand_period[self.preferred]
        return 0

    def get_preferred_strength(self):
        if len(self.cand_period) > 0:
            return self.cand_strength[self.preferred]
        return 0


def _centre(index):
    return int(np.round(index))                                     # Periodicity.py:106


class PeriodSeries(object):
    def __init__(self, x, sr=48000, window=None, hop=None, threshold=.8, vthresh=.2, fmin=50, fmax=5000, ncand=8,
                 method='xcorr', cand_method='fft', fftthresh=0.1):
        """Periodicity (f0 candidates) of x frame by frame (Periodicity.py:252-332).

        x: signal -- a host array, or a float64 1-D tensor already on the GPU (analysed in place)
        sr: sample rate; window: array, or a length for np.ones (default 3 * sr / fmin);
        threshold: PeakFinder minval of the candidates; vthresh: voicing threshold;
        fmin / fmax: bounds of f0 (maxdelay = int(sr/fmin), mindelay = int(sr/fmax), 2 for fmax None);
        ncand: maximum number of candidates; method: 'xcorr' or 'amdf';
        cand_method: 'fft', 'min' or 'similar'; fftthresh: threshold of the fft peaks ('fft')."""
        self.method = method
        self._xdev = None
        if _lib.is_device_array(x):
            self._xdev = _lib.DeviceSignal(x)
            if len(self._xdev.shape) != 1 or self._xdev.dtype != np.float64:
                raise ValueError("PeriodSeries takes a 1-D float64 device signal")
            self.x = x
            self.nx = self._xdev.shape[0]
        else:
            self.x = np.asarray(x).astype(float)
            self.nx = len(x)
        self.sr = sr
        maxdelay = None if fmin is None else int(sr / fmin)
        mindelay = 2 if fmax is None else int(sr / fmax)
        if window is None:
            window = self.nx if maxdelay is None else 3 * maxdelay
        if not np.iterable(window):
            window = np.ones(window)
        self.wind = window
        self.nwind = len(window)
        self.mindelay = mindelay
        self.maxdelay = int(round(self.nwind / 2)) if maxdelay is None else maxdelay
        if hop is None:
            hop = self.nwind // 2
        self.hop = hop
        self.threshold = threshold
        self.vthresh = vthresh
        self.ncand = ncand
        self.cand_method = cand_method
        self.fftthresh = fftthresh
        self._res = None                 # arrays of the last calc(): the Periodicity objects are built on first use
        self._periods = []

    # ---- the launch --------------------------------------------------------------------------------------------
    def _run(self, centres):
        """One pvx_periodicity launch for the frames centred at `centres` (int64); host arrays back."""
        if self.method not in _METHODS:
            raise ValueError("unknown periodicity method %r (use 'xcorr' or 'amdf')" % (self.method,))
        method = _METHODS[self.method]
        cm = _CAND_METHODS.get(self.cand_method, 3)
        nwl = self.nwind // 2
        bad = (centres - nwl < 0) | (centres - nwl + self.nwind > self.nx)
        if bad.any():
            raise ValueError("the frame centred at %d leaves the signal (%d samples, window %d)"
                             % (int(centres[bad][0]), self.nx, self.nwind))
        lib = _lib.load()
        _lib.init()
        nf, ncand = len(centres), int(self.ncand)
        wind = np.ascontiguousarray(self.wind, dtype=np.float64)
        centres = np.ascontiguousarray(centres, dtype=np.int64)
        args = (int(self.nwind), centres.ctypes.data_as(_lib.c_int64_p), nf, method, cm, int(self.mindelay), int(self.maxdelay),
                float(self.threshold), float(self.vthresh), ncand, float(self.fftthresh))
        if self._xdev is None:
            per = np.empty(nf * ncand)
            st = np.empty(nf * ncand)
            cnt = np.empty(nf, dtype=np.int32)
            pref = np.empty(nf, dtype=np.int32)
            _lib.check(lib.pvx_periodicity(_lib.dptr(self.x) if self.x.flags.c_contiguous else _lib.dptr(np.ascontiguousarray(self.x)),
                                           self.nx, _lib.dptr(wind), *args, _lib.dptr(per), _lib.dptr(st),
                                           cnt.ctypes.data_as(_lib.c_int32_p), pref.ctypes.data_as(_lib.c_int32_p)),
                       "pvx_periodicity")
        else:
            import torch
            dev = _lib.bound_torch_device()   # the outputs and the stream must be the bound device's
            dper = torch.empty(max(nf * ncand, 1), dtype=torch.float64, device=dev)
            dst = torch.empty_like(dper)
            dcnt = torch.empty(max(nf, 1), dtype=torch.int32, device=dev)
            dpref = torch.empty_like(dcnt)
            stream = torch.cuda.current_stream()
            _lib.check(lib.pvx_periodicity_dev(ctypes.c_void_p(self._xdev.ptr), self.nx, _lib.dptr(wind), *args,
                                               ctypes.c_void_p(dper.data_ptr()), ctypes.c_void_p(dst.data_ptr()),
                                               ctypes.c_void_p(dcnt.data_ptr()), ctypes.c_void_p(dpref.data_ptr()),
                                               ctypes.c_void_p(stream.cuda_stream)),
                       "pvx_periodicity_dev")
            per = dper.cpu().numpy()[:nf * ncand]
            st = dst.cpu().numpy()[:nf * ncand]
            cnt = dcnt.cpu().numpy()[:nf]
            pref = dpref.cpu().numpy()[:nf]
        return {"period": per.reshape(nf, ncand), "strength": st.reshape(nf, ncand), "count": cnt, "preferred": pref}

    def _frame(self, res, i, index):
        pp = Periodicity(self, index, _row=(res["period"][i], res["strength"][i], int(res["count"][i]), int(res["preferred"][i])))
        pp.set_time_properties(index)
        return pp

    # ---- the reference's interface ------------------------------------------------------------------------------
    @property
    def periods(self):
        if self._res is not None:                                    # calc(): build the frames now
            res, self._res = self._res, None
            self._periods = [self._frame(res, i, ix) for i, ix in enumerate(res["index"])]
        return self._periods

    @periods.setter
    def periods(self, value):
        self._res = None
        self._periods = value

    def per_at_index(self, index):
        """Periodicity of the frame centred at round(index) (Periodicity.py:346-360)."""
        res = self._run(np.array([_centre(index)], dtype=np.int64))
        return self._frame(res, 0, index)

    def calc(self, hop=None, threshold=None):
        """Local periodicity over the whole signal (Periodicity.py:362-394): frames arange(nwind, nx - nwind, hop),
        all in one launch."""
        if hop is None:
            hop = self.hop
        oldthresh = self.threshold
        if threshold is not None:
            self.threshold = threshold
        try:
            idxvec = np.arange(self.nwind, self.nx - self.nwind, hop)
            centres = np.array([_centre(i) for i in idxvec], dtype=np.int64) if idxvec.dtype.kind == "f" else idxvec.astype(np.int64)
            res = self._run(centres) if len(centres) else {"period": np.empty((0, self.ncand)), "strength": np.empty((0, self.ncand)),
                                                           "count": np.empty(0, np.int32), "preferred": np.empty(0, np.int32)}
            res["index"] = idxvec
            self._periods = []
            self._res = res
        finally:
            self.threshold = oldthresh

    def calcPeriodByPeriod(self, threshold=None, tf=None, f=None):
        """Period-by-period walk (Periodicity.py:396-444): one frame per step, the next one a period further on."""
        self.periods = []
        oldthresh = self.threshold
        if threshold is not None:
            self.threshold = threshold
        try:
            idxmax = self.nx - self.nwind
            idx = self.nwind
            while idx < idxmax:
                pp = self.per_at_index(idx)
                if f is None:
                    di = pp.get_preferred_period()
                else:
                    thisf = np.interp(pp.time, tf, f)
                    if len(pp.cand_period) > 0 and thisf > 0:
                        imin = np.argmin(np.abs(self.sr / thisf - pp.cand_period))
                        pp.preferred = imin
                        di = pp.cand_period[imin]
                    else:
                        di = 0
                if di:
                    idx += di
                    self._periods.append(pp)
                else:
                    idx += self.mindelay
        finally:
            self.threshold = oldthresh

    def _preferred(self):
        """(period, strength, index) of the preferred candidate per frame, 0 / 0 where there is none."""
        if self._res is not None:
            r = self._res
            n = len(r["count"])
            pref = np.maximum(r["preferred"], 0).astype(np.intp)
            has = r["count"] > 0
            rows = np.arange(n)
            per = np.where(has, r["period"][rows, pref] if n else np.empty(0), 0.0)
            st = np.where(has, r["strength"][rows, pref] if n else np.empty(0), 0.0)
            return per, st, np.asarray(r["index"], dtype=float)
        per = np.array([p.get_preferred_period() for p in self._periods], dtype=float)
        st = np.array([p.get_preferred_strength() for p in self._periods], dtype=float)
        return per, st, np.array([p.index for p in self._periods], dtype=float)

    def get_f0(self, thresh=0.0):
        """f0 per frame (Periodicity.py:472-484): sr / preferred period where its strength > thresh, else NaN."""
        per, st, _ = self._preferred()
        keep = st > thresh
        if np.any(keep & (per == 0)):
            raise ZeroDivisionError("a frame without candidates passes thresh=%r (the reference divides by 0 there)" % (thresh,))
        f0 = np.full(len(per), np.nan)
        f0[keep] = self.sr / per[keep]
        return f0

    def get_times(self):
        if self._res is not None:
            return np.asarray(self._res["index"], dtype=float) / self.sr
        return np.array([p.time for p in self._periods], dtype=float)

    def get_strength(self):
        return self._preferred()[1]


class PeriodTimeSeries(PeriodSeries):
    pass


def _unsupported_fn(name, where, see=""):
    def fn(*args, **kwargs):
        raise NotImplementedError(
            "%s (Periodicity.py:%s) is a sequential scalar walk, one decision per period, and is not mirrored by "
            "pypevoc_amd; use the reference for it (see INTEGRATION.md, 'not mirrored')%s" % (name, where, see))
    fn.__name__ = name
    fn.__doc__ = "Not mirrored: Periodicity.py:%s." % where
    return fn


amdf = _unsupported_fn("amdf", "38-52")
period_marks_amdf = _unsupported_fn("period_marks_amdf", "525-570")
period_marks_corr = _unsupported_fn("period_marks_corr", "573-618", "; pypevoc_amd.marks.period_marks_corr runs it on the GPU (MARKS.md)")
period_marks_peak = _unsupported_fn("period_marks_peak", "621-709", "; pypevoc_amd.marks.period_marks_peak runs it on the GPU (MARKS.md)")


class PeriodByPeriod(PeriodSeries):
    """Not mirrored (Periodicity.py:509-522; its __init__ cannot run in the reference)."""

    def __init__(self, *args, **kwargs):
        _unsupported_fn("PeriodByPeriod", "509-522")()
