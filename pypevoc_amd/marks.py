"""Period marks on the GPU: the reference's period_marks_corr (pypevoc/Periodicity.py:573-618) and period_marks_peak
(:621-709) as walks in k_marks.hip (pvx_marks_corr / pvx_marks_peak; MARKS.md states both walks, the limits and the bounds).

period_marks_corr and period_marks_peak are drop-in: one signal, the reference's arguments, the reference's results.  Where
the reference raises, truncates a slice or would not end (MARKS.md, "Row status") they raise ValueError.  period_marks_rows
runs many stretches x[start : stop] of one signal as one launch and returns the status bits instead.  x is a host array or a
float64 / float32 / int16 tensor already on the GPU; integers and float32 widen exactly.  No CPU fallback.

The names pypevoc_amd.Periodicity.period_marks_corr / period_marks_peak stay stubs, as INTEGRATION.md says."""
import ctypes
import math

import numpy as np

from . import _lib

# PVX_MARKS_* of include/pvx.h
NO_PEAK, PAST_END, BAD_F0, NO_ADVANCE, CAPACITY, STEPS, SHORT_FIT = 1, 2, 4, 8, 16, 32, 64
CORR_MAX_LDS = 8000
MAX_FIT_POINTS = 64

_MESSAGES = (
    (NO_PEAK, "a step's correlation has no local maximum (the reference: argmin of an empty sequence)"),
    (PAST_END, "the target window s + P + W leaves the signal after the period grew"),
    (BAD_F0, "f0 <= 0, a period below one sample, t0 < 0 or no finite f0"),
    (NO_ADVANCE, "a step with NaN f0 has no positive delay to advance by"),
    (CAPACITY, "max_marks reached"),
    (STEPS, "max_steps reached"),
)


def status_message(status):
    """The words for a row's status bits (SHORT_FIT is a note on the marks, not an end of the walk)."""
    return "; ".join(m for b, m in _MESSAGES if status & b)


def marks_last_kernels():
    """The kernel the calling thread's last marks launch ran: 'k_marks_corr' or 'k_marks_peak' ('' if nothing ran)."""
    return _lib.load().pvx_marks_last_kernels().decode()


def _signal(x):
    """(device signal or None, float64 host array or None, length)"""
    if _lib.is_device_array(x):
        sig = _lib.DeviceSignal(x)
        if len(sig.shape) != 1:
            raise ValueError("a 1-D signal is expected")
        if sig.dtype != np.float64:                                  # float32 / int16: every value is a float64 value
            import torch
            x = torch.as_tensor(x).to(torch.float64)
            sig = _lib.DeviceSignal(x)
        return sig, None, sig.shape[0]
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("a 1-D signal is expected")
    if x.dtype.kind not in "fiub":
        raise TypeError("a real signal is expected, got %s" % x.dtype)
    return None, np.ascontiguousarray(x, dtype=np.float64), len(x)


def _rows(starts, stops, n):
    starts = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
    stops = np.ascontiguousarray(stops, dtype=np.int64).reshape(-1)
    if len(starts) != len(stops):
        raise ValueError("starts and stops differ in length")
    if len(starts) and (starts.min() < 0 or (starts > stops).any() or stops.max() > n):
        raise ValueError("a row does not lie inside the %d samples of the signal" % n)
    return starts, stops


def _per_row(v, nrows, name):
    if v is None:
        return None
    v = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (nrows,)) if np.ndim(v) == 0 else v, dtype=np.float64)
    if v.shape != (nrows,):
        raise ValueError("%s: one value per row is expected" % name)
    return v


def _track(tf, f):
    tf = np.ascontiguousarray(tf, dtype=np.float64).reshape(-1)
    f = np.ascontiguousarray(f, dtype=np.float64).reshape(-1)
    if len(tf) == 0 or len(tf) != len(f):
        raise ValueError("tf and f must hold the same, non-zero number of values (%d, %d)" % (len(tf), len(f)))
    if not np.isfinite(tf).all() or (np.diff(tf) <= 0).any():
        raise ValueError("tf must be finite and strictly increasing")
    return tf, f


def _opt(a):
    return _lib.dptr(a) if a is not None else None


def corr_max_steps(nsamp, sr, min_per, f):
    """The bound the host gives the corr walk: a step that places a mark advances by more than min_per and one that does not
    by 1 / f0 >= 1 / max(f), so (L / sr) / min(min_per, 1 / max f) + 2 steps reach the end; never more than 4 L + 16 (a
    walk that creeps by less -- NaN-f0 steps repeating a tiny delay, min_per <= 0 -- ends with STEPS)."""
    ceiling = 4 * int(nsamp) + 16
    fin = f[np.isfinite(f) & (f > 0)]
    if min_per > 0 and len(fin):
        adv = min(float(min_per), 1.0 / float(fin.max()))
        steps = (nsamp / float(sr)) / adv + 2
        if steps < ceiling:
            return int(math.ceil(steps))
    return ceiling


def _run_corr(x, starts, stops, t0, toff, sr, tf, f, window_size, min_per, max_marks, max_steps):
    sig, xh, n = _signal(x)
    starts, stops = _rows(starts, stops, n)
    nrows = len(starts)
    tf, f = _track(tf, f)
    t0 = _per_row(t0, nrows, "t0")
    toff = _per_row(toff, nrows, "toff")
    W = int(window_size)
    if W < 2:
        raise ValueError("window_size must be at least 2 (got %d)" % W)
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            fallback = float(np.nanmean(f))                          # Periodicity.py:587
    longest = int((stops - starts).max()) if nrows else 0
    if max_steps is None:
        max_steps = corr_max_steps(longest, sr, float(min_per), f)
    if max_marks is None:
        max_marks = int(max_steps) + 1
    max_marks, max_steps = int(max_marks), int(max_steps)
    marks = np.zeros((nrows, max_marks))
    count = np.zeros(nrows, dtype=np.int32)
    status = np.zeros(nrows, dtype=np.int32)
    if nrows == 0:
        return marks, count, status
    lib = _lib.load()
    _lib.init()
    args = (n, starts.ctypes.data_as(_lib.c_int64_p), stops.ctypes.data_as(_lib.c_int64_p), _lib.dptr(t0), _opt(toff), nrows, _lib.dptr(tf),
            _lib.dptr(f), len(tf), fallback, float(sr), W, float(min_per), max_marks, max_steps)
    if sig is not None:
        import torch
        tdev = _lib.bound_torch_device()
        dm = torch.zeros((nrows, max_marks), dtype=torch.float64, device=tdev)
        di = torch.empty((2, nrows), dtype=torch.int32, device=tdev)
        stream = torch.cuda.current_stream()
        _lib.check(lib.pvx_marks_corr_dev(ctypes.c_void_p(sig.ptr), *args, ctypes.c_void_p(dm.data_ptr()), ctypes.c_void_p(di[0].data_ptr()),
                                          ctypes.c_void_p(di[1].data_ptr()), ctypes.c_void_p(stream.cuda_stream)), "pvx_marks_corr_dev")
        marks = dm.cpu().numpy()
        hi = di.cpu().numpy()
        count, status = hi[0].copy(), hi[1].copy()
    else:
        _lib.check(lib.pvx_marks_corr(_lib.dptr(xh), *args, _lib.dptr(marks), count.ctypes.data_as(_lib.c_int32_p),
                                      status.ctypes.data_as(_lib.c_int32_p)), "pvx_marks_corr")
    return marks, count, status


def _peak_track(tf, f, n):
    """(tf or None, f) as the C entry takes them: with tf=None one value, or one per sample of x (:643-647)"""
    if tf is not None:
        return _track(tf, f)
    if np.ndim(f) == 0:
        return None, np.array([float(f)])
    f = np.ascontiguousarray(f, dtype=np.float64).reshape(-1)
    if len(f) != n:
        raise ValueError("without tf, f holds one value per sample of x (%d values, %d samples)" % (len(f), n))
    return None, (f if n != 1 else f.copy())


def _run_peak(x, starts, stops, toff, sr, tf, f, fit_points, max_marks, max_steps):
    sig, xh, n = _signal(x)
    starts, stops = _rows(starts, stops, n)
    nrows = len(starts)
    scalar_f = tf is None and np.ndim(f) == 0
    tf, f = _peak_track(tf, f, n)
    toff = _per_row(toff, nrows, "toff")
    fit_points = int(fit_points)
    if fit_points < 3:
        raise ValueError("fit_points must be at least 3 (got %d; the reference cannot run below 3)" % fit_points)
    longest = int((stops - starts).max()) if nrows else 0
    if max_steps is None:
        max_steps = longest + 1                                      # a step advances by at least one sample
    if max_marks is None:
        max_marks = max(1, min(longest, int(max_steps)))
    max_marks, max_steps = int(max_marks), int(max_steps)
    marks = np.zeros((nrows, max_marks))
    vals = np.zeros((nrows, max_marks))
    count = np.zeros(nrows, dtype=np.int32)
    status = np.zeros(nrows, dtype=np.int32)
    if nrows == 0:
        return marks, vals, count, status
    lib = _lib.load()
    _lib.init()
    nf = 1 if scalar_f else len(f)
    args = (n, starts.ctypes.data_as(_lib.c_int64_p), stops.ctypes.data_as(_lib.c_int64_p), _opt(toff), nrows, _opt(tf), _lib.dptr(f),
            0 if tf is None else len(tf), nf, float(sr), fit_points, max_marks, max_steps)
    if sig is not None:
        import torch
        tdev = _lib.bound_torch_device()
        dm = torch.zeros((2, nrows, max_marks), dtype=torch.float64, device=tdev)
        di = torch.empty((2, nrows), dtype=torch.int32, device=tdev)
        stream = torch.cuda.current_stream()
        _lib.check(lib.pvx_marks_peak_dev(ctypes.c_void_p(sig.ptr), *args, ctypes.c_void_p(dm[0].data_ptr()), ctypes.c_void_p(dm[1].data_ptr()),
                                          ctypes.c_void_p(di[0].data_ptr()), ctypes.c_void_p(di[1].data_ptr()),
                                          ctypes.c_void_p(stream.cuda_stream)), "pvx_marks_peak_dev")
        hm = dm.cpu().numpy()
        marks, vals = hm[0].copy(), hm[1].copy()
        hi = di.cpu().numpy()
        count, status = hi[0].copy(), hi[1].copy()
    else:
        _lib.check(lib.pvx_marks_peak(_lib.dptr(xh), *args, _lib.dptr(marks), _lib.dptr(vals), count.ctypes.data_as(_lib.c_int32_p),
                                      status.ctypes.data_as(_lib.c_int32_p)), "pvx_marks_peak")
    return marks, vals, count, status


def period_marks_corr(x, sr=1.0, t0=0.0, tf=[], f=[], window_size=1024, min_per=0.001):
    """add period marks information to file,
    based on correlation between adjacent periods

    :t0: first mark position
    :window_size: window to use for comparison between periods
    :returns: the mark times (float64), the first one t0

    (Periodicity.py:573-618 in k_marks.hip; ValueError where MARKS.md's status cases end the walk)
    """
    n = _signal(x)[2]
    marks, count, status = _run_corr(x, [0], [n], [float(t0)], None, sr, tf, f, window_size, min_per, None, None)
    if status[0]:
        raise ValueError("period_marks_corr: " + status_message(int(status[0])))
    return marks[0, :count[0]].copy()


def period_marks_peak(x, sr=1.0, tf=None, f=[], fit_points=3):
    """calculate period marks for x based on peak
    positions of the signal

    :x: signal
    :sr: sample rate (defalut 1 sample/sec)
    :tf: time at which frequency values are calulated
         (defaults to same samples as x)
    :f: frequency values
    :fit_points: number of points to use for peak fitting
    :returns: time markers, and the fitted values at them

    (Periodicity.py:621-709 in k_marks.hip; ValueError where MARKS.md's status cases end the walk)
    """
    n = _signal(x)[2]
    marks, vals, count, status = _run_peak(x, [0], [n], None, float(sr), tf, f, fit_points, None, None)
    if status[0] & ~SHORT_FIT:
        raise ValueError("period_marks_peak: " + status_message(int(status[0])))
    return marks[0, :count[0]].copy(), vals[0, :count[0]].copy()


def period_marks_rows(x, starts, stops, sr=1.0, tf=None, f=[], method="corr", t0=0.0, toff=None, window_size=1024, min_per=0.001,
                      fit_points=3, max_marks=None, max_steps=None):
    """The walks of the stretches x[starts[r] : stops[r]] in one launch: row r is what the single-signal function gives for
    that stretch, in row time (0 at the stretch's first sample).  The track (tf, f) is shared and read at toff[r] + t: toff[r] =
    starts[r] / sr puts a track in the recording's time under every stretch; None reads it in row time.  method 'corr'
    (t0: one first mark for all rows, or one per row) or 'peak'.  Returns a dict: marks [R, max_marks] (padded with 0), count,
    status (the bits NO_PEAK ... SHORT_FIT; 0: the walk ended by its own test), and for 'peak' vals.  max_marks / max_steps
    default to what the longest row can need."""
    if method == "corr":
        if tf is None:
            raise ValueError("method 'corr' needs a track (tf, f)")
        nrows = len(np.atleast_1d(starts))
        marks, count, status = _run_corr(x, starts, stops, np.broadcast_to(np.asarray(t0, dtype=np.float64), (nrows,)).copy()
                                         if np.ndim(t0) == 0 else t0, toff, sr, tf, f, window_size, min_per, max_marks, max_steps)
        return {"marks": marks, "count": count, "status": status}
    if method == "peak":
        marks, vals, count, status = _run_peak(x, starts, stops, toff, float(sr), tf, f, fit_points, max_marks, max_steps)
        return {"marks": marks, "vals": vals, "count": count, "status": status}
    raise ValueError("method %r: 'corr' or 'peak'" % (method,))
