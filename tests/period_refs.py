"""A plain float64 restatement of one PeriodSeries frame, for the differential tests of k_period.hip.

It follows the formulation of the library pypevoc_amd mirrors, not the kernel's: the full similarity array (xcorr: the
2*nwind-1 entries of the frame's autocorrelation over the window's; amdf: nwind entries, divisor n - lag) sliced with
numpy's own index rules, the builtin max() for the normaliser and the voicing test, an arg-max-and-overwrite peak
loop, the three-point parabola, 'fft' / 'min' / 'similar' and argsort(strength)[::-1].  Nothing of pypevoc_amd is used.

Every lag is summed on its own, in np.longdouble where that is an extended type (x86: 64-bit mantissa), with
math.fsum otherwise, so the similarities are correctly rounded to a few units of 1e-19 before the one rounding to
float64: closer to the exact values than the kernel's float64 FMAs and than numpy's float64 sums.  Only the entries
some slice reads are summed; the first negative lag is searched over every lag 0 .. nwind-1, in order.

Beside the result, period_frame_ref returns how far every discrete decision of the frame is from flipping (margins):
inputs whose margins are far above the kernel's error have one right answer, so a test can ask for it exactly.
"""
import math

import numpy as np

EXTENDED = bool(np.finfo(np.longdouble).eps < 1e-18)                 # checked at import; math.fsum otherwise
EXACT_TIE = "exact_tie"


def _wide(a):
    return a.astype(np.longdouble) if EXTENDED else a


def _total(v):
    return v.sum(dtype=np.longdouble) if EXTENDED else np.float64(math.fsum(v))      # numpy scalars: 0 / 0 is NaN


class FrameSimilarity(object):
    """The windowed frame xw = (xs - mean(xs)) * wind centred at round(centre) and its similarity array, summed lag by
    lag on demand.  `take(slice)` is full_array[slice] under numpy's rules (negative bounds wrap once, then clip)."""

    def __init__(self, x, centre, wind, method):
        if method not in ("xcorr", "amdf"):
            raise ValueError("method %r" % (method,))
        wind = np.asarray(wind, dtype=np.float64)
        n = len(wind)
        start = int(np.round(centre)) - n // 2
        xs = np.asarray(x, dtype=np.float64)[start:start + n]
        if start < 0 or len(xs) != n:
            raise ValueError("the frame centred at %r leaves the signal" % (centre,))
        self.n, self.method = n, method
        self.xw = (xs - float(_total(_wide(xs)) / n)) * wind
        self.length = 2 * n - 1 if method == "xcorr" else n
        self._x = _wide(self.xw)
        self._w = _wide(wind)
        self._lags = {}
        self.zero = set()                                            # lags whose every term is 0: exactly 0 in any order of summation

    def lag(self, l):
        """xcorr: sum_i xw[i] xw[i+l] / sum_i w[i] w[i+l];  amdf: sum_i |xw[i] - xw[i+l]| / (n - l)."""
        v = self._lags.get(l)
        if v is None:
            n = self.n
            a, b = self._x[:n - l], self._x[l:]
            terms = a * b if self.method == "xcorr" else np.abs(a - b)
            if not terms.any():
                self.zero.add(l)
            with np.errstate(all="ignore"):
                v = float(_total(terms) / (_total(self._w[:n - l] * self._w[l:]) if self.method == "xcorr" else n - l))
            self._lags[l] = v
        return v

    def at(self, j):
        return self.lag(abs(j - (self.n - 1)) if self.method == "xcorr" else j)

    def take(self, sl):
        return np.array([self.at(int(j)) for j in np.arange(self.length)[sl]], dtype=np.float64)

    def take_zero(self, sl):
        """Which entries of take(sl) are sums of nothing but zeros."""
        return np.array([abs(int(j) - (self.n - 1)) in self.zero if self.method == "xcorr" else int(j) in self.zero
                         for j in np.arange(self.length)[sl]], dtype=bool)


def _pick_peaks(y, minval, npeaks, exact=None):
    """The peak finder on y: interior maxima y[k-1] < y[k] >= y[k+1] score y[k] - min(y), everything else 0; the best
    score is taken and overwritten until none is above minval - min(y) or npeaks are found (a minval of 0 or None means
    min(y)).  Returns the ascending positions and the margins of these decisions (on y's own scale).  exact: which values of
    y are exact whatever the arithmetic; a kept maximum followed by its equal, both exact, is a plateau by design."""
    y = np.asarray(y, dtype=np.float64)
    if len(y) < 3:
        raise ValueError("peaks need three values")
    miny = np.min(y)
    numeric_th = bool(minval)
    th = (minval if numeric_th else miny) - miny
    inner = y[1:-1]
    mask = (y[:-2] < inner) & (inner >= y[2:])
    score = mask.astype(int) * (inner - miny)
    work = score.copy()
    picked = []
    while len(picked) < npeaks:
        b = int(np.argmax(work))
        if not work[b] > th:
            break
        picked.append(b)
        work[b] = th - 1
    marg = {}
    if not np.isnan(miny):
        gaps = list(np.abs(score[mask] - th))
        if numeric_th:
            gaps.append(abs(th))                                     # the zeros of the non-maxima against th
        if gaps:
            marg["pick_threshold"] = (float(min(gaps)), None)
        left = np.ones(len(score), bool)
        left[picked] = False
        left &= score > th
        if len(picked) == npeaks and left.any():
            r = int(np.flatnonzero(left)[np.argmax(score[left])])
            last = picked[-1]
            if not mask[last] and not mask[r]:                       # both are the literal 0: the lower index wins
                marg["ncand_cap"] = (0.0, EXACT_TIE)
            else:
                marg["ncand_cap"] = (float(score[last] - score[r]), None)
        shape = []
        for b in picked:
            up, down = inner[b] - y[b], inner[b] - y[b + 2]
            if mask[b] and down == 0 and exact is not None and exact[b + 1] and exact[b + 2]:
                marg["plateau"] = (0.0, EXACT_TIE)
                shape.append(up)
            else:
                shape.append(min(up, abs(down)) if mask[b] else max(-up, -down))
        if shape:
            marg["peak_shape"] = (float(min(shape)), None)
    return np.sort(np.array(picked, dtype=np.intp) + 1), marg


def _refine(y, k):
    """Three-point parabola through y[k-1 .. k+1] where y[k] is a maximum; position clamped to y's index range."""
    s0, s1, s2 = y[k - 1], y[k], y[k + 1]
    if s1 > s0 and s1 >= s2:
        c = s1
        b = (s2 - s0) / 2
        a = (s2 + s0) / 2 - c
        off = -b / 2 / a
        pos, val = float(k) + off, a * off * off + b * off + c
    else:
        pos, val = k, s1
    grid = np.arange(len(y))
    return float(np.interp(pos, grid, grid)), float(val)


def _top_two_gap(values, largest):
    v = np.sort(np.asarray(values, dtype=np.float64))
    return float(v[-1] - v[-2]) if largest else float(v[1] - v[0])


def period_frame_ref(x, centre, wind, method, cand_method, mindelay, maxdelay, threshold, vthresh, ncand, fftthresh,
                     sim=None):
    """One frame of PeriodSeries(x, window=wind, ...) centred at round(centre).

    Returns (period, strength, count, preferred, margins): the candidates sorted by strength, strongest first,
    preferred the index of the chosen one among them (-1 for none).  margins maps a decision to (distance, tag): the
    distance by which the deciding quantity would have to move to flip it, tag None or EXACT_TIE for a decision between
    two literal zeros (by index, not by value).  Similarities are normalised to a maximum of 1, so the distances are
    absolute on that scale, except 'preferred' of 'min' / 'fft' (samples) and the fft_* ones (fractions of the largest
    FFT peak).  Keys: firstneg (|xc[l]| / xc[0] over the lags up to and including the first negative one, every lag
    when there is none), firstneg_outcome (a string, no distance: 'early', 'past_maxdelay' or 'nowhere'), voicing,
    pick_threshold, ncand_cap, peak_shape, sort, preferred, fft_threshold, fft_cap, fft_peak_shape; and the exact ties
    firstneg_zeros (lags before the first negative one whose every product is 0) and plateau (a kept maximum whose next
    value is the same exact number: y[k] >= y[k+1] holds with equality).

    `sim`: a FrameSimilarity of the same x, centre, wind and method, to share its sums between calls.
    Raises ValueError where the library does (an empty normaliser slice, fewer than three values to pick peaks from)."""
    mindelay, maxdelay = int(mindelay), int(maxdelay)
    fs = sim if sim is not None else FrameSimilarity(x, centre, wind, method)
    n = fs.n
    marg = {}
    with np.errstate(all="ignore"):
        if method == "amdf":
            norm = max(fs.take(slice(n - 1 - maxdelay, n - 1 + maxdelay)))
            imin = mindelay
            y = (norm - fs.take(slice(imin, maxdelay))) / norm
            exact = fs.take_zero(slice(imin, maxdelay))              # (norm - 0) / norm is 1
        else:
            firstneg = None
            for l in range(n):
                if fs.lag(l) < 0:
                    firstneg = l
                    break
            upto = range(n if firstneg is None else firstneg + 1)
            seen = np.array([fs.lag(l) for l in upto if l not in fs.zero])
            if fs.lag(0) > 0 and not np.isnan(seen).all():
                marg["firstneg"] = (float(np.nanmin(np.abs(seen)) / fs.lag(0)), None)
            if len(seen) < len(upto):                                # an exact 0 is not negative, in any arithmetic
                marg["firstneg_zeros"] = (0.0, EXACT_TIE)
            marg["firstneg_outcome"] = "nowhere" if firstneg is None else ("early" if firstneg < maxdelay else "past_maxdelay")
            imin = max(mindelay if firstneg is None else firstneg, mindelay)
            norm = max(fs.take(slice(n - 1 - maxdelay, n - 1 + maxdelay)))
            y = fs.take(slice(n - 1 + imin, n - 1 + maxdelay)) / norm
            exact = fs.take_zero(slice(n - 1 + imin, n - 1 + maxdelay))

        pos = np.empty(0)
        val = np.empty(0)
        if len(y) > 0:
            top = max(y)
            if top == top:
                marg["voicing"] = (float(abs(top - vthresh)), None)
            if top > vthresh:
                idx, pm = _pick_peaks(y, threshold, ncand, exact)
                marg.update(pm)
                fine = [_refine(y, int(k)) for k in idx]
                pos = np.array([f[0] for f in fine]) + imin
                val = np.array([f[1] for f in fine])

        preferred = 0
        if len(pos) > 0:
            if cand_method == "fft":
                spec = np.abs(np.fft.rfft(fs.xw))[:int(n / 2)]
                fidx, fm = _pick_peaks(spec, None, ncand)
                fval = spec[fidx]
                thr = np.max(fval * fftthresh)
                fper = n / fidx[fval > thr]
                dist = [np.min(np.abs(fper - p)) for p in pos]
                preferred = int(np.argmin(dist))
                scale = float(np.max(fval))
                marg["fft_threshold"] = (float(np.min(np.abs(fval - thr))) / scale, None)
                if "ncand_cap" in fm:
                    rejected = np.setdiff1d(np.flatnonzero((spec[:-2] < spec[1:-1]) & (spec[1:-1] >= spec[2:])) + 1, fidx)
                    if len(rejected) and spec[rejected].max() > thr:
                        marg["fft_cap"] = (fm["ncand_cap"][0] / scale, fm["ncand_cap"][1])
                above = fidx[fval > thr]
                marg["fft_peak_shape"] = (float(min(min(spec[k] - spec[k - 1], abs(spec[k] - spec[k + 1])) for k in above)) / scale, None)
                if len(pos) > 1:
                    marg["preferred"] = (_top_two_gap(dist, largest=False), None)
            elif cand_method == "min":
                preferred = int(np.argmin(pos))
                if len(pos) > 1:
                    marg["preferred"] = (_top_two_gap(pos, largest=False), None)
            elif cand_method == "similar":
                preferred = int(np.argmax(val))
                if len(pos) > 1:
                    marg["preferred"] = (_top_two_gap(val, largest=True), None)
        if len(val) > 1:
            marg["sort"] = (float(np.min(np.diff(np.sort(val)))), None)
        order = np.argsort(val)[::-1]
        at = np.flatnonzero(order == preferred)
    return pos[order], val[order], len(pos), (int(at[0]) if len(at) else -1), marg


def failing_margins(margins, floor):
    """The decisions of a margins dict that are nearer than `floor` to flipping, exact ties by design apart."""
    return {k: v for k, v in margins.items() if isinstance(v, tuple) and v[1] != EXACT_TIE and not v[0] >= floor}
