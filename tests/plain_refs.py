"""Plain float64 references for the kernels beside the analysis path (k_desc.hip, k_reduce.hip).

Every function is a Python loop over frames (and, inside a frame, over peaks or samples) that states the operation once
more in the obvious order, one rounding per addition, left to right.  Nothing is vectorised over frames: the product's
host path (PVAnalysis.py's numpy branch) broadcasts over (frames, K, K) and sums pairwise, so a slip in that restatement
and one in the kernels cannot hide behind each other here.  tests/test_plain_refs_cpu.py pins these functions to the
reference's recorded values (D1, W1, W2), to the oracle and to the host path before a GPU test relies on them."""
import numpy as np


# ------------------------------------------------------------------ descriptors on the (F, K) result arrays
def calc_f0_ref(f, mag, fmin=50, fmax=10000, thr=0.1):
    """PV.calc_f0: per frame the lowest frequency among the peaks with fmin < f < fmax and mag > thr * max(mag); the first
    one on a tie; (0.0, slot 0) where no peak qualifies.  The maximum is numpy's: a NaN magnitude makes it NaN, every
    comparison with the limit then fails and the frame has no candidate."""
    f = np.asarray(f, dtype=np.float64)
    mag = np.asarray(mag, dtype=np.float64)
    F = f.shape[0]
    fm = np.zeros(F)
    idx = np.zeros(F, dtype=np.int32)
    for fr in range(F):
        maxmag = float(mag[fr, 0])
        for k in range(1, f.shape[1]):
            m = float(mag[fr, k])
            if m != m or (maxmag == maxmag and m > maxmag):      # a NaN enters and stays
                maxmag = m
        lim = maxmag * thr
        found = False
        for k in range(f.shape[1]):
            fk = float(f[fr, k])
            if fk > fmin and fk < fmax and float(mag[fr, k]) > lim and (not found or fk < fm[fr]):
                fm[fr] = fk
                idx[fr] = k
                found = True
    return fm, idx


def harmonic_power_ref(f, mag, f_threshold=0.01):
    """PV.calc_harmonic_power: for every valid peak j of a frame (f > 0) the valid peaks c with |f_c / n / f_j - 1| <
    f_threshold, n = round-half-even(f_c / f_j) or 1 where that is 0, are its harmonic set; nharmonics counts them.

    The row-indexing quirk stays: the reference selects `mag[valid_idx]`, the ROWS of mag numbered like the frame's valid
    slots, so hpower adds the power of whole rows mag[c, :] over the harmonic set, and a frame with a valid slot >= F is an
    IndexError.  Sums run left to right: the squares of a row, then the rows of a set."""
    f = np.asarray(f, dtype=np.float64)
    mag = np.asarray(mag, dtype=np.float64)
    F, K = f.shape
    hpower = np.zeros((F, K))
    nharm = np.zeros((F, K))
    rowpow = {}

    def row_power(r):
        if r not in rowpow:
            s = 0.0
            for v in mag[r]:
                s += float(v) * float(v)
            rowpow[r] = s
        return rowpow[r]

    with np.errstate(divide="ignore", invalid="ignore"):
        for fr in range(F):
            slots = [k for k in range(K) if f[fr, k] > 0]
            for c in slots:
                if c >= F:
                    raise IndexError("index %d is out of bounds for axis 0 with size %d" % (c, F))
            vf = f[fr, slots]
            for j in slots:
                n = np.round(vf / f[fr, j])
                n[n == 0] = 1
                inh = np.abs(vf / n / f[fr, j] - 1)
                s = 0.0
                cnt = 0
                for c, d in zip(slots, inh):
                    if d < f_threshold:
                        s += row_power(c)
                        cnt += 1
                hpower[fr, j] = s
                nharm[fr, j] = cnt
    return hpower, nharm


# ------------------------------------------------------------------ hop-strided windowed reductions
def frame_starts(n, wlen, hop):
    """Frames start at i * hop while i * hop < n - wlen (strict): a frame that would end on the last sample is not taken."""
    return list(range(0, n - wlen, hop))


def heterodyne_ref(x, hetsig, wind, hop):
    """heterodyne: 2 * sum_j (x * hetsig)[pos + j] * wind[j] / sum(wind) per frame, and the frame's centre sample."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(hetsig, dtype=np.complex128)
    wind = np.asarray(wind, dtype=np.float64)
    wlen = len(wind)
    norm = float(np.sum(wind))
    x, h, wind = x.tolist(), h.tolist(), wind.tolist()               # Python floats: the same float64 arithmetic
    out, icent = [], []
    for pos in frame_starts(len(x), wlen, hop):
        sr = si = 0.0
        for j in range(wlen):
            sr += (x[pos + j] * h[pos + j].real) * wind[j]
            si += (x[pos + j] * h[pos + j].imag) * wind[j]
        out.append(complex(sr / norm * 2.0, si / norm * 2.0))
        icent.append(pos + wlen // 2)
    return np.array(out, dtype=np.complex128), np.array(icent, dtype=np.int64)


def rms_ref(x, wind, hop):
    """RMSWind: sqrt(sum_j ((x[pos + j] * wind[j]) ** 2 / sum(wind ** 2))) per frame."""
    x = np.asarray(x, dtype=np.float64)
    wind = np.asarray(wind, dtype=np.float64)
    wlen = len(wind)
    norm = float(np.sum(wind ** 2))
    x, wind = x.tolist(), wind.tolist()
    out = []
    for pos in frame_starts(len(x), wlen, hop):
        s = 0.0
        for j in range(wlen):
            xw = x[pos + j] * wind[j]
            s += xw * xw / norm
        out.append(np.sqrt(s))
    return np.array(out, dtype=np.float64)


def funcwind_ref(name, x, wind, hop, power=1):
    """FuncWind with a named reducer: func(x[pos : pos + wlen] * wind) / sum(wind ** power) per frame (divisor 1 for power
    0).  sum / mean of a complex signal are complex; std / var are numpy's two-pass population forms (for complex frames
    the mean of |xw - mean| ** 2, a real number); max / min propagate a NaN and are refused for complex frames."""
    x = np.asarray(x)
    cpx = np.iscomplexobj(x)
    x = x.astype(np.complex128 if cpx else np.float64)
    wind = np.asarray(wind, dtype=np.float64)
    wlen = len(wind)
    divisor = float(sum(wind ** power)) if power > 0 else 1.0
    if cpx and name in ("max", "min"):
        raise TypeError("max / min of complex frames")
    x, wind = x.tolist(), wind.tolist()
    out = []
    for pos in frame_starts(len(x), wlen, hop):
        xw = [x[pos + j] * wind[j] for j in range(wlen)]
        if name in ("max", "min"):
            r = xw[0]
            for v in xw[1:]:
                if r != r:
                    break
                if v != v or (v > r if name == "max" else v < r):
                    r = v
        else:
            s = 0.0
            for v in xw:
                s = s + v
            if name == "sum":
                r = s
            else:
                m = s / wlen
                if name == "mean":
                    r = m
                else:
                    q = 0.0
                    for v in xw:
                        d = v - m
                        q += d.real * d.real + d.imag * d.imag if cpx else d * d
                    q /= wlen
                    r = np.sqrt(q) if name == "std" else q
        out.append(r / divisor)
    complex_out = cpx and name in ("sum", "mean")
    return np.array(out, dtype=np.complex128 if complex_out else np.float64)
