"""Plain numpy references of the LPC spectral envelope and of PeakFinder's scan and three-point refinement (ENVELOPE.md), for
test_envelope_cpu.py and test_envelope_gpu.py.  numpy only.

  env_f64    y_k = 1 / |sum_j c_j z_k^j|, z_k = exp(-i pi k / npts), by Horner from c_p down in float64 complex arithmetic:
             what abs(scipy.signal.freqz([1], c, worN=npts)[1]) computes
  env_ld     the same in np.longdouble with a long-double pi: the reference the bound is measured against
  env_bound  per point, the relative error a float64 evaluation may have against env_ld:
                 4 [(2 p S + 8 D) 2^-53 / |A_k| + 3 2^-53],  S = sum |c_j|,  D = sum j |c_j|
             2 p S 2^-53 is Horner's rounding at |z| = 1 (p complex multiply-adds of at most 2 roundings per part each),
             8 D 2^-53 an 8-ulp error of z_k through |A'| <= D, 3 2^-53 the modulus and the reciprocal, 4 the project's factor
  peaks_ref  the scan (index i in 1 .. npts - 2 with y[i-1] < y[i] >= y[i+1], ascending), the fit through the three points
             and np.interp on the axis, per peak: idx, pos, val
  peak_margin  per peak of a row, min(y_i - y_{i-1}, y_i - y_{i+1}): how far the scan's comparisons are from flipping
"""
import numpy as np

LD = np.longdouble
PI_LD = 4 * np.arctan(LD(1))


def env_f64(c, npts):
    c = np.asarray(c, dtype=np.float64)
    w = np.pi * np.arange(npts) / npts
    z = np.cos(w) - 1j * np.sin(w)
    a = np.full(npts, c[-1], dtype=np.complex128)
    for j in range(len(c) - 2, -1, -1):
        a = a * z + c[j]
    with np.errstate(divide="ignore"):
        return 1.0 / np.abs(a)


def env_ld(c, npts):
    c = np.asarray(c, dtype=np.float64).astype(LD)
    w = PI_LD * np.arange(npts).astype(LD) / LD(npts)
    zr, zi = np.cos(w), -np.sin(w)
    ar, ai = np.full(npts, c[-1], dtype=LD), np.zeros(npts, dtype=LD)
    for j in range(len(c) - 2, -1, -1):
        ar, ai = ar * zr - ai * zi + c[j], ar * zi + ai * zr
    with np.errstate(divide="ignore"):
        return LD(1) / np.hypot(ar, ai)


def env_bound(c, npts, y_ld=None):
    c = np.asarray(c, dtype=np.float64)
    p = len(c) - 1
    S = float(np.sum(np.abs(c)))
    D = float(np.sum(np.arange(p + 1) * np.abs(c)))
    y = env_ld(c, npts) if y_ld is None else y_ld                     # 1 / |A_k|
    return 4 * ((2 * p * S + 8 * D) * 2.0**-53 * y.astype(np.float64) + 3 * 2.0**-53)


def scan(y):
    y = np.asarray(y)
    if len(y) < 3:
        return np.zeros(0, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        return np.nonzero((y[:-2] < y[1:-1]) & (y[1:-1] >= y[2:]))[0] + 1


def refine(y, i, x=None, fit=None):
    """(pos, val, lpos, a, b, c) of the peak at index i; fit None: refine's own test decides."""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    x = np.arange(n) if x is None else np.asarray(x)
    s0, s1, s2 = y[i - 1], y[i], y[i + 1]
    if fit is None:
        fit = bool(s1 > s0 and s1 >= s2)
    if not fit:
        return float(np.interp(i, np.arange(n), x)), float(s1), 0.0, 0.0, 0.0, float(s1)
    c = s1
    b = (s2 - s0) / 2
    a = (s2 + s0) / 2 - c
    with np.errstate(divide="ignore", invalid="ignore"):
        lpos = - b / 2 / a
        fpos = float(i) + lpos
        fval = a * lpos * lpos + b * lpos + c
    return float(np.interp(fpos, np.arange(n), x)), float(fval), float(lpos), float(a), float(b), float(c)


def peaks_ref(y, x=None):
    idx = scan(np.asarray(y, dtype=np.float64))
    r = [refine(y, int(i), x, True) for i in idx]
    return idx, np.array([t[0] for t in r], dtype=np.float64), np.array([t[1] for t in r], dtype=np.float64)


def peak_margin(y, idx):
    y = np.asarray(y)
    idx = np.asarray(idx, dtype=np.int64)
    return np.minimum(y[idx] - y[idx - 1], y[idx] - y[idx + 1])


def pad_lists(rows, maxpk):
    """npk [n], idx [n][maxpk] (-1), pos, val [n][maxpk] (NaN) of a list of peaks_ref results."""
    n = len(rows)
    npk = np.array([len(r[0]) for r in rows], dtype=np.int32).reshape(n)
    idx = -np.ones((n, maxpk), dtype=np.int32)
    pos, val = np.nan * np.ones((n, maxpk)), np.nan * np.ones((n, maxpk))
    for f, (i, p, v) in enumerate(rows):
        idx[f, :len(i)], pos[f, :len(i)], val[f, :len(i)] = i, p, v
    return npk, idx, pos, val
