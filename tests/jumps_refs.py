"""Restatements of the three jump stages (pvx_jump_select, pvx_winstat, pvx_jump_pick; JUMPS.md) with the closed forms the
kernels use -- the centred least-squares line, two-pass means and sums of squares, the pooled-variance t --, in three
arithmetics:

  PLAIN  float64, every sum np.sum (numpy's pairwise order)
  BFLY   float64, every sum in k_jumps.hip's order: lane l adds the points l, l + 64, .. in ascending order from 0.0, then the
         butterfly s += s[lane ^ d] for d = 32, 16, .., 1
  LD     np.longdouble throughout

The magnitudes of the selection are np.sum's order in PLAIN and BFLY alike (the kernel follows numpy there).  Order
statistics (kind ZMEDIAN) are numpy's own np.median / np.percentile.  Nothing here is shared with pypevoc_amd."""
import numpy as np

LD = np.longdouble
ZMEAN, ZMEDIAN, LINREG, LINREG2 = 0, 1, 2, 3
USE_L, USE_R = 1, 2
SHORT_SIDE, NAN_BIT = 1, 2

_LANE = np.arange(64)


class Arith(object):
    def __init__(self, name, dtype, total):
        self.name, self.dtype, self.sum = name, dtype, total

    def arr(self, v):
        return np.asarray(v, dtype=self.dtype)


def _sum_np(v):
    return np.sum(v) if len(v) else v.dtype.type(0)


def _sum_bfly(v):
    n = len(v)
    pad = np.zeros(-(-max(n, 1) // 64) * 64)
    pad[:n] = v
    s = np.zeros(64)
    for row in pad.reshape(-1, 64):                                   # (+ 0.0 for a lane without a point there: exact)
        s = s + row
    for d in (32, 16, 8, 4, 2, 1):
        s = s + s[_LANE ^ d]
    return s[0]


PLAIN = Arith("plain", np.float64, _sum_np)
BFLY = Arith("bfly", np.float64, _sum_bfly)
LONG = Arith("ld", LD, _sum_np)


# ---- selection --------------------------------------------------------------------------------------------------------------
def select(mag, f0, t, thr, ar=PLAIN):
    """(m, isel, tsel, fsel) of one row: mag [n][K]."""
    mag = ar.arr(mag)
    if mag.shape[0] == 0:
        return np.zeros(0, dtype=ar.dtype), np.zeros(0, dtype=bool), np.zeros(0), np.zeros(0)
    m = np.sqrt(np.sum(mag**2, axis=1))
    with np.errstate(invalid="ignore"):
        isel = m > np.max(m) * ar.dtype(thr)
    return m, isel, np.asarray(t)[isel], np.asarray(f0)[isel]


# ---- windowed statistics ----------------------------------------------------------------------------------------------------
def fit_line(t, x, ar):
    n = len(t)
    tm, xm = ar.sum(t) / n, ar.sum(x) / n
    b = ar.sum((t - tm) * (x - xm)) / ar.sum((t - tm) * (t - tm))
    return xm - b * tm, b


def resid(line, t, x):
    a, b = line
    return x - (b * t + a)


def mean_ss(r, ar):
    m = ar.sum(r) / len(r)
    d = r - m
    return m, ar.sum(d * d)


def pooled_t(line, t1, x1, t2, x2, ar):
    n1, n2 = len(t1), len(t2)
    m1, s1 = mean_ss(resid(line, t1, x1), ar)
    m2, s2 = mean_ss(resid(line, t2, x2), ar)
    v1, v2 = s1 / (n1 - 1), s2 / (n2 - 1)
    df = n1 + n2 - 2
    sp = ((n1 - 1) * v1 + (n2 - 1) * v2) / df
    one = ar.dtype(1.0)
    return (m1 - m2) / np.sqrt(sp * (one / n1 + one / n2))


def winstat(t, x, kind, wl, wr, hop=1, flags=USE_L | USE_R, ar=PLAIN):
    """out [n] of one row."""
    t, x = ar.arr(t), ar.arr(x)
    n = len(x)
    out = np.zeros(n, dtype=ar.dtype)
    with np.errstate(all="ignore"):
        for i in range(wl, n - max(wr, 0), hop):
            tw, xw = t[i - wl:i + wr], x[i - wl:i + wr]
            W = wl + wr
            if kind == ZMEAN:
                m, ss = mean_ss(xw, ar)
                out[i] = (x[i] - m) / np.sqrt(ss / W)
            elif kind == ZMEDIAN:
                if np.any(np.isnan(xw)):
                    out[i] = np.nan
                else:
                    out[i] = (x[i] - np.median(xw)) / (np.percentile(xw, 75) - np.percentile(xw, 25))
            elif kind == LINREG:
                line = fit_line(tw, xw, ar)
                _, ss = mean_ss(resid(line, tw, xw), ar)
                out[i] = resid(line, t[i], x[i]) / np.sqrt(ss / W)
            else:
                tl, xl, tr, xr = t[i - wl:i], x[i - wl:i], t[i:i + wr], x[i:i + wr]
                ts = []
                if flags & USE_L:
                    ts.append(pooled_t(fit_line(tl, xl, ar), tl, xl, tr, xr, ar))
                if flags & USE_R:
                    ts.append(-pooled_t(fit_line(tr, xr, ar), tr, xr, tl, xl, ar))
                out[i] = (ts[0] + ts[1]) / 2 if len(ts) == 2 else (ts[0] if ts else np.nan)
    return out


def window_spreads(t, x, kind, wl, wr, hop=1):
    """Per computed index the smallest spread a denominator of that kind rests on, relative to max|x| of the window: the
    builders require 1e-6 (JUMPS.md: degenerate windows)."""
    t, x = np.asarray(t, dtype=np.float64), np.asarray(x, dtype=np.float64)
    out = []
    for i in range(wl, len(x) - max(wr, 0), hop):
        tw, xw = t[i - wl:i + wr], x[i - wl:i + wr]
        scale = np.abs(xw).max()
        if kind == ZMEAN:
            s = [np.std(xw)]
        elif kind == ZMEDIAN:
            s = [np.percentile(xw, 75) - np.percentile(xw, 25)]
        elif kind == LINREG:
            s = [np.std(resid(fit_line(tw, xw, PLAIN), tw, xw))]
        else:
            tl, xl, tr, xr = t[i - wl:i], x[i - wl:i], t[i:i + wr], x[i:i + wr]
            s = [np.std(resid(fit_line(tl, xl, PLAIN), tl, xl)), np.std(resid(fit_line(tr, xr, PLAIN), tr, xr))]
        out.append(min(s) / scale)
    return np.array(out)


# ---- pick and fits ----------------------------------------------------------------------------------------------------------
def pick(zs, thr):
    """(idx, dir): the strict interior extrema beyond +-thr, ascending."""
    zs = np.asarray(zs, dtype=np.float64)
    idx, dirs = [], []
    with np.errstate(invalid="ignore"):
        for i in range(1, len(zs) - 1):
            if zs[i] > zs[i - 1] and zs[i] > zs[i + 1] and zs[i] > thr:
                idx.append(i), dirs.append(1)
            elif zs[i] < zs[i - 1] and zs[i] < zs[i + 1] and zs[i] < -thr:
                idx.append(i), dirs.append(-1)
    return np.array(idx, dtype=np.intp), np.array(dirs, dtype=np.int32)


def jump_fits(idx, t, x, nsl, ar=PLAIN):
    """(intcpts [nj][2], sumres [nj][2], status [nj])."""
    t, x = ar.arr(t), ar.arr(x)
    n = len(x)
    ic, sr = np.full((len(idx), 2), np.nan, dtype=ar.dtype), np.full((len(idx), 2), np.nan, dtype=ar.dtype)
    st = np.zeros(len(idx), dtype=np.int32)
    with np.errstate(all="ignore"):
        for j, i in enumerate(idx):
            il, ir = max(0, i - nsl), min(i + nsl, n)
            for side, (a, b, div) in enumerate(((il, i, i - il), (i + 1, ir, ir - i))):
                if b - a < 2:
                    st[j] |= SHORT_SIDE
                    continue
                ts, xs = t[a:b], x[a:b]
                line = fit_line(ts, xs, ar)
                r = resid(line, ts, xs)
                ic[j, side] = line[1] * t[i] + line[0]
                sr[j, side] = np.sqrt(ar.sum(r * r) / div)
                if np.isnan(ic[j, side]) or np.isnan(sr[j, side]):
                    st[j] |= NAN_BIT
    return ic, sr, st


def detect(mag, t, f0, pitch_t_hop=0.02, regressor_t=0.5, t_threshold=10, mag_threshold=0.01, slope_t=None, ar=PLAIN):
    """All three stages on one track whose magnitudes are `mag` [n] (JumpDetector.detect_jumps + calc_jump_params): a dict."""
    wle = int(regressor_t / pitch_t_hop)
    nsl = int((regressor_t if slope_t is None else slope_t) / pitch_t_hop)
    m, isel, tsel, fsel = select(np.asarray(mag)[:, None], f0, t, mag_threshold, ar)
    le = winstat(tsel, fsel, LINREG2, wle, wle, 1, USE_L | USE_R, ar)
    idx, dirs = pick(le, t_threshold)
    ic, sr, st = jump_fits(idx, tsel, fsel, nsl, ar)
    return {"isel": isel, "tsel": tsel, "fsel": fsel, "le": le, "up_idx": idx[dirs > 0], "dn_idx": idx[dirs < 0], "idx": idx,
            "intcpts": ic, "sumres": sr, "jump_status": st}


def rel_distance(a, ld):
    """max |a - ld| / |ld| over the elements where ld is finite and not 0 (0.0 without one)."""
    a, ld = np.asarray(a, dtype=LD), np.asarray(ld, dtype=LD)
    ok = np.isfinite(ld) & (ld != 0)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(a[ok] - ld[ok]) / np.abs(ld[ok])))
