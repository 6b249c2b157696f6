"""Plain numpy restatement of SpeechSegmenter's three stages on given band-energy tables (pypevoc/speech/SpeechSegmenter.py:
process :203-222 with the parabolic fit :224-260, refine_segment_all_bands :262-302, refine_transition_points :39-124), and
np.longdouble evaluations of the dB-derived quantities for the stage tests' tolerances.  No GPU, no reference import: the
expressions are the reference's own, in its order, on float64 (or long double) arrays."""
import warnings

import numpy as np

OK, OUTSIDE, EMPTY_SIDE, NO_CROSSING = 0, 1, 2, 3


def _db(spec, dtype=np.float64):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10 * np.log10(np.asarray(spec, dtype=dtype))


def detect(spec, thresh, dtype=np.float64):
    """(det [nfr-1], kept peak indices, their parabolic fpos) of an energy table [nfr][nband]."""
    dbspec = _db(spec, dtype)
    with np.errstate(invalid="ignore"):
        det = np.sum(np.abs(np.diff(dbspec, axis=0)), axis=1)
        pk = np.flatnonzero(np.logical_and(det[:-2] < det[1:-1], det[2:] < det[1:-1])) + 1
        pk = pk[det[pk] > thresh]
    fpos = np.empty(len(pk), dtype=dtype)
    for j, p in enumerate(pk):
        s0, s1, s2 = det[p - 1], det[p], det[p + 1]
        c = s1
        b = (s2 - s0) / 2
        a = (s2 + s0) / 2 - c
        fpos[j] = dtype(p) + (- b / 2 / a)
    return det, pk, fpos


def side_ranges(tfine, tsegs, intbef):
    """[nseg][6]: ibef, iaft, iall of :276-278 as [first, last + 1), from the masks themselves."""
    out = np.zeros((len(tsegs), 6), dtype=np.int32)
    for s, tseg in enumerate(tsegs):
        masks = (np.logical_and(tfine > tseg - intbef, tfine < tseg), np.logical_and(tfine > tseg, tfine < tseg + intbef),
                 np.logical_and(tfine > tseg - intbef, tfine < tseg + intbef))
        lo = int(np.searchsorted(tfine, tseg - intbef, side="right")) if np.isfinite(tseg) else len(tfine)
        for j, m in enumerate(masks):
            i = np.flatnonzero(m)
            if len(i):
                assert np.array_equal(i, np.arange(i[0], i[-1] + 1))
                out[s, 2 * j:2 * j + 2] = (i[0], i[-1] + 1)
            else:
                out[s, 2 * j:2 * j + 2] = (lo, lo)
        # an empty side sits where it would begin, inside iall
        if out[s, 1] == out[s, 0]:
            out[s, 0:2] = out[s, 4]
        if out[s, 3] == out[s, 2]:
            out[s, 2:4] = out[s, 5]
    return out


def refine(spec, ranges, tsegs, hop, half, tsr, sr, thr, dtype=np.float64):
    """valb, vala [nseg][nband], cross (int, -1 for none), bandpk, weight, out [nseg] of :283-302 on an energy table."""
    db = _db(spec, dtype)
    nseg, nband = len(tsegs), db.shape[1] if db.ndim == 2 else 0
    valb, vala = np.empty((nseg, nband), dtype=dtype), np.empty((nseg, nband), dtype=dtype)
    cross = np.empty((nseg, nband), dtype=np.int32)
    bandpk, weight = np.empty((nseg, nband), dtype=dtype), np.empty((nseg, nband), dtype=dtype)
    out = np.empty(nseg, dtype=dtype)
    tfine = (np.arange(len(db), dtype=np.int64) * int(hop) + half) / float(tsr)
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore")
        for s in range(nseg):
            b0, b1, a0, a1, l0, l1 = (int(v) for v in ranges[s])
            for b in range(nband):
                vb = np.median(db[b0:b1, b])
                va = np.median(db[a0:a1, b])
                valm = (vb + va) / 2. if not thr else np.min((va, vb)) + thr
                f = db[l0:l1, b]
                rr = np.flatnonzero((f[:-1] - valm) * (f[1:] - valm) < 0)
                if len(rr) > 0:
                    ir = np.argmin(np.abs(rr - (b1 - b0)))
                    cross[s, b] = rr[ir]
                    pk = tfine[rr[ir] + b0] * sr
                else:
                    cross[s, b] = -1
                    pk = tsegs[s]
                valb[s, b], vala[s, b], bandpk[s, b], weight[s, b] = vb, va, pk, np.abs(vb - va)
            out[s] = np.sum(bandpk[s] * weight[s]) / np.sum(weight[s])
    return valb, vala, cross, bandpk, weight, out


def transitions_row(x, tx, trt, mode="minmax", thr=0.5, dtype=np.float64):
    """(ttr, vbef, vaft, status) of refine_transition_points on one series whose tx already ascends."""
    x, tx = np.asarray(x, dtype=dtype), np.asarray(tx, dtype=np.float64)
    if trt > max(tx) or trt < min(tx):
        return trt, 0.0, 0.0, OUTSIDE
    before, after = x[tx < trt], x[tx > trt]
    percent = float(mode[3:]) if mode[:3] == "pct" else None
    if len(after) == 0 or (len(before) == 0 and (mode == "minmax" or percent is not None)):
        return np.nan, np.nan, np.nan, EMPTY_SIDE
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore")
        if mode == "median":
            vbef, vaft = np.median(before), np.median(after)
        elif mode == "mean":
            vbef, vaft = np.mean(before), np.mean(after)
        elif mode == "minmax" or percent is not None:
            falls = np.median(before) > np.median(after)               # the medians say which way the series goes
            if percent is None:
                vbef, vaft = (np.max(before), np.min(after)) if falls else (np.min(before), np.max(after))
            else:
                qb, qa = (100 - percent, percent) if falls else (percent, 100 - percent)
                vbef, vaft = np.percentile(before, qb), np.percentile(after, qa)
        else:
            raise ValueError(mode)
        lo, hi = x[:-1], x[1:]
        if vaft > vbef:
            level = vbef * thr + vaft * (1 - thr)
            hits = np.flatnonzero((lo < level) & (hi > level))
        else:
            level = vaft * thr + vbef * (1 - thr)
            hits = np.flatnonzero((lo > level) & (hi < level))
    if len(hits) == 0:
        return np.nan, vbef, vaft, NO_CROSSING
    k = hits[np.argmin(np.abs((tx[hits] + tx[hits + 1]) / 2. - trt))]
    ttr = tx[k] + (tx[k + 1] - tx[k]) * (level - x[k]) / (x[k + 1] - x[k])
    return ttr, vbef, vaft, OK


def transitions(x, tx, trt, mode="minmax", thr=0.5, dtype=np.float64):
    """Rows of transitions_row: ttr, vbef, vaft [rows] and status [rows]; tx [n] or [rows][n], trt a scalar or [rows]."""
    x = np.asarray(x)
    rows = x.shape[0]
    tx = np.asarray(tx, dtype=np.float64)
    trt = np.broadcast_to(np.asarray(trt, dtype=np.float64), (rows,))
    res = [transitions_row(x[r], tx if tx.ndim == 1 else tx[r], trt[r], mode, thr, dtype) for r in range(rows)]
    return (np.array([r[0] for r in res], dtype=dtype), np.array([r[1] for r in res], dtype=dtype),
            np.array([r[2] for r in res], dtype=dtype), np.array([r[3] for r in res], dtype=np.int32))


# ---- the U* fixtures (tests/golden/make_golden_segment.py) -----------------------------------------------------------
def golden_cases():
    """[(file name, the file's arrays, case dict, the case's signal)] of every U*.npz case."""
    import glob
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = []
    for path in sorted(glob.glob(os.path.join(here, "U*.npz"))):
        g = dict(np.load(path))
        if "x_from" in g:
            g["x"] = np.load(os.path.join(here, str(g["x_from"]) + ".npz"))["x"][:int(g["x_len"])]
        for c in json.loads(str(g["cases"])):
            x = g[c["x"]]
            out.append((os.path.basename(path)[:-4], g, c, x if not c.get("slice") else x[c["slice"][0]:c["slice"][1]]))
    return out


def same(a, b):
    """Equal element for element, NaN at the same places."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
