"""Reference for k_marks.hip (pvx_marks_corr / pvx_marks_peak, include/pvx.h): the statements of MARKS.md evaluated
literally, one step at a time.

corr_walk sums every lag it needs on its own in np.longdouble (math.fsum where that is no extended type) and returns with
the marks
  * the margin of every discrete decision -- the loop test, both int() truncations, each `<` / `>=` of the local-maximum
    tests at the chosen lag and at every lag nearer to 0, delay_t > min_per -- relative to the scale its operands' rounding
    errors have, so that a test can require the reference ALONE to be far from every flip before it asks the kernel for the
    same walk, and
  * a rounding bound per mark (MARKS.md, "Bounds"), derived from the kernel's summation order.
Decisions of the walk's first step are tagged: their operands are the inputs themselves (t0 sr, sr / f0 from the knots), the
same IEEE operations on both sides, and need no margin.  exact=False is the same text in plain float64 numpy (np.correlate,
as the reference calls it), with the deliberately wrong readings the bounds must tell apart.

peak_walk is the reference's loop with np.polyfit (exact=False) or a long-double least-squares parabola (exact=True); it
returns the index and the offset behind every mark and the margin of abs(rel) <= fit_points.

FIXTURES lists what tests/golden/make_golden_marks.py records; the signals live in the golden files."""
import collections
import functools
import json
import math
import os

import numpy as np

EXTENDED = bool(np.finfo(np.longdouble).eps < 1e-18)
U = 2.0 ** -53
MARGIN_FLOOR = 1e-6
NO_PEAK, PAST_END, BAD_F0, NO_ADVANCE, CAPACITY, STEPS, SHORT_FIT = 1, 2, 4, 8, 16, 32, 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# measured on the CPU (test_marks_refs_cpu.py re-measures and requires no more): the largest |rel(np.polyfit) - rel(long
# double)| in samples over the peak fixtures; the kernel is allowed 16 times that (MARKS.md, "Bounds")
PEAK_REL_MEASURED = 5e-14
PEAK_VAL_MEASURED = 2.5e-15                                            # the same for the fitted value, relative to max |x|
KERNEL_FACTOR = 16.0

Margin = collections.namedtuple("Margin", "kind step value tagged")
CorrRef = collections.namedtuple("CorrRef", "marks status margins bounds steps")
PeakRef = collections.namedtuple("PeakRef", "marks vals idx rel fitted status margins")


def rel_margin(a, b):
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else 0.0


def _trunc_margin(q):
    """How far q is from the integers around it, relative to q (int(q) flips at either)."""
    fl = math.floor(q)
    return min(q - fl, fl + 1 - q) / max(abs(q), 1.0)


def _lag_sum(src, tgt, k, exact):
    """xc[k] = sum_n src[n + k] tgt[n] over the n where both exist"""
    W = len(src)
    n0, n1 = max(0, -k), min(W, W - k)
    a, b = src[n0 + k:n1 + k], tgt[n0:n1]
    if not exact:
        return float(np.dot(a, b))
    if EXTENDED:
        return float(np.dot(a.astype(np.longdouble), b.astype(np.longdouble)))
    return math.fsum(a * b)


def corr_walk(x, sr=1.0, t0=0.0, tf=(), f=(), window_size=1024, min_per=0.001, exact=True, variant=None, max_marks=None,
              max_steps=None, toff=0.0):
    """The corr walk of MARKS.md.  variant: None, 'by_value' (the highest peak instead of the nearest), 'mark_after' (the
    mark computed after next_t moved).  Status cases end the walk with their bit, as the kernel does."""
    x = np.asarray(x, dtype=np.float64)
    tf, f = np.asarray(tf, dtype=np.float64), np.asarray(f, dtype=np.float64)
    L, W = len(x), int(window_size)
    slope = float(np.max(np.abs(np.diff(f) / np.diff(tf)))) if len(f) > 1 and np.isfinite(f).all() else 0.0
    marks, margins, bounds, steps = [t0], [], [0.0], []
    status = 0
    next_t = t0
    f0 = float(np.interp(toff + t0, tf, f))
    if math.isnan(f0):
        with np.errstate(all="ignore"):
            f0 = float(np.nanmean(f)) if np.isfinite(f).any() else math.nan

    def period(f0):
        if not f0 > 0:
            return -1
        q = sr / f0
        return int(q) if 1.0 <= q < 2.0 ** 31 else -1
    P = period(f0)
    if not t0 >= 0 or P < 0:
        return CorrRef(np.array(marks), BAD_F0, margins, np.array(bounds), steps)
    b_next = 0.0                                                     # bound on |next_t - its exact-arithmetic value|
    delay_t = None
    it = 0
    while True:
        first = next_t == t0 and it == 0
        lhs, rhs = next_t * sr, float(L - P - W)
        margins.append(Margin("loop", it, rel_margin(lhs, rhs), first))
        if not lhs < rhs:
            break
        if max_steps is not None and it == max_steps:
            status |= STEPS
            break
        if not math.isnan(f0):
            P = period(f0)
            if P < 0 or not lhs >= 0:
                status |= BAD_F0
                break
            margins.append(Margin("int_P", it, _trunc_margin(sr / f0), first or slope == 0.0))
            margins.append(Margin("int_s", it, _trunc_margin(lhs), first))
            s = int(lhs)
            if s + P + W > L:
                status |= PAST_END
                break
            src, tgt = x[s:s + W], x[s + P:s + P + W]
            scale = math.sqrt(float(np.dot(src, src)) * float(np.dot(tgt, tgt)))
            if exact:
                xc = {}

                def val(k):
                    if k not in xc:
                        xc[k] = _lag_sum(src, tgt, k, True)
                    return xc[k]
            else:
                full = np.correlate(src, tgt, "full")

                def val(k):
                    return float(full[k + W - 1])
            pick = None
            peaks = []
            for d in range(0, W - 1):                                # |k| <= W - 2: the interior of xc
                for k in ((-d, d) if d else (0,)):
                    a, b, c = val(k - 1), val(k), val(k + 1)
                    if scale > 0:
                        margins.append(Margin("rise", it, abs(b - a) / scale, False))
                        margins.append(Margin("fall", it, abs(b - c) / scale, False))
                    if a < b and b >= c:
                        peaks.append(k)
                        if pick is None:
                            pick = k
                if pick is not None and variant != "by_value":
                    break
            if pick is None:
                status |= NO_PEAK
                break
            if variant == "by_value":
                pick = max(peaks, key=lambda k: val(k))
            pos = pick + W - 1
            s0, s1, s2 = val(pick - 1), val(pick), val(pick + 1)
            c = s1                                                   # PeakFinder.py:353-359
            b = (s2 - s0) / 2
            a = (s2 + s0) / 2 - c
            with np.errstate(all="ignore"):
                lpos = float(-np.float64(b) / 2 / np.float64(a))
            fpos = float(np.interp(float(pos) + lpos, np.arange(2 * W - 1), np.arange(2 * W - 1)))
            delay_samp = fpos - (W - 1)
            delay_t = (-delay_samp + P) / sr
            # the bound: every lag within e of its exact value, through b, a and lpos = -b / (2 a)
            e = (W + 2) * U * scale
            db, da = e + 2 * U * abs(b), 2 * e + 4 * U * (abs(a) + abs(c))
            b_lpos = (db + 2 * abs(lpos) * da) / (2 * (abs(a) - da)) + 4 * U * abs(lpos) if abs(a) > da else math.inf
            b_delay = b_lpos / sr + 6 * U * abs(delay_t) + 2 * U * (W + P) / sr
            margins.append(Margin("min_per", it, rel_margin(delay_t, min_per), False))
            steps.append(dict(step=it, s=s, P=P, pick=pick, lpos=lpos, delay_t=delay_t, b_next=b_next, b_delay=b_delay))
            if delay_t > min_per:
                if max_marks is not None and len(marks) == max_marks:
                    status |= CAPACITY
                    break
                if variant == "mark_after":
                    marks.append(next_t + delay_t + (W + P / 2) / sr)
                else:
                    marks.append(next_t + (W + P / 2) / sr)
                bounds.append(b_next + 4 * U * abs(marks[-1]))
                next_t += delay_t
                b_next += b_delay + U * abs(next_t)
            else:
                db_f = slope * b_next + 6 * U * abs(f0)
                next_t += 1 / f0
                b_next += db_f / (f0 * (f0 - db_f)) + 2 * U / f0 + U * abs(next_t)
        else:
            if delay_t is None or not delay_t > 0:
                status |= NO_ADVANCE
                break
            next_t = next_t + delay_t
            b_next += U * abs(next_t)
        f0 = float(np.interp(toff + next_t, tf, f))
        it += 1
    return CorrRef(np.array(marks), status, margins, np.array(bounds), steps)


def _parabola_ld(y):
    """Least-squares p0 i^2 + p1 i + p2 over (i, y[i]) in long double: (p0, p1, p2)"""
    t = np.longdouble if EXTENDED else np.float64
    y = np.asarray(y, dtype=t)
    i = np.arange(len(y)).astype(t)
    A = np.stack([i * i, i, np.ones(len(y), dtype=t)], axis=1)
    N, r = A.T.dot(A), A.T.dot(y - y[0])
    c = [[N[1, 1] * N[2, 2] - N[1, 2] * N[2, 1], N[1, 0] * N[2, 2] - N[1, 2] * N[2, 0], N[1, 0] * N[2, 1] - N[1, 1] * N[2, 0]]]
    D = N[0, 0] * c[0][0] - N[0, 1] * c[0][1] + N[0, 2] * c[0][2]

    def det(col):
        M = N.copy()
        M[:, col] = r
        return (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])
                + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))
    return det(0) / D, det(1) / D, det(2) / D + y[0]


def peak_walk(x, sr=1.0, tf=None, f=(), fit_points=3, exact=False, toff=0.0, max_marks=None, max_steps=None):
    """The peak walk of MARKS.md (Periodicity.py:621-709); marks with fewer than 3 fit points take the sample."""
    x = np.asarray(x, dtype=np.float64)
    sr = float(sr)
    L = len(x)
    if tf is None:
        fs = np.asarray(f, dtype=np.float64) * np.ones(L) if np.ndim(f) == 0 else np.asarray(f, dtype=np.float64)
    else:
        fs = np.interp(toff + np.arange(L) / sr, tf, f)
    marks, vals, idxs, rels, fitted, margins, shorts = [], [], [], [], [], [], []
    status = 0

    def period(f0):
        if not f0 > 0:
            return -1
        q = sr / f0
        return int(q) if 1.0 <= q < 2.0 ** 31 else -1

    def done():
        n = max(len(marks) - 1, 0)
        st = status | (SHORT_FIT if any(shorts[:n]) else 0)
        return PeakRef(np.array(marks[:n]), np.array(vals[:n]), np.array(idxs[:n], dtype=np.int64), np.array(rels[:n]),
                       np.array(fitted[:n], dtype=bool), st, margins)
    fin = np.nonzero(np.isfinite(fs))[0]
    P = period(fs[fin[0]]) if len(fin) else -1
    if P < 0:
        status = BAD_F0
        return done()
    idx_0 = int(fin[0])
    idx_start = idx_0 + int(np.argmin(x[idx_0:idx_0 + P]))
    it = 0
    while idx_start < L:
        if max_steps is not None and it == max_steps:
            status |= STEPS
            break
        idx_end = min(idx_start + P, L)
        idx_max = int(np.argmax(x[idx_start:idx_end])) + idx_start
        m = min(fit_points, L - idx_max - 1)
        t_max, v_max, rel, ok = idx_max / sr, x[idx_max], 0.0, False
        if m >= 2:
            yy = x[idx_max:idx_max + m + 1]
            with np.errstate(all="ignore"):
                if exact:
                    p0, p1, p2 = _parabola_ld(yy)
                    r = -p1 / p0 / 2
                else:
                    import warnings
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        p0, p1, p2 = np.polyfit(np.arange(m + 1), yy, 2)
                    r = -p1 / p0 / 2
            if math.isfinite(float(r)):
                margins.append(Margin("fit", it, rel_margin(abs(float(r)), float(fit_points)), False))
            if abs(r) <= fit_points:
                ok, rel = True, float(r)
                t_max = float((idx_max + r) / sr)
                v_max = float((p0 * r + p1) * r + p2)
        f0 = fs[idx_max]
        if np.isfinite(f0):
            P = period(f0)
            if P < 0:
                status |= BAD_F0
                break
            if max_marks is not None and len(marks) == max_marks:
                status |= CAPACITY
                break
            marks.append(t_max); vals.append(v_max); idxs.append(idx_max); rels.append(rel); fitted.append(ok); shorts.append(m < 2)
        adv = int(np.argmin(x[idx_max:min(idx_max + P, L)]))
        idx_start = idx_max + adv if adv > 0 else idx_max + 1
        it += 1
    return done()


def peak_tolerance(sr, t, xmax):
    """(on a fitted mark's time, on its value): 16 times what the float64 restatement is measured to differ by from the long-
    double one, plus the roundings of (idx + rel) / sr"""
    return KERNEL_FACTOR * PEAK_REL_MEASURED / sr + 4 * U * abs(t), KERNEL_FACTOR * PEAK_VAL_MEASURED * xmax


# ---- the fixtures ---------------------------------------------------------------------------------------------------
def vowel(n, sr, f0, seed, jitter=0.0, nharm=5):
    """A float32-exact synthetic vowel: nharm harmonics of a (slowly moving) f0 under 1/h, a little seeded noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(sr)
    fi = f0 * (1.0 + jitter * np.sin(2 * np.pi * 3.0 * t))
    ph = 2 * np.pi * np.cumsum(fi) / sr
    x = sum(0.4 / h * np.sin(h * ph + 0.3 * h) for h in range(1, nharm + 1)) + 1e-3 * rng.standard_normal(n)
    return x.astype(np.float32)


def _c(name, sig, sr, W, tf, f, t0=0.0, min_per=0.001):
    return dict(name=name, sig=sig, sr=sr, W=W, tf=list(map(float, tf)), f=[float(v) for v in f], t0=t0, min_per=min_per)


# signal key -> (n, sr, f0, seed, jitter[, nharm])
SIGNALS = {
    "v8k": (2400, 8000, 151.3, 11, 0.02),
    "v8k_long": (4000, 8000, 151.3, 12, 0.02),
    "fast8k": (1200, 8000, 8000 / 20.37, 13, 0.0),
    "low16k": (4000, 16000, 16000 / 300.7, 14, 0.0),
    "sine16k": (7000, 16000, 16000 / 611.7, 17, 0.0, 1),           # one harmonic: the correlation peaks once per period
}
NAN = float("nan")
CORR_FIXTURES = [_c("w%d" % W, "v8k", 8000, W, [0.0, 0.3], [149.0, 153.0]) for W in (63, 64, 65, 255, 256, 257)] + [
    _c("w1024", "v8k_long", 8000, 1024, [0.0, 0.5], [149.0, 153.0]),
    _c("small_P", "fast8k", 8000, 256, [0.0, 0.15], [8000 / 20.6, 8000 / 20.5]),          # P = 20, much smaller than W
    _c("P_above_W", "low16k", 16000, 128, [0.0, 0.25], [16000 / 300.2, 16000 / 300.4]),   # P = 300 > W
    _c("off35", "v8k", 8000, 256, [0.0, 0.3], [151.3 * 1.35, 151.3 * 1.35 + 1.0]),        # the nearest peak lies ~0.35 P out
    # 35 % off at a period of 600 samples: P = 444 and the nearest peak at lag -156, beyond the first ring of 127 lags
    _c("ring2", "sine16k", 16000, 1024, [0.0, 0.5], [16000 / 611.7 * 1.35, 16000 / 611.7 * 1.35 + 0.1]),
    _c("nan_gap", "v8k_long", 8000, 256, [0.0, 0.1, 0.11, 0.2, 0.21, 0.5], [150.0, 151.0, NAN, NAN, 152.0, 151.0]),
    _c("t0", "v8k", 8000, 256, [0.0, 0.3], [149.0, 153.0], t0=0.0123),
    _c("min_per", "v8k", 8000, 256, [0.0, 0.3], [149.0, 153.0], min_per=0.00664),         # some delays fall below: 1 / f0 steps
]
CORR = {c["name"]: c for c in CORR_FIXTURES}


def _p(name, sig, sr, tf, f, fit_points=3):
    return dict(name=name, sig=sig, sr=sr, tf=tf, f=f, fit_points=fit_points)


PEAK_FIXTURES = [
    _p("track3", "v8k", 8000, [0.0, 0.3], [149.0, 153.0]),
    _p("track5", "v8k", 8000, [0.0, 0.3], [149.0, 153.0], 5),
    _p("scalar", "v8k", 8000, None, 151.0),
    _p("per_sample", "v8k", 8000, None, "ramp"),                     # f per sample: 149 .. 153 over the signal
    _p("nan_head", "v8k_long", 8000, [0.0, 0.05, 0.06, 0.5], [NAN, NAN, 150.0, 152.0]),
    _p("flat_top", "flat", 8000, None, 160.0),                       # a coarsely quantised wave: ties in arg-max and arg-min
    _p("last_sample", "rising", 8000, None, 151.0, 5),               # the last arg-max is the last sample
]
PEAK = {c["name"]: c for c in PEAK_FIXTURES}


def make_signal(key):
    """What the golden generator stores (float32)."""
    if key == "flat":
        x = vowel(2000, 8000, 160.0, 15).astype(np.float64)
        return (np.round(x * 32) / 32).astype(np.float32)          # coarse steps: equal neighbours at the tops
    if key == "rising":
        x = vowel(1501, 8000, 151.0, 16).astype(np.float64)
        x[-40:] += np.linspace(0.0, 2.0, 40)
        return x.astype(np.float32)
    n, sr, f0, seed, jit = SIGNALS[key][:5]
    return vowel(n, sr, f0, seed, jit, *SIGNALS[key][5:])


@functools.lru_cache(maxsize=None)
def golden(fname):
    with np.load(os.path.join(GOLDEN, fname + ".npz")) as z:
        return {k: z[k] for k in z.files}


def signal(key):
    """The stored float32 signal, widened."""
    g = golden("K1_marks_corr" if key in SIGNALS else "K2_marks_peak")
    return g["sig_" + key].astype(np.float64)


def peak_f(case, n):
    return np.linspace(149.0, 153.0, n) if isinstance(case["f"], str) else case["f"]


@functools.lru_cache(maxsize=None)
def corr_ref(name, exact=True, variant=None):
    c = CORR[name]
    return corr_walk(signal(c["sig"]), c["sr"], c["t0"], c["tf"], c["f"], c["W"], c["min_per"], exact=exact, variant=variant)


@functools.lru_cache(maxsize=None)
def peak_ref(name, exact=True):
    c = PEAK[name]
    x = signal(c["sig"])
    return peak_walk(x, c["sr"], c["tf"], peak_f(c, len(x)), c["fit_points"], exact=exact)


def cases_json(cases):
    return np.array(json.dumps(cases))


# ---- rows that end by a status, each in a call of its own with healthy rows beside it -----------------------------------
TRACK = ([0.0, 0.3], [149.0, 153.0])


def status_call(kind):
    """dict(x, starts, stops, t0, toff, tf, f, W, min_per, max_marks, max_steps, expect): the middle row ends with the status
    `kind` names, the rows beside it by their own loop test (expect: the status per row)."""
    v = signal("v8k_long")
    click = np.zeros(1200)                                           # one click: its correlation is 1 at lag P and 0 elsewhere
    click[100] = 1.0
    x = np.concatenate([v, np.zeros(2400), v[:2400], click])
    n = len(v)
    c = dict(x=x, starts=[0, 0, n + 2400], stops=[2400, 2400, n + 4800], t0=[0.0, 0.0, 0.0131], toff=[0.0, 0.0, 0.0], tf=TRACK[0],
             f=TRACK[1], W=256, min_per=0.001, max_marks=None, max_steps=None)
    if kind == "no_peak":                                            # (a) silence
        c.update(starts=[0, n, n + 2400], stops=[2400, n + 2400, n + 4800])
    elif kind == "past_end":                                         # (b) P grows from 53 to 133 at 0.27 s: one step lands behind
        c.update(tf=[0.0, 0.27, 0.2701, 1.0], f=[150.0, 150.0, 60.0, 60.0], stops=[2400, 2540, n + 4800])
    elif kind == "bad_t0":                                           # (c)
        c.update(t0=[0.0, -0.1, 0.0131])
    elif kind == "bad_f0":                                           # (c) the track turns negative under the middle row
        c.update(tf=[0.0, 0.3, 1.0, 2.0], f=[149.0, 153.0, -5.0, -5.0], toff=[0.0, 1.5, 0.0])
    elif kind == "no_advance":       # (d) the click against itself: the only peak is lag P, the delay exactly 0, the walk advances
        # by 1 / f0; there the track is NaN and there is nothing to advance by
        c.update(tf=[0.0, 1.0, 1.0001, 1.002, 1.0021, 2.0], f=[150.0, 150.0, 400.0, 400.0, NAN, NAN], toff=[0.0, 1.0001, 0.0],
                 starts=[0, n + 4800, n + 2400], stops=[2400, n + 6000, n + 4800])
    elif kind == "capacity":                                         # (e) the first row fills its capacity exactly
        c.update(max_marks=5, stops=[500, 2400, n + 4800], starts=[0, 0, n + 4300])
    elif kind == "steps":                                            # (f)
        c.update(max_steps=5, stops=[500, 2400, n + 4800], starts=[0, 0, n + 4300])
    else:
        raise KeyError(kind)
    bit = {"no_peak": NO_PEAK, "past_end": PAST_END, "bad_t0": BAD_F0, "bad_f0": BAD_F0, "no_advance": NO_ADVANCE,
           "capacity": CAPACITY, "steps": STEPS}[kind]
    c["expect"] = [0, bit, 0]
    return c


STATUS_KINDS = ("no_peak", "past_end", "bad_t0", "bad_f0", "no_advance", "capacity", "steps")


def rows_ref(c, rows=None):
    """The restatement of every row (or of `rows`) of a call dict"""
    out = {}
    for r in (range(len(c["starts"])) if rows is None else rows):
        out[r] = corr_walk(c["x"][c["starts"][r]:c["stops"][r]], c.get("sr", 8000), c["t0"][r], c["tf"], c["f"], c["W"], c["min_per"],
                           max_marks=c["max_marks"], max_steps=c["max_steps"], toff=c["toff"][r])
    return out


def lds_limit_call(past):
    """W = 2048 at 16 kHz under a track whose largest period is 1856 (3 W + P = 8000, the limit) or 1857 samples"""
    n = np.arange(9000)
    x = (np.sin(2 * np.pi * n / 1800.0) + 0.3 * np.sin(2 * np.pi * n / 450.0 + 1.0)).astype(np.float32).astype(np.float64)
    per = 1857.5 if past else 1856.5
    return dict(x=x, sr=16000, starts=[0], stops=[len(x)], t0=[0.0], toff=[0.0], tf=[0.0, 1.0], f=[16000 / per, 16000 / (per - 0.3)],
                W=2048, min_per=0.001, max_marks=None, max_steps=None)


def many_rows_call(nrows=1100):
    """More rows than the persistent grid has workgroups, of unequal length, over one signal"""
    x = signal("v8k_long")
    starts = [3 * i for i in range(nrows)]
    stops = [s + 450 + 20 * (i % 7) for i, s in enumerate(starts)]
    assert max(stops) <= len(x)
    return dict(x=x, starts=starts, stops=stops, t0=[0.0] * nrows, toff=[s / 8000.0 for s in starts], tf=[0.0, 0.5], f=[149.0, 153.0],
                W=64, min_per=0.001, max_marks=None, max_steps=None)
