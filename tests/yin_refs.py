"""Reference for k_yin.hip (pvx_yin, include/pvx.h): the statements of YIN.md evaluated literally, one frame at a time.

yin_frame_ref sums every d[tau] on its own in np.longdouble where that is an extended type (x86: 64-bit mantissa) and with
math.fsum otherwise (as period_refs.py does), takes S as a long-double cumulative sum rounded to float64 once, and returns
with the results
  * the margin of every discrete decision of the frame -- how far the two compared values are apart -- so that a test can
    require the reference ALONE to be far from every flip before it asks the kernel for the identical pick, and
  * a rounding bound for tau, freq and conf, derived (YIN.md, "Bounds") from the kernel's summation order: a relative
    perturbation of (L + 64) 2^-53 on every d and S, propagated through d' = d tau / S and the parabola of step 5.
Comparisons between two literal 1.0 of the S == 0 rule are ties by construction: they are tagged, not measured, and the
kernel has to order them as the statements do (`<` is false, the first arg-min wins).

yin_frame_plain is the same text in plain float64 numpy, with the deliberately wrong variants the bounds must tell apart.
CASES lists every frame the GPU tests compare; test_yin_refs_cpu.py checks the margins over exactly those."""
import collections
import functools
import math

import numpy as np

EXTENDED = bool(np.finfo(np.longdouble).eps < 1e-18)                 # checked at import; math.fsum otherwise
U = 2.0 ** -53
MARGIN_FLOOR = 1e-6
FALLBACK, SILENT = 1, 2

Margin = collections.namedtuple("Margin", "kind tau value tagged")
FrameRef = collections.namedtuple("FrameRef", "pick tau freq conf flag dprime margins b_tau b_freq b_conf")


def _diff_sums(xs, L, nlag, count=None):
    """d[0 .. nlag): d[t] = sum_{j < count(t)} (xs[j] - xs[j + t])^2, each summed on its own; long double (or float64 from fsum)."""
    d = np.zeros(nlag, dtype=np.longdouble if EXTENDED else np.float64)
    w = xs.astype(np.longdouble) if EXTENDED else xs
    for t in range(1, nlag):
        m = L if count is None else count(t)
        e = w[:m] - w[t:t + m]
        d[t] = (e * e).sum(dtype=np.longdouble) if EXTENDED else math.fsum(e * e)
    return d


def yin_bounds(L, s0, s1, s2, tau_f, sr):
    """Rounding bounds (b_tau, b_freq, b_conf) of step 5 for d' values s0, s1, s2 (YIN.md, "Bounds")."""
    eps = (L + 64) * U                                               # relative, on every d and every S
    epsd = (2.0 * eps + 4.0 * U) * (1.0 + 1e-6)                      # on d' = d tau / S: two roundings more on either side
    e0, e1, e2 = abs(s0) * epsd, abs(s1) * epsd, abs(s2) * epsd
    b_conf = e1 + 2.0 * U
    num, den = s0 - s2, s0 - 2.0 * s1 + s2
    e_num = e0 + e2 + U * abs(num)
    e_den = e0 + 2.0 * e1 + e2 + 2.0 * U * (abs(s0) + 2.0 * abs(s1) + abs(s2))
    if not abs(den) > e_den:
        return math.inf, math.inf, b_conf
    r = num / den
    b_r = (e_num + abs(r) * e_den) / (abs(den) - e_den) + 2.0 * U * abs(r)
    b_tau = 0.5 * b_r + 2.0 * U * abs(tau_f)
    if not abs(tau_f) > b_tau:
        return b_tau, math.inf, b_conf
    b_freq = sr * b_tau / (abs(tau_f) * (abs(tau_f) - b_tau)) + 2.0 * U * abs(sr / tau_f)
    return b_tau, b_freq, b_conf


def _decide(dp, rule_one, tol, lo, hi, first_dip=True):
    """Steps 3 and 4 on d' (float64): (pick, flag, margins).  rule_one[t]: d'[t] is the literal 1.0 of the S == 0 rule."""
    margins = []
    pick, flag = None, 0
    if first_dip:
        for t in range(lo, hi + 1):
            margins.append(Margin("tol", t, abs(float(dp[t]) - tol), False))
            margins.append(Margin("rise", t, abs(float(dp[t + 1]) - float(dp[t])), bool(rule_one[t] and rule_one[t + 1])))
            if dp[t] < tol and dp[t] < dp[t + 1]:
                pick = t
                break
    if pick is None:
        flag |= FALLBACK
        seg = dp[lo:hi + 1]
        pick = lo + int(np.argmin(seg))                              # the first arg-min
        if len(seg) > 1:
            order = np.argsort(seg, kind="stable")
            a, b = lo + int(order[0]), lo + int(order[1])
            margins.append(Margin("argmin", pick, float(dp[b]) - float(dp[a]), bool(rule_one[a] and rule_one[b])))
    return pick, flag, margins


def yin_frame_ref(xs, tol, lo, hi, sr):
    """The frame xs (float64, nwind samples) by the statements of YIN.md: a FrameRef."""
    xs = np.asarray(xs, dtype=np.float64)
    L = len(xs) // 2
    assert len(xs) >= 8 and 2 <= lo <= hi <= L - 2
    d = _diff_sums(xs, L, hi + 2)
    S = np.cumsum(d).astype(np.float64)                              # long double sums, rounded once
    rule_one = S == 0.0
    rule_one[0] = False
    dp = np.ones(hi + 2)
    nz = ~rule_one
    nz[0] = False
    t = np.arange(hi + 2)
    dp[nz] = (d[nz] * t[nz] / S[nz]).astype(np.float64)
    margins = [Margin("S", int(k), float(S[k]), False) for k in range(1, hi + 2) if S[k] != 0.0]
    if S[hi + 1] == 0.0:                                             # step 6
        return FrameRef(0, 0.0, 0.0, 0.0, SILENT, dp, margins, 0.0, 0.0, 0.0)
    pick, flag, m2 = _decide(dp, rule_one, tol, lo, hi)
    s0, s1, s2 = float(dp[pick - 1]), float(dp[pick]), float(dp[pick + 1])
    den = s0 - 2.0 * s1 + s2
    tau_f = pick + 0.5 * (s0 - s2) / den if den != 0.0 else float(pick)
    with np.errstate(divide="ignore"):
        freq = float(np.float64(sr) / np.float64(tau_f))
    b_tau, b_freq, b_conf = yin_bounds(L, s0, s1, s2, tau_f, sr)
    return FrameRef(pick, tau_f, freq, 1.0 - s1, flag, dp, margins + m2, b_tau, b_freq, b_conf)


VARIANTS = ("nocmnd", "Lplus1", "shrink", "argmin")


def yin_frame_plain(xs, tol, lo, hi, sr, variant=None):
    """(pick, tau, freq, conf, flag) in plain float64 numpy.  variant: None, or one of the wrong readings of the text --
    'nocmnd' no cumulative normalisation (d' = d), 'Lplus1' sums over nwind//2 + 1 samples, 'shrink' sums over nwind - tau
    samples, 'argmin' the arg-min without the first-dip rule."""
    xs = np.asarray(xs, dtype=np.float64)
    n = len(xs)
    L = n // 2
    cnt = {None: L, "nocmnd": L, "argmin": L, "Lplus1": L + 1}.get(variant)
    d = np.zeros(hi + 2)
    for t in range(1, hi + 2):
        m = min(n - t, cnt) if cnt is not None else n - t
        e = xs[:m] - xs[t:t + m]
        d[t] = np.sum(e * e)
    S = np.cumsum(d)
    dp = np.ones(hi + 2)
    nz = S != 0.0
    nz[0] = False
    t = np.arange(hi + 2)
    dp[nz] = d[nz] if variant == "nocmnd" else d[nz] * t[nz] / S[nz]
    if S[hi + 1] == 0.0:
        return 0, 0.0, 0.0, 0.0, SILENT
    pick, flag, _ = _decide(dp, np.zeros(hi + 2, dtype=bool), tol, lo, hi, first_dip=variant != "argmin")
    s0, s1, s2 = dp[pick - 1], dp[pick], dp[pick + 1]
    den = s0 - 2.0 * s1 + s2
    tau_f = pick + 0.5 * (s0 - s2) / den if den != 0.0 else float(pick)
    with np.errstate(divide="ignore"):
        freq = float(np.float64(sr) / np.float64(tau_f))
    return pick, float(tau_f), freq, float(1.0 - s1), flag


def frame_errors(ref, pick, tau, freq, conf, flag):
    """What of (pick, tau, freq, conf, flag) misses the reference frame: a list of strings, empty when all is inside."""
    bad = []
    if int(pick) != ref.pick:
        bad.append("pick %d != %d" % (pick, ref.pick))
    if int(flag) != ref.flag:
        bad.append("flag %d != %d" % (flag, ref.flag))
    for name, got, want, bound in (("tau", tau, ref.tau, ref.b_tau), ("freq", freq, ref.freq, ref.b_freq), ("conf", conf, ref.conf, ref.b_conf)):
        if bound == math.inf or (got == want):
            continue
        if not abs(got - want) <= bound:
            bad.append("%s %r != %r (bound %.3g)" % (name, got, want, bound))
    return bad


def worst_ratio(ref, tau, freq, conf):
    """max |error| / bound over tau, freq, conf (bounds of 0 or inf skipped) and the largest absolute tau error."""
    w = 0.0
    for got, want, bound in ((tau, ref.tau, ref.b_tau), (freq, ref.freq, ref.b_freq), (conf, ref.conf, ref.b_conf)):
        if 0.0 < bound < math.inf:
            w = max(w, abs(got - want) / bound)
    return w, abs(tau - ref.tau) if math.isfinite(ref.b_tau) else 0.0


# ---- the signals and cases of the GPU tests ---------------------------------------------------------------------------
def harmonic(sr, n, f0, seed, noise=0.05):
    """Six harmonics of a 3 Hz vibrato around f0, white noise at `noise` of the fundamental; float32-exact (the recipe of
    tests/test_periodicity_diff_gpu.py)."""
    t = np.arange(n) / float(sr)
    ph = 2 * np.pi * np.cumsum(f0 * (1.0 + 0.03 * np.sin(2 * np.pi * 3.0 * t))) / sr
    x = sum(0.5 / h * np.sin(h * ph) for h in range(1, 7)) + noise * 0.5 * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32).astype(np.float64)


SR = 16000


@functools.lru_cache(maxsize=None)
def signal(key):
    if key.startswith("harm"):                                       # harm<nwind>: 40 frames at hop 64
        nwind = int(key[4:])
        return harmonic(SR, nwind + 64 * 40, 220.0, 11)
    if key == "dc":                                                  # a DC offset of ten times the amplitude
        x = signal("harm256")
        return x + 10.0 * np.abs(x).max()
    if key == "b1024":
        return harmonic(SR, 1024 + 512 * 6, 220.0, 12)
    if key == "b8192":
        return harmonic(SR, 8192 + 1024 * 3, 220.0, 13)
    if key == "grid":                                                # 1100 frames of 64 samples at hop 1, period 20
        return harmonic(SR, 64 + 1100, 800.0, 14)
    if key == "szero":                                               # silence, signal, a constant, signal, silence
        h = harmonic(SR, 4096, 220.0, 15)
        x = np.zeros(2560)
        x[512:1024] = h[1000:1512]
        x[1024:1536] = 0.25
        x[1536:2048] = h[2000:2512]
        return x
    if key.startswith("noise"):                                      # noise<nwind>: 6 frames at hop nwind/2
        nwind = int(key[5:])
        return 0.1 * np.random.default_rng(7).standard_normal(nwind + (nwind // 2) * 6)
    raise KeyError(key)


# sig: key of signal(); nwind, hop; kw: tolerance / fmin / fmax of f0yin
Case = collections.namedtuple("Case", "name sig nwind hop kw")
CASES = tuple(
    [Case("a%d" % n, "harm%d" % n, n, 64, ()) for n in (255, 256, 257)] +
    [Case("a%d_band" % n, "harm%d" % n, n, 64, (("fmin", 150.0), ("fmax", 400.0))) for n in (255, 256, 257)] + [
        Case("a_pick_lo", "harm256", 256, 64, (("fmax", 219.0),)),               # lo = 73: above the period of most frames
        Case("a_pick_hi", "harm256", 256, 64, (("fmin", 223.0),)),               # hi = 72: below the period of most frames
        Case("b1024", "b1024", 1024, 512, ()),
        Case("b8192", "b8192", 8192, 1024, ()),
        Case("c_grid", "grid", 64, 1, ()),
        Case("d_silence", "szero", 256, 64, ()),
        Case("e_noise256", "noise256", 256, 128, ()),
        Case("e_noise1024", "noise1024", 1024, 512, ()),
        Case("e_tol005", "harm256", 256, 64, (("tolerance", 0.05),)),
        Case("e_tol05", "harm256", 256, 64, (("tolerance", 0.5),)),
        Case("e_noise_tol05", "noise256", 256, 128, (("tolerance", 0.5),)),
        Case("g_dc", "dc", 256, 64, ()),
    ])
CASE = {c.name: c for c in CASES}


def case_params(case):
    """(starts, lo, hi, tol) of a case, by the text of YIN.md (not through the package)."""
    kw = dict(case.kw)
    L = case.nwind // 2
    lo, hi = 2, L - 2
    if "fmin" in kw:
        hi = min(int(math.ceil(SR / kw["fmin"])), L - 2)
    if "fmax" in kw:
        lo = max(2, int(math.floor(SR / kw["fmax"])))
    starts = np.arange(0, len(signal(case.sig)) - case.nwind, case.hop, dtype=np.int64)
    return starts, lo, hi, kw.get("tolerance", 0.15)


@functools.lru_cache(maxsize=None)
def case_refs(name):
    """The FrameRef of every frame of a case (computed once, shared by the tests)."""
    case = CASE[name]
    x = signal(case.sig)
    starts, lo, hi, tol = case_params(case)
    return tuple(yin_frame_ref(x[s:s + case.nwind], tol, lo, hi, SR) for s in starts)
