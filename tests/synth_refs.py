"""Plain numpy references for the resynthesis (SinSum.synth / RegPartial.synth, PVAnalysis.py:1053-1070 and 684-756)
and the seeded edge cases that tests/test_synth_refs_cpu.py pins and tests/test_synth_diff_gpu.py holds k_synth.hip to.

Nothing here imports pypevoc_amd or the oracle: `synth` restates the reference statement by statement (np.interp by hand,
because np.interp itself narrows to float64), so that it can run on a 64-bit mantissa (dtype=np.longdouble, pi to 36
digits) and measure how far float64 round-off alone moves a case's waveform.  The sample counts (edgsam, edgsamp, the
length of np.arange(hop * (nfr + dfr))) are float64 in both: they decide the waveform's structure, not its values.
"""
import math
from types import SimpleNamespace

import numpy as np

SR = 44100.0
_PI_36 = "3.14159265358979323846264338327950288"


def has_longdouble():
    return np.finfo(np.longdouble).nmant >= 63


def _pi(T):
    return np.longdouble(_PI_36) if T is np.longdouble else T(np.pi)


def _interp(x, xp, fp):
    """np.interp(x, xp, fp) for increasing xp, in the arrays' own type (numpy's compiled_interp, branch by branch)."""
    n = len(xp)
    if n == 1:
        return np.full(x.shape, fp[0], dtype=fp.dtype)
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, n - 1)      # xp[j] <= x < xp[j+1]
    j1 = np.minimum(j + 1, n - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = (fp[j1] - fp[j]) / (xp[j1] - xp[j])
        y = slope * (x - xp[j]) + fp[j]
    y = np.where((j == n - 1) | (xp[j] == x), fp[j], y)
    y = np.where(x > xp[n - 1], fp[n - 1], y)
    y = np.where(x < xp[0], fp[0], y)
    return y


def _partial(pf, pm, pr, overlap, overlap64, fstep, sr, hop, edge, T, unit):
    """RegPartial.synth.  unit: every cosine of a phase replaced by 1 and msig by |msig| (the amplitude scale)."""
    nfr = len(pf)
    one, two, half = T(1), T(2), T(0.5)
    pi = _pi(T)
    pi2 = two * pi
    dfr64 = 1. / overlap64 / 2.                                          # :687, float64: it sizes arrays
    dfr = one / overlap / two
    nnew = int(math.ceil(hop * (nfr + dfr64)))                           # len(np.arange(hop*(nfr + dfr))), :689
    newt = np.arange(nnew).astype(T)
    jj = np.arange(nfr).astype(T)
    fsig = _interp(newt, T(hop) * (dfr + half + jj), pf)                 # :701
    msig = _interp(newt, T(hop) * (dfr + jj), pm)                        # :702
    if unit:
        msig = np.abs(msig)
    sig = np.zeros(hop * nfr, dtype=T)
    ph = np.zeros(1, dtype=T)
    phcornext = T(0)
    for ii in range(nfr):                                                # :703
        fsam = fsig[hop * ii:(hop * (ii + 1) - 1)]
        ph = pi2 * np.cumsum(fsam / sr)                                  # :707
        ph = np.insert(ph, 0, T(0))
        phcor = pi * (fsig[hop * (ii + 1)] - fsig[hop * ii]) / fstep / two           # :715
        if ii < nfr - 1:
            phcornext = pi * (fsig[hop * (ii + 2)] - fsig[hop * (ii + 1)]) / fstep / two
        ph0 = pr[ii] + phcor                                             # :721
        ph = ph + ph0
        if ii < nfr - 1:                                                 # :724-729
            phend = ph[-1] + pi2 * fsig[hop * (ii + 1)] / sr
            dph = np.mod(pr[ii + 1] + phcornext - phend + pi, pi2) - pi
            ph = ph + np.arange(hop).astype(T) * (dph / T(hop))          # np.linspace(0.0, dph, num=hop+1)[:-1]
        c = np.ones(hop, dtype=T) if unit else np.cos(ph)
        sig[hop * ii:hop * (ii + 1)] = msig[hop * ii:hop * (ii + 1)] * c            # :734-736
    edgsam = int(dfr64 * hop * edge)                                     # :740
    k = np.arange(edgsam).astype(T)
    es = T(edgsam) if edgsam else one
    mag = msig[0] * (one - np.cos(pi * k / es)) / two                    # :742
    phb = np.flipud(pr[0] - pi2 * np.cumsum(pf[0] * np.ones(edgsam, dtype=T) / sr))
    sig = np.insert(sig, 0, mag * (np.ones(edgsam, dtype=T) if unit else np.cos(phb)))
    mag = msig[hop * nfr] * (one + np.cos(pi * k / es)) / two            # :748 (ii + 1 == nfr after the loop)
    phb = ph[-1] + pi2 * np.cumsum(pf[-1] * np.ones(edgsam, dtype=T) / sr)
    sig = np.append(sig, mag * (np.ones(edgsam, dtype=T) if unit else np.cos(phb)))
    return sig, edgsam


def _sinsum(f, mag, realph, pid, st, ln, sr, nfft, hop_a, hop_s, edge, minframes, T, unit):
    f = np.asarray(f, dtype=np.float64).astype(T)
    mag = np.asarray(mag, dtype=np.float64).astype(T)
    realph = np.asarray(realph, dtype=np.float64).astype(T)
    pid = np.asarray(pid)
    hop = int(hop_s)
    overlap = T(hop_a) / T(nfft)                                         # :824
    fstep = T(sr) / T(nfft)                                              # :825
    overlap64 = hop_a / float(nfft)
    dfr_s = float(nfft) / float(hop_a) / 2.                              # :1055
    edgsamp = int(float(edge) * hop * dfr_s)                             # :1056 (an integer, as under Python 2)
    end = np.asarray(st, dtype=np.int64) + np.asarray(ln, dtype=np.int64) - 1
    w = np.zeros((int(end.max()) + 2) * hop + 2 * edgsamp, dtype=T)      # :1059
    for p in range(len(st)):
        nfr = int(ln[p])
        if nfr < minframes or nfr < 1:                                   # :1061
            continue
        rows = int(st[p]) + np.arange(nfr)
        hit = pid[rows] == p
        assert np.all(hit.sum(axis=1) == 1), "partial %d is not one slot per frame" % p
        slot = hit.argmax(axis=1)
        wi, edgsam = _partial(f[rows, slot], mag[rows, slot], realph[rows, slot], overlap, overlap64,
                              fstep, T(sr), hop, float(edge), T, unit)
        spl_st = int(int(st[p]) * hop - edgsam) + edgsamp                # :756, :1066
        if spl_st >= 0:                                                  # :1067 (a negative start: the partial is dropped)
            if spl_st + len(wi) > len(w):
                raise ValueError("partial %d does not fit the waveform (numpy would raise)" % p)
            w[spl_st:spl_st + len(wi)] += wi
    return w[edgsamp:]


def synth(f, mag, realph, pid, st, ln, sr, nfft, hop_a, hop_s, edge, minframes, dtype=np.float64):
    """SinSum.synth(sr, hop_s, edge, minframes) of the table (f, mag, realph, pid: [F, K]; st, ln: [P]) in `dtype`."""
    return _sinsum(f, mag, realph, pid, st, ln, sr, nfft, hop_a, hop_s, edge, minframes, dtype, False)


def envelope(f, mag, realph, pid, st, ln, sr, nfft, hop_a, hop_s, edge, minframes):
    """S[n]: the sum over sounding partials of |msig| times the edge ramp, every cosine of a phase replaced by 1 (float64)."""
    return _sinsum(f, mag, realph, pid, st, ln, sr, nfft, hop_a, hop_s, edge, minframes, np.float64, True)


def args(c):
    """A case as the positional arguments of synth / envelope / pvoracle.synth / _device_synth."""
    return (c.f, c.mag, c.realph, c.pid, c.st, c.ln, c.sr, c.nfft, c.hop_a, c.hop_s, c.edge, c.minframes)


def bound(c, ref):
    """The float64 loop's bound: 1e-10 max(1, Phi / 1e4) max(1, max|ref|), Phi = max|realph| + pi hop_s (the largest
    phase argument: 1e-10 is what the kernel is held to on fixtures whose phases reach 1e4 rad)."""
    phi = float(np.abs(c.realph).max()) + np.pi * c.hop_s
    return 1e-10 * max(1.0, phi / 1e4) * max(1.0, float(np.abs(ref).max()) if len(ref) else 0.0)


# ---- which path of pvx_launch_synth (k_synth.hip) a case takes, from the host code's own formulas ------------------------
def plan(c, run=0):
    h, K = int(c.hop_s), c.f.shape[1]
    overlap = c.hop_a / float(c.nfft)
    dfr = 1. / overlap / 2.
    offf = dfr + .5
    edgsam = int(dfr * h * c.edge)
    edgsamp = int(c.edge * h * (float(c.nfft) / float(c.hop_a) / 2.))
    EF = (edgsam + h - 1) // h if edgsam > 0 else 0
    maxend = int((c.st.astype(np.int64) + c.ln - 1).max())
    wlen = (maxend + 2) * h + edgsamp
    nseg = (wlen + h - 1) // h
    R = 32 if nseg * ((h + 31) // 32) >= 256 * 64 else (16 if nseg * ((h + 15) // 16) >= 256 * 64 else 8)
    if run in (8, 16, 32):
        R = run

    def brk(off):
        fr = off - math.floor(off)
        return h if fr == 0.0 else int(math.ceil(h * fr))

    def dyadic(off):
        t = math.ldexp(off, 20)
        return t == math.floor(t) and off < 1024.0

    b1, b2 = sorted((brk(offf), brk(dfr)))
    irregular = not (dyadic(offf) and dyadic(dfr) and h < (1 << 20))
    rps = (b1 + R - 1) // R + (b2 - b1 + R - 1) // R + (h - b2 + R - 1) // R
    WB = int(math.ceil(dfr + 0.5)) + 2
    direct = K <= 16 and WB + 4 <= 16
    need = ((64 + rps - 1) // rps + 1) * K                               # records a wave's 64 runs can span; the LDS tile holds 128 at most
    tile = max(40, min(128, (need + 7) & ~7))
    F = c.f.shape[0]
    loops = any((min(F, (min(g0 + 63, nseg * rps - 1)) // rps + 1) - min(F, g0 // rps)) * K > tile for g0 in range(0, nseg * rps, 64))
    sounding = [p for p in range(len(c.st)) if c.ln[p] >= max(1, c.minframes) and int(c.st[p]) * h - edgsam + edgsamp >= 0]
    dropped = [p for p in range(len(c.st)) if c.ln[p] >= max(1, c.minframes) and int(c.st[p]) * h - edgsam + edgsamp < 0]
    x = []                                                               # expm1i's arguments: 2 pi / sr times a slope of fsig
    for p in sounding:
        rows = int(c.st[p]) + np.arange(int(c.ln[p]))
        slot = (c.pid[rows] == p).argmax(axis=1)
        x.extend(2 * np.pi * np.abs(np.diff(c.f[rows, slot])) / (c.sr * h))
    x = np.asarray(x)
    br = set()
    br.add("rows" if direct else "copy")
    br.add("irregular" if irregular else "regular")
    br.add("edges_kernel" if irregular else "edges_inline")
    br.add("tile_clamp" if loops else "tile_fit")                      # (a wave walks its records in more than one tile, or not)
    if np.any(x >= 2.0 ** -6):
        br.add("expm1i_sincos")
    if np.any((x < 2.0 ** -6) & (x > 0)):
        br.add("expm1i_series")
    if EF >= 2:
        br.add("attack_spans_segments")
    if any(0 < edgsam and int(c.st[p]) * h - edgsam < 0 for p in sounding):
        br.add("attack_cropped")
    if not sounding:
        br.add("silent")
    if dropped:
        br.add("negative_start")
    if h < R:
        br.add("hop_below_run")
    if h % 8:
        br.add("hop_not_8n")
    return SimpleNamespace(tile=tile, h=h, K=K, dfr=dfr, edgsam=edgsam, edgsamp=edgsamp, EF=EF, wlen=wlen, nseg=nseg, R=R, rps=rps,
                           irregular=irregular, direct=direct, need=need, x=x, branches=br, dropped=dropped)


# ---- the cases -----------------------------------------------------------------------------------------------------------
# the first frames of the first eight lanes: (start, length) -- every length 1 .. 8, one partial at frame 0, starts at frames 1 and 2
_HEAD = [[(0, 8)], [(1, 5), (7, 1)], [(0, 2), (3, 4)], [(2, 6)], [(0, 7)], [(0, 3), (4, 1), (6, 2)], [(1, 1), (3, 3)], [(2, 2), (5, 3)]]


def _table(rng, K, F=16, jump=60.0, phmax=1e3, fmax=0.45 * SR):
    """A partial table that no tracker made.  Frames [0, 8): partials of every length 1 .. 8, one from frame 0, others from
    frames 1 and 2; frame 8: no peak at all; frames 9 .. 9 + B - 1 (B = 3; 1 when F = 10): every one of the K slots starts and
    ends together; the rest: partials, one of which runs to frame F-1.  A partial's slot changes from row to row."""
    A = 8
    B = 3 if F >= 13 else F - A - 1
    assert F >= 10 and B >= 1
    lanes = []                                                           # per lane: [(start, length)]
    for k in range(K):
        if K == 1:
            head = [(0, 1), (2, A - 2)]                                  # (one lane: a start at frame 0 and one within two frames of it)
        elif k < 8:
            head = list(_HEAD[k])
        else:
            head, pos = [], int(rng.integers(0, 3))
            while pos < A:
                n = int(rng.integers(1, min(8, A - pos) + 1))
                head.append((pos, n))
                pos += n + int(rng.integers(0, 3))
        tail0 = A + 1 + B
        if tail0 >= F:
            tail = []
        elif k == 0:
            tail = [(tail0, F - tail0)]                                  # ends at frame F - 1
        elif k == 1:
            tail = [(tail0 + 1, 1)] if F - tail0 > 1 else []
        else:
            s0 = tail0 + int(rng.integers(0, F - tail0))
            tail = [(s0, int(rng.integers(1, F - s0 + 1)))]
        lanes.append(head + [(A + 1, B)] + tail)
    parts = [(k, s, n) for k in range(K) for (s, n) in lanes[k]]
    order = rng.permutation(len(parts))                                  # partial numbers in no particular order
    P = len(parts)
    st = np.zeros(P, dtype=np.int32)
    ln = np.zeros(P, dtype=np.int32)
    lane_pid = -np.ones((F, K), dtype=np.int32)
    lane_f = np.zeros((F, K))
    lane_m = np.zeros((F, K))
    lane_r = np.zeros((F, K))
    for i, (k, s, n) in enumerate(parts):
        p = int(order[i])
        st[p], ln[p] = s, n
        base = rng.uniform(100.0, fmax)
        fr = np.clip(base + np.cumsum(rng.uniform(-jump, jump, n)), 20.0, SR / 2)
        lane_pid[s:s + n, k] = p
        lane_f[s:s + n, k] = fr
        lane_m[s:s + n, k] = rng.uniform(0.01, 1.0, n)
        lane_r[s:s + n, k] = rng.uniform(-phmax, phmax, n)
    # the points that divide by zero somewhere or sit on a limit (all in lane 0, which every table has)
    lane_m[2, 0] = 0.0
    lane_f[4, 0] = 0.0
    lane_f[A - 1, 0] = 0.0
    lane_m[A - 1, 0] = 0.0
    lane_f[A + 1, 0] = SR / 2
    lane_r[0, 0] = -abs(lane_r[0, 0])
    lane_r[1, 0] = abs(lane_r[1, 0])
    f = np.zeros((F, K))
    mag = np.zeros((F, K))
    realph = np.zeros((F, K))
    pid = -np.ones((F, K), dtype=np.int32)
    for r in range(F):
        perm = rng.permutation(K)                                        # lane k sits in slot perm[k] of this row
        f[r, perm], mag[r, perm], realph[r, perm], pid[r, perm] = lane_f[r], lane_m[r], lane_r[r], lane_pid[r]
    assert not np.any(pid[A] >= 0) and np.all(pid[A + 1:A + 1 + B] >= 0)
    assert np.any(st == 0) and np.any((st == 1) | (st == 2)) and int((st + ln).max()) == F
    return f, mag, realph, pid, st, ln


def _case(name, group, seed, meant, K=8, nfft=2048, hop_a=512, hop_s=512, edge=1.0, minframes=1, **kw):
    rng = np.random.default_rng(seed)
    # frequencies up to 0.45 sr, lower where a segment or an edge is long: the phase that a partial accumulates over one (2 pi f / sr
    # per sample; the reference adds it up sample by sample) stays within 1e3 rad, the size of realph, so that float64 round-off of
    # the reference's own sums keeps a tenth of the bound (the bound's Phi knows realph and the hop, not the edges' length)
    edgsam = int(1. / (hop_a / float(nfft)) / 2. * hop_s * edge)
    kw.setdefault("fmax", min(0.45 * SR, 1e3 * SR / (2 * np.pi * max(hop_s, edgsam, 1))))
    f, mag, realph, pid, st, ln = _table(rng, K, **kw)
    return SimpleNamespace(name=name, group=group, meant=tuple(meant), f=f, mag=mag, realph=realph, pid=pid, st=st, ln=ln,
                           sr=SR, nfft=nfft, hop_a=hop_a, hop_s=hop_s, edge=edge, minframes=minframes)


_CASES = None


def cases():
    """The named cases, each from its own seed (built once; nothing may write to them)."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    seed = [20250]

    def add(name, group, meant, **kw):
        seed[0] += 1
        out.append(_case(name, group, seed[0], meant, **kw))

    # Hop: nfft / hop_a = 4 (regular cuts, rows path, attacks inline).  The 128 records of 16 frames x 8 slots fit one tile even
    # where the host clamps it (hop_s <= 32); a hop below the run length leaves a run shorter than R, one that is no multiple
    # of 8 a ragged last run; 2 pi df / (sr h) passes 2^-6 for jumps of 110 h Hz: the sincos branch of expm1i at the small hops
    for h in (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100, 300, 512):
        meant = ["rows", "regular", "edges_inline", "tile_fit"]
        meant += ["hop_below_run"] if h < 8 else []
        meant += ["hop_not_8n"] if h % 8 else []
        meant += ["expm1i_sincos"] if h <= 8 else ["expm1i_series"]
        add("hop_%d" % h, "hop", meant, hop_s=h)
    # Overlap: dfr = nfft / hop_a / 2 = .5, 1, 4, 8 (rows: WB + 4 = 15 <= 16), 16 (copy: WB + 4 = 23); 2/3, 5/3 and 5.12 are
    # not dyadic: every body through k_synth_extras<, true>, the edges as a launch of their own
    for (nfft, hop_a), meant in (((1024, 1024), ["rows", "regular"]), ((1024, 512), ["rows", "regular"]), ((2048, 256), ["rows", "regular"]),
                                 ((2048, 128), ["rows", "regular"]), ((2048, 64), ["copy", "regular"]), ((1024, 768), ["rows", "irregular", "edges_kernel"]),
                                 ((1000, 300), ["rows", "irregular", "edges_kernel"]), ((1024, 100), ["rows", "irregular", "edges_kernel"])):
        for h in (33, 256):
            add("overlap_%d_%d_h%d" % (nfft, hop_a, h), "overlap", meant + (["attack_spans_segments"] if nfft // hop_a >= 4 else []),
                nfft=nfft, hop_a=hop_a, hop_s=h)
    # K: rows of at most 16 peaks are read in place, wider ones through the partial-major copy; 17 and 100 are no multiple of
    # anything in the kernel; a wave's 64 runs are 32 segments at hop 8 and 8 at hop 64: more than the 128 records of a tile from
    # K = 16 and K = 17, so that k_synth_bodies walks them tile by tile
    for K in (1, 16, 17, 64, 100, 128):
        for h in (8, 64):
            add("K_%d_h%d" % (K, h), "K", ["rows" if K <= 16 else "copy", "tile_clamp" if K * (32 if h == 8 else 8) > 128 else "tile_fit"], K=K, hop_s=h)
    # Edge: edgsam = 2 h edge: none, one segment, four segments, 7.4 segments (attacks of frames 1 .. 7 cropped at sample 0)
    for e in (0.0, 0.5, 2.0, 3.7):
        for h in (8, 300):
            add("edge_%g_h%d" % (e, h), "edge", ["edges_inline"] + (["attack_spans_segments", "attack_cropped"] if e >= 2 else []), edge=e, hop_s=h)
    # Minframes: 3 silences the short partials, 9 all of them
    for mf in (3, 9):
        for h in (8, 300):
            add("minframes_%d_h%d" % (mf, h), "minframes", ["silent"] if mf == 9 else ["rows"], minframes=mf, hop_s=h)
    # steep: frame-to-frame jumps of up to 4 kHz pass expm1i's threshold at hop 8 (877 Hz); at hop 64 the threshold is a jump
    # of 7 019 Hz, so that case jumps by up to 16 kHz
    add("steep_h8", "steep", ["expm1i_sincos", "expm1i_series"], hop_s=8, jump=4000.0)
    add("steep_h64", "steep", ["expm1i_sincos", "expm1i_series"], hop_s=64, jump=16000.0)
    # ... and one whose frequencies swing over the whole band at hop 8: 2 pi df / (sr h) up to 0.39, where a series cut at x^8 is
    # wrong by 1e-9 (at 4 kHz it would still be exact to 1e-16: only such slopes tell the two branches apart)
    add("steep_h8_wide", "steep", ["expm1i_sincos", "expm1i_series"], hop_s=8, jump=20000.0)
    for c in out[-3:]:
        x = plan(c).x
        assert np.any(x >= 2.0 ** -6) and np.any(x < 2.0 ** -6), c.name
    # stretch: three synthesis hops per analysis hop (F = 10 keeps the waveform under 20 000 samples)
    add("stretch", "stretch", ["tile_fit", "expm1i_series"], hop_s=1536, F=10)
    # bigphase: phase arguments of 1e6 rad (the bound scales with their ulp)
    add("bigphase", "bigphase", ["rows", "expm1i_series"], hop_s=512, phmax=1e6)
    for c in out:
        for a in (c.f, c.mag, c.realph, c.pid, c.st, c.ln):
            a.setflags(write=False)
    _CASES = out
    return out


def group(name):
    return [c for c in cases() if c.group == name]


GROUPS = ("hop", "overlap", "K", "edge", "minframes", "steep", "stretch", "bigphase")
