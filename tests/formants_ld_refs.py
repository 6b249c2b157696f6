"""Long-double references of the formant kernels' hard cases (FORMANTS.md, "Differential tests"), shared by
test_formants_refs_cpu.py and test_formants_diff_gpu.py.  Plain numpy, np.longdouble; nothing runs on a device here.

Roots: hard_polys() lists real polynomials the root finder of pvx_roots.h has to get right (nearly real pairs, close and
multiple roots, roots of unity, wide spreads of moduli, random and LPC rows); polish() turns starting values into roots
of the float64 coefficients themselves by Newton's method in long double and certifies them; aberth_model() restates
the device iteration in float64 numpy.  The bounds hb, delta and rho are computed from the references alone.

Frames: frame_shapes() lists signals whose last frame ends on the last decimated sample; frame_chain() is the
pre-emphasis, the polyphase sum over the zero extension and the window in long double with the rounding bound of a
float64 evaluation carried along, glottal_ld_refs.lpc_stage turns that into an LPC row and its bound.  WRONG_CHAINS are
five plausible mistakes the bounds have to exclude."""
import numpy as np

from . import formants_refs as refs
from . import glottal_ld_refs as gl

LD = np.longdouble
CLD = np.clongdouble
EPS = 2.0 ** -53
MAX_ITER = 200                                                         # kMaxIter of pvx_roots.h


# ---- polynomials -----------------------------------------------------------------------------------------------------
def _conv(a, b):
    out = np.zeros(len(a) + len(b) - 1, dtype=LD)
    for i, v in enumerate(b):
        out[i:i + len(a)] += a * v
    return out


def poly_ld(roots, lead=1.0):
    """float64 coefficients of lead * prod (z - r), the product of the real factors in long double and one rounding per
    coefficient at the end.  roots: complex128, real ones and the members with imag > 0 of the pairs."""
    c = np.array([LD(lead)])
    for z in roots:
        z = complex(z)
        if z.imag == 0:
            c = _conv(c, np.array([LD(1), -LD(z.real)]))
        else:
            assert z.imag > 0
            c = _conv(c, np.array([LD(1), -2 * LD(z.real), LD(z.real) * LD(z.real) + LD(z.imag) * LD(z.imag)]))
    return c.astype(np.float64)


def with_conj(roots):
    out = []
    for z in roots:
        out += [complex(z)] if complex(z).imag == 0 else [complex(z), complex(z).conjugate()]
    return np.array(out, dtype=np.complex128)


def horner_ld(c, z):
    """(p(z), p'(z)) in complex long double; z an array"""
    c = np.asarray(c, dtype=np.float64)
    z = np.asarray(z, dtype=CLD)
    p = np.full(z.shape, CLD(c[0]))
    d = np.zeros(z.shape, dtype=CLD)
    for k in range(1, len(c)):
        d = d * z + p
        p = p * z + LD(c[k])
    return p, d


def hb(c, z):
    """2p 2^-53 sum |c_k| |z|^(p-k): formants_refs.horner_bound's second return, for an array of points"""
    c = np.asarray(c, dtype=np.float64)
    az = np.abs(np.asarray(z, dtype=CLD)).astype(LD)
    s = np.full(az.shape, LD(abs(c[0])))
    for k in range(1, len(c)):
        s = s * az + LD(abs(c[k]))
    return 2 * (len(c) - 1) * LD(EPS) * s


def separation(z):
    """per root the distance to the nearest other one"""
    z = np.asarray(z, dtype=CLD)
    if len(z) < 2:
        return np.full(len(z), np.inf)
    d = np.abs(z[:, None] - z[None, :]).astype(LD)
    d[np.arange(len(z)), np.arange(len(z))] = np.inf
    return d.min(axis=1)


def polish(c, roots):
    """Newton's method in long double on the float64 coefficients c from the starting values `roots`: the references are
    roots of the polynomial the device gets, not of the one the generator meant.  A start with imag == 0 stays on the real
    axis.  Returns (z, |p'(z)|, separation per root, cert): cert = p |p(z)| / |p'(z)| in long double is the radius of a disc
    about z that holds a root of c (Henrici), so p values whose discs are disjoint are all the roots."""
    c = np.asarray(c, dtype=np.float64)
    p = len(c) - 1
    start = np.asarray(roots, dtype=np.complex128)
    real = start.imag == 0
    z = start.astype(CLD)
    with np.errstate(all="ignore"):
        for _ in range(100):
            f, d = horner_ld(c, z)
            step = np.where(d != 0, f / np.where(d != 0, d, 1), 0)
            z = z - step
            z[real] = z[real].real
            if np.all(np.abs(step) <= LD(2.0) ** -62 * np.abs(z)):
                break
        f, d = horner_ld(c, z)
        ad = np.abs(d).astype(LD)
        cert = np.where(ad > 0, p * np.abs(f).astype(LD) / np.where(ad > 0, ad, 1), np.inf)
    return z, ad, separation(z), cert


def delta(c, z, dabs):
    """the forward radius 4 hb(r) / |p'(r)|"""
    with np.errstate(divide="ignore"):
        return 4 * hb(c, z) / dabs


def rho(c, r, m, others):
    """2 (4 hb(r) / |q(r)|)^(1/m) for the m-fold root r of c, q = c[0] prod (r - s) over the other roots s (with
    their multiplicities)"""
    q = LD(abs(c[0]))
    for s in others:
        q = q * np.abs(CLD(r) - CLD(s))
    return 2 * (4 * hb(c, np.array([r]))[0] / q) ** (LD(1) / m)


def aberth_model(c, normalise=True):
    """The loop of pvx_roots.h's wave_roots in float64 numpy, statement by statement (no fma): the start circle, Horner
    for p, p' and sum |c_k| |z|^(q-k), the Aberth sum in index order, both stop tests, the bound of MAX_ITER iterations.
    normalise: the coefficients are divided by c[0] first, as k_polyroots loads them.  Returns (the p iterates before the
    canonical form: complex128, exact zeros for trailing zero coefficients; iterations run; converged?)."""
    c = np.asarray(c, dtype=np.float64)
    p = len(c) - 1
    if normalise:
        c = c / c[0]
    q = p
    while q > 0 and c[q] == 0.0:
        q -= 1
    out = np.zeros(p, dtype=np.complex128)
    if q == 0:
        return out, 0, True
    with np.errstate(all="ignore"):
        lane = np.arange(q, dtype=np.float64)
        rad = np.exp(np.log(np.abs(c[q] / c[0])) / q)
        ang = (6.283185307179586 * lane + 0.7) / q
        zr, zi = rad * np.cos(ang), rad * np.sin(ang)
        done = np.zeros(q, dtype=bool)
        tol = q * EPS
        off = ~np.eye(q, dtype=bool)
        its, conv = MAX_ITER, False
        for it in range(MAX_ITER):
            pr, pi = np.full(q, c[0]), np.zeros(q)
            dr, di = np.zeros(q), np.zeros(q)
            s = np.full(q, abs(c[0]))
            az = np.hypot(zr, zi)
            for k in range(1, q + 1):
                ndr, ndi = dr * zr + (-di * zi + pr), dr * zi + (di * zr + pi)
                npr, npi = pr * zr + (-pi * zi + c[k]), pr * zi + pi * zr
                dr, di, pr, pi = ndr, ndi, npr, npi
                s = s * az + abs(c[k])
            dx, dy = zr[:, None] - zr[None, :], zi[:, None] - zi[None, :]
            m = dx * dx + dy * dy
            use = off & (m > 0.0)
            ms = np.where(use, m, 1.0)
            sr, si = np.zeros(q), np.zeros(q)
            for j in range(q):                                         # j ascending, as the lanes add
                sr = np.where(use[:, j], sr + dx[:, j] / ms[:, j], sr)
                si = np.where(use[:, j], si - dy[:, j] / ms[:, j], si)
            small = np.hypot(pr, pi) <= tol * s
            dm = dr * dr + di * di
            wr, wi = (pr * dr + pi * di) / dm, (pi * dr - pr * di) / dm
            er, ei = 1.0 - (wr * sr - wi * si), -(wr * si + wi * sr)
            em = er * er + ei * ei
            sx, sy = (wr * er + wi * ei) / em, (wi * er - wr * ei) / em
            move = ~done & ~small
            zr, zi = np.where(move, zr - sx, zr), np.where(move, zi - sy, zi)
            still = np.hypot(sx, sy) <= 2.0 ** -52 * np.hypot(zr, zi)
            done = done | small | (move & still)
            if done.all():
                its, conv = it + 1, True
                break
    out[:q] = zr + 1j * zi
    return out, its, conv


def _lpc_row(x, order):
    """[1, a] of the Hann-windowed vector x: float64 lags, float64 recursion (host)"""
    v = np.asarray(x, dtype=np.float64) * np.hanning(len(x))
    r = np.array([np.dot(v[k:], v[:len(v) - k]) for k in range(order + 1)])
    return gl.levinson(r, order)


# degree-64 rows of formants_refs.poly_from_roots over its whole range 0.3 .. 1.2: (seed, real roots).  The seeds of
# WIDE_REFUSED are rows the rule 8 delta <= separation refuses (test_formants_refs_cpu.py asserts that it does): they stay
# in the residual and canonical-form tests, outside the forward test.
WIDE_SEEDS = [(200, 2), (202, 6)]
WIDE_REFUSED = [(201, 2)]

_POLYS = []


def hard_polys():
    """[dict(label, c, start, exact, mult, nreal)]: c the float64 coefficients; start the values polish() starts from
    (the prescribed roots; None: aberth_model's iterates); exact: the prescribed roots are the exact roots of the
    long-double product c was rounded from (the cluster families); mult: [(root, multiplicity)] for those; nreal: the
    prescribed count of real roots (None where roots were not prescribed)."""
    if _POLYS:
        return _POLYS
    out = []

    def add(label, c, start=None, mult=None, nreal=None):
        out.append(dict(label=label, c=np.asarray(c, dtype=np.float64), start=start, mult=mult, nreal=nreal))

    def prescribed(label, roots, lead=1.0):
        roots = np.asarray(roots, dtype=np.complex128)
        add(label, poly_ld(roots, lead), start=with_conj(roots), nreal=int(np.sum(roots.imag == 0)))

    far = [0.5 * np.exp(2.0j), -0.4]                                   # a pair and a real root well away from the hard ones
    for k, lead in ((2, 1.0), (4, 3.0), (6, 1.0)):
        e = 10.0 ** -k
        z = 0.6 + 0j
        prescribed("nearreal_1e-%d" % k, [complex(0.6, e * 0.6)] + far, lead)
        prescribed("realpair_1e-%d" % k, [z, z + e] + far, -0.37 if k == 2 else 1.0)
        w = 0.6 * np.exp(1.0j)
        prescribed("pairpair_1e-%d" % k, [w, w + e, -0.4])
    # exact multiple roots: the coefficients are one rounding away from the long-double product
    for label, roots, lead in (("double_real", [(0.5, 2), (0.5 * np.exp(2.0j), 1), (-0.4, 1)], 1.0),
                               ("quad_real", [(-0.75, 4), (0.5 * np.exp(1.0j), 1)], 3.0),
                               ("z_minus_0.9_pow8", [(0.9, 8)], 1.0),
                               ("double_pair", [(0.7 * np.exp(1.2j), 2), (-0.4, 1)], 1.0)):
        flat = [complex(r) for r, m in roots for _ in range(m)]
        mult = []
        for r, m in roots:
            mult += [(complex(r), m)] if complex(r).imag == 0 else [(complex(r), m), (complex(r).conjugate(), m)]
        add(label, poly_ld(flat, lead), mult=mult, nreal=int(sum(m for r, m in roots if complex(r).imag == 0)))
    for label, n, sign in (("z16_minus_1", 16, -1.0), ("z64_minus_1", 64, -1.0), ("z63_plus_1", 63, 1.0)):
        c = np.zeros(n + 1)
        c[0], c[n] = 1.0, sign
        k = np.arange(n)
        th = 2 * np.pi * k / n if sign < 0 else (2 * k + 1) * np.pi / n
        start = np.exp(1j * th)
        start[np.abs(start.imag) < 1e-9] = start[np.abs(start.imag) < 1e-9].real
        add(label, c, start=start, nreal=int(np.sum(start.imag == 0)))
    prescribed("moduli_1e-3_to_1e3", [1e-3, -3e-2, 0.2 * np.exp(0.7j), 5.0 * np.exp(2.1j), -40.0, 1e3 * np.exp(1.3j)])
    for n in (10, 20):
        c = np.array([LD(1)])
        for k in range(1, n + 1):
            c = _conv(c, np.array([LD(1), -LD(k)]))
        add("wilkinson%d" % n, c.astype(np.float64), start=np.arange(1, n + 1) + 0j, nreal=n)
    for n, seed in ((10, 301), (32, 302), (64, 303)):
        add("gauss%d" % n, np.random.default_rng(seed).standard_normal(n + 1))
    for order in (16, 48, 64):
        n = 4 * order + 37
        add("lpc%d_noise" % order, _lpc_row(np.random.default_rng(400 + order).standard_normal(n), order))
        t = np.arange(n)
        x = np.sin(0.3 * t) + 0.5 * np.sin(1.1 * t + 0.4) + 1e-6 * np.random.default_rng(500 + order).standard_normal(n)
        add("lpc%d_two_sines" % order, _lpc_row(x, order))
    for seed, nreal in WIDE_SEEDS + WIDE_REFUSED:
        c, roots = refs.poly_from_roots(np.random.default_rng(seed), 64, nreal)
        add("wide64_seed%d" % seed, c, start=roots, nreal=nreal)
    c, roots = refs.poly_from_roots(np.random.default_rng(WIDE_SEEDS[0][0]), 64, WIDE_SEEDS[0][1])
    add("wide64_seed%d_times_3" % WIDE_SEEDS[0][0], 3.0 * c, start=roots, nreal=WIDE_SEEDS[0][1])
    _POLYS.extend(out)
    return _POLYS


_ANALYSIS = {}


def analyse(poly):
    """The reference side of one hard polynomial, computed once: dict(kind, z, delta, sep, cert, rho, model, its, conv).
    kind 'cluster': z the prescribed roots with multiplicity, rho per distinct root, gap the distance to the next distinct
    root; 'forward': the rule 8 delta <= sep holds at every root and the certificate is a small part of delta;
    'residual': neither (the row is still held to the residual and the canonical form)."""
    label = poly["label"]
    if label in _ANALYSIS:
        return _ANALYSIS[label]
    c = poly["c"]
    model, its, conv = aberth_model(c)
    a = dict(model=model, its=its, conv=conv)
    if poly["mult"] is not None:
        mult = poly["mult"]
        a["kind"] = "cluster"
        a["rho"], a["gap"] = [], []
        for i, (r, m) in enumerate(mult):
            others = [s for j, (s, k) in enumerate(mult) if j != i for _ in range(k)]
            a["rho"].append(rho(c, r, m, others))
            a["gap"].append(min([abs(r - s) for j, (s, k) in enumerate(mult) if j != i] or [np.inf]))
        a["ok"] = all(8 * rr <= g for rr, g in zip(a["rho"], a["gap"]))
    else:
        z, dabs, sep, cert = polish(c, poly["start"] if poly["start"] is not None else model)
        snap = (z.imag != 0) & (np.abs(z.imag) <= cert)                # a real root found from a complex start
        if poly["start"] is None and snap.any():
            st = z.astype(np.complex128)
            st[snap] = st[snap].real
            z, dabs, sep, cert = polish(c, st)
        dl = delta(c, z, dabs)
        a.update(z=z, delta=dl, sep=sep, cert=cert)
        with np.errstate(invalid="ignore"):
            a["ok"] = bool(np.all(np.isfinite(dl.astype(np.float64))) and np.all(8 * dl <= sep) and np.all(8 * cert <= dl))
        a["kind"] = "forward" if a["ok"] else "residual"
    _ANALYSIS[label] = a
    return a


def residual_ratio(c, roots):
    """worst |p(z)| / hb(z) over the roots, p in long double on the caller's coefficients (0 where both are 0)"""
    f, _ = horner_ld(c, roots)
    b = hb(c, roots)
    af = np.abs(f).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(af == 0, LD(0), af / b)
    return float(np.max(r)) if len(r) else 0.0


def forward_ratio(got, a):
    """(worst distance / delta over a one-to-one assignment of `got` to the polished references, or inf where there is
    none): every reference's disc of radius delta must hold exactly one of `got`.  The discs are disjoint (8 delta <=
    separation), so that is an assignment, and with p roots on each side it is complete."""
    got = np.asarray(got).astype(CLD)
    z, dl = a["z"], a["delta"]
    if got.shape != z.shape:
        return np.inf
    d = np.abs(got[None, :] - z[:, None]).astype(LD)                   # [reference][device root]
    inside = d <= dl[:, None]
    if not (np.all(inside.sum(axis=1) == 1) and np.all(inside.sum(axis=0) == 1)):
        return np.inf
    return float(np.max(d[inside] / np.broadcast_to(dl[:, None], d.shape)[inside]))


def cluster_ok(got, poly, a):
    """(every m-fold root has exactly m of `got` within rho, the worst distance / rho of those)"""
    got = np.asarray(got).astype(CLD)
    worst, ok = 0.0, len(got) == sum(m for _, m in poly["mult"])
    for (r, m), rr in zip(poly["mult"], a["rho"]):
        d = np.abs(got - CLD(r)).astype(LD)
        near = d <= rr
        ok = ok and int(near.sum()) == m
        if near.any():
            worst = max(worst, float(np.max(d[near] / rr)))
    return ok, worst


def check_canonical(c, r):
    """The canonical form and order of one row of roots_frames (FORMANTS.md), on any row: asserts, returns the count of
    exactly-real roots."""
    c = np.asarray(c, dtype=np.float64)
    p = len(c) - 1
    assert r.shape == (p,) and r.dtype == np.complex128 and np.all(np.isfinite(r.real)) and np.all(np.isfinite(r.imag))
    nzero = 0
    while nzero < p and c[p - nzero] == 0.0:
        nzero += 1
    assert int(np.sum(r == 0)) >= nzero                                # trailing zero coefficients: exact zero roots
    real = r.imag == 0
    assert not np.any(np.signbit(r.imag[real]))                        # +0.0
    nk = int(np.sum(r.imag >= 0))
    up, lo = r[:nk], r[nk:]
    assert np.all(up.imag >= 0) and np.all(lo.imag < 0)
    cplx = up[up.imag > 0]
    assert np.conj(cplx).tobytes() == lo.tobytes()                     # bit-exact pairs, the conjugates in their partners' order
    assert int(real.sum()) == p - 2 * len(cplx)
    ang, mag = np.arctan2(up.imag, up.real), np.abs(up)
    assert np.all((np.diff(ang) > 0) | ((np.diff(ang) == 0) & (np.diff(mag) >= 0)))
    return int(real.sum())


def canonical_model(c, rounds=True):
    """aberth_model's iterates through the canonical-root rule of wave_roots and formants_refs.canon's order (host).
    rounds False: the rule as it was, an iterate whose choice is not returned is real at once."""
    z, its, conv = aberth_model(c)
    c = np.asarray(c, dtype=np.float64)
    p = len(c) - 1
    q = p
    while q > 0 and c[q] == 0.0:
        q -= 1
    zr, zi = z.real.copy(), z.imag.copy()
    m = (zr[:q, None] - zr[None, :q]) ** 2 + (-zi[:q, None] - zi[None, :q]) ** 2
    nr, ni = zr.copy(), zi.copy()
    open_ = np.ones(q, dtype=bool)
    for _ in range(64 if rounds else 1):
        if not open_.any():
            break
        mm = np.where(open_[None, :], m, np.inf)
        best = np.argmin(mm, axis=1)                                   # the lowest index among equals
        for i in np.nonzero(open_)[0]:
            b = best[i]
            if not mm[i, b] < np.inf:
                b = i
            if b == i:
                ni[i] = 0.0
            elif best[b] == i:
                mine = zi[i] > zi[b] or (zi[i] == zi[b] and i < b)
                mi = abs(zi[i] if mine else zi[b])
                nr[i] = zr[i] if mine else zr[b]
                ni[i] = 0.0 if mi == 0.0 else (mi if mine else -mi)
            else:
                continue
            open_[i] = False
    ni[:q][open_] = 0.0
    return refs.canon(nr + 1j * ni), its, conv


# ---- frames ----------------------------------------------------------------------------------------------------------
def frame_shapes():
    """[dict(label, down, L, sym, nwind, hop, order, nfr, j, pre, dtype, seed)]: n = ((nfr - 1) hop + nwind) down - j, so
    the last frame ends exactly on decimated sample ceil(n / down) - 1 and n mod down = (down - j) mod down.  L: taps
    (glottal_ld_refs.taps, asymmetric; sym: the package's own firwin_np)."""
    out = []

    def add(down, L, nwind, hop, order, nfr, j=0, pre=1, dtype="float64", sym=False):
        out.append(dict(down=down, L=L, sym=sym, nwind=nwind, hop=hop, order=order, nfr=nfr, j=j, pre=pre, dtype=dtype, seed=0,
                        label="down%d-L%d-nwind%d-hop%d-p%d-j%d-pre%d-%s%s" % (down, L, nwind, hop, order, j, pre, dtype, "-firwin" if sym else "")))

    add(1, 0, 12, 7, 4, 8, pre=1)                                      # n 61
    add(1, 0, 12, 7, 4, 8, pre=0)
    add(2, 41, 17, 5, 6, 6, j=0)
    add(2, 41, 18, 5, 6, 6, j=1, dtype="float32")
    for j in range(3):
        add(3, 61, 23 + j, 6, 8, 5, j=j)
    for j in range(4):
        add(4, 81, 29 + j, 9, 10, 5, j=j, dtype="int16" if j == 2 else "float64")
    add(8, 161, 40, 11, 12, 4, j=5)
    add(8, 161, 33, 11, 12, 4, j=0, pre=0)
    add(2, 1, 19, 4, 5, 6, j=1)
    add(3, 3, 21, 5, 7, 5, j=2)
    add(4, 7, 25, 6, 9, 5, j=3)
    add(4, 81, 276, 138, 10, 4, j=1, sym=True)                         # the package's own geometry at 44.1 kHz
    add(2, 41, 17, 3, 16, 5, j=1)                                      # nwind = order + 1
    return out


def shape_n(sh):
    return ((sh["nfr"] - 1) * sh["hop"] + sh["nwind"]) * sh["down"] - sh["j"]


def shape_inputs(sh):
    """(x in the shape's sample type, taps or None, window): integer-valued samples, exact in all three types"""
    n = shape_n(sh)
    seed = 9000 + 1000 * sh["down"] + 10 * sh["nwind"] + sh["L"] + sh["j"] + 100000 * sh["seed"]
    x = gl.ar2_noise(seed, n)
    x = np.round(x * (2e4 / np.max(np.abs(x)))).astype(sh["dtype"])
    h = None
    if sh["down"] > 1:
        if sh["sym"]:
            from pypevoc_amd.speech.formants import firwin_np         # host numpy only: no device is touched
            h = firwin_np(sh["down"])
            assert len(h) == sh["L"]
        else:
            h = gl.taps(seed + 1, sh["L"])
    return x, h, gl.ramp_window(sh["nwind"])


WRONG_CHAINS = ("base_off_by_one", "ends_clamped", "taps_not_reversed", "last_difference_dropped", "floor_for_ceil")
FRAMES_CHECKED = (0, 1, -2, -1)


def decimated(x, pre, down, h, wrong=None, dtype=LD):
    """(y, e_y): the pre-emphasised, decimated signal, ceil(n / down) samples, and the bound of a float64 evaluation.
    d[i] = x[i] - x[i+1], the last sample unchanged: one rounding, 2^-53 |d|.  y[m] = sum_k h[L-1-k] dz[m down + k - half],
    dz the zero extension: (L + 1) 2^-53 sum |h| |d| + sum |h| e_d, the argument of glottal_ld_refs.highpass.  down 1: y = d.
    wrong: one of WRONG_CHAINS; dtype: np.float64 evaluates the same chain in float64."""
    x = np.asarray(x).astype(dtype)
    n = len(x)
    d = x.copy()
    if pre:
        d[:-1] = x[:-1] - x[1:]
        if wrong == "last_difference_dropped":
            d[-1] = 0
    e_d = (EPS * np.abs(d) if pre else np.zeros(n)).astype(LD)
    if down == 1 and wrong is None:
        return d, e_d
    hh = np.ones(1, dtype=dtype) if down == 1 else np.asarray(h).astype(dtype)
    L = len(hh)
    half = (L - 1) // 2
    nd = n // down if wrong == "floor_for_ceil" else -(-n // down)
    full = -(-n // down)
    y, e = np.zeros(full, dtype=dtype), np.zeros(full, dtype=LD)
    ah = np.abs(hh).astype(LD)
    for m in range(nd):
        base = m * down - half + (1 if wrong == "base_off_by_one" else 0)
        i = base + np.arange(L)
        if wrong == "ends_clamped":
            ok = np.ones(L, dtype=bool)
            i = np.clip(i, 0, n - 1)
        else:
            ok = (i >= 0) & (i < n)
        taps = hh[np.arange(L)] if wrong == "taps_not_reversed" else hh[L - 1 - np.arange(L)]
        at = ah[np.arange(L)] if wrong == "taps_not_reversed" else ah[L - 1 - np.arange(L)]
        y[m] = np.dot(taps[ok], d[i[ok]])
        e[m] = (L + 1) * EPS * np.dot(at[ok], np.abs(d[i[ok]]).astype(LD)) + np.dot(at[ok], e_d[i[ok]])
    if down == 1:
        e = e_d                                                        # (the product by 1 is exact)
    return y, e


def frame_inputs(sh, x, h, wind, wrong=None, dtype=LD):
    """[(v, e_v)] of the frames FRAMES_CHECKED: the decimated frame times the window, one more rounding"""
    y, e = decimated(x, sh["pre"], sh["down"], h, wrong, dtype)
    w = np.asarray(wind).astype(dtype)
    out = []
    for f in FRAMES_CHECKED:
        f = f % sh["nfr"]
        sl = slice(f * sh["hop"], f * sh["hop"] + sh["nwind"])
        v = y[sl] * w
        out.append((v, np.abs(w).astype(LD) * e[sl] + EPS * np.abs(v).astype(LD)))
    return out


_FRAME_REFS = {}


def frame_refs(sh):
    """[(a long double [order + 1], bound)] of the frames FRAMES_CHECKED, computed once per shape"""
    if sh["label"] not in _FRAME_REFS:
        x, h, wind = shape_inputs(sh)
        _FRAME_REFS[sh["label"]] = [gl.lpc_stage(v, e_v, sh["order"]) for v, e_v in frame_inputs(sh, x, h, wind)]
    return _FRAME_REFS[sh["label"]]


def lpc_f64(v, order):
    """the LPC of a float64 frame by float64 lags and the float64 recursion"""
    v = np.asarray(v, dtype=np.float64)
    r = np.array([np.dot(v[k:], v[:len(v) - k]) for k in range(order + 1)])
    return gl.levinson(r, order)
