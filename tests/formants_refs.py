"""Host-side helpers of the formant tests (and of tests/golden/make_golden_formants.py): the documented order of a
polynomial's roots (FORMANTS.md), the rows lpc2form derives from np.roots' output, and the rounding bound of Horner's rule.
Plain numpy."""
import numpy as np


def canon(r):
    """np.roots' output in the order of pvx_polyroots: the roots with imag >= 0 by ascending angle, equal angles by
    ascending modulus, then those with imag < 0 in the order of their conjugates."""
    r = np.asarray(r, dtype=np.complex128)
    kept, drop = r[r.imag >= 0], r[r.imag < 0]
    kept = kept[np.lexsort((np.abs(kept), np.arctan2(kept.imag, kept.real)))]
    drop = drop[np.lexsort((np.abs(drop), np.arctan2(-drop.imag, drop.real)))]
    return np.concatenate((kept, drop))


def lpc2form_rows(roots, Fs):
    """(nkept [n], freq [n][order], bw [n][order]) as pvx_formants returns them, from np.roots rows [n][order], with
    lpc2form's own expressions and np.argsort (SpeechAnalysis.py:197-207); NaN beyond nkept."""
    n, order = roots.shape
    nkept = np.zeros(n, dtype=np.int32)
    freq, bw = np.full((n, order), np.nan), np.full((n, order), np.nan)
    for i in range(n):
        RTS = roots[i][np.imag(roots[i]) >= 0]
        nFreq = np.arctan2(np.imag(RTS), np.real(RTS)) * (Fs / (2 * np.pi))
        Indices = np.argsort(nFreq)
        nkept[i] = len(RTS)
        freq[i, :len(RTS)] = nFreq[Indices]
        with np.errstate(divide="ignore"):
            bw[i, :len(RTS)] = -1 / 2 * (Fs / (2 * np.pi)) * np.log(np.abs(RTS[Indices]))
    return nkept, freq, bw


def horner_bound(c, z):
    """(|p(z)| in np.longdouble, 2p * 2^-53 * sum |c_k| |z|^(p-k)): the residual of z as a root of the polynomial c and the
    rounding bound of Horner's rule at z."""
    c = np.asarray(c, dtype=np.float64)
    p = len(c) - 1
    zr, zi = np.longdouble(z.real), np.longdouble(z.imag)
    pr, pi = np.longdouble(c[0]), np.longdouble(0)
    for k in range(1, p + 1):
        pr, pi = pr * zr - pi * zi + np.longdouble(c[k]), pr * zi + pi * zr
    s = float(np.sum(np.abs(c) * np.abs(z) ** np.arange(p, -1, -1.0)))
    return float(np.hypot(pr, pi)), 2 * p * 2.0**-53 * s


def poly_from_roots(rng, degree, nreal, lo=0.3, hi=1.2):
    """(coefficients, prescribed roots) of a real polynomial of the given degree with nreal real roots of both signs and
    conjugate pairs with |imag| >= 0.05 |z|, all with lo <= |z| <= hi; leading coefficient 1."""
    assert (degree - nreal) % 2 == 0
    mag = rng.uniform(lo, hi, nreal)
    sign = np.where(np.arange(nreal) % 2 == 0, 1.0, -1.0)
    roots = list(mag * sign + 0j)
    for _ in range((degree - nreal) // 2):
        m = rng.uniform(lo, hi)
        th = rng.uniform(np.arcsin(0.05) + 0.01, np.pi - np.arcsin(0.05) - 0.01)
        z = m * np.exp(1j * th)
        roots += [z, np.conj(z)]
    c = np.array([1.0])
    for z in roots:                                                  # real factors only: the coefficients are exactly real
        if z.imag == 0:
            c = np.convolve(c, [1.0, -z.real])
        elif z.imag > 0:
            c = np.convolve(c, [1.0, -2 * z.real, abs(z) ** 2])
    return c, np.array(roots)


# (degree, real roots, seed, modulus range) of the polynomials of test_formants_gpu.py::test_roots_frames.  Degrees up to 16
# draw the moduli from the whole range 0.3 .. 1.2; at 63 and 64 np.roots itself misses four times Horner's bound by factors
# of 1e2 .. 1e6 over that range (the companion matrix is too badly conditioned), so those draw from 0.8 .. 1.1, where it
# meets it: test_formants_cpu.py::test_np_roots_meets_the_residual_bound_on_the_root_polynomials checks every row below.
ROOT_POLYS = [(1, 1, 1, 0.3, 1.2), (2, 0, 2, 0.3, 1.2), (2, 2, 3, 0.3, 1.2), (3, 1, 4, 0.3, 1.2), (3, 3, 5, 0.3, 1.2),
              (5, 1, 6, 0.3, 1.2), (5, 3, 7, 0.3, 1.2), (10, 0, 8, 0.3, 1.2), (10, 2, 9, 0.3, 1.2), (11, 3, 10, 0.3, 1.2),
              (16, 4, 11, 0.3, 1.2), (63, 3, 12, 0.8, 1.1), (64, 2, 13, 0.8, 1.1), (64, 6, 14, 0.8, 1.1)]


def root_polys():
    """[(label, coefficients, count of roots with imag == 0, count of exact zero roots)]: ROOT_POLYS, one of them times
    z^2 (two trailing zero coefficients), and z^2 - 1."""
    out = []
    for deg, nreal, seed, lo, hi in ROOT_POLYS:
        c, _ = poly_from_roots(np.random.default_rng(seed), deg, nreal, lo, hi)
        out.append(("deg%d_real%d" % (deg, nreal), c, nreal, 0))
    c, _ = poly_from_roots(np.random.default_rng(6), 5, 1)
    out.append(("deg5_times_z2", np.concatenate((c, [0.0, 0.0])), 3, 2))
    out.append(("z2_minus_1", np.array([1.0, 0.0, -1.0]), 2, 0))
    return out
