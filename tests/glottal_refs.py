"""Plain float64 numpy restatements of glottal inverse filtering, one frame (InverseFilter.apply) and the overlap-add
(iaif_ola), written from the formulas of GLOTTAL.md with their loops: what the fixtures tests/golden/V*.npz are checked
against without a GPU, and the Levinson recursion test_glottal_gpu.py compares the device LPC with.  No scipy."""
import numpy as np


def autocorr(v, p):
    """r[k] = sum_i v[i+k] v[i], k = 0 .. p"""
    v = np.asarray(v, dtype=np.float64)
    n = len(v)
    return np.array([np.dot(v[k:], v[:n - k]) if k < n else 0.0 for k in range(p + 1)])


def levinson(r, p):
    """[1, a_1 .. a_p] with toeplitz(r[:p]) a = -r[1:p+1]; np.linalg.LinAlgError when a prediction error is exactly 0."""
    a = np.zeros(p + 1)
    a[0] = 1.0
    err = float(r[0])
    for i in range(1, p + 1):
        if err == 0.0:
            raise np.linalg.LinAlgError("Singular principal minor")
        acc = r[i]
        for j in range(1, i):
            acc += a[j] * r[i - j]
        k = -acc / err
        new = a.copy()
        for j in range(1, i):
            new[j] = a[j] + k * a[i - j]
        new[i] = k
        a = new
        err *= 1.0 - k * k
    return a


def lpc(v, p):
    return levinson(autocorr(v, p), p)


def fir(h, u):
    """out[j] = sum_k h[k] u[j-k], zeros before u"""
    out = np.zeros(len(u))
    for j in range(len(u)):
        ke = min(j, len(h) - 1)
        out[j] = np.dot(h[:ke + 1], u[j::-1][:ke + 1])
    return out


def integ(v, leak):
    out = np.zeros(len(v))
    prev = 0.0
    for j in range(len(v)):
        prev = v[j] + leak * prev
        out[j] = prev
    return out


def highpass(xf, b):
    """y[i] = sum_k b[k] xz[i + hp - k], xz = xf followed by hp zeros, hp = round_half_even(L/2 - 1)"""
    xf = np.asarray(xf, dtype=np.float64)
    n, L = len(xf), len(b)
    hp = int(np.round(L / 2 - 1))
    y = np.zeros(n)
    for i in range(n):
        top = i + hp
        klo, khi = max(0, top - (n - 1)), min(L - 1, top)
        if khi >= klo:
            y[i] = np.dot(b[klo:khi + 1], xf[top - khi:top - klo + 1][::-1])
    return y


def frame(xf, b, hw, pt, pg, leak, n_it, lpc=lpc):
    """g, dg, Hvt, Hg of one frame; lpc: the linear prediction to use (a test's perturbed one)"""
    P = pt + 1
    y = highpass(xf, b)
    u = np.concatenate([np.linspace(-y[0], y[0], P), y])
    Hg = lpc(y * hw, 1)
    y = fir(Hg, u)[P:]
    for _ in range(n_it):
        Hvt = lpc(y * hw, pt)
        g = integ(fir(Hvt, u), leak)[P:]
        Hg = lpc(g * hw, pg)
        y = integ(fir(Hg, u), leak)[P:]
    Hvt = lpc(y * hw, pt)
    dfull = fir(Hvt, u)
    return integ(dfull, leak)[P:], dfull[P:], Hvt, Hg


def frame_starts(n, nwind, nhop):
    out, ist = [], 0
    while ist < n - nwind:
        out.append(ist)
        ist += nhop
    return out


def ola(x, nwind, nhop, b, hw, wind, pt, pg, leak, n_it, frames=None):
    """glot, dglot, vt_coef, glot_coef, wins; frames: the (g, dg, Hvt, Hg) of every frame if they are known already"""
    x = np.asarray(x)
    n = len(x)
    glot, dglot, wins = np.zeros(n), np.zeros(n), np.zeros(n)
    vt, gc = [], []
    for q, ist in enumerate(frame_starts(n, nwind, nhop)):
        g, dg, Hvt, Hg = frames[q] if frames is not None else frame(x[ist:ist + nwind], b, hw, pt, pg, leak, n_it)
        glot[ist:ist + nwind] += g * wind
        dglot[ist:ist + nwind] += dg * wind
        wins[ist:ist + nwind] += wind
        vt.append(Hvt)
        gc.append(Hg)
    idx = wins > 0
    glot[idx] /= wins[idx]
    dglot[idx] /= wins[idx]
    return glot, dglot, np.array(vt), np.array(gc), wins
