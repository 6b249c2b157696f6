"""Plain float64 numpy restatement of HeterodyneHarmonic's fixed-resolution path, frame by frame and harmonic by harmonic:
what pypevoc_amd/Heterodyne.py and k_hetharm.hip compute, written from the formulas (HETHARM.md), with no import of the
reference and none of the package.  tests/test_hetharm_cpu.py holds it against the recorded Q*.npz."""
import numpy as np


def nframes(nsamp, nwind, nhop):
    """frames start at 0, nhop, .. while the start is < nsamp - nwind"""
    return len(range(0, nsamp - nwind, nhop))


def frame_times(nsamp, sr, nwind, nhop):
    """th: centre time of every frame; idxh: the centres as samples (one more than th when nwind is odd and the last fits)"""
    c = nwind // 2
    th = np.arange(c, nsamp - (nwind - c), nhop) / sr
    idxh = np.arange(c, nsamp - c, nhop).astype('i')
    return th, idxh


def track(nsamp, sr, f, tf=None, fmin=0.1):
    """(fvec in cycles per sample, fmin raised to the track's minimum) from a number, a per-sample array or tf / f pairs"""
    tvec = np.arange(nsamp) / sr
    hz = np.interp(tvec, tf, f) if tf is not None else np.asarray(f, dtype=float) * np.ones(nsamp)
    return hz / sr, max(fmin, hz.min())


def hetsig(fvec, n):
    return np.exp(1j * np.cumsum(fvec * n * 2 * np.pi))


def extract(x, fvec, n, wind, hop):
    """harmonic n: 2 * windowed mean of x * hetsig per frame, and the frames' centre samples"""
    hs = hetsig(fvec, n)
    wlen, norm = len(wind), np.sum(wind)
    out, icent = [], []
    for start in range(0, len(x) - wlen, hop):
        seg = x[start:start + wlen] * hs[start:start + wlen] * wind
        out.append(2 * np.sum(seg) / norm)
        icent.append(start + wlen // 2)
    return np.array(out, dtype=complex), np.array(icent, dtype=np.int64)


def extract_all(x, fvec, nharm, wind, hop):
    ah = np.zeros((nframes(len(x), len(wind), hop), nharm), dtype=complex)
    for n in range(nharm):
        ah[:, n] = extract(x, fvec, n, wind, hop)[0]
    ah[:, 0] /= 2
    return ah


def interp_amp(nsamp, nwind, nhop, col):
    """the frame values `col` linearly interpolated to every sample, clamped to the end values outside the frame centres"""
    t = np.arange(nsamp)
    if len(col) == 1:
        return np.full(nsamp, col[0], dtype=complex)
    r = t - nwind // 2
    i0 = np.clip(r // nhop, 0, len(col) - 2)
    fr = np.clip((r - i0 * nhop) / nhop, 0.0, 1.0)
    return col[i0] + (col[i0 + 1] - col[i0]) * fr


def filter_mask(hf, f0, n, sr, fmin, fmax, ampthr):
    """the four terms of the mask, each as a boolean array"""
    return {"fmin": f0 < fmin, "fmax": f0 > fmax, "nyquist": f0 * n > sr / 2.2, "amp": np.abs(hf) < np.max(np.abs(hf)) * ampthr}


def filter_harmonic(ah, fvec, n, sr, nwind, nhop, fmin, fmax, ampthr):
    hf = interp_amp(len(fvec), nwind, nhop, ah[:, n])
    m = filter_mask(hf, fvec * sr, n, sr, fmin, fmax, ampthr)
    hf[m["fmin"] | m["fmax"] | m["nyquist"] | m["amp"]] = 0
    return hf


def resynth_partial(ah, fvec, n, sr, nwind, nhop, filter=False, fmin=None, fmax=None, ampthr=None):
    hf = filter_harmonic(ah, fvec, n, sr, nwind, nhop, fmin, fmax, ampthr) if filter else interp_amp(len(fvec), nwind, nhop, ah[:, n])
    return np.real(np.conj(hetsig(fvec, n)) * hf)


def resynth(ah, fvec, sr, nwind, nhop):
    y = np.zeros(len(fvec))
    for n in range(ah.shape[1]):
        y += resynth_partial(ah, fvec, n, sr, nwind, nhop)
    return y


def calc_adjusted_freq(x, fvec, sr, wind, nhop):
    h, ic = extract(x, fvec, 1, wind, nhop)
    dph = np.concatenate(([0], np.diff(np.unwrap(np.angle(h)))))
    return fvec[ic] - dph / nhop / 2 / np.pi, ic / sr


def f_cols(fvec, sr, th, nharm, include_dc):
    f0t = np.interp(th, np.arange(len(fvec)) / sr, fvec * sr)
    return np.array([f0t * n for n in range(0 if include_dc else 1, nharm)]).T


def angle_ratios(ah, include_dc):
    camp = ah if include_dc else ah[:, 1:]
    ang = np.angle(camp / camp[:, :1])
    return np.hstack((np.zeros((len(ang), 1)), ang)) if include_dc else ang


def partial_frequencies(ah, fcols, sr, nhop, include_dc):
    camp = ah if include_dc else ah[:, 1:]
    newf = fcols[1:, :] - np.diff(np.unwrap(np.angle(camp)), axis=0) / (nhop / sr) / 2 / np.pi
    return np.hstack((np.zeros((len(newf), 1)), newf)) if include_dc else newf
