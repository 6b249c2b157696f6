"""The transforms of the four spectral kernels on the MI355X -- k_fbank.hip, k_specdesc.hip, k_xspec.hip, k_fric.hip, each
its fused route at 512 / 1024 / 2048 and its rows route (k_frames or k_fric_frames, then rocFFT) -- bin by bin against a direct
DFT in long double, at the derived bound of tests/spectrum_ld_refs.py: about 100 u of the frame's ||X||_2, absolute, so bins
without signal count like any other (SPECTRA.md).

None of the kernels hands out its spectrum; each is driven to report single bins:
  k_fbank     one-hot filter rows, 128 bands a call: spec[i][b] = |X_i[k]|^2; a one-hot at the mirrored column nwind - k gives
              the bits of column k;
  k_specdesc  the periodogram of one frame is |X[k]|^2 for k < nwind/2, of three frames their mean; the ratio and flux tails
              are probed with one-hot weights (flux against an all-zero second frame is |X[k]| itself);
  k_xspec     sxx, syy, sxy come back unscaled per bin, the Nyquist bin included; one and three segments, two blocks or more;
  k_fric      Welch rows of one and of three segments with fr_scale undone on the host; the reference has the segment mean
              removed in long double and the bound carries the mean term.
Every case and sample type of spectrum_ld_refs runs at every length and route; a handful of frames per call (grid walking,
batching and chunking are the older suites').  Every test prints its worst error in u of ||X||_2 (pytest -s)."""
import numpy as np
import pytest

from . import spectrum_ld_refs as sr
from .spectrum_ld_refs import LD, U

pytestmark = pytest.mark.gpu

RUNS = [(N, "fused") for N in sr.FUSED] + [(N, "rows") for N in sr.FUSED + sr.ROWS_ONLY]


def set_route(monkeypatch, env, N, route):
    assert route == "rows" or N in sr.FUSED
    if route == "rows" and N in sr.FUSED:
        monkeypatch.setenv(env, "1")
    else:
        monkeypatch.delenv(env, raising=False)


def onehot(n, k):
    a = np.zeros(n)
    a[k] = 1.0
    return a


def amp_of(power):
    p = np.asarray(power, dtype=np.float64)
    assert (p >= 0).all()
    return np.sqrt(p.astype(LD))


def rms(v):
    return float(np.sqrt(np.mean(np.square(np.asarray(v, dtype=np.float64)))))


# ---- k_fbank ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,route", RUNS)
def test_fbank_bins(N, route, monkeypatch):
    from pypevoc_amd import FFTFilters as ff
    set_route(monkeypatch, "PVX_FBANK_ROWS", N, route)
    kernels = "k_fbank_fused<%d>" % N if route == "fused" else "k_frames+rocfft+k_fbank_rows"
    K = N // 2 + 1
    worst = 0.0
    for name in sr.CASE_NAMES:
        case = sr.get_case(name, N)
        bank = ff.FilterBank(nwind=N, windfunc=lambda n: case.wind.copy(), nhop=N)
        for dt in case.dtypes:
            s = case.samples(dt)
            F = len(s)
            sig = np.concatenate([s.ravel(), np.zeros(1, dtype=s.dtype)])        # F frames at hop N need one sample more
            P = np.empty((F, K))
            for b0 in range(0, K, ff.MAX_NBAND):
                ks = np.arange(b0, min(b0 + ff.MAX_NBAND, K))
                bank.fb = np.zeros((len(ks), N))
                bank.fb[np.arange(len(ks)), ks] = 1.0
                spec, _ = bank.specout(sig)
                assert ff.last_kernels() == kernels
                assert spec.shape == (F, len(ks))
                P[:, ks] = spec
            r = case.ref(dt)
            e = sr.check_bins("k_fbank %s N=%d %s %s" % (route, N, name, dt), amp_of(P), r.amp, r.tol, r.xnorm)
            worst = max(worst, e)
            mk = np.array([1, 64, N // 2 - 1])                         # the mirrored columns fold onto the same bins
            bank.fb = np.zeros((len(mk), N))
            bank.fb[np.arange(len(mk)), N - mk] = 1.0
            spec, _ = bank.specout(sig)
            assert np.array_equal(spec, P[:, mk]), (name, dt)
    print("SPECTRA k_fbank %s N=%d: worst %.2f u of ||X||_2" % (route, N, worst))


# ---- k_specdesc ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,route", RUNS)
def test_specdesc_bins(N, route, monkeypatch):
    from pypevoc_amd import SoundUtils as su
    set_route(monkeypatch, "PVX_SPECDESC_ROWS", N, route)
    base = "k_specdesc_fused<%d>" % N if route == "fused" else "k_frames+rocfft+k_specdesc_rows"
    K, H = N // 2 + 1, N // 2                                          # the periodogram keeps bins 0 .. N//2 - 1
    worst = worst_ratio = 0.0
    for name in sr.CASE_NAMES:
        case = sr.get_case(name, N)
        w = case.wind
        for dt in case.dtypes:
            s = case.samples(dt)
            F = len(s)
            r = case.ref(dt)
            what = "k_specdesc %s N=%d %s %s" % (route, N, name, dt)
            zeros = np.zeros(N, dtype=s.dtype)
            # one frame's periodogram, frame by frame; three frames' mean
            P = np.empty((F, H))
            for i in range(F):
                P[i] = su.specdesc_run(s[i], w, N, 1, su.SD_PSD)
                assert su.last_kernels() == base + "+k_specdesc_mean"
            worst = max(worst, sr.check_bins(what + " psd", amp_of(P), r.amp[:, :H], r.tol, r.xnorm))
            idx = np.arange(3) % F
            P3 = su.specdesc_run(s[idx].ravel(), w, N, 3, su.SD_PSD)
            worst = max(worst, sr.check_bins(what + " psd of 3", amp_of(P3), sr.mean_amp(r.amp[idx, :H]), sr.mean_tol(r.tol[idx], H),
                                             rms(r.xnorm[idx])))
            # the ratio tail (it carries the Nyquist bin) and the flux tail at the probe bins, against the frame's largest bin
            for i in range(F):
                kref = sr.peak_bin(r.amp[i])
                ks = sr.probe_bins(N, kref)
                xr = float(r.amp[i, kref])
                tr = float(r.tol[i, 0]) + 4 * U * xr
                assert xr > 2 * tr
                ratio, flux = np.empty(len(ks)), np.empty(len(ks))
                for j, k in enumerate(ks):
                    ratio[j] = su.specdesc_run(s[i], w, N, 1, su.SD_RATIO, onehot(K, k), onehot(K, kref))[0]
                    assert su.last_kernels() == base
                    flux[j] = su.specdesc_run(np.concatenate([s[i], zeros]), w, N, 1, su.SD_FLUX, onehot(K, k))[0]
                    assert su.last_kernels() == base
                xk = r.amp[i, ks].astype(np.float64)
                worst = max(worst, sr.check_bins(what + " flux frame %d bins %s" % (i, ks), flux, r.amp[i, ks], r.tol[i, 0], r.xnorm[i]))
                tk = r.tol[i, 0] + 4 * U * xk
                bound = (tk + xk * tr / xr) / (xr - tr)                # first order in the two bins' errors
                worst_ratio = max(worst_ratio, sr.check_bins(what + " ratio frame %d bins %s over %d" % (i, ks, kref), ratio, r.amp[i, ks] / r.amp[i, kref],
                                                             bound, r.xnorm[i] / xr))
    # frames with identical samples (the period divides the hop): their flux over the whole band is within the two frames' bounds
    case = sr.get_case("asym", N)
    r = case.ref("f64")
    for i in range(len(case.frames)):
        fl = su.specdesc_run(np.tile(case.frames[i], 2), case.wind, N, 1, su.SD_FLUX, np.ones(K))[0]
        print("k_specdesc %s N=%d: flux of two identical frames %.3e (2 tol = %.3e)" % (route, N, fl, 2 * r.tol[i, 0]))
        assert 0.0 <= fl <= 2 * r.tol[i, 0]
    print("SPECTRA k_specdesc %s N=%d: worst %.2f u of ||X||_2 (ratio tail: %.2f u of ||X||_2 / |X_ref|)" % (route, N, worst, worst_ratio))


# ---- k_xspec ---------------------------------------------------------------------------------------------------------
def xspec_check(tf, what, kernels, N, xs, ys, rx, ry, nseg):
    """x, y: samples [F][N] and their references; slot i of the call is frame i % F.  Returns the worst errors: of the
    amplitudes in u of ||X||_2, of sxy in u of ||X||_2 ||Y||_2."""
    F = len(xs)
    nblk = max(F, 2) if nseg == 1 else 2
    slots = np.arange(nblk * nseg) % F
    K = N // 2 + 1
    sxy, sxx, syy = tf.xspec_run(xs[slots].ravel(), None if ys is None else ys[slots].ravel(), rx.wind, N, 0, nseg * N, nblk, nseg)
    assert tf.last_kernels() == kernels
    assert sxx.shape == (nblk, K)
    worst = worst_xy = 0.0
    for b in range(nblk):
        idx = slots[b * nseg:(b + 1) * nseg]
        X = rx.ref
        worst = max(worst, sr.check_bins("%s sxx block %d" % (what, b), amp_of(sxx[b]), sr.mean_amp(X.amp[idx]), sr.mean_tol(X.tol[idx], K),
                                         rms(X.xnorm[idx])))
        if ys is None:
            assert sxy is None and syy is None
            continue
        Y = ry.ref
        worst = max(worst, sr.check_bins("%s syy block %d" % (what, b), amp_of(syy[b]), sr.mean_amp(Y.amp[idx]), sr.mean_tol(Y.tol[idx], K),
                                         rms(Y.xnorm[idx])))
        ref = ((Y.re[idx] * X.re[idx] + Y.im[idx] * X.im[idx]).mean(axis=0)
               + 1j * (Y.re[idx] * X.im[idx] - Y.im[idx] * X.re[idx]).mean(axis=0))                  # mean conj(Y) X
        ax, ay = X.amp[idx].astype(np.float64), Y.amp[idx].astype(np.float64)
        tx, ty = np.broadcast_to(X.tol[idx], ax.shape), np.broadcast_to(Y.tol[idx], ay.shape)
        bound = (ax * ty + ay * tx + tx * ty).mean(axis=0)
        worst_xy = max(worst_xy, sr.check_bins("%s sxy block %d" % (what, b), sxy[b], ref, bound, rms(X.xnorm[idx]) * rms(Y.xnorm[idx]),
                                               rel=4 * U * (ax * ay).mean(axis=0)))
    return worst, worst_xy


class Side(object):
    def __init__(self, ref, wind):
        self.ref, self.wind = ref, wind


@pytest.mark.parametrize("N,route", RUNS)
def test_xspec_bins(N, route, monkeypatch):
    from pypevoc_amd import TransferFunctions as tf
    set_route(monkeypatch, "PVX_XSPEC_ROWS", N, route)
    kernels = "k_xspec_fused<%d>" % N if route == "fused" else "k_frames+rocfft+k_xspec_rows"
    worst = np.zeros(2)
    for name in sr.CASE_NAMES + sr.XSPEC_ONLY:
        case = sr.get_case(name, N)
        for dt in case.dtypes:
            what = "k_xspec %s N=%d %s %s" % (route, N, name, dt)
            xs = case.samples(dt)
            rx = Side(case.ref(dt), case.wind)
            if case.y is None:                                         # y: the case's frames, one further on
                order = (np.arange(len(xs)) + 1) % len(xs)
                pairs = [(xs, xs[order], rx, Side(_reordered(rx.ref, order), case.wind))]
            else:                                                      # loud and quiet, both ways round
                ys = case.samples(dt, "y")
                ry = Side(case.ref(dt, "y"), case.wind)
                pairs = [(xs, ys, rx, ry), (ys, xs, ry, rx)]
            for nseg in (1, 3):
                for a, b, ra, rb in pairs:
                    worst = np.maximum(worst, xspec_check(tf, what + " nseg %d" % nseg, kernels, N, a, b, ra, rb, nseg))
                worst = np.maximum(worst, xspec_check(tf, what + " nseg %d, no y" % nseg, kernels, N, xs, None, rx, None, nseg))
    print("SPECTRA k_xspec %s N=%d: worst %.2f u of ||X||_2 (sxy: %.2f u of ||X||_2 ||Y||_2)" % (route, N, worst[0], worst[1]))


def _reordered(r, order):
    return sr.Ref(r.re[order], r.im[order], r.xnorm[order], r.tol[order])


# ---- k_fric ----------------------------------------------------------------------------------------------------------
def unscale(psd, wind, N):
    """mean_s |X_s[k]|^2 from a Welch row: fr_scale undone -- the one-sided factor (1 at DC and at an even length's last bin,
    2 elsewhere) and sr sum(w^2), with sr = 1 and the sum in the library's order; the division by nseg stays, it makes the mean"""
    s2 = 0.0
    for v in np.asarray(wind, dtype=np.float64):
        s2 += float(v) * float(v)
    c = np.full(N // 2 + 1, 2.0)
    c[0] = 1.0
    if N % 2 == 0:
        c[-1] = 1.0
    return (np.asarray(psd, dtype=np.float64).astype(LD) * LD(s2) / c.astype(LD)).astype(np.float64)


@pytest.mark.parametrize("N,route", RUNS)
def test_fric_bins(N, route, monkeypatch):
    from pypevoc_amd.speech import fricatives as fr
    set_route(monkeypatch, "PVX_FRIC_ROWS", N, route)
    kernels = "k_fric_fused<%d>" % N if route == "fused" else "k_fric_frames+rocfft+k_fric_acc"
    K = N // 2 + 1
    step = N - N // 2
    L3 = N + 2 * step
    assert fr.geometry(N, N)[:3] == (N, step, 1) and fr.geometry(L3, N)[:3] == (N, step, 3)
    worst = {False: 0.0, True: 0.0}                                    # dc_tiny apart: its error is the mean's, not the transform's
    for name in sr.CASE_NAMES:
        case = sr.get_case(name, N)
        tiny = name == "dc_tiny"
        for dt in case.dtypes:
            s = case.samples(dt)
            F = len(s)
            what = "k_fric %s N=%d %s %s" % (route, N, name, dt)
            # one segment per snippet: a snippet per frame
            freq, psd = fr.welch_rows(s.ravel(), np.arange(F) * N, N, nwind=N, sr=1.0, window=case.wind)
            assert fr.last_kernels() == kernels
            assert psd.shape == (F, K)
            r = case.ref(dt, demean=True)
            worst[tiny] = max(worst[tiny], sr.check_bins(what, amp_of(unscale(psd, case.wind, N)), r.amp, r.tol, r.xnorm))
            # three half-overlapping segments across two frames (and, at an odd length, a sample of a third)
            sig = np.concatenate([s[0], s[1 % F], s[0]])[:L3]
            segs = np.array([sig[i * step:i * step + N] for i in range(3)])
            r3 = sr.spectrum_ref(case.key(dt) + ("welch3", dt == "i16"), segs.astype(np.float64), case.wind, demean=True, exact_sums=dt == "i16")
            freq, psd = fr.welch_rows(sig, [0], L3, nwind=N, sr=1.0, window=case.wind)
            assert fr.last_kernels() == kernels
            assert psd.shape == (1, K)
            worst[tiny] = max(worst[tiny], sr.check_bins(what + " three segments", amp_of(unscale(psd, case.wind, N)), sr.mean_amp(r3.amp),
                                                         sr.mean_tol(r3.tol, K), rms(r3.xnorm)))
    print("SPECTRA k_fric %s N=%d: worst %.2f u of ||X||_2 (dc_tiny, where the mean's rounding leads: %.2f u of what is left)"
          % (route, N, worst[False], worst[True]))
