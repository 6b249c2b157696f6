"""The formant tracker on the GPU (pypevoc_amd.speech.formants -> pvx_formants / pvx_polyroots; k_formant.hip, pvx_roots.h)
against the reference's recorded results tests/golden/L*.npz.  Every fixture bound is 4 * sens_<output> of the case
(test_formants_cpu.py, FORMANTS.md); the worst errors measured on an MI355X are in FORMANTS.md."""

import numpy as np
import pytest

from . import formants_refs as refs
from .test_formants_cpu import all_cases, bound, case_signal, get_case

pytestmark = pytest.mark.gpu

_RUN = {}


def run_case(name, cname):
    """Formants of the case's host signal, computed once: (Time, Form, BandWidths, kernels)"""
    from pypevoc_amd.speech import formants
    if (name, cname) not in _RUN:
        g, case = get_case(name, cname)
        x = case_signal(g, case)
        keep = np.array(x)
        out = formants.Formants(x, case["Fs"], **case["kw"])
        assert np.array_equal(np.asarray(x), keep)                   # the caller's samples are not touched
        kern = formants.last_kernels()
        for a in out:
            a.setflags(write=False)
        _RUN[(name, cname)] = out + (kern,)
    return _RUN[(name, cname)]


def same_bits(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name,cname", all_cases())
def test_fixture_cases(name, cname):
    g, case = get_case(name, cname)
    Time, Form, BW, kern = run_case(name, cname)
    ref_t, ref_f, ref_b, stable = g[cname + "_Time"], g[cname + "_Form"], g[cname + "_BandWidths"], g[cname + "_stable"]
    assert Time.shape == ref_t.shape and Time.dtype == np.float64 and Time.tobytes() == ref_t.tobytes()
    assert Form.shape == ref_f.shape and BW.shape == ref_b.shape and Form.dtype == BW.dtype == np.float64
    if case["nframes"] == 0:
        return
    assert kern == "k_preemph_decim+k_formant_frames"
    assert stable.mean() >= 0.95
    assert np.array_equal(np.isnan(Form[stable]), np.isnan(ref_f[stable])) and np.array_equal(np.isnan(BW[stable]), np.isnan(ref_b[stable]))
    ok = ~np.isnan(ref_f[stable])
    assert ok.any()
    ef = float(np.max(np.abs(Form[stable][ok] - ref_f[stable][ok])))
    eb = float(np.max(np.abs(BW[stable][ok] - ref_b[stable][ok])))
    print("%s: |Form - reference| %.3e, bound %.3e; |BandWidths - reference| %.3e, bound %.3e"
          % (cname, ef, bound(g, cname, "form"), eb, bound(g, cname, "bw")))
    assert ef <= bound(g, cname, "form") and eb <= bound(g, cname, "bw"), (ef, eb)


@pytest.mark.parametrize("name,cname", [c for c in all_cases() if c[1] in ("a_44k", "d_16k", "e_nopre_o11", "f_o16", "g_i16")])
def test_frame_rows_are_the_references_roots(name, cname):
    """The C ABI's per-frame rows: canonical roots in the documented order against np.roots' (reordered by
    formants_refs.canon), nkept, and freq / bw as lpc2form derives them."""
    from pypevoc_amd.speech import formants
    g, case = get_case(name, cname)
    kw = case["kw"]
    x = case_signal(g, case)
    down, nwind, hop, nfr, order = case["down"], case["nwind"], case["hop"], case["nframes"], case["order"]
    rows = formants._formants_run(x, kw.get("hpFreq", 50) > 0, down, formants.firwin_np(down) if down > 1 else None,
                                  formants.hamming(nwind), hop, nfr, order, case["FsN"], want=("nkept", "freq", "bw", "re", "im", "lpc"))
    stable = g[cname + "_stable"]
    ref = np.array([refs.canon(r) for r in g[cname + "_roots"]])
    got = rows["re"] + 1j * rows["im"]
    assert np.all(rows["lpc"][:, 0] == 1.0) and rows["lpc"].shape == (nfr, order + 1)
    assert np.array_equal(rows["nkept"][stable], np.sum(ref.imag >= 0, axis=1)[stable])
    assert np.array_equal(np.sum(got.imag == 0, axis=1)[stable], np.sum(ref.imag == 0, axis=1)[stable])
    err = float(np.max(np.abs(got[stable] - ref[stable])))
    print("%s: |roots - np.roots| %.3e, bound %.3e" % (cname, err, bound(g, cname, "roots")))
    assert err <= bound(g, cname, "roots")
    nk, freq, bw = refs.lpc2form_rows(got, case["FsN"])
    assert np.array_equal(np.isnan(rows["freq"]), np.isnan(freq)) and np.array_equal(np.isnan(rows["bw"]), np.isnan(bw))
    m = ~np.isnan(freq)
    assert np.max(np.abs(rows["freq"][m] - freq[m])) <= 1e-12 * case["FsN"] and np.max(np.abs(rows["bw"][m] - bw[m])) <= 1e-12 * case["FsN"]


def test_roots_frames():
    """Seeded polynomials from prescribed roots (formants_refs.ROOT_POLYS), one with two trailing zero coefficients, and
    z^2 - 1.  Per root |p(z)| in np.longdouble <= 4 * 2p * 2^-53 * sum |c_k| |z|^(p-k), four times Horner's own rounding
    bound; np.roots meets the same bound on these inputs (test_formants_cpu.py)."""
    from pypevoc_amd.speech import formants
    polys = refs.root_polys()
    by_degree = {}
    for label, c, nreal, nzero in polys:
        by_degree.setdefault(len(c) - 1, []).append((label, c, nreal, nzero))
    assert sorted(by_degree) == [1, 2, 3, 5, 7, 10, 11, 16, 63, 64]
    for deg, group in sorted(by_degree.items()):
        z = formants.roots_frames(np.array([c for _, c, _, _ in group]))
        assert formants.last_kernels() == "k_polyroots" and z.shape == (len(group), deg) and z.dtype == np.complex128
        for (label, c, nreal, nzero), r in zip(group, z):
            worst = 0.0
            for v in r:
                res, hb = refs.horner_bound(c, v)
                assert res <= 4 * hb, (label, v, res, hb)
                worst = max(worst, res / hb if hb > 0 else 0.0)
            print("%s: worst |p(z)| / Horner's bound %.3f (allowed 4)" % (label, worst))
            assert np.sum(r.imag == 0) == nreal and np.sum(r == 0) == nzero, label
            assert not np.any(np.signbit(r.imag[r.imag == 0])), label                 # a real root's imaginary part is +0.0
            nk = int(np.sum(r.imag >= 0))
            up, lo = r[:nk], r[nk:]
            assert np.all(up.imag >= 0) and np.all(lo.imag < 0), label
            cplx = up[up.imag > 0]
            assert same_bits([np.conj(cplx)], [lo]), label                            # exact pairs, the conjugates in their partners' order
            ang, mag = np.arctan2(up.imag, up.real), np.abs(up)
            assert np.all((np.diff(ang) > 0) | ((np.diff(ang) == 0) & (np.diff(mag) >= 0))), label
            assert same_bits([refs.canon(r)], [r]), label
    z = formants.roots_frames(np.array([[1.0, 0.0, -1.0]]))[0]
    # |z^2 - 1| <= 4 * 4 * 2^-53 * (|z|^2 + 1) puts z within 16 * 2^-53 of +-1; the positive root (angle 0) comes first
    assert not z.imag.any() and z.real[0] > 0 > z.real[1] and np.max(np.abs(np.abs(z.real) - 1.0)) <= 17 * 2.0**-53


def test_lpc2form_and_lpcc2pole_on_the_fixture_rows():
    from pypevoc_amd.speech import formants
    g, case = get_case("L1_rates", "c_11k")
    Fs, a = case["FsN"], g["c_11k_lpc"]
    nkept, freq, bw = refs.lpc2form_rows(g["c_11k_roots"], Fs)
    bf, bb = bound(g, "c_11k", "form"), bound(g, "c_11k", "bw")
    for i in (0, 7, 20):
        k = nkept[i]
        FreqS, BW = formants.lpc2form(a[i], Fs)
        k0 = int(np.sum(~(freq[i, :k] > 0)))
        assert k0 == 1 and FreqS.shape == (k - k0,) and BW.shape == (k,)           # one positive real root: the shift is live
        assert np.max(np.abs(FreqS - freq[i, k0:k])) <= bf and np.max(np.abs(BW - bw[i, :k])) <= bb, i
        fp, pb = formants.lpcc2pole(np.concatenate(([1.0], a[i])), sr=Fs)
        assert fp.shape == pb.shape == (k,) and fp[0] == 0.0
        assert np.max(np.abs(fp - freq[i, :k])) <= bf and np.max(np.abs(pb - bw[i, :k])) <= bb, i
    b = np.hstack((np.ones((len(a), 1)), a))
    poles, bws = formants.lpcc2pole(b, sr=Fs)
    assert poles.shape == bws.shape == (len(a), b.shape[1] + 1)
    for i in range(len(a)):
        k = nkept[i]
        assert np.max(np.abs(poles[i, :k] - freq[i, :k])) <= bf and np.max(np.abs(bws[i, :k] - bw[i, :k])) <= bb, i
        assert not poles[i, k:].any() and not bws[i, k:].any()
    # lpc: the reference's return, without the leading 1
    x = case_signal(g, case)
    got = formants.lpc(x[:276], 10)
    assert got.shape == (10,) and same_bits([got], [formants.glottal.lpc(x[:276], 10)[1:]])


def test_lpcc2pole_of_iaif_olas_vocal_tract_rows():
    from pypevoc_amd.speech import formants, glottal
    from .test_glottal_cpu import case_signal as glottal_signal, get_case as glottal_case
    g, case = glottal_case("V1_11k", "v11k")
    vt = glottal.iaif_ola(glottal_signal(g, case), Fs=case["Fs"])[2]
    poles, bws = formants.lpcc2pole(vt, sr=case["Fs"])
    assert poles.shape == bws.shape == (vt.shape[0], vt.shape[1] + 1) and poles.dtype == np.float64
    z = formants.roots_frames(vt)
    nk = np.sum(z.imag >= 0, axis=1)
    for i in range(len(vt)):
        assert not poles[i, nk[i]:].any() and not bws[i, nk[i]:].any()
        assert np.all(np.diff(poles[i, :nk[i]]) >= 0) and np.all(poles[i, :nk[i]] >= 0) and np.all(poles[i, :nk[i]] <= case["Fs"] / 2)
        assert np.all(np.isfinite(bws[i, :nk[i]])) and np.all(bws[i, :nk[i]] > 0)     # an autocorrelation LPC is minimum phase


@pytest.mark.parametrize("name,cname", [c for c in all_cases() if c[1] in ("a_44k", "b_22k")])
def test_bits_do_not_depend_on_where_the_samples_are_or_on_the_grouping(name, cname, monkeypatch):
    import torch
    from pypevoc_amd.speech import formants
    g, case = get_case(name, cname)
    x = case_signal(g, case)
    want = run_case(name, cname)[:3]
    assert same_bits(formants.Formants(torch.from_numpy(np.array(x)).cuda(), case["Fs"], **case["kw"]), want)
    # per buffer: the float64 samples three frames read, one frame, every frame
    three = ((2 * case["hop"] + case["nwind"] - 1) * case["down"] + 20 * case["down"] + 2) * 8
    for limit in (three, 1, 1 << 30):
        monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(limit))
        assert same_bits(formants.Formants(x, case["Fs"], **case["kw"]), want), limit
        if limit == 1:
            assert same_bits(formants.Formants(torch.from_numpy(np.array(x)).cuda(), case["Fs"], **case["kw"]), want)


def test_silent_stretch_raises_and_names_the_first_frame():
    from pypevoc_amd.speech import formants
    g, case = get_case("L1_rates", "c_11k")
    x = np.array(case_signal(g, case))
    nwind, hop = case["nwind"], case["hop"]
    x[500:500 + nwind + 2 * hop] = 0            # the differences x[i] - x[i+1] vanish on 500 .. 1050: frames 4 and 5 are silent
    first = -(-500 // hop)
    assert first == 4 and not x[first * hop:first * hop + nwind + 1].any() and x[(first - 1) * hop:(first - 1) * hop + nwind].any()
    with pytest.raises(np.linalg.LinAlgError) as e:
        formants.Formants(x, case["Fs"])
    assert "Singular principal minor" in str(e.value) and "frame %d" % first in str(e.value)


def test_limits_are_refused_without_a_launch():
    from pypevoc_amd import PvxError, _lib
    from pypevoc_amd.speech import formants
    x = np.random.default_rng(3).standard_normal(20000)
    tw = (formants.LPC_MAX_NWIND + 1) / 11025.
    assert formants.geometry(len(x), 11025, tw)[3] == formants.LPC_MAX_NWIND + 1
    for call in (lambda: formants.roots_frames(np.ones((3, formants.ROOTS_MAX_ORDER + 2))),
                 lambda: formants.Formants(x, 11025, tWind=tw, tHop=0.05),
                 lambda: formants.Formants(x, 11025, modelOrd=formants.ROOTS_MAX_ORDER + 1)):
        formants.roots_frames(np.array([[1.0, 0.0, -0.25]]))
        assert formants.last_kernels() == "k_polyroots"
        with pytest.raises(PvxError) as e:
            call()
        assert "status %d" % _lib.PVX_ERR_UNSUPPORTED in str(e.value) and formants.last_kernels() == ""
    with pytest.raises(PvxError) as e:
        formants.roots_frames(np.array([[1.0, 2.0, 3.0], [0.0, 1.0, 1.0]]))
    assert "zero leading coefficient" in str(e.value) and "row 1" in str(e.value)
    # the largest degree, the largest window: more than 64 KB of LDS for the frame
    T, F, B = formants.Formants(x, 11025, tWind=formants.LPC_MAX_NWIND / 11025., tHop=0.05, modelOrd=64, bwMax=1e9)
    assert F.shape == B.shape == (len(T), 32) and len(T) == 6 and np.all(np.sum(~np.isnan(F), axis=1) >= 20)
