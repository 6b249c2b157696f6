"""The spectral-envelope half of the formant tracker on the GPU (pypevoc_amd.speech.envelope -> pvx_lpc_envelope /
pvx_peaks_refine; k_lpcenv.hip, pvx_peakref.h) against the reference's recorded results tests/golden/E*.npz, against the
long-double envelope of envelope_refs.py, and on exact rows against numpy's own arithmetic.  Fixture bounds are 4 * sens_<output>
of the case (test_envelope_cpu.py, ENVELOPE.md); the worst errors measured on an MI355X are in ENVELOPE.md."""
import ctypes

import numpy as np
import pytest

from . import envelope_refs as er
from . import test_formants_cpu as tf
from .test_envelope_cpu import UNIT_PARABOLAS, all_cases, bound, coef_rows, env_polys, get_case
from .test_formants_gpu import same_bits

pytestmark = pytest.mark.gpu

NPTS = (3, 4, 63, 64, 65, 128, 1000, 1024, 4096, 16384)
_RUN = {}


def run_case(name, cname):
    """Formants(full=True) of the case's host signal, computed once: (Time, Form, BandWidths, Peaks, Amplitudes, kernels)"""
    from pypevoc_amd.speech import envelope
    if (name, cname) not in _RUN:
        e, ec, g, lc = get_case(name, cname)
        x = tf.case_signal(g, lc)
        keep = np.array(x)
        out = envelope.Formants(x, lc["Fs"], full=True, **lc["kw"])
        assert np.array_equal(np.asarray(x), keep)                   # the caller's samples are not touched
        kern = envelope.last_kernels()
        for a in out:
            a.setflags(write=False)
        _RUN[(name, cname)] = out + (kern,)
    return _RUN[(name, cname)]


def ulps(got, ref):
    return np.abs(got - ref) / np.spacing(np.abs(ref))


@pytest.mark.parametrize("name,cname", all_cases())
def test_formants_full_on_the_fixture_cases(name, cname):
    import torch
    from pypevoc_amd.speech import envelope, formants
    e, ec, g, lc = get_case(name, cname)
    Time, Form, BW, Peaks, Amp, kern = run_case(name, cname)
    ref_t, ref_f, ref_b = g[cname + "_Time"], g[cname + "_Form"], g[cname + "_BandWidths"]
    ref_p, ref_a, stable = e[cname + "_Peaks"], e[cname + "_Amplitudes"], e[cname + "_stable"]
    assert Time.shape == ref_t.shape and Time.dtype == np.float64 and Time.tobytes() == ref_t.tobytes()
    for got, ref in ((Form, ref_f), (BW, ref_b), (Peaks, ref_p), (Amp, ref_a)):
        assert got.shape == ref.shape and got.dtype == np.float64
    x = tf.case_signal(g, lc)
    assert str(x.dtype) == lc["dtype"]
    dev = envelope.Formants(torch.from_numpy(np.array(x)).cuda(), lc["Fs"], full=True, **lc["kw"])
    assert same_bits(dev, (Time, Form, BW, Peaks, Amp))
    assert same_bits(formants.Formants(x, lc["Fs"], **lc["kw"]), (Time, Form, BW)) and same_bits(envelope.Formants(x, lc["Fs"], **lc["kw"]), (Time, Form, BW))
    if ec["nframes"] == 0:                                           # (no call reaches the library)
        return
    assert kern == "k_lpc_envelope" and stable.mean() >= 0.95
    for got, ref in ((Form, ref_f), (BW, ref_b), (Peaks, ref_p), (Amp, ref_a)):
        assert np.array_equal(np.isnan(got[stable]), np.isnan(ref[stable]))
    ok = ~np.isnan(ref_f[stable])
    assert ok.any() and np.array_equal(np.isnan(ref_p[stable]), ~ok)
    err = {k: float(np.max(np.abs(got[stable][ok] - ref[stable][ok])))
           for k, got, ref in (("form", Form, ref_f), ("bw", BW, ref_b), ("peaks", Peaks, ref_p), ("amp", Amp, ref_a))}
    bnd = dict(form=tf.bound(g, cname, "form"), bw=tf.bound(g, cname, "bw"), peaks=bound(e, cname, "peaks"), amp=bound(e, cname, "amp"))
    print("%s: " % cname + "; ".join("|%s - reference| %.3e, bound %.3e" % (k, err[k], bnd[k]) for k in err))
    for k in err:
        assert err[k] <= bnd[k], (k, err[k], bnd[k])


@pytest.mark.parametrize("name,cname", [c for c in all_cases() if c[1] != "i_noframe"])
def test_envelope_peaks_of_the_recorded_lpc_rows(name, cname):
    from pypevoc_amd.speech import envelope
    e, ec, g, lc = get_case(name, cname)
    stable = e[cname + "_stable"]
    npk, idx, pos, val = envelope.envelope_peaks_frames(coef_rows(g, cname), ec["FsN"], ec["npts"])
    assert envelope.last_kernels() == "k_lpc_envelope"
    assert npk.dtype == idx.dtype == np.int32 and idx.shape == pos.shape == val.shape == (ec["nframes"], ec["order"])
    assert np.array_equal(npk[stable], e[cname + "_npk"][stable]) and np.array_equal(idx[stable], e[cname + "_idx"][stable])
    pad = np.arange(ec["order"])[None, :] >= npk[:, None]
    assert np.all(idx[pad] == -1) and np.all(np.isnan(pos[pad])) and np.all(np.isnan(val[pad])) and not np.any(np.isnan(pos[~pad]))
    ok = ~pad[stable]
    ef = float(np.max(np.abs(pos[stable][ok] - e[cname + "_pkF"][stable][ok])))
    ea = float(np.max(np.abs(val[stable][ok] - e[cname + "_pkA"][stable][ok])))
    print("%s: |pos - pkF| %.3e, bound %.3e; |val - pkA| %.3e, bound %.3e" % (cname, ef, bound(e, cname, "pkF"), ea, bound(e, cname, "pkA")))
    assert ef <= bound(e, cname, "pkF") and ea <= bound(e, cname, "pkA")
    # lpc2form_full: one row through the same kernel, beside formants.lpc2form
    from pypevoc_amd.speech import formants
    FreqS, BWs, pkF, pkA = envelope.lpc2form_full(g[cname + "_lpc"][0], ec["FsN"])
    assert same_bits((FreqS, BWs), formants.lpc2form(g[cname + "_lpc"][0], ec["FsN"]))
    assert same_bits((pkF, pkA), (pos[0, :npk[0]], val[0, :npk[0]]))


@pytest.mark.parametrize("npts", NPTS)
def test_envelope_frames_against_the_long_double_envelope(npts):
    """Every root polynomial (degrees 1 .. 64) at this npts: the envelope within env_bound of env_ld, and -- the long-double
    peaks' margins being at least twice what the bound lets two neighbouring points move -- the same peak indices, on
    every row."""
    from pypevoc_amd.speech import envelope
    by_degree = {}
    for label, c in env_polys():
        by_degree.setdefault(len(c) - 1, []).append((label, c))
    assert sorted(by_degree) == [1, 2, 3, 5, 7, 10, 11, 16, 63, 64]
    worst, margin = 0.0, np.inf
    for deg, group in sorted(by_degree.items()):
        coef = np.array([c for _, c in group])
        env, (npk, idx, pos, val) = envelope._envelope_run(coef, npts, 1.0, deg, True, True)
        assert envelope.last_kernels() == "k_lpc_envelope" and env.shape == (len(group), npts)
        assert same_bits([envelope.envelope_frames(coef, npts)], [env])
        for (label, c), y, k, ix in zip(group, env, npk, idx):
            y_ld = er.env_ld(c, npts)
            b = er.env_bound(c, npts, y_ld)
            ratio = float(np.max(np.abs(y - y_ld).astype(np.float64) / y_ld.astype(np.float64) / b))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (label, npts, ratio)
            ref = er.scan(y_ld)
            if len(ref):
                m = float(np.min(er.peak_margin(y_ld, ref).astype(np.float64) / (b[ref] * y_ld[ref].astype(np.float64))))
                margin = min(margin, m)
                assert m >= 2.0, (label, npts, m)
            assert k == len(ref) and np.array_equal(ix[:k], ref), (label, npts)
    print("npts %5d: worst |env - env_ld| / bound %.3f; smallest peak margin / (bound * y) %.3g" % (npts, worst, margin))


def exact_rows(npts, rng):
    """Ten integer-valued rows (one with a NaN): every branch of the scan and of the packing."""
    B = -(-npts // 64)
    k = np.arange(npts)
    base = ((k * 7) % 5).astype(np.float64)
    rows = []
    rows.append((k % 2).astype(np.float64))                           # 0, 1, 0, 1 ..: (npts - 1) // 2 peaks
    r = np.zeros(npts); r[1], r[npts - 2] = 5, 7; rows.append(r)       # the first and the last interior index
    step = B if B > 1 else 2
    for first in (B - 1, B):                                          # the last / the first point of every lane's block
        r = base.copy()
        at = np.arange(first, npts - 1, step)
        at = at[(at >= 1) & (at <= npts - 2)]
        r[at] = 10 + (at % 3)
        rows.append(r)
    r = np.zeros(npts)                                                # plateaus: y[i] == y[i+1] is a peak at i, y[i-1] == y[i] is none
    r[3:5] = 4
    r[7], r[8], r[9] = 2, 2, 3
    rows.append(r)
    rows.append(np.full(npts, 3.0))                                   # constant
    rows.append(np.arange(npts, 0, -1.0))                             # monotone: the maximum at index 0
    rows.append(np.arange(npts) * 2.0)                                # monotone: the maximum at index npts - 1
    r = rng.integers(0, 10, npts).astype(np.float64)
    r[npts // 2] = np.nan
    rows.append(r)                                                    # a NaN inside
    rows.append(rng.integers(0, 10, npts).astype(np.float64))
    return np.array(rows)


@pytest.mark.parametrize("npts", (64, 65, 128, 1000))
def test_peaks_frames_on_exact_rows(npts):
    from pypevoc_amd.speech import envelope
    rows = exact_rows(npts, np.random.default_rng(npts))
    assert len(rows) == 10
    maxpk = (npts - 1) // 2
    refs = [er.peaks_ref(r) for r in rows]
    assert len(refs[0][0]) == maxpk and refs[1][0].tolist() == [1, npts - 2]
    B = -(-npts // 64)
    for r, first in ((2, B - 1), (3, B)):                             # both sides of every lane-block boundary
        at = np.arange(first, npts - 1, B if B > 1 else 2)
        assert set(at[(at >= 1) & (at <= npts - 2)].tolist()) <= set(refs[r][0].tolist())
    assert refs[4][0].tolist() == [3, 7, 9]                           # not 4 and not 8: y[i-1] == y[i] is no peak
    assert all(len(refs[i][0]) == 0 for i in (5, 6, 7))
    got = {}
    for lo, hi in ((0, 1), (1, 5), (5, 10), (0, 9), (1, 10)):         # n = 1, 4, 5, 9: one workgroup, one past it, more
        npk, idx, pos, val = envelope.peaks_frames(rows[lo:hi])
        assert envelope.last_kernels() == "k_peaks_refine" and idx.shape == pos.shape == val.shape == (hi - lo, maxpk)
        for r in range(lo, hi):
            out = (npk[r - lo:r - lo + 1], idx[r - lo], pos[r - lo], val[r - lo])
            if r in got:
                assert same_bits(out, got[r]), (r, lo, hi)            # a row's bits do not depend on its place or its batch
            got[r] = out
    worst_pos, worst_val = 0.0, 0.0
    for r, (ref_i, ref_p, ref_v) in enumerate(refs):
        npk, idx, pos, val = got[r]
        k = len(ref_i)
        assert npk[0] == k and np.array_equal(idx[:k], ref_i) and np.all(idx[k:] == -1), r
        assert np.all(np.isnan(pos[k:])) and np.all(np.isnan(val[k:]))
        for j, i in enumerate(ref_i):
            _, fval, lpos, a, b, c = er.refine(rows[r], int(i), None, True)
            assert abs(lpos) <= 0.5
            up = float(ulps(pos[j], ref_p[j]))
            vb = 4 * 2.0**-53 * (abs(a) * lpos * lpos + abs(b * lpos) + abs(c))
            worst_pos = max(worst_pos, up)
            worst_val = max(worst_val, abs(val[j] - ref_v[j]) / vb if vb else 0.0)
            assert up <= 2 and abs(val[j] - ref_v[j]) <= vb, (r, i, pos[j], ref_p[j], val[j], ref_v[j])
    print("npts %4d: worst |pos - numpy| %.1f ulp (allowed 2), worst |val - numpy| / bound %.3f" % (npts, worst_pos, worst_val))


def test_dyadic_parabolas_axis_and_given_indices():
    from pypevoc_amd import PvxError, _lib
    from pypevoc_amd.speech import envelope
    npts = 70
    k = np.arange(npts, dtype=np.float64)
    tops = [(9.25, -0.25, 3.0), (20.625, -2.0, 7.5), (33.5, -1.0, 1.0), (1.0, -0.5, 2.0), (67.75, -4.0, 9.0), (40.0, -1.0, 5.0)]
    rows = np.array([a * (k - p) * (k - p) + v for p, a, v in tops])
    npk, idx, pos, val = envelope.peaks_frames(rows)
    for r, (p, a, v) in enumerate(tops):                              # every operation of the fit is exact: so are the results
        assert npk[r] == 1 and idx[r, 0] == int(np.floor(p + 0.5) if p != 33.5 else 33) and pos[r, 0] == p and val[r, 0] == v, (r, pos[r, 0], val[r, 0])
    # a caller's axis: the interpolation between its points
    x = np.cumsum(1.0 + (np.arange(npts) % 7) / 3.0)
    _, idx2, pos2, val2 = envelope.peaks_frames(rows, x=x)
    assert same_bits((idx2, val2), (idx, val))
    for r in range(len(tops)):
        ref = er.refine(rows[r], int(idx[r, 0]), x, True)
        assert ulps(pos2[r, 0], ref[0]) <= 2 and ref[1] == val2[r, 0]
    # given indices: a peak (the fit), a point on a slope (refine's else branch: the point itself), padding
    sel = np.array([[9, 30, -1], [21, 5, 68], [33, -1, -1], [1, 2, 3], [68, 67, 1], [40, 41, 39]], dtype=np.int32)
    npk3, idx3, pos3, val3 = envelope.peaks_frames(rows, x=x, sel=sel)
    assert npk3.tolist() == [2, 3, 1, 3, 3, 3] and np.array_equal(idx3, sel)
    branches = set()
    for r in range(len(tops)):
        for j, i in enumerate(sel[r]):
            if i < 0:
                assert np.isnan(pos3[r, j]) and np.isnan(val3[r, j])
                continue
            ref = er.refine(rows[r], int(i), x)
            fit = bool(rows[r, i] > rows[r, i - 1] and rows[r, i] >= rows[r, i + 1])
            branches.add(fit)
            if fit:
                assert ulps(pos3[r, j], ref[0]) <= 2 and val3[r, j] == ref[1]
            else:
                assert pos3[r, j] == x[i] and val3[r, j] == rows[r, i]
    assert branches == {True, False}
    for bad in (0, npts - 1, npts, -2):
        s = sel.copy()
        s[3, 1] = bad
        with pytest.raises(PvxError) as e:
            envelope.peaks_frames(rows, sel=s)
        assert "status %d" % _lib.PVX_ERR_INVALID in str(e.value) and "row 3" in str(e.value)


def test_peakfinder_class_refines_on_the_device():
    from pypevoc_amd.PeakFinder import PeakFinder
    from pypevoc_amd.speech import envelope
    for label, y, want, places in UNIT_PARABOLAS:
        peaks = PeakFinder(y)
        peaks.refine_all()
        assert envelope.last_kernels() == "k_peaks_refine" and len(peaks.pos) == 1, label
        if places is None:
            assert peaks.pos[0] == want, label
        else:
            assert round(abs(peaks.pos[0] - want), places) == 0, label
        ref = er.peaks_ref(y)
        assert ulps(peaks.pos[0], ref[1][0]) <= 2 and abs(peaks.val[0] - ref[2][0]) <= 4 * 2.0**-53 * 8, label
        fpos, fval = peaks.refine(0)
        assert fpos == peaks.pos[0] and fval == peaks.val[0] and isinstance(fval, float)
    # thresholds of the constructor are honoured (the selected indices are what is refined), a caller's axis, logarithmic
    rng = np.random.default_rng(5)
    y = rng.integers(1, 50, 200).astype(np.float64)
    x = np.linspace(100.0, 900.0, 200)
    for kw in ({}, dict(npeaks=5), dict(minval=30.0)):
        peaks = PeakFinder(y, x=x, **kw)
        sel = np.array(peaks._idx)
        assert len(sel) >= 1 and (not kw or len(sel) < len(er.scan(y)))
        peaks.refine_all()
        ref = [er.refine(y, int(i), x) for i in sel]
        assert np.all(ulps(peaks.pos, np.array([t[0] for t in ref])) <= 2)
        assert np.allclose(peaks.val, np.array([t[1] for t in ref]), rtol=1e-14, atol=0)
    peaks = PeakFinder(y, x=x)
    peaks.refine_all(logarithmic=True)
    ref = [er.refine(np.log10(y), int(i), x) for i in peaks._idx]
    assert np.allclose(peaks.pos, np.array([t[0] for t in ref]), rtol=1e-13, atol=0)
    assert np.allclose(peaks.val, 10 ** np.array([t[1] for t in ref]), rtol=1e-13, atol=0)
    for call in (lambda: peaks.refine_all(rad=2), lambda: peaks.refine(0, fun=np.log), lambda: peaks.refine_opt(0)):
        with pytest.raises(NotImplementedError):
            call()


def test_contracts():
    from pypevoc_amd import PvxError, _lib
    from pypevoc_amd.speech import envelope
    lib = _lib.load()
    _lib.init()
    g, lc = tf.get_case("L1_rates", "d_16k")
    coef = coef_rows(g, "d_16k")
    n, order = coef.shape[0], coef.shape[1] - 1

    def call(coef, npts, maxpk, n=None):
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        n = coef.shape[0] if n is None else n
        npk, idx, pos, val = envelope._lists(max(n, 1), max(maxpk, 1))
        over = ctypes.c_int64(-7)
        rc = lib.pvx_lpc_envelope(_lib.dptr(coef), n, coef.shape[1] - 1, npts, 1.0, maxpk, None, envelope._i32p(npk), envelope._i32p(idx),
                                  _lib.dptr(pos), _lib.dptr(val), ctypes.byref(over))
        return rc, over.value, npk

    npk_ref = tf.load("E1_full")["d_16k_npk"]
    rc, over, npk = call(coef, 1024, 4)                               # frames with five peaks do not fit four slots
    first = int(np.nonzero(npk_ref > 4)[0][0])
    assert rc == _lib.PVX_ERR_SIZE and over == first and first > 0 and np.array_equal(npk[:first + 1], npk_ref[:first + 1])
    with pytest.raises(PvxError) as e:
        envelope._envelope_run(coef, 1024, 1.0, 4, False, True)
    assert "row %d" % first in str(e.value) and "status %d" % _lib.PVX_ERR_SIZE in str(e.value)
    rc, over, _ = call(coef, 1024, 5)
    assert rc == n and over == -1 and envelope.last_kernels() == "k_lpc_envelope"
    assert call(coef, 2, 5)[0] == _lib.PVX_ERR_INVALID and envelope.last_kernels() == ""
    envelope.envelope_frames(coef[:1], 16)
    assert envelope.last_kernels() == "k_lpc_envelope"
    for c, npts in ((coef, 16385), (np.ones((2, 66)), 1024), (coef, 0)):
        assert call(c, npts, 5)[0] == _lib.PVX_ERR_UNSUPPORTED and envelope.last_kernels() == ""
    with pytest.raises(PvxError) as e:
        envelope.peaks_frames(np.ones((2, 16385)))
    assert "status %d" % _lib.PVX_ERR_UNSUPPORTED in str(e.value) and envelope.last_kernels() == ""
    with pytest.raises(PvxError) as e:
        envelope.peaks_frames(np.ones((2, 2)))
    assert "status %d" % _lib.PVX_ERR_INVALID in str(e.value)
    assert call(coef, 1024, 5, n=0)[0] == 0 and envelope.last_kernels() == ""
    assert envelope.envelope_frames(np.ones((0, 11)), 64).shape == (0, 64)
    assert [a.shape for a in envelope.peaks_frames(np.ones((0, 9)))] == [(0,), (0, 4), (0, 4), (0, 4)]
    bad = coef.copy()
    bad[2, 0] = 0.0
    with pytest.raises(PvxError) as e:
        envelope.envelope_frames(bad, 64)
    assert "zero leading coefficient" in str(e.value) and "row 2" in str(e.value)
    # the leading coefficient need not be 1: a row times 4 is its envelope over 4
    assert np.allclose(envelope.envelope_frames(4 * coef[:2], 64), envelope.envelope_frames(coef[:2], 64) / 4, rtol=1e-14, atol=0)
    # the alternating row in one slot fewer than it needs
    y = (np.arange(65) % 2).astype(np.float64)[None, :]
    npk, idx, pos, val = envelope._lists(1, 31)
    over = ctypes.c_int64(-7)
    rc = lib.pvx_peaks_refine(_lib.dptr(y), 1, 65, None, 31, None, envelope._i32p(npk), envelope._i32p(idx), _lib.dptr(pos), _lib.dptr(val),
                              ctypes.byref(over))
    assert rc == _lib.PVX_ERR_SIZE and over.value == 0 and npk[0] == 32 and idx[0].tolist() == list(range(1, 63, 2))


def test_bits_do_not_depend_on_where_the_rows_are_or_on_the_grouping(monkeypatch):
    import torch
    from pypevoc_amd import _lib
    from pypevoc_amd.speech import envelope
    lib = _lib.load()
    g, lc = tf.get_case("L2_options", "f_o16")
    coef = coef_rows(g, "f_o16")
    n, order, npts = coef.shape[0], coef.shape[1] - 1, 1000
    env, lists = envelope._envelope_run(coef, npts, 11025.0, order, True, True)
    want = (env,) + lists
    rng = np.random.default_rng(8)
    rows = rng.integers(0, 6, (n, 130)).astype(np.float64)
    want_rows = envelope.peaks_frames(rows)
    # device rows: the _dev forms on torch's stream
    dc = torch.from_numpy(coef).cuda().reshape(-1)
    assert same_bits(envelope._envelope_run_dev(dc, n, order, npts, 11025.0, order), lists)
    dy = torch.from_numpy(rows).cuda()
    maxpk = want_rows[1].shape[1]
    dk = torch.empty(n, dtype=torch.int32, device="cuda")
    di = torch.empty((n, maxpk), dtype=torch.int32, device="cuda")
    dp, dv = torch.empty((n, maxpk), dtype=torch.float64, device="cuda"), torch.empty((n, maxpk), dtype=torch.float64, device="cuda")
    over = ctypes.c_int64(-7)
    rc = lib.pvx_peaks_refine_dev(ctypes.c_void_p(dy.data_ptr()), n, 130, None, maxpk, None, *[ctypes.c_void_p(t.data_ptr()) for t in (dk, di, dp, dv)],
                                  ctypes.byref(over), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == n and over.value == -1 and envelope.last_kernels() == "k_peaks_refine"
    assert same_bits([t.cpu().numpy() for t in (dk, di, dp, dv)], want_rows)
    # per buffer: three rows, one row, every row
    for limit in (3 * npts * 8, 1, 1 << 30):
        monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(limit))
        env2, lists2 = envelope._envelope_run(coef, npts, 11025.0, order, True, True)
        assert same_bits((env2,) + lists2, want), limit
        assert same_bits(envelope.peaks_frames(rows), want_rows), limit
    monkeypatch.delenv("PVX_MAX_DEVICE_BYTES")
    # a row alone against the same row inside the batch
    for r in (0, 5, n - 1):
        env1, lists1 = envelope._envelope_run(coef[r:r + 1], npts, 11025.0, order, True, True)
        assert same_bits((env1,) + lists1, [a[r:r + 1] for a in want]), r
        assert same_bits(envelope.peaks_frames(rows[r:r + 1]), [a[r:r + 1] for a in want_rows]), r
