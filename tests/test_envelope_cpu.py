"""The spectral-envelope half of the formant tracker (pypevoc_amd.speech.envelope) without a GPU: the matching of formants
to envelope peaks against the fixtures tests/golden/E*.npz (make_golden_envelope.py), the numpy references of
envelope_refs.py against their own bound and against the recorded peaks, the reference's refine_all unit-test parabolas, the
stubs that stay and the errors raised before the device is touched.  Also the helpers test_envelope_gpu.py shares.

Bounds: 4 * sens_<output> of the case for what the reference recorded (the factor is SPECDESC.md's; sens is the largest
change of the output over the 8 lag-perturbed reruns of the generator: ENVELOPE.md); envelope_refs.env_bound for an
envelope against its long-double evaluation."""
import glob
import os

import numpy as np
import pytest

from . import envelope_refs as er
from . import formants_refs as fr
from . import test_formants_cpu as tf
from .conftest import GOLDEN

NPTS_SET = (64, 1000, 4096)


def golden_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "E*.npz")))


def all_cases():
    return [(n, c["name"]) for n in golden_names() for c in tf.load(n)["cases"]]


def get_case(name, cname):
    """(E file, E case, L file, L case)"""
    e = tf.load(name)
    ec = next(c for c in e["cases"] if c["name"] == cname)
    g, lc = tf.get_case(ec["file"][:-4], cname)
    return e, ec, g, lc


def bound(e, cname, key):
    return 4.0 * float(e[cname + "_sens_" + key])


def coef_rows(g, cname):
    a = g[cname + "_lpc"]
    return np.hstack((np.ones((len(a), 1)), a))


def env_polys():
    """[(label, coefficient row)] of the envelope tests: formants_refs.root_polys() without z^2 - 1, whose root 1 is the
    grid's point 0."""
    return [(label, c) for label, c, _, _ in fr.root_polys() if label != "z2_minus_1"]


def parabola(max_pos, n, a=-1.0, max_val=1.0):
    """a (x - max_pos)^2 + max_val on x = 0 .. n - 1, expanded: the shape of the reference's PeakFinder unit tests."""
    x = np.arange(n)
    return a * x * x + (-2 * a * max_pos) * x + (max_val + a * max_pos * max_pos)


# (label, row, refined position, places): tests/test_peak_finder.py of the reference, its four refine_all cases
UNIT_PARABOLAS = [("centered", parabola(1.0, 3), 1.0, None), ("at_1.2", parabola(1.2, 4), 1.2, 12),
                  ("between_samples", parabola(1.5, 4), 1.5, None), ("almost_between", parabola(1.499, 4), 1.499, 7)]


def test_import_from_the_speech_package():
    from pypevoc_amd import speech
    from pypevoc_amd.speech import envelope
    assert speech.envelope is envelope
    for f in ("Formants", "lpc2form_full", "envelope_frames", "envelope_peaks_frames", "peaks_frames", "match_peaks", "last_kernels"):
        assert callable(getattr(envelope, f))
    assert envelope.ENV_MAX_NPTS == 16384


def test_fixture_list_is_complete():
    assert golden_names() == ["E1_full", "E2_edges"]
    assert sorted(c for _, c in all_cases()) == sorted(c for _, c in tf.all_cases())
    for name, cname in all_cases():
        e, ec, g, lc = get_case(name, cname)
        nfr, order = ec["nframes"], ec["order"]
        assert (nfr, order, ec["FsN"]) == (lc["nframes"], lc["order"], lc["FsN"]) and ec["npts"] == 1024
        assert e[cname + "_npk"].shape == (nfr,) and e[cname + "_idx"].shape == e[cname + "_pkF"].shape == e[cname + "_pkA"].shape == (nfr, order)
        assert e[cname + "_Peaks"].shape == e[cname + "_Amplitudes"].shape == g[cname + "_Form"].shape
        stable = e[cname + "_stable"]
        assert stable.shape == (nfr,) and (nfr == 0 or stable.mean() >= 0.95)
        assert not np.any(stable & ~g[cname + "_stable"])


@pytest.mark.parametrize("name,cname", all_cases())
def test_match_peaks_reproduces_the_recorded_peaks_bit_for_bit(name, cname):
    from pypevoc_amd.speech import envelope
    e, ec, g, lc = get_case(name, cname)
    P, A = envelope.match_peaks(g[cname + "_Form"], e[cname + "_npk"], e[cname + "_pkF"], e[cname + "_pkA"])
    for got, ref in ((P, e[cname + "_Peaks"]), (A, e[cname + "_Amplitudes"])):
        assert got.shape == ref.shape and got.dtype == ref.dtype and got.tobytes() == ref.tobytes()
    if ec["nframes"]:
        assert np.array_equal(np.isnan(P), np.isnan(g[cname + "_Form"]))  # every recorded frame has a peak


def test_match_peaks_edges():
    from pypevoc_amd.speech import envelope
    Form = np.array([[100.0, 300.0, np.nan], [100.0, np.nan, np.nan], [150.0, 250.0, 1000.0]])
    pkF = np.array([[90.0, 310.0, 500.0], [1.0, 2.0, 3.0], [100.0, 200.0, 300.0]])
    pkA = pkF * 2
    P, A = envelope.match_peaks(Form, np.array([3, 0, 3]), pkF, pkA)      # frame 1 has no peak; frame 2 has ties: the first wins
    assert np.array_equal(P, np.array([[90.0, 310.0, np.nan], [np.nan] * 3, [100.0, 200.0, 300.0]]), equal_nan=True)
    assert np.array_equal(A, 2 * P, equal_nan=True)
    P, A = envelope.match_peaks(Form, np.array([1, 2, 2]), pkF, pkA)      # entries beyond npk are never taken
    assert np.array_equal(P, np.array([[90.0, 90.0, np.nan], [2.0, np.nan, np.nan], [100.0, 200.0, 200.0]]), equal_nan=True)
    P, A = envelope.match_peaks(np.zeros((0, 5)), np.zeros(0, dtype=np.int32), np.zeros((0, 10)), np.zeros((0, 10)))
    assert P.shape == A.shape == (0, 5)
    P, A = envelope.match_peaks(Form[:1], np.array([2]), pkF[:1], pkA[:1])
    assert P.tolist()[0][:2] == [90.0, 310.0] and np.isnan(P[0, 2])


def bound_inputs():
    """[(label, coefficient row, npts)]: the first three frames of every recorded `_lpc` row set at 1024 points, and the
    root polynomials at 64, 1000 and 4096."""
    out = []
    for name, cname in tf.all_cases():
        g, _ = tf.get_case(name, cname)
        for f, c in enumerate(coef_rows(g, cname)[:3]):
            out.append(("%s[%d]" % (cname, f), c, 1024))
    for label, c in env_polys():
        for npts in NPTS_SET:
            out.append(("%s@%d" % (label, npts), c, npts))
    return out


def running_rotation(c, npts):
    """A wrong variant: z_k by repeated multiplication with z_1 (the error of a point grows with k)."""
    c = np.asarray(c, dtype=np.float64)
    z1 = np.cos(np.pi / npts) - 1j * np.sin(np.pi / npts)
    z = np.empty(npts, dtype=np.complex128)
    z[0] = 1.0
    for k in range(1, npts):
        z[k] = z[k - 1] * z1
    return horner(c, z)


def horner(c, z):
    a = np.full(len(z), c[-1], dtype=np.complex128)
    for j in range(len(c) - 2, -1, -1):
        a = a * z + c[j]
    return 1.0 / np.abs(a)


def float32_twiddles(c, npts):
    """A wrong variant: z_k from float32 sine and cosine."""
    w = (np.pi * np.arange(npts) / npts).astype(np.float32)
    return horner(np.asarray(c, dtype=np.float64), np.cos(w).astype(np.float64) - 1j * np.sin(w).astype(np.float64))


def endpoint_grid(c, npts):
    """A wrong variant: the grid with its end point, w_k = pi k / (npts - 1)."""
    w = np.pi * np.arange(npts) / (npts - 1)
    return horner(np.asarray(c, dtype=np.float64), np.cos(w) - 1j * np.sin(w))


def test_env_f64_meets_the_bound_and_wrong_variants_do_not():
    worst, margin = 0.0, np.inf
    variants = (running_rotation, float32_twiddles, endpoint_grid)
    miss = {fn.__name__: 0 for fn in variants}
    for label, c, npts in bound_inputs():
        y_ld = er.env_ld(c, npts)
        assert np.all(np.isfinite(y_ld)), label
        b = er.env_bound(c, npts, y_ld)
        y = er.env_f64(c, npts)
        ratio = float(np.max(np.abs(y - y_ld).astype(np.float64) / y_ld.astype(np.float64) / b))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (label, ratio)
        idx = er.scan(y_ld)
        assert np.array_equal(er.scan(y), idx), label
        if len(idx):                                                 # the scan's comparisons are far from flipping
            m = float(np.min(er.peak_margin(y_ld, idx).astype(np.float64) / (b[idx] * y_ld[idx].astype(np.float64))))
            margin = min(margin, m)
        for fn in variants:
            yw = fn(c, npts)
            bad = float(np.max(np.abs(yw - y_ld).astype(np.float64) / y_ld.astype(np.float64) / b)) > 1.0
            miss[fn.__name__] += int(bad or not np.array_equal(er.scan(yw), idx))
    print("env_f64 against env_ld: worst error / bound %.3f; smallest peak margin / (bound * y) %.3g; inputs the wrong variants miss: %s"
          % (worst, margin, miss))
    assert margin >= 4.0
    # the rotation's error grows with k: it shows on the long grids; the other two on every input of degree >= 2
    assert miss["running_rotation"] >= 10 and min(miss["float32_twiddles"], miss["endpoint_grid"]) >= len(bound_inputs()) - 6


def test_the_exponents_sign_and_the_rows_direction_cannot_be_told_from_an_envelope():
    """|A(e^{-jw})| = |A(e^{+jw})| = |sum_j c_{p-j} z^j| for real coefficients: neither exp(+i ..) nor a row read from its
    other end is a wrong variant (which is why the list above holds others).  Both equalities hold to rounding."""
    for label, c in env_polys():
        y = er.env_f64(c, 65)
        w = np.pi * np.arange(65) / 65
        assert np.allclose(horner(c, np.cos(w) + 1j * np.sin(w)), y, rtol=1e-9), label
        assert np.allclose(er.env_f64(c[::-1], 65), y, rtol=1e-9), label


@pytest.mark.parametrize("name,cname", all_cases())
def test_peaks_ref_reproduces_the_recorded_envelope_peaks(name, cname):
    e, ec, g, lc = get_case(name, cname)
    stable = e[cname + "_stable"]
    x = np.arange(1024) * ec["FsN"] / (2.0 * 1024)
    rows = [er.peaks_ref(er.env_f64(c, 1024), x) for c in coef_rows(g, cname)]
    npk, idx, pos, val = er.pad_lists(rows, ec["order"])
    assert np.array_equal(npk[stable], e[cname + "_npk"][stable]) and np.array_equal(idx[stable], e[cname + "_idx"][stable])
    if ec["nframes"] == 0:
        return
    ok = idx[stable] >= 0
    ef = float(np.max(np.abs(pos[stable][ok] - e[cname + "_pkF"][stable][ok])))
    ea = float(np.max(np.abs(val[stable][ok] - e[cname + "_pkA"][stable][ok])))
    print("%s: |pos - pkF| %.3e, bound %.3e; |val - pkA| %.3e, bound %.3e" % (cname, ef, bound(e, cname, "pkF"), ea, bound(e, cname, "pkA")))
    assert ef <= bound(e, cname, "pkF") and ea <= bound(e, cname, "pkA")


@pytest.mark.parametrize("label,y,want,places", UNIT_PARABOLAS, ids=[p[0] for p in UNIT_PARABOLAS])
def test_reference_refine_all_unit_tests_on_peaks_ref(label, y, want, places):
    idx, pos, val = er.peaks_ref(y)
    assert idx.tolist() == [1] and len(pos) == 1
    if places is None:
        assert pos[0] == want
    else:
        assert round(abs(pos[0] - want), places) == 0
    assert abs(val[0] - 1.0) <= 1e-12                                # a parabola's own maximum


def test_stubs_stay_and_host_side_errors_come_before_the_device():
    from pypevoc_amd.PeakFinder import PeakFinder
    from pypevoc_amd.speech import SpeechAnalysis, envelope, formants
    x = np.sin(2 * np.pi * 120 / 8000. * np.arange(3000))
    with pytest.raises(NotImplementedError) as e:
        formants.Formants(x, 11025, full=True)
    assert "refine_all" in str(e.value) and "envelope" in str(e.value)
    for call in (lambda: SpeechAnalysis.lpc2form_full(np.ones(3)), lambda: SpeechAnalysis.Formants(x, 11025, full=True)):
        with pytest.raises(NotImplementedError):
            call()
    for full in (False, True):
        with pytest.raises(ValueError) as e:
            envelope.Formants(x, 8000, full=full)
        assert "up and down must be >= 1" in str(e.value)
        with pytest.raises(ValueError) as e:
            envelope.Formants(x, 11025, modelOrd=300, full=full)
        assert "Order must be smaller than size of vector" in str(e.value)
        with pytest.raises(ValueError) as e:
            envelope.Formants(x[:100], 11025, full=full)
        assert "negative dimensions" in str(e.value)
    keep = x.copy()
    out = envelope.Formants(x[:300], 11025, full=True)
    assert len(out) == 5 and out[0].shape == (0,) and all(a.shape == (0, 5) and a.dtype == np.float64 for a in out[1:]) and np.array_equal(x, keep)
    assert len(envelope.Formants(x[:300], 11025)) == 3
    # what stays unmirrored says so
    for name in ("refine_opt", "get_areas", "find_prominence", "filter_by_prominence", "to_dict", "plot"):
        assert getattr(PeakFinder, name).__doc__.startswith("Not mirrored")
    for name in ("refine", "refine_all"):
        assert not getattr(PeakFinder, name).__doc__.startswith("Not mirrored")
    for call in (lambda: envelope.envelope_frames(np.ones(4)), lambda: envelope.envelope_peaks_frames(np.ones((2, 1))),
                 lambda: envelope.peaks_frames(np.ones(5)), lambda: envelope.peaks_frames(np.ones((2, 5)), x=np.ones(4)),
                 lambda: envelope.peaks_frames(np.ones((2, 5)), sel=np.ones((3, 2)))):
        with pytest.raises(ValueError):
            call()


def test_documents_name_the_new_module():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    assert "speech.envelope" in integ and "ENVELOPE.md" in integ
    assert "ENVELOPE.md" in open(os.path.join(root, "FORMANTS.md")).read()
    assert "ENVELOPE.md" in open(os.path.join(root, "README.md")).read()
    doc = open(os.path.join(root, "ENVELOPE.md")).read()
    for word in ("pvx_lpc_envelope", "pvx_peaks_refine", "k_lpcenv.hip", "cross-compiled, not measured", "measured once"):
        assert word in doc, word
