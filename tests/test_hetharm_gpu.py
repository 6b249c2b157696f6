"""HeterodyneHarmonic on the MI355X (k_hetharm.hip through pypevoc_amd.HeterodyneHarmonic) against the reference's recorded
outputs (tests/golden/Q*.npz): every array within 4 * self_dist + 1e-13 of the recording, relative to the array's maximum
(self_dist: the reference's own distance from a long double evaluation, make_golden_hetharm.py; the device may be as far
from the truth as the reference is, on either side, with a factor 2 for the different summation order).  Plus what pins
the new kernels to themselves and to the trusted one: a column does not depend on the other harmonics of its launch (bit
for bit), the host and device-resident entries agree bit for bit, and every column of Q2 agrees with k_heterodyne fed the
numpy heterodyning signal.

Distances measured on an MI355X (relative to the array's maximum; tolerance in brackets):
  Q1 ah 3.8e-11 (1.5e-10)  resynth 1.9e-11 (7.8e-11)      Q2 ah 2.1e-12 (8.7e-12)  resynth_partial(19) 1.7e-11 (6.8e-11)
  Q3 ah 3.3e-13 (1.5e-12)  resynth 2.9e-13 (9.1e-13)      Q4 ah 7.8e-13 (3.2e-12)  resynth 1.8e-12 (7.2e-12)
  Q5 ah 1.2e-13 (6.2e-13)  resynth_partial(3) 2.8e-13 (6.0e-13, the closest of all)   filter_harmonic zero patterns identical
  Q6 ah 2.9e-11 (1.2e-10)  calc_adjusted_freq 4.0e-14 (2.6e-13)     Q2 ah against k_heterodyne 2.1e-12 (8.7e-12)
The device sits next to the long double value: its distance from the recording is about the recording's own self_dist."""
import numpy as np
import pytest

from .test_hetharm_cpu import ALL, check, ctor_f, load_case

pytestmark = pytest.mark.gpu

_BUILT = {}


def build(fname, name, device=False, **over):
    """the class on one recorded case (host signal, or the same samples resident on the GPU); built once per variant"""
    key = (fname, name, device, tuple(sorted(over.items())))
    if key not in _BUILT:
        from pypevoc_amd import HeterodyneHarmonic
        case, g = load_case(fname, name)
        f, tf = ctor_f(case, g)
        x = g["x"]
        if device:
            import torch
            x = torch.from_numpy(np.array(x)).cuda()
        kw = dict(case["ctor"])
        kw.update(over)
        _BUILT[key] = HeterodyneHarmonic(x, tf=tf, f=f, **kw)
    return _BUILT[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("fname,name", ALL)
def test_recorded_case(fname, name):
    case, g = load_case(fname, name)
    sd = case["self_dist"]
    h = build(fname, name)
    assert h.ah.shape == g["ah"].shape and h.ah.dtype == np.complex128
    assert np.array_equal(h.th, g["th"]) and np.array_equal(h.idxh, g["idxh"]) and np.array_equal(h.t, g["th"])
    assert h.fmin == float(g["fmin"]) and np.array_equal(h.fvec, g["fvec"]) and np.array_equal(h.f0, g["fvec"] * h.sr)
    if h.ah.shape[0] == 0:                                            # no frame: no launch, zeros
        assert h.extract_partial(1)[0].shape == (0,)
        for y in (h.resynth(), h.resynth_partial(1), h.resynth_partial(1, filter=True)):
            assert y.shape == (h.nsamp,) and not y.any()
        assert h.filter_harmonic(1).dtype == np.complex128 and not h.filter_harmonic(1).any()
        return
    check(h.ah, g["ah"], sd["ah"], 4, "%s ah" % fname)
    check(h.resynth(), g["resynth"], sd["resynth"], 4, "%s resynth" % fname)
    for n in case["filtered"]:
        fh = h.filter_harmonic(n)
        if fname.startswith("Q5"):
            assert np.array_equal(fh == 0, g["fh_%d" % n] == 0), "zero pattern of filter_harmonic(%d)" % n
        check(fh, g["fh_%d" % n], sd["fh_%d" % n], 4, "%s filter_harmonic(%d)" % (fname, n))
    for n, flt in case["partials"]:
        k = "rp_%d_%d" % (n, flt)
        check(h.resynth_partial(n, filter=bool(flt)), g[k], sd[k], 4, "%s resynth_partial(%d, %s)" % (fname, n, bool(flt)))
    assert np.array_equal(h.harmonic_amplitudes(2), h.ah[:, 2]) and h.harmonic_times(2) is h.th
    if case["adjust"]:
        f0c, tha = h.calc_adjusted_freq(h.fvec, nwind=case["adjust"]["nwind"], nhop=case["adjust"]["nhop"])
        assert np.array_equal(tha, g["adj_th"])
        check(f0c, g["adj_f0c"], sd["adj_f0c"], 4, "%s calc_adjusted_freq" % fname)
    # the per-frame properties are numpy on ah: on the recorded ah they give the recorded values
    c = h.clone()
    c.camp = np.array(g["ah"])
    assert c.ah is not h.ah and np.allclose(c.f, g["fcols"], rtol=1e-14, atol=0)
    assert np.allclose(c.angle_ratios, g["angle_ratios"], rtol=0, atol=1e-12)
    if "partial_frequencies" in g:
        assert np.allclose(c.partial_frequencies, g["partial_frequencies"], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("fname,name", [("Q2_vibrato_nharm20", "vibrato"), ("Q3_pairs_dc", "pairs"), ("Q4_one_and_no_frame", "one_frame")])
def test_extract_partial_is_the_column(fname, name):
    h = build(fname, name)
    for n in range(h.nharm):
        col, ic = h.extract_partial(n)
        want = h.ah[:, n] * 2 if n == 0 else h.ah[:, n]               # the DC column is halved in ah only
        assert np.array_equal(bits(col), bits(want)), n
        assert ic.dtype == np.int64 and np.array_equal(ic, h.nwind // 2 + np.arange(len(col)) * h.nhop)


def test_columns_do_not_depend_on_nharm():
    """nharm 8 (one full group), 9 (one past it), 16 (two full) and 20 (the last one partial): shared columns are identical"""
    hs = {n: build("Q2_vibrato_nharm20", "vibrato", nharm=n) for n in (8, 9, 16, 20)}
    for n in (8, 9, 16):
        assert hs[n].ah.shape[1] == n and np.array_equal(bits(hs[n].ah), bits(hs[20].ah[:, :n])), n


@pytest.mark.parametrize("fname,name", [("Q2_vibrato_nharm20", "vibrato"), ("Q5_filter", "filter"), ("Q4_one_and_no_frame", "one_frame"),
                                        ("Q4_one_and_no_frame", "no_frame")])
def test_device_resident_signal_gives_the_same_bits(fname, name):
    case, _ = load_case(fname, name)
    h, d = build(fname, name), build(fname, name, device=True)
    assert d._xdev is not None and isinstance(d.ah, np.ndarray)
    assert np.array_equal(bits(d.ah), bits(h.ah))
    assert np.array_equal(bits(d.resynth()), bits(h.resynth()))
    for n in case["filtered"][:2]:
        assert np.array_equal(bits(d.filter_harmonic(n)), bits(h.filter_harmonic(n)))
        assert np.array_equal(bits(d.resynth_partial(n, filter=True)), bits(h.resynth_partial(n, filter=True)))
    assert np.array_equal(bits(d.extract_partial(1)[0]), bits(h.extract_partial(1)[0]))
    a, b = d.calc_adjusted_freq(d.fvec, nwind=300, nhop=77), h.calc_adjusted_freq(h.fvec, nwind=300, nhop=77)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def test_columns_agree_with_the_single_carrier_kernel():
    """column n against pypevoc_amd.heterodyne (k_heterodyne) fed heterodyner_signal(n), the numpy phase of the reference"""
    import pypevoc_amd
    case, g = load_case("Q2_vibrato_nharm20", "vibrato")
    h = build("Q2_vibrato_nharm20", "vibrato")
    old = np.zeros_like(h.ah)
    for n in range(h.nharm):
        col, ic = pypevoc_amd.heterodyne(g["x"], h.heterodyner_signal(n), h.wind, h.nhop)
        old[:, n] = col / 2 if n == 0 else col
        assert np.array_equal(ic, h.extract_partial(n)[1])
    check(h.ah, old, case["self_dist"]["ah"], 4, "Q2 ah against k_heterodyne")


def test_resynth_is_the_sum_of_its_partials():
    """resynth() adds the harmonics in the reference's order: the same bits as adding resynth_partial(n) one by one"""
    h = build("Q3_pairs_dc", "pairs")
    y = np.zeros(h.nsamp)
    for n in range(h.nharm):
        y += h.resynth_partial(n)
    assert np.array_equal(bits(y), bits(h.resynth()))


def test_bad_arguments_fail_loudly():
    from pypevoc_amd import _lib
    h = build("Q4_one_and_no_frame", "one_frame")
    with pytest.raises(IndexError):
        h.resynth_partial(h.nharm)
    with pytest.raises(ValueError):
        h.extract_partial(-1)
    with pytest.raises(ValueError):
        h.calc_adjusted_freq(h.fvec[:-1])
    c = h.clone()
    c.camp = np.zeros((3, h.nharm), dtype=complex)                   # rows that are not this signal's frames
    with pytest.raises(_lib.PvxError, match="frames"):
        c.resynth()
