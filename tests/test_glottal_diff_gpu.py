"""k_iaif.hip and pvx_lpc.h against the long-double stage references of tests/glottal_ld_refs.py, seeded, at the edge
shapes of the kernels (GLOTTAL.md, "Stage-wise check"; the cases and what each is for are listed there).

A frame is bit-deterministic, so InverseFilter.apply with n_it = 0, 1, 2, 3 exposes every intermediate of the chain: each
FIR and integrator output is held to the long-double formula on the filter row the device returned (a bound of pure
rounding), each LPC row to the LPC of the long-double input it had (4 * the lag sensitivity of that one LPC).  Every
sample of every row is compared.  The bounds are a priori (test_glottal_refs_cpu.py shows a float64 evaluation inside
them and a set of wrong ones outside); the tests print the worst error / bound per stage (-s), GLOTTAL.md records them."""
import numpy as np
import pytest

from . import glottal_ld_refs as ld
from . import glottal_refs as refs

pytestmark = pytest.mark.gpu


def make_filter(nwind, pt, pg, leak, b, hw):
    """an InverseFilter with the case's taps and LPC window in place of its own design"""
    from pypevoc_amd.speech import glottal
    inv = glottal.InverseFilter(Fs=11025, nwind=nwind, tract_order=pt, glottal_order=pg, leaky_integration=leak)
    inv.hpfilt_b = np.array(b, dtype=np.float64)
    inv.wind = np.array(hw, dtype=np.float64)
    return inv


def bits(arrays):
    return [(a.shape, a.dtype, a.tobytes()) for a in arrays]


def applied(inv, xf):
    """run(n_it) for check_frame: InverseFilter.apply, twice, the same bits both times"""
    from pypevoc_amd.speech import glottal

    def run(n_it):
        out = inv.apply(xf, n_it=n_it)
        assert glottal.last_kernels() == "k_iaif_frames"
        assert bits(inv.apply(xf, n_it=n_it)) == bits(out)
        return out
    return run


def report(what, ratios):
    print("%s: error / bound %s" % (what, " ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    assert all(r <= 1.0 for r in ratios.values()), (what, ratios)


def exactly_zero(a):
    return not a.any() and not np.signbit(a).any()


@pytest.mark.parametrize("case", ld.FRAME_CASES, ids=ld.case_id)
def test_single_frame_stage_by_stage(case):
    nwind, L, pt, pg, leak, _ = case
    xf, b, hw = ld.case_inputs(case)
    ratios, _ = ld.check_frame(applied(make_filter(nwind, pt, pg, leak, b, hw), xf), xf, b, hw, pt, pg, leak, key=case)
    assert set(ratios) == {"gc0", "gc", "vt", "dg", "g"}
    report(ld.case_id(case), ratios)


def test_sample_types_of_one_integer_signal_give_the_same_bits():
    nwind, L, pt, pg, leak, _ = ld.TYPES_CASE
    xf, b, hw = ld.case_inputs(ld.TYPES_CASE)
    assert np.max(np.abs(xf)) == 2e4 and np.all(xf == np.round(xf))
    inv = make_filter(nwind, pt, pg, leak, b, hw)
    for n_it in (0, 1, 3):
        want = bits(inv.apply(xf, n_it=n_it))
        assert bits(inv.apply(xf.astype(np.float32), n_it=n_it)) == want
        assert bits(inv.apply(xf.astype(np.int16), n_it=n_it)) == want


def many_frames_setup():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = 4 * cus                                                     # four resident workgroups per CU at this size
    nfr = 2 * grid + 1
    nwind, hop, pt, pg, leak = 40, 1, 7, 3, 0.99
    x = ld.ar2_noise(4040, (nfr - 1) * hop + nwind + 1)
    assert len(refs.frame_starts(len(x), nwind, hop)) == nfr
    return grid, nfr, nwind, hop, pt, pg, leak, x, ld.taps(4041, 5), np.hanning(nwind)


def test_many_frames_take_the_second_trip_of_the_frame_loop(monkeypatch):
    from pypevoc_amd.speech import glottal
    grid, nfr, nwind, hop, pt, pg, leak, x, b, hw = many_frames_setup()
    inv = make_filter(nwind, pt, pg, leak, b, hw)

    def whole():
        out = glottal._iaif_run(x, nwind, hop, nfr, b, hw, None, pt, pg, leak, 1, False, True)
        assert glottal.last_kernels() == "k_iaif_frames" and out[0] is None and out[1] is None
        return out[2:]
    rows = whole()
    assert [r.shape for r in rows] == [(nfr, nwind), (nfr, nwind), (nfr, pt + 1), (nfr, pg + 1)]
    assert all(np.all(np.isfinite(r)) for r in rows)
    for q in (0, 1, grid - 1, grid, grid + 1, 2 * grid, nfr - 1):
        assert bits(inv.apply(x[q * hop:q * hop + nwind], n_it=1)) == bits([r[q] for r in rows]), q
    for q in (grid - 1, grid, nfr - 1):
        xf = x[q * hop:q * hop + nwind]
        ratios, _ = ld.check_frame(applied(inv, xf), xf, b, hw, pt, pg, leak)
        report("frame %d of %d" % (q, nfr), ratios)
    monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(5 * nwind * 8))     # five rows of g to a group
    assert bits(whole()) == bits(rows)


@pytest.mark.parametrize("wname", ["hanning", "hamming"])
@pytest.mark.parametrize("hop", [1, 13, 63, 64, 67])
def test_overlap_add_of_the_devices_own_frame_rows(hop, wname, monkeypatch):
    import torch
    from pypevoc_amd.speech import glottal
    nwind, n, pt, pg, leak = 64, 389, 8, 4, 0.99
    x, b, hw, wind = ld.ar2_noise(6400 + hop, n), ld.taps(6401, 5), np.hanning(nwind), getattr(np, wname)(nwind)
    nfr = len(refs.frame_starts(n, nwind, hop))
    cover = (nfr - 1) * hop + nwind
    assert nfr >= 5 and cover < n

    def call(sig):
        out = glottal._iaif_run(sig, nwind, hop, nfr, b, hw, wind, pt, pg, leak, 1, True, True)
        assert glottal.last_kernels() == "k_iaif_frames+k_iaif_ola"
        return out
    out = call(x)
    glot, dglot, g, dg, vt, gc = out
    ratios, ws = ld.check_ola(glot, dglot, g, dg, wind, hop, n)
    report("overlap-add hop %d %s" % (hop, wname), ratios)
    # no window, or only a window's zero end points: exactly 0.0; so are the samples past the last frame
    assert exactly_zero(glot[ws == 0]) and exactly_zero(dglot[ws == 0])
    assert not ws[cover:].any() and np.all(ws[1:nwind - 1] > 0)
    if wname == "hanning":
        assert ws[0] == 0 and (hop != 63 or (ws[63] == 0 and ws[126] == 0)) and (hop != 67 or not ws[64:67].any())
    else:
        assert ws[0] > 0 and (hop != 67 or not ws[64:67].any())
    # the rows are the frames' own
    inv = make_filter(nwind, pt, pg, leak, b, hw)
    for q in (0, nfr - 1):
        assert bits(inv.apply(x[q * hop:q * hop + nwind], n_it=1)) == bits([g[q], dg[q], vt[q], gc[q]]), q
    # the same bits with the signal on the GPU and whatever the grouping
    assert bits(call(torch.from_numpy(x).cuda())) == bits(out)
    ov = -(-(nwind - 1) // hop)
    for limit in (1, (ov + 3) * nwind * 8):
        monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(limit))
        assert bits(call(x)) == bits(out), limit
    assert bits(call(torch.from_numpy(x).cuda())) == bits(out)


def lpc_rows_check(order, nwind):
    from pypevoc_amd.speech import glottal
    x, hop = ld.lpc_case_signal(order, nwind)
    worst = 0.0
    for wind in (None, np.hamming(nwind)):
        rows = glottal.lpc_frames(x, order, nwind, hop, wind)
        assert glottal.last_kernels() == "k_lpc_frames" and rows.shape == (4, order + 1)
        for q in (0, 3):
            fr = x[q * hop:q * hop + nwind]
            r, bnd = ld.check_lpc_row(rows[q], fr if wind is None else fr * wind, order)
            assert r <= 1.0, (order, nwind, wind is None, q, r, bnd)
            worst = max(worst, r)
        # a frame's row does not depend on its place in the call
        alone = glottal.lpc_frames(x[2 * hop:2 * hop + nwind], order, nwind, hop, wind)
        assert alone.shape == (1, order + 1) and alone[0].tobytes() == rows[2].tobytes()
    return worst


@pytest.mark.parametrize("order", ld.LPC_ORDERS)
def test_lpc_frames_at_the_seams_of_the_recursion(order):
    for nwind in ld.lpc_nwinds(order):
        print("lpc order %d nwind %d: error / bound %.3f" % (order, nwind, lpc_rows_check(order, nwind)))


def test_lpc_frames_with_fewer_samples_than_lanes():
    print("lpc order 8 nwind 33: error / bound %.3f" % lpc_rows_check(8, 33))
