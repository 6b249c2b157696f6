"""The formant kernels (k_formant.hip, pvx_roots.h) against the long-double references of tests/formants_ld_refs.py at
the hard polynomials and the edge frames (FORMANTS.md, "Differential tests").  Every bound is computed from the
references alone; test_formants_refs_cpu.py checks, without a GPU, that the bounds are meaningful: the families admitted
here, the float64 chain inside them, wrong root sets and wrong chains outside."""
import ctypes

import numpy as np
import pytest

from . import formants_ld_refs as fl
from . import formants_refs as refs

pytestmark = pytest.mark.gpu

POLYS = fl.hard_polys()
IDS = [p["label"] for p in POLYS]
SHAPES = fl.frame_shapes()
SCALE_ROWS = ("nearreal_1e-6", "lpc16_noise", "wide64_seed202")       # degree 5, 16 and 64, forward families
FS = 11025.0

_ROOTS = {}


def device_roots(label):
    """The row's roots from roots_frames, every row of its degree in one batch, computed once.  A row that met the bound
    of iterations would raise here: no hard row returns PVX_ERR_NOCONV."""
    from pypevoc_amd.speech import formants
    if not _ROOTS:
        by_degree = {}
        for p in POLYS:
            by_degree.setdefault(len(p["c"]) - 1, []).append(p)
        for deg, group in sorted(by_degree.items()):
            z = formants.roots_frames(np.array([p["c"] for p in group]))
            assert formants.last_kernels() == "k_polyroots" and z.shape == (len(group), deg) and z.dtype == np.complex128
            z.setflags(write=False)
            for p, r in zip(group, z):
                _ROOTS[p["label"]] = r
    return _ROOTS[label]


def by_label(label):
    return POLYS[IDS.index(label)]


@pytest.mark.parametrize("label", IDS)
def test_residual_and_canonical_form(label):
    p = by_label(label)
    r = device_roots(label)
    ratio = fl.residual_ratio(p["c"], r)
    print("%s: worst |p(z)| / hb %.3f (allowed 4)" % (label, ratio))
    assert ratio <= 4.0
    nreal = fl.check_canonical(p["c"], r)
    a = fl.analyse(p)
    if a["kind"] == "forward":                                         # roots apart by more than 8 delta: the count itself
        assert nreal == int(np.sum(a["z"].imag == 0))
        if p["nreal"] is not None:
            assert nreal == p["nreal"]
    elif a["kind"] == "cluster":                                       # how a multiple root splits is arbitrary: the parity
        assert (nreal - p["nreal"]) % 2 == 0


@pytest.mark.parametrize("label", [l for l in IDS if fl.analyse(by_label(l))["kind"] != "residual"])
def test_completeness_and_forward_error(label):
    p = by_label(label)
    a = fl.analyse(p)
    r = device_roots(label)
    if a["kind"] == "forward":
        ratio = fl.forward_ratio(r, a)
        print("%s: worst |z - reference| / delta %.3f (allowed 1), delta %.1e .. %.1e"
              % (label, ratio, float(np.min(a["delta"])), float(np.max(a["delta"]))))
        assert ratio <= 1.0
    else:
        ok, worst = fl.cluster_ok(r, p, a)
        print("%s: worst distance / rho %.3f (allowed 1), rho %s" % (label, worst, ", ".join("%.1e" % float(x) for x in a["rho"])))
        assert ok


def test_every_family_takes_part():
    kinds = [fl.analyse(p)["kind"] for p in POLYS]
    assert kinds.count("forward") >= 20 and kinds.count("cluster") == 4
    assert all(fl.analyse(by_label(l))["kind"] == "forward" for l in SCALE_ROWS)
    assert [len(by_label(l)["c"]) - 1 for l in SCALE_ROWS] == [5, 16, 64]


def test_trailing_zero_coefficients_give_exact_zero_roots():
    from pypevoc_amd.speech import formants
    p = by_label("pairpair_1e-4")
    c = np.concatenate((p["c"], [0.0, 0.0, 0.0]))
    r = formants.roots_frames(c[None, :])[0]
    assert fl.check_canonical(c, r) == 1 + 3 and int(np.sum(r == 0)) == 3
    assert fl.residual_ratio(c, r) <= 4.0
    rest = r[r != 0]
    assert fl.forward_ratio(rest, fl.analyse(p)) <= 1.0


@pytest.mark.parametrize("label", SCALE_ROWS)
def test_scale_of_the_row(label):
    from pypevoc_amd.speech import formants
    p = by_label(label)
    a = fl.analyse(p)
    c = p["c"]
    want = device_roots(label)
    for k in (-600, -100, 100, 600):                                   # a power of two changes no significand: the same bits
        cs = c * 2.0 ** k
        assert np.array_equal(np.frexp(cs)[0], np.frexp(c)[0])
        got = formants.roots_frames(cs[None, :])[0]
        assert got.tobytes() == want.tobytes(), k
    for s in (1e-200, 3e150, -1e-160):
        cs = c * s
        assert np.all(np.isfinite(cs)) and np.all((cs == 0) == (c == 0))
        got = formants.roots_frames(cs[None, :])[0]
        res, fwd = fl.residual_ratio(cs, got), fl.forward_ratio(got, a)
        print("%s * %g: worst |p(z)| / hb %.3f (allowed 4), worst |z - reference| / delta %.3f (allowed 1)" % (label, s, res, fwd))
        assert res <= 4.0 and fwd <= 1.0
        assert fl.check_canonical(cs, got) == int(np.sum(a["z"].imag == 0))


def polyroots_dev(coef):
    """pvx_polyroots_dev on a device tensor of rows: (re + 1j im, nkept, status) as host arrays"""
    import torch
    from pypevoc_amd import _lib
    lib = _lib.load()
    _lib.init()
    n, order = coef.shape[0], coef.shape[1] - 1
    d = torch.from_numpy(np.ascontiguousarray(coef, dtype=np.float64)).cuda()
    re, im = (torch.empty(n * order, dtype=torch.float64, device=d.device) for _ in range(2))
    nk, st = (torch.empty(n, dtype=torch.int32, device=d.device) for _ in range(2))
    noconv = ctypes.c_int64(-1)
    rc = lib.pvx_polyroots_dev(ctypes.c_void_p(d.data_ptr()), n, order, ctypes.c_void_p(re.data_ptr()), ctypes.c_void_p(im.data_ptr()),
                               ctypes.c_void_p(nk.data_ptr()), ctypes.c_void_p(st.data_ptr()), ctypes.byref(noconv),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == n and noconv.value == -1, (rc, noconv.value)
    return (re.cpu().numpy() + 1j * im.cpu().numpy()).reshape(n, order), nk.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("label,filler", [("pairpair_1e-6", "realpair_1e-2"), ("double_pair", "nearreal_1e-4"), ("wide64_seed201", "gauss64")])
def test_batch_position_and_device_input(label, filler):
    """kWaves = 4 rows share a workgroup: batches of 1, 4, 5 and 9 rows put the hard row in every wave of a full and of a
    partial workgroup"""
    from pypevoc_amd.speech import formants
    c, f = by_label(label)["c"], by_label(filler)["c"]
    want = device_roots(label)
    for n in (1, 4, 5, 9):
        for pos in sorted({0, n // 2, n - 1}):
            rows = np.array([c if i == pos else f for i in range(n)])
            z = formants.roots_frames(rows)
            assert z[pos].tobytes() == want.tobytes(), (n, pos)
            assert all(z[i].tobytes() == device_roots(filler).tobytes() for i in range(n) if i != pos), (n, pos)
    rows = np.array([f, c, f, f, c])
    z, nk, st = polyroots_dev(rows)
    assert z[1].tobytes() == want.tobytes() and z[4].tobytes() == want.tobytes() and z[0].tobytes() == device_roots(filler).tobytes()
    assert not st.any() and nk[1] == nk[4] == int(np.sum(want.imag >= 0))


# ---- frames ----------------------------------------------------------------------------------------------------------
ROWS = ("nkept", "freq", "bw", "re", "im", "lpc")


def run_shape(sh, x, h, wind):
    from pypevoc_amd.speech import formants
    rows = formants._formants_run(x, sh["pre"], sh["down"], h, wind, sh["hop"], sh["nfr"], sh["order"], FS, want=ROWS)
    assert formants.last_kernels() == "k_preemph_decim+k_formant_frames"
    return rows


def same_rows(a, b):
    return all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in ROWS)


@pytest.mark.parametrize("sh", SHAPES, ids=[s["label"] for s in SHAPES])
def test_edge_frames(sh, monkeypatch):
    import torch
    x, h, wind = fl.shape_inputs(sh)
    keep = np.array(x)
    rows = run_shape(sh, x, h, wind)
    assert np.array_equal(x, keep)
    nfr, order = sh["nfr"], sh["order"]
    assert rows["lpc"].shape == (nfr, order + 1) and np.all(rows["lpc"][:, 0] == 1.0)
    ref = fl.frame_refs(sh)
    worst = 0.0
    for f, (a, bound) in zip(fl.FRAMES_CHECKED, ref):
        f = f % nfr
        assert np.isfinite(bound) and 0 < bound <= 1e-8
        worst = max(worst, fl.gl.ratio(rows["lpc"][f, 1:], a[1:], bound))
    print("%s: worst |lpc - reference| / bound %.4f (allowed 1), bounds %.1e .. %.1e"
          % (sh["label"], worst, min(b for _, b in ref), max(b for _, b in ref)))
    assert worst <= 1.0
    # the roots of those frames are roots of the device's own LPC row, in canonical form; freq / bw as lpc2form derives them
    got = rows["re"] + 1j * rows["im"]
    res = 0.0
    for f in fl.FRAMES_CHECKED:
        f = f % nfr
        res = max(res, fl.residual_ratio(rows["lpc"][f], got[f]))
        fl.check_canonical(rows["lpc"][f], got[f])
    print("%s: worst |p(z)| / hb against the device's lpc rows %.3f (allowed 4)" % (sh["label"], res))
    assert res <= 4.0
    nk, freq, bw = refs.lpc2form_rows(got, FS)
    assert np.array_equal(rows["nkept"], nk)
    assert np.array_equal(np.isnan(rows["freq"]), np.isnan(freq)) and np.array_equal(np.isnan(rows["bw"]), np.isnan(bw))
    m = ~np.isnan(freq)
    assert np.max(np.abs(rows["freq"][m] - freq[m])) <= 1e-12 * FS and np.max(np.abs(rows["bw"][m] - bw[m])) <= 1e-12 * FS
    # from a device tensor; one frame per group (the last group's sample range is clamped at n), host and device
    dx = torch.from_numpy(np.array(x)).cuda()
    assert same_rows(run_shape(sh, dx, h, wind), rows)
    monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", "1")
    assert same_rows(run_shape(sh, x, h, wind), rows)
    assert same_rows(run_shape(sh, dx, h, wind), rows)
