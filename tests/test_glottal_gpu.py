"""Glottal inverse filtering on the GPU (pypevoc_amd.speech.glottal -> pvx_iaif / pvx_lpc; k_iaif.hip, pvx_lpc.h) against
the reference's recorded results tests/golden/V*.npz.  Every bound is 4 * sens_<output> of the case (test_glottal_cpu.py,
GLOTTAL.md); the worst errors measured on an MI355X are in GLOTTAL.md."""

import numpy as np
import pytest

from . import glottal_refs as refs
from .test_glottal_cpu import OUTPUTS, all_cases, bound, case_kwargs, case_signal, get_case

pytestmark = pytest.mark.gpu

_RUN = {}


def run_case(name, cname):
    """iaif_ola of the case's host signal, computed once"""
    from pypevoc_amd.speech import glottal
    if (name, cname) not in _RUN:
        g, case = get_case(name, cname)
        out = glottal.iaif_ola(case_signal(g, case), Fs=case["Fs"], **case_kwargs(case))
        kern = glottal.last_kernels()
        for a in out:
            a.setflags(write=False)
        _RUN[(name, cname)] = out + (kern,)
    return _RUN[(name, cname)]


def same_bits(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name,cname", all_cases())
def test_fixture_cases(name, cname):
    g, case = get_case(name, cname)
    out = run_case(name, cname)
    pos = g[cname + "_winspos"]
    for key, got in zip(OUTPUTS, out):
        ref = g[cname + "_" + key]
        assert got.shape == ref.shape and got.dtype == ref.dtype == np.float64, key
        if ref.size == 0:
            continue
        err = float(np.max(np.abs(got - ref)))
        print("%s %s: |device - reference| %.3e, bound %.3e" % (cname, key, err, bound(g, cname, key)))
        assert np.all(np.isfinite(got)) and err <= bound(g, cname, key), (key, err, bound(g, cname, key))
    if len(g[cname + "_vt"]) == 0:
        assert out[4] == "" and not out[0].any() and not out[1].any()
        return
    assert out[4] == "k_iaif_frames+k_iaif_ola"
    # the samples no window reaches are exactly zero, and no other sample was left out
    assert not out[0][~pos].any() and not out[1][~pos].any()
    assert np.all(out[0][pos] != 0) and np.all(out[2][:, 0] == 1.0) and np.all(out[3][:, 0] == 1.0)


@pytest.mark.parametrize("name,cname", [c for c in all_cases() if c[1] in ("v11k", "v22k_it0", "v22k_it2", "v44k", "e_i16", "e_oneframe")])
def test_apply_is_the_full_calls_frame(name, cname):
    from pypevoc_amd.speech import glottal
    g, case = get_case(name, cname)
    x = case_signal(g, case)
    nwind, nhop = case["nwind"], case["nhop"]
    n_it = case["kw"].get("n_it", 1)
    inv = glottal.InverseFilter(Fs=case["Fs"], nwind=nwind, tract_order=case["tract_order"], glottal_order=case["glottal_order"])
    full = run_case(name, cname)
    # per-frame g and dg of the whole call, through the C ABI's optional outputs
    _, _, fg, fdg, fvt, fgc = glottal._iaif_run(x, nwind, nhop, len(full[2]), inv.hpfilt_b, inv.wind, None, case["tract_order"],
                                                case["glottal_order"], 0.99, n_it, False, True)
    assert glottal.last_kernels() == "k_iaif_frames"
    assert same_bits((fvt, fgc), full[2:4])
    for k, q in enumerate(int(v) for v in g[cname + "_frames"]):
        got = inv.apply(x[q * nhop:q * nhop + nwind], n_it=n_it)
        for key, a, ref in zip(("glot", "dglot", "vt", "gc"), got, (g[cname + "_fg"][k], g[cname + "_fdg"][k], g[cname + "_fvt"][k], g[cname + "_fgc"][k])):
            assert a.shape == ref.shape and np.max(np.abs(a - ref)) <= bound(g, cname, key), (q, key, np.max(np.abs(a - ref)))
        assert same_bits(got, (fg[q], fdg[q], fvt[q], fgc[q])), q


@pytest.mark.parametrize("name,cname", [c for c in all_cases() if c[1] in ("v11k_w256_h100", "v22k_it1", "e_i16", "e_f64", "e_hamming")])
def test_bits_do_not_depend_on_where_the_samples_are_or_on_the_chunking(name, cname, monkeypatch):
    import torch
    from pypevoc_amd.speech import glottal
    g, case = get_case(name, cname)
    x = case_signal(g, case)
    want = run_case(name, cname)[:4]
    assert same_bits(glottal.iaif_ola(torch.from_numpy(np.array(x)).cuda(), Fs=case["Fs"], **case_kwargs(case)), want)
    nwind = case["nwind"]
    # per buffer: rows of nwind float64 -- the overlap rows and three frames of a chunk's own, one frame, every frame
    ov = -(-(nwind - 1) // case["nhop"])
    for limit in ((ov + 3) * nwind * 8, 1, 1 << 30):
        monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(limit))
        assert same_bits(glottal.iaif_ola(x, Fs=case["Fs"], **case_kwargs(case)), want), limit
        if limit == 1:
            assert same_bits(glottal.iaif_ola(torch.from_numpy(np.array(x)).cuda(), Fs=case["Fs"], **case_kwargs(case)), want)


def lag_bound(v, p):
    """Largest change of lpc(v, p) over 8 seeded perturbations of every lag by up to len(v) * 2^-53 * r[0]"""
    r = refs.autocorr(v, p)
    a = refs.levinson(r, p)
    rng = np.random.default_rng(77)
    return a, max(float(np.max(np.abs(refs.levinson(r + rng.uniform(-1, 1, p + 1) * len(v) * 2.0**-53 * r[0], p) - a))) for _ in range(8))


def test_lpc_against_correlate_and_levinson():
    import torch
    from pypevoc_amd.speech import glottal
    g, case = get_case("V3_44k", "v44k")
    x = case_signal(g, case)
    for n, p in ((1102, 48), (300, 1), (4097, 128), (257, 7)):
        v = x[:n].astype(np.float64)
        r = np.correlate(v, v, "full")[n - 1:n + p]
        assert np.max(np.abs(refs.autocorr(v, p) - r)) <= 1e-12 * r[0]
        a, sens = lag_bound(v, p)
        got = glottal.lpc(x[:n], p)
        assert glottal.last_kernels() == "k_lpc_frames"
        print("lpc n %d order %d: |device - levinson| %.3e, bound %.3e" % (n, p, np.max(np.abs(got - a)), 4 * sens))
        assert got.shape == (p + 1,) and got[0] == 1.0 and np.max(np.abs(got - a)) <= 4 * sens, (n, p)
    # the batched form: more frames than one workgroup, an odd window, a hop that does not divide it
    nwind, hop, p = 333, 77, 12
    w = np.hamming(nwind)
    rows = glottal.lpc_frames(x, p, nwind, hop, w)
    nfr = (len(x) - nwind) // hop + 1
    assert rows.shape == (nfr, p + 1)
    for i in (0, 1, nfr // 2, nfr - 1):
        a, sens = lag_bound(x[i * hop:i * hop + nwind].astype(np.float64) * w, p)
        assert np.max(np.abs(rows[i] - a)) <= 4 * sens, i
    assert same_bits([glottal.lpc_frames(torch.from_numpy(np.array(x)).cuda(), p, nwind, hop, w)], [rows])
    assert same_bits([glottal.lpc_frames(x[5 * hop:5 * hop + nwind], p, nwind, hop, w)[0]], [rows[5]])
    assert glottal.lpc_frames(x[:nwind - 1], p, nwind, hop, w).shape == (0, p + 1) and glottal.last_kernels() == ""


def test_silent_stretch_raises_and_names_the_first_frame():
    from pypevoc_amd.speech import glottal
    g, case = get_case("V1_11k", "v11k")
    x = np.array(case_signal(g, case))
    nwind, nhop = case["nwind"], case["nhop"]
    x[500:500 + nwind + 2 * nhop] = 0                                   # frames 10 and 11 (550 .. 825, 605 .. 880) are silent
    first = -(-500 // nhop)
    assert first == 10 and not x[first * nhop:first * nhop + nwind].any() and x[(first - 1) * nhop:(first - 1) * nhop + nwind].any()
    with pytest.raises(np.linalg.LinAlgError) as e:
        glottal.iaif_ola(x, Fs=case["Fs"])
    assert "Singular principal minor" in str(e.value) and "frame %d" % first in str(e.value)
    with pytest.raises(np.linalg.LinAlgError) as e:
        glottal.lpc_frames(x, 8, nwind, nhop)
    assert "frame %d" % first in str(e.value)
    with pytest.raises(np.linalg.LinAlgError):
        glottal.lpc(np.zeros(64), 4)


def test_too_short_a_signal_launches_nothing():
    import torch
    from pypevoc_amd.speech import glottal
    for x in (np.ones(276, dtype=np.float32), torch.ones(100, dtype=torch.float64).cuda(), np.zeros(0)):
        glottal.lpc(np.arange(8.0) ** 2, 2)
        assert glottal.last_kernels() == "k_lpc_frames"
        glot, dglot, vt, gc = glottal.iaif_ola(x, Fs=11025)
        assert glottal.last_kernels() == ""
        assert glot.shape == dglot.shape == (len(x),) and glot.dtype == np.float64 and not glot.any() and not dglot.any()
        assert vt.shape == gc.shape == (0,)


def test_limits_are_refused_without_a_launch():
    from pypevoc_amd import PvxError, _lib
    from pypevoc_amd.speech import glottal
    x = np.random.default_rng(3).standard_normal(9000)
    glottal.lpc(x[:64], 2)
    for call in (lambda: glottal.iaif_ola(x, Fs=11025, nwind=glottal.IAIF_MAX_NWIND + 1),
                 lambda: glottal.iaif_ola(x, Fs=11025, tract_order=glottal.LPC_MAX_ORDER + 1),
                 lambda: glottal.lpc(x[:400], glottal.LPC_MAX_ORDER + 1)):
        with pytest.raises(PvxError) as e:
            call()
        assert "status %d" % _lib.PVX_ERR_UNSUPPORTED in str(e.value) and glottal.last_kernels() == ""
        glottal.lpc(x[:64], 2)
    # the largest window the kernel takes, with the longest filter orders: more than 64 KB of LDS
    f = glottal.InverseFilter(Fs=11025, nwind=glottal.IAIF_MAX_NWIND, tract_order=128, glottal_order=128)
    got = f.apply(x[:4096])
    ref = refs.frame(x[:4096], f.hpfilt_b, f.wind, 128, 128, 0.99, 1)
    rng = np.random.default_rng(11)

    def moved(v, p):                                                  # every lag off by up to n * 2^-53 * r[0], as the fixtures' sens_*
        r = refs.autocorr(v, p)
        return refs.levinson(r + rng.uniform(-1, 1, p + 1) * len(v) * 2.0**-53 * r[0], p)
    reruns = [refs.frame(x[:4096], f.hpfilt_b, f.wind, 128, 128, 0.99, 1, lpc=moved) for _ in range(4)]
    for k, (a, b) in enumerate(zip(got, ref)):
        sens = max(float(np.max(np.abs(r[k] - b))) for r in reruns)
        print("nwind 4096 output %d: |device - restatement| %.3e, bound %.3e" % (k, np.max(np.abs(a - b)), 4 * sens))
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 4 * sens, k
