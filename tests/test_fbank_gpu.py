"""FFT filter banks on the MI355X (k_fbank.hip through pypevoc_amd.FFTFilters) against the reference's outputs
(tests/golden/F*.npz, make_golden_fbank.py).

Bounds (FILTERBANK.md): band energies within 1e-9 relative of the reference, exact zeros exactly zero, no frame or band
left out; cepstra within 2 * nband * 1e-9 absolute (DCT: an error e in an energy is e in its log, matrix entries are at
most 2) or 1e-9 (IFFT, which divides by nband); rows with a non-finite log energy: the same non-finite mask, and for
all-silent rows the same kind of value.  Host and device-resident input, chunked and unchunked: identical bits.  The fused
and the rows route are different transforms: within the same 1e-9 of each other."""

import numpy as np
import pytest

from .test_fbank_cpu import MODES, all_cases, build_bank, case_signal, cep_matrix, get_case, specout_numpy

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ROWS = "k_frames+rocfft+k_fbank_rows"


def expected_kernels(nwind):
    return "k_fbank_fused<%d>" % nwind if nwind in (512, 1024, 2048) else ROWS


def assert_spec(got, ref, what):
    assert got.shape == ref.shape and got.dtype == np.float64, what
    assert np.array_equal(got == 0, ref == 0), what                   # exact zeros stay exact zeros
    nz = ref != 0
    err = float(np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]), initial=0.0))
    print("%s: spec max rel err %.3e" % (what, err))
    assert err <= RTOL, (what, err)


def kind(a):
    """nan / +inf / -inf / finite per entry (real and imaginary part apart)."""
    a = np.asarray(a)
    parts = [a.real, a.imag] if np.iscomplexobj(a) else [a]
    return np.stack([np.where(np.isnan(p), 3, np.where(np.isposinf(p), 2, np.where(np.isneginf(p), 1, 0))) for p in parts])


def assert_cep(got, ref, spec_ref, mode, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    nband = ref.shape[1]
    fin = (spec_ref != 0).all(axis=1) & np.isfinite(spec_ref).all(axis=1)
    silent = (spec_ref == 0).all(axis=1)
    tol = RTOL if mode == "IFFT" else 2 * nband * RTOL
    err = float(np.max(np.abs(got[fin] - ref[fin]), initial=0.0))
    print("%s %s: cepstra max abs err %.3e (bound %.1e), %d silent rows, %d partly silent" % (what, mode, err, tol, silent.sum(), (~fin & ~silent).sum()))
    assert np.isfinite(ref[fin]).all() and err <= tol, (what, mode, err)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref)), (what, mode)
    assert np.array_equal(kind(got[silent]), kind(ref[silent])), (what, mode)


@pytest.mark.parametrize("name,cname", all_cases())
def test_matches_reference(name, cname):
    from pypevoc_amd import FFTFilters as ft
    g, case = get_case(name, cname)
    bank = build_bank(ft, case)
    x = case_signal(ft, g, case)
    spec, t = bank.specout(x)
    ref, tref = g[cname + "_spec"], g[cname + "_t"]
    if ref.size == 0:
        assert spec.shape == (0,) and t.shape == (0,) and spec.dtype == np.float64 and ft.last_kernels() == ""
        for mode in case["modes"]:
            assert case["raises"]["mfcc"] == "ValueError"
            with pytest.raises(ValueError):
                bank.mfcc(x, mode=mode)
        return
    assert ft.last_kernels() == expected_kernels(bank.nwind)
    assert_spec(spec, ref, cname)
    assert t.dtype == np.float64 and np.array_equal(t, tref)
    for mode in case["modes"]:
        cep, spec2, t2 = bank.mfcc_and_mel(x, mode=mode)
        assert np.array_equal(spec2, spec) and np.array_equal(t2, t)
        assert_cep(cep, g[cname + "_cep_" + mode], ref, mode, cname)
        cep1, t1 = bank.mfcc(x, mode=mode)
        assert cep1.tobytes() == cep.tobytes() and np.array_equal(t1, t)


@pytest.mark.parametrize("name,cname,dtype", [("F1_mel44k", "mel44k", "float32"), ("F1_mel44k", "mel44k", "float64"),
                                              ("F3_mel8k", "mel8k", "float32"), ("F7_perlman_triangular", "rough_int16", "int16"),
                                              ("F6_nonpow2", "n999_odd", "float64"), ("F4_silence_gaps", "gaps16k", "float32")])
def test_device_resident_input_is_bit_identical(name, cname, dtype):
    import torch
    from pypevoc_amd import FFTFilters as ft
    g, case = get_case(name, cname)
    bank = build_bank(ft, case)
    x = case_signal(ft, g, case).astype(dtype)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    assert str(xd.dtype) == "torch." + dtype
    s_h, t_h = bank.specout(x)
    s_d, t_d = bank.specout(xd)
    assert s_h.tobytes() == s_d.tobytes() and np.array_equal(t_h, t_d)
    if isinstance(bank, ft.MelFilterBank):
        for mode in ("DCT2", "IFFT"):
            c_h, _ = bank.mfcc(x, mode=mode)
            c_d, _ = bank.mfcc(xd, mode=mode)
            assert c_h.dtype == c_d.dtype and c_h.tobytes() == c_d.tobytes()


def test_route_by_window_length():
    from pypevoc_amd import FFTFilters as ft
    x = np.random.default_rng(3).standard_normal(12000).astype(np.float32)
    for nwind in (256, 512, 1000, 1024, 2048, 4096, 333):
        bank = ft.FilterBank(nwind=nwind)
        spec, t = bank.specout(x)
        assert ft.last_kernels() == expected_kernels(nwind), nwind
        assert_spec(spec, specout_numpy(x, bank.wind, bank.hop, bank.fb), "nwind %d against numpy" % nwind)


@pytest.mark.parametrize("name,cname", [("F1_mel44k", "mel44k"), ("F2_mel16k_96k", "mel16k"), ("F2_mel16k_96k", "mel96k"),
                                        ("F4_silence_gaps", "gaps16k")])
def test_fused_and_rows_routes_agree(name, cname, monkeypatch):
    from pypevoc_amd import FFTFilters as ft
    g, case = get_case(name, cname)
    bank = build_bank(ft, case)
    x = case_signal(ft, g, case)
    cf, sf, tf = bank.mfcc_and_mel(x, mode="DCT2")
    assert ft.last_kernels().startswith("k_fbank_fused")
    monkeypatch.setenv("PVX_FBANK_ROWS", "1")
    cr, sr_, tr = bank.mfcc_and_mel(x, mode="DCT2")
    assert ft.last_kernels() == ROWS
    monkeypatch.delenv("PVX_FBANK_ROWS")
    assert_spec(sr_, sf, cname + " rows against fused")
    assert_spec(sr_, g[cname + "_spec"], cname + " rows against the reference")
    assert_cep(cr, g[cname + "_cep_DCT2"], g[cname + "_spec"], "DCT2", cname + " rows")
    assert np.array_equal(tf, tr)


@pytest.mark.parametrize("sr", [16000., 8000.])
def test_chunked_host_signal_equals_unchunked(sr, monkeypatch):
    from pypevoc_amd import MelFilterBank
    rng = np.random.default_rng(5)
    n = int(4 * sr)
    x = (np.sin(2 * np.pi * 300 / sr * np.arange(n)) + 1e-3 * rng.standard_normal(n)).astype(np.float32)
    x[n // 3: n // 3 + 3000] = 0
    bank = MelFilterBank(sr=sr)
    want = {m: bank.mfcc_and_mel(x, mode=m) for m in ("DCT2", "IFFT")}
    for limit in (20000, 4 * bank.nwind + 4, 100000):                 # a few frames, ONE frame, many frames per chunk
        monkeypatch.setenv("PVX_MAX_DEVICE_BYTES", str(limit))
        for m, (c, s, t) in want.items():
            c2, s2, t2 = bank.mfcc_and_mel(x, mode=m)
            assert s2.tobytes() == s.tobytes() and c2.tobytes() == c.tobytes() and np.array_equal(t2, t), (limit, m)
    monkeypatch.delenv("PVX_MAX_DEVICE_BYTES")


def test_long_signal_equals_its_pieces():
    """Another grid, another position in the call: frame i of a long call has the bits of frame 0 of a call starting there."""
    from pypevoc_amd import MelFilterBank
    sr = 44100.
    rng = np.random.default_rng(6)
    x = rng.standard_normal(int(20 * sr)).astype(np.float32)
    bank = MelFilterBank(sr=sr)
    c, s, t = bank.mfcc_and_mel(x)
    assert s.shape == (len(t), 26) and len(t) == (len(x) - 1024 + 440) // 441
    for i in (0, 1, 777, len(t) - 1):
        ci, si, ti = bank.mfcc_and_mel(x[i * 441: i * 441 + 1025])
        assert si.shape == (1, 26) and si.tobytes() == s[i].tobytes() and ci.tobytes() == c[i].tobytes()


def test_shapes_dtypes_and_zero_frames():
    import torch
    from pypevoc_amd import FFTFilters as ft
    bank = ft.MelFilterBank(sr=16000.)
    for w in (np.zeros(512), np.zeros(100, dtype=np.float32), np.zeros(0), torch.zeros(512, dtype=torch.float64, device="cuda")):
        spec, t = bank.specout(w)
        assert spec.shape == (0,) and t.shape == (0,) and spec.dtype == np.float64 and t.dtype == np.float64
        with pytest.raises(ValueError):
            bank.mfcc(w)
    x = np.random.default_rng(1).standard_normal(4000)
    c, s, t = bank.mfcc_and_mel(x, mode="IFFT")
    assert c.shape == s.shape == (22, 26) and c.dtype == np.complex128 and s.dtype == np.float64 and t.shape == (22,)
    assert bank.mfcc(x.astype(np.int16))[0].shape == (22, 26)
    assert bank.mfcc(list(x))[0].shape == (22, 26)                    # anything numpy takes
    with pytest.raises(ValueError):
        bank.specout(np.zeros((2, 4000)))
    bank.fb = bank.fb[:, :100]
    with pytest.raises(ValueError):
        bank.specout(x)


def test_silent_signal():
    from pypevoc_amd import MelFilterBank
    for sr in (16000., 8000.):
        bank = MelFilterBank(sr=sr)
        x = np.zeros(3000, dtype=np.float32)
        s, t = bank.specout(x)
        assert (s == 0).all() and not np.signbit(s).any()
        want = {"DCT1": (1, 3), "DCT2": (1, 3), "DCT3": (3, 3), "DCT4": (3, 3)}
        for mode in MODES:
            c, _ = bank.mfcc(x, mode=mode)
            k = kind(c)
            if mode == "IFFT":
                assert (k[0, :, 0] == 1).all() and (k[1, :, 0] == 0).all() and (c[:, 0].imag == 0).all() and (k[:, :, 1:] == 3).all()
            else:
                assert (k[0, :, 0] == want[mode][0]).all() and (k[0, :, 1:] == want[mode][1]).all()


@pytest.mark.parametrize("nwind", [512, 256])
def test_many_bands_and_edited_weights(nwind):
    """fb is read at call time and need not be triangles: 128 bands (the cap) of arbitrary non-negative weights, some rows
    zero, against the float64 numpy restatement; the cepstra against the defining sums."""
    from pypevoc_amd import FFTFilters as ft
    rng = np.random.default_rng(nwind)
    sr = 16000.
    bank = ft.MelFilterBank(sr=sr, n=8, twind=nwind / sr)
    assert bank.nwind == nwind and ft.MAX_NBAND == 128
    x = (np.sin(2 * np.pi * 440 / sr * np.arange(6000)) + 1e-3 * rng.standard_normal(6000)).astype(np.float32)
    fb = rng.random((128, nwind)) * (rng.random((128, nwind)) < 0.3)
    fb[5] = 0.0
    fb[127] = 0.0
    fb[64, : nwind // 2 + 1] = 0.0                                   # a band that lives in the mirrored half only
    bank.fb = fb
    want = specout_numpy(x, bank.wind, bank.hop, fb)
    for mode in MODES:
        c, s, t = bank.mfcc_and_mel(x, mode=mode)
        assert_spec(s, want, "128 bands at %d" % nwind)
        assert (s[:, 5] == 0).all() and (s[:, 64] != 0).all()
        assert not np.isfinite(c).any()                               # two bands are -inf in every frame
    bank.fb = fb + 0.01
    want = specout_numpy(x, bank.wind, bank.hop, bank.fb)
    for mode in MODES:
        c, s, t = bank.mfcc_and_mel(x, mode=mode)
        assert_spec(s, want, "128 bands at %d, no zero row" % nwind)
        ref = np.log(want) @ cep_matrix(mode, 128)
        err = float(np.max(np.abs(c - ref)))
        print("128 bands at %d %s: cepstra max abs err %.3e" % (nwind, mode, err))
        assert err <= (RTOL if mode == "IFFT" else 2 * 128 * RTOL)


def test_threads_on_one_device_give_the_sequential_results():
    import threading
    from pypevoc_amd import MelFilterBank
    rng = np.random.default_rng(9)
    jobs = [(MelFilterBank(sr=sr), rng.standard_normal(int(sr)).astype(np.float32)) for sr in (16000., 8000., 44100., 8000., 16000., 22050.)]
    want = [b.mfcc_and_mel(x) for b, x in jobs]
    got = [None] * len(jobs)

    def work(i):
        got[i] = jobs[i][0].mfcc_and_mel(jobs[i][1])
    ths = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    for w, g_ in zip(want, got):
        assert g_ is not None and all(a.tobytes() == b.tobytes() for a, b in zip(w, g_))
